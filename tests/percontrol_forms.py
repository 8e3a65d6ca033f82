"""The compile-time forms and unit sizes of the column kernel with a TABLE PER CONTROL (csrc/sdp_colu_kernel.h,
codegen.column_percontrol_unit) as a table of cases (test infrastructure, like tests/column_forms.py and
tests/staged_forms.py; not a test file, and no GPU code).  tests/window_forms.py, the table of the row window, takes
the split rule, the inputs and the node sample from here.

The unit is compiled per (rows of axis 0, W, real type): 16-byte table builds where n0 is a multiple of 16 / sizeof(real)
(SDP_COLU_WIDE_LOADS) and one row per thread elsewhere, tables of `wchunk = 32768 // (n0 * sizeof(real))` perturbation
points at a time (SDP_COL_WCHUNK), min(512, n0 rounded up to 64) threads.  The launch code (column_grid of
csrc/sdp_hip.hip) then cuts every column into units of rows, by the number of columns and of compute units.  Every
shape the suite ran before this table has an even n0 (in 4 bytes a multiple of 4) of at most 600 rows with wchunk = W
and units of at most 128 rows: the narrow build, a second chunk of perturbation points, more row groups than threads,
four state variables, three of the four (SDP_LEAD_HAS_W, SDP_COST_HAS_W) pairs and the XCD-cut walk of
sdp_col_of_unit were never run.

A case is a model, its leading axis and W, the real type, the macros its unit must define (`claims`: a value, or None
for 'not defined') and per geometry the rows its units must have on the device (`units`: the set of row counts).  The
trailing axes are sized when the case is made, from the compute units of the chip:

  'many'    at least 4 * cus columns in ONE launch (the phased downloads of large grids, which cut a sweep into four
            launches of a quarter of the columns, are switched off: DPSolver.host_overlap): column_grid splits a
            column only as far as the unit allows (512 rows)
  'few'     7 to 9 columns: columns are split down to units of 64 to 127 rows

tests/test_percontrol_forms_plan.py checks on the CPU that every case plans what it claims, that the split rule gives
the claimed units for 256 compute units and that the table reaches what it is for;
tests/test_gpu_percontrol_forms.py runs every case at every geometry on the GPU against the direct kernel and the
numpy oracle, bit for bit."""
import re

import numpy as np

from stodynprog_amd import models, SysDescription, DPSolver
from stodynprog_amd.models import NormalLaw

CUS = 256                      # compute units of an MI355X: what the CPU tests restate the split rule for
INPUTS = ('zeros', 'smooth', 'random', 'kinked', 'flat', 'special')


# ---------------------------------------------------------------------------------------------------------------------
# column_grid of csrc/sdp_hip.hip, restated: the row ranges a column of n0 rows is cut into
# ---------------------------------------------------------------------------------------------------------------------
def splits(n0, cols, cus, seg_nodes=0):
    """clamp(ceil(4 * cus / cols), 1, n0 // 64), raised to ceil(n0 / seg_nodes) where the unit has a segment length"""
    s = max(1, min(-(-4 * int(cus) // int(cols)), max(int(n0) // 64, 1)))
    if seg_nodes > 0:
        s = max(s, -(-int(n0) // int(seg_nodes)))
    return s


def unit_bounds(n0, cols, cus, seg_nodes=0):
    """[(i_lo, i_hi)] of the units of a column: unit `part` covers rows n0 * part // splits .. n0 * (part + 1) // splits"""
    s = splits(n0, cols, cus, seg_nodes)
    return [(n0 * part // s, n0 * (part + 1) // s) for part in range(s)]


def unit_rows(n0, cols, cus, seg_nodes=0):
    """the set of row counts of a column's units"""
    return {hi - lo for lo, hi in unit_bounds(n0, cols, cus, seg_nodes)}


def launch_columns(shape, rs, host_overlap=True):
    """columns of the launches of one value_iteration call on one GPU (sdp_problem_backup_host of csrc/sdp_hip.hip):
    a grid of 8 MiB and more with at least 256 columns is swept in four launches of a quarter of the columns each, so
    that the rows of one travel to the host under the kernel of the next (DPSolver.host_overlap) -- and column_grid,
    which sees the columns of ONE launch, splits them up to four times as far"""
    cols = int(np.prod(shape[1:]))
    if host_overlap and int(np.prod(shape)) * rs >= (8 << 20) and cols >= 4 * 64:
        return [cols * (ph + 1) // 4 - cols * ph // 4 for ph in range(4)]
    return [cols]


def sweep_bounds(solver, cus, seg_nodes=0):
    """[(i_lo, i_hi)], sorted: the units of a column in every launch of a sweep of `solver`"""
    shape = solver._shape()
    out = set()
    for cols in launch_columns(shape, solver.dtype.itemsize, solver.host_overlap):
        out.update(unit_bounds(shape[0], cols, cus, seg_nodes))
    return sorted(out)


# ---------------------------------------------------------------------------------------------------------------------
# inputs and the sample of nodes the oracle is run on
# ---------------------------------------------------------------------------------------------------------------------
def inputs(shape, rs=8, seed=50):
    """the six cost-to-go arrays every case runs on, {name: float64 array}:
    'zeros';  'smooth': waves of a different length along every axis;  'random': seeded standard normal;
    'kinked': piecewise linear along the first and the last axis;
    'flat': constants so large that the cost of a control is lost in their rounding -- the lower half of axis 0 holds
    2^60 (2^40 in 4 bytes): the controls of a node differ by the rounding of their interpolation weights alone, most of
    them give the same bits, in every chunk of the control lattice, and the lowest index among the smallest must win;
    the upper half 2^44 (2^14), whose unit in the last place (2^-8, 2^-9) is coarser than the cost's change between
    neighbouring controls near its minimum: a few controls around it tie exactly;
    'special': the random field with a NaN, a +inf and a -inf at one entry in 2000 each, and at three fixed places."""
    shape = tuple(int(n) for n in shape)
    rng = np.random.default_rng(seed + len(shape))
    axes = np.meshgrid(*[np.linspace(0., 1., n) for n in shape], indexing='ij', sparse=True)
    smooth = 0.5 * axes[0] * axes[-1]
    for k, x in enumerate(axes):
        smooth = smooth + np.cos((11.0 - 3 * k) * x + 0.7 * k + 2.0 * axes[-1]) / (1 + k)
    rand = rng.standard_normal(shape)
    kinked = np.abs(axes[0] - 0.37) * 2 + 3 * np.maximum(axes[-1] - 0.6, 0.) + np.minimum(axes[0] - 0.8, 0.) + 0 * smooth
    big, coarse = (2. ** 60, 2. ** 44) if rs == 8 else (2. ** 40, 2. ** 14)
    flat = np.where(np.arange(shape[0]).reshape((-1,) + (1,) * (len(shape) - 1)) < shape[0] // 2, big, coarse) + 0 * smooth
    special = rand.copy()
    kind = rng.integers(0, 2000, size=shape)
    special[kind == 0] = np.nan
    special[kind == 1] = np.inf
    special[kind == 2] = -np.inf
    special.ravel()[[special.size // 3, special.size // 2, 2 * special.size // 3]] = np.nan, np.inf, -np.inf    # (a small grid too)
    return {'zeros': np.zeros(shape), 'smooth': smooth, 'random': rand, 'kinked': kinked, 'flat': flat,
            'special': special}


def sample_nodes(shape, bounds, n=300, seed=0):
    """flat C-order node ids, sorted: `n` random ones; rows 0 and n0 - 1 and the rows on either side of every unit
    boundary in `bounds` ([(i_lo, i_hi)]), in the first column, the last but one, one in the middle and three random
    ones; the whole last column"""
    n0, cols = int(shape[0]), int(np.prod(shape[1:]))
    rng = np.random.default_rng(seed + n0 + cols)
    picked = set(rng.choice(n0 * cols, size=min(n, n0 * cols), replace=False).tolist())
    rows = {0, n0 - 1}
    for lo, hi in bounds:
        rows.update(r for r in (lo - 1, lo, hi - 1, hi) if 0 <= r < n0)
    for col in [0, max(cols - 2, 0), cols // 2] + rng.integers(0, cols, size=3).tolist():
        picked.update(r * cols + col for r in rows)
    picked.update(r * cols + cols - 1 for r in range(n0))
    return np.array(sorted(picked), dtype=np.int64)


def macro(source, name):
    """value of `#define name value` in a generated source, or None"""
    m = re.search(r'^#define {} (\S+)'.format(re.escape(name)), source, re.M)
    return m.group(1) if m else None


def missing_claims(claims, source):
    """the claims that `source` does not meet: [(macro, claimed, found)]"""
    return [(k, v, macro(source, k)) for k, v in sorted(claims.items()) if macro(source, k) != v]


# ---------------------------------------------------------------------------------------------------------------------
# the models
# ---------------------------------------------------------------------------------------------------------------------
def price_maker(n_E, n_w=5, lead_w=False, cost_w=True, box_on_price=False):
    """the price maker of tests/test_gpu_percontrol.py (a stock whose use moves the price process, two controls, 27
    lattice points); `lead_w`: the perturbation also reaches the stock (SDP_LEAD_HAS_W), `cost_w`: and the cost"""
    def make(trailing):
        sysd = SysDescription((2, 2, 1), name='price maker')
        if lead_w:
            sysd.dyn = lambda E, P, u, v, w: (E + u - 0.1 * v + 0.2 * w, 0.7 * P + w + 0.05 * u - 0.02 * v)
        else:
            sysd.dyn = lambda E, P, u, v, w: (E + u - 0.1 * v, 0.7 * P + w + 0.05 * u - 0.02 * v)
        if cost_w:
            sysd.cost = lambda E, P, u, v, w: P * u + 0.1 * u * u + 0.3 * (v - 0.2) ** 2 + 0.01 * E + w * v
        else:
            sysd.cost = lambda E, P, u, v, w: P * u + 0.1 * u * u + 0.3 * (v - 0.2) ** 2 + 0.01 * E
        sysd.control_box = lambda E, P: ((-1.0, 1.0 + (0.1 * P if box_on_price else 0.0)), (0.0, 0.5))
        sysd.perturb_laws = [NormalLaw(0, 0.3)]
        s = DPSolver(sysd)
        s.discretize_state(0, 10, n_E, -2, 2, trailing[0])
        s.discretize_perturb(-0.6, 0.6, n_w)
        s.control_steps = (0.25, 0.25)
        return s
    return make


def deterministic(n_E):
    """no perturbation: SDP_HAS_W 0, one table per control"""
    def make(trailing):
        sysd = SysDescription((2, 1, 0), name='deterministic price maker')
        sysd.dyn = lambda E, P, u: (E + u, 0.8 * P + 0.1 * u)
        sysd.cost = lambda E, P, u: P * u + 0.2 * u * u + 0.01 * E
        sysd.control_box = lambda E, P: ((-1., 1.),)
        s = DPSolver(sysd)
        s.discretize_state(0, 10, n_E, -2, 2, trailing[0])
        s.control_steps = (0.125,)
        return s
    return make


def coupled3d(n0, n_w=6):
    """models.synthetic3d_coupled (three state variables, 64 controls) re-discretised"""
    def make(trailing):
        _, s = models.synthetic3d_coupled(N=8, n_w=n_w)
        s.discretize_state(0, 1, n0, 0, 1, trailing[0], 0, 1, trailing[1])
        return s
    return make


def four_states(n0=96, n_w=5):
    """four state variables (SDP_D 4, SDP_DT 3: tables of 8-vertex cells), a constant box"""
    def make(trailing):
        sysd = SysDescription((4, 1, 1), name='four states')
        sysd.dyn = lambda E, P, Q, R, u, w: (E + u, 0.7 * P + w + 0.05 * u, 0.5 * Q + 0.1 * u, 0.9 * R + 0.3 * w)
        sysd.cost = lambda E, P, Q, R, u, w: P * u + 0.1 * u * u + 0.01 * E + Q * R * 0.1
        sysd.control_box = lambda E, P, Q, R: ((-1.0, 1.0),)
        sysd.perturb_laws = [NormalLaw(0, 0.3)]
        s = DPSolver(sysd)
        s.discretize_state(0, 10, n0, -2, 2, trailing[0], -1, 1, trailing[1], -1, 1, trailing[2])
        s.discretize_perturb(-0.6, 0.6, n_w)
        s.control_steps = (0.25,)
        return s
    return make


# trailing axes per geometry, from the compute units of the chip (odd lengths of the price axis hold P = 0, where the
# price maker's controls u and -u tie exactly on a constant cost-to-go)
_LINE = {'many': lambda cus: (4 * cus + 1,), 'few': lambda cus: (7,)}
_XCD_CUT = {'many': lambda cus: (8 * -(-cus // 128), 64)}            # n1 % 8 == 0, n2 % 64 == 0, >= 4 * cus columns
_TILES = {'many': lambda cus: (-(-4 * cus // 40), 40)}               # n2 % 8 == 0 only: 8 x 8 tiles of columns
_IDENTITY = {'many': lambda cus: (-(-4 * cus // 41), 41)}            # neither: columns in their own order
_FOUR = {'many': lambda cus: (-(-4 * cus // 24), 6, 4), 'few': lambda cus: (2, 2, 2)}


class Case(object):
    """name; make(trailing axes) -> solver; n0, W; dtype; claims {macro: value or None}; trailing {geometry: cus ->
    trailing axes}; units {geometry: the set of row counts of its units}; walk: the branch of sdp_col_of_unit its
    'many' geometry takes ('xcd', 'tiles', 'identity')"""

    def __init__(self, name, make, n0, W, claims, units, dtype=np.float64, trailing=_LINE, walk='identity'):
        self.name, self.make, self.n0, self.W, self.walk = name, make, int(n0), int(W), walk
        self.dtype, self.claims, self.trailing = np.dtype(dtype), dict(claims), dict(trailing)
        self.units = {g: set(u) for g, u in units.items()}
        self.geometries = tuple(g for g in ('many', 'few') if g in self.units)
        assert set(self.units) <= set(self.trailing), name

    def __repr__(self):
        return self.name

    @property
    def rs(self):
        return self.dtype.itemsize

    def solver(self, geometry, kernel='column', cus=CUS):
        s = self.make(self.trailing[geometry](cus))
        s.dtype = self.dtype
        s.kernel = kernel
        s.host_overlap = geometry != 'many'
        return s

    def wchunk(self):
        """perturbation points per table, and the sizes of its chunks"""
        wc = int(self.claims['SDP_COL_WCHUNK'])
        Wn = max(self.W, 1)
        return wc, [min(wc, Wn - w) for w in range(0, Wn, wc)]


def _unit(n0, W, rs, wide, lead_w=0, cost_w=1, d=2, has_w=1):
    threads = min(512, max(64, (n0 + 63) // 64 * 64))
    return {'SDP_TRAIL_HAS_U': '1', 'SDP_COL_N0': str(n0), 'SDP_COL_W': str(max(W, 1)), 'SDP_COL_THREADS': str(threads),
            'SDP_COL_WCHUNK': str(max(1, min(max(W, 1), 32768 // (n0 * rs)))), 'SDP_COLU_WIDE_LOADS': '1' if wide else None,
            'SDP_LEAD_HAS_W': str(lead_w), 'SDP_COST_HAS_W': str(cost_w), 'SDP_D': str(d), 'SDP_HAS_W': str(has_w),
            'SDP_COL_FILTER': None, 'SDP_COL_ROWS': None}


def _pm(name, n0, W, wide, units, dtype=np.float64, **kw):
    rs = np.dtype(dtype).itemsize
    return Case(name, price_maker(n0, W, **kw), n0, W,
                _unit(n0, W, rs, wide, int(kw.get('lead_w', False)), int(kw.get('cost_w', True))), units, dtype)


_F4 = np.float32
CASES = [
    # ---- 8-byte reals: wide and narrow builds, wchunk = W / between / 1, one to three trips of the build's row loop
    _pm('wide_n600', 600, 5, True, {'many': {300}, 'few': {66, 67}}),                # wchunk 5 = W, 300 row groups
    _pm('narrow_n601', 601, 5, False, {'many': {300, 301}, 'few': {66, 67}}),        # two trips of the row loop
    _pm('wide_n1500_chunks_2_2_1', 1500, 5, True, {'many': {500}, 'few': {65, 66}}),      # 750 row groups on 512 threads
    _pm('narrow_n1501_chunks_2_2_2_1', 1501, 7, False, {'many': {500, 501}, 'few': {65, 66}}),     # three trips
    _pm('wide_n2050_wchunk1', 2050, 5, True, {'many': {410}, 'few': {64, 65}}),
    _pm('narrow_n65', 65, 5, False, {'many': {65}, 'few': {65}}),                    # 128 threads, 63 of them idle
    _pm('wide_n70_three_groups_along_w', 70, 5, True, {'many': {70}, 'few': {70}}),  # 35 row groups on 128 threads
    # ---- 4-byte reals: four rows a lane in the wide build
    _pm('f32_narrow_n63', 63, 5, False, {'many': {63}, 'few': {63}}, _F4),           # 64 threads
    _pm('f32_wide_n600', 600, 5, True, {'many': {300}, 'few': {66, 67}}, _F4),       # wchunk 5 = W
    _pm('f32_wide_n2052_chunks_3_3_1', 2052, 7, True, {'many': {410, 411}, 'few': {64, 65}}, _F4),    # 513 row groups
    _pm('f32_narrow_n2731_chunks_2x4_1', 2731, 9, False, {'many': {455, 456}, 'few': {65, 66}}, _F4),
    # ---- the four (SDP_LEAD_HAS_W, SDP_COST_HAS_W) pairs where wchunk < W: `w_lo + j` in SDP_COLU_LOCATE and the cost
    _pm('lead_w_cost_w_n1500', 1500, 5, True, {'many': {500}, 'few': {65, 66}}, lead_w=True, cost_w=True),
    _pm('lead_w_n1501', 1501, 5, False, {'many': {500, 501}}, lead_w=True, cost_w=False),
    _pm('no_w_in_lead_or_cost_n1500', 1500, 5, True, {'many': {500}}, lead_w=False, cost_w=False),
    _pm('f32_lead_w_cost_w_n2052', 2052, 7, True, {'many': {410, 411}}, _F4, lead_w=True, cost_w=True),
    # ---- no perturbation, and a box that depends on the trailing state
    Case('deterministic_n601', deterministic(601), 601, 0, _unit(601, 0, 8, False, 0, 0, has_w=0),
         {'many': {300, 301}, 'few': {66, 67}}),
    _pm('box_on_price_n1500', 1500, 5, True, {'many': {500}, 'few': {65, 66}}, box_on_price=True),
    # ---- three state variables: the three branches of sdp_col_of_unit, whole columns (col_splits == 1)
    Case('d3_xcd_cut', coupled3d(130), 130, 6, _unit(130, 6, 8, True, 0, 0, d=3), {'many': {130}}, trailing=_XCD_CUT,
         walk='xcd'),
    Case('d3_tiles', coupled3d(131), 131, 6, _unit(131, 6, 8, False, 0, 0, d=3), {'many': {131}}, trailing=_TILES,
         walk='tiles'),
    Case('d3_identity', coupled3d(130), 130, 6, _unit(130, 6, 8, True, 0, 0, d=3), {'many': {130}}, trailing=_IDENTITY),
    # ---- four state variables
    Case('d4_n96', four_states(96), 96, 5, _unit(96, 5, 8, True, 0, 0, d=4), {'many': {96}, 'few': {96}}, trailing=_FOUR),
]
BY_NAME = {c.name: c for c in CASES}
PAIRS = [(c, g) for c in CASES for g in c.geometries]
RUNS = [(c, g, v) for c, g in PAIRS for v in INPUTS]


def walk_branch(shape, col_splits, launches=1):
    """the branch of sdp_col_of_unit (csrc/sdp_column_kernel.h) the launches of a sweep take"""
    if len(shape) != 3:
        return 'identity'
    n1, n2 = shape[1], shape[2]
    if col_splits == 1 and launches == 1 and n2 % 64 == 0 and n1 % 8 == 0:
        return 'xcd'
    return 'tiles' if n2 % 8 == 0 and n1 >= 8 else 'identity'


def unit_sources(case, cus=CUS):
    """{what: generated source} of every unit tests/test_gpu_percontrol_forms.py runs for the case on a chip of `cus`
    compute units: the table per control and the direct kernel, per geometry"""
    out = {}
    for g in case.geometries:
        for kernel in ('column', 'generic'):
            out['{}, {}'.format(g, kernel)] = case.solver(g, kernel, cus)._kernel_plan()['source']
    return out
