"""The shapes and decision paths of the filtered line kernel (csrc/sdp_line_kernel.h) as a table of cases (test
infrastructure, like tests/column_forms.py; not a test file, and no GPU code).

DPSolver._kernel_plan_now (the line kernel's own part of it; codegen.translation_unit then gets W as the family it
prints) turns three numbers -- nodes S, the largest control lattice and the perturbation points W -- into
SDP_LANES = min(64, max(need, want)): `need` keeps a tile's (node, perturbation point) terms within the kernel's LDS
table (64 / lanes x W <= 2048), `want` fills the chip and keeps at least 8 controls in a slice.  The lane count sets the
shape of everything the kernel merges: NPW = 64 / lanes nodes per tile, P = 4 lanes slices of the control lattice, the
rounds of the shuffles in sdp_line_merge.  Each case below names a model, a shape, and what it claims: the lane count
with the branch of the formula that decided it, SDP_LINE_W, SDP_LINE_CHAIN, the kind of span, whether the lattice is
usable -- and, per input value array, which of the nine counters of the SDP_LINE_DIAG build it makes non-zero (PATHS:
these exist only on the device; they were read off a run on an MI355X and are asserted from then on).

tests/test_line_forms_plan.py checks on the CPU that every case still plans what it claims, that the table covers what
it is for, and that its units compile; tests/test_gpu_line_forms.py runs every case and input on the GPU against the
direct kernel and the numpy oracle, bit for bit, and checks the counters."""
import re

import numpy as np

from stodynprog_amd import SysDescription, DPSolver, models

# the words of SdpSweepArgs.stamps a SDP_LINE_DIAG build counts in (csrc/sdp_line_kernel.h, SDP_LN_COUNT), in order
COUNTERS = ('single1', 'pair1', 'undecided1', 'single2', 'pair2', 'left2', 'bad', 'evals2', 'long way')
DIAG = {'SDP_EXTRA_DEFINES': 'SDP_LINE_DIAG=1'}
# every half-width x 1e18: nothing is decided by either level, every control of every node goes the long way
DIAG_WIDE = dict(DIAG, SDP_LINE_FILTER_SCALE='1e18')


# ---- the shop model of tests/test_gpu_line.py and how its tests run and compare sweeps
def shop(n_x=600, n_u=257, n_w=16, dyn=None, cost=None, box=None, grid=(-8., 24.), wgrid=(0., 4.), law=None, steps=None):
    sysd = SysDescription((1, 1, 1), name='shop')
    sysd.dyn = dyn or (lambda x, u, w: (x + u - w,))
    sysd.cost = cost or (lambda x, u, w: np.where(x > 0, x * 0.5, -x * 3.) + u * 1.)
    sysd.control_box = box or (lambda x: ((0., 8.),))
    sysd.perturb_laws = [law or models.NormalLaw(2.0, 0.8)]
    s = DPSolver(sysd)
    s.discretize_state(grid[0], grid[1], n_x)
    s.discretize_perturb(wgrid[0], wgrid[1], n_w)
    s.control_steps = steps or (8. / (n_u - 1),)
    return s


def two_orders(n_x, steps, grid=(-8., 24.), n_w=9):
    """two controls (SDP_NU = 2: sdp_line_pass1 is never PLAIN)"""
    sysd = SysDescription((1, 2, 1), name='two orders')
    sysd.dyn = lambda x, u, v, w: (x + (u + 0.5 * v) - w,)
    sysd.cost = lambda x, u, v, w: np.where(x > 0, x * 0.5, -x * 3.) + u * 1. + v * 0.45 + 0.01 * v * v
    sysd.control_box = lambda x: ((0., 4.), (0., 6.))
    sysd.perturb_laws = [models.NormalLaw(2.0, 0.8)]
    s = DPSolver(sysd)
    s.discretize_state(grid[0], grid[1], n_x)
    s.discretize_perturb(0., 4., n_w)
    s.control_steps = steps
    return s


def chain(make, kernel, V0, sweeps=3, debug=None):
    s = make()
    s.kernel = kernel
    s.debug_defines = debug
    out, V = [], V0
    with np.errstate(all='ignore'):
        for _ in range(sweeps):
            J, pol = s.value_iteration(V, report_time=False)
            out.append((J.copy(), pol.copy(), s.last_policy_index.copy()))
            V = J
    return out, s.backend_info


def same(a, b):
    return all(np.array_equal(x[0], y[0], equal_nan=True) and np.array_equal(x[1], y[1], equal_nan=True) and np.array_equal(x[2], y[2])
               for x, y in zip(a, b))


V_OF = {
    'zeros': lambda x, rng: np.zeros_like(x),
    'smooth': lambda x, rng: 0.3 * (x - 3) ** 2 + np.sin(x),
    'random': lambda x, rng: rng.standard_normal(x.size),
    'kinked': lambda x, rng: np.abs(x - 1.3) * 2 + np.maximum(x - 7, 0) ** 2,
}

# the input value arrays of every case: the four above; 'flat', the near-tie construction of
# test_flat_objective_near_ties (tests/test_gpu_line.py) -- a cost-to-go linear in the stock with the opposite slope of
# the cost in the control, so that every control of a node gives the same value up to rounding --; and 'special', a
# smooth array with NaN, +inf and -inf entries (the first pass's steepest step is then infinite: every node is bad)
INPUTS = ('zeros', 'smooth', 'random', 'kinked', 'flat', 'special')


def lane_formula(S, max_u, W):
    """(need, want) of DPSolver._kernel_plan, restated (the plan test holds min(64, max(need, want)) against the plan)"""
    pow2 = lambda v: 1 << max(int(np.ceil(np.log2(max(v, 1)))), 0)
    need = pow2(W * 64 / 2048.)
    want = min(pow2(131072. / S), max(1 << int(np.floor(np.log2(max(max_u / 32., 1)))), 1))
    return need, want


class Case(object):
    """n_x nodes x n_u controls x n_w perturbation points of `model` ('shop': keywords `kw` of shop(); 'two orders':
    n_u = (points of u, points of v)).  Claims: `lanes`; `by`, the branch of the lane formula that decided ('need' /
    'want': the larger one; 'floor': both give 1); `chain` (SDP_LINE_CHAIN); `pow2` (the span of the axis is a power of
    two); `usable` (False: the shifts need more than 2 S + 64 rows, the kernel's c.ok fails and every node is bad);
    `collapsed` (nodes whose control box collapses to one point); `slope`: the slope of the cost in the control, which
    the 'flat' input takes the other way; `tie`: the node value at which the 'tied pair' input has its kink (below)"""
    def __init__(self, name, n_x, n_u, n_w, lanes, by, chain=0, pow2=True, usable=True, collapsed=0, model='shop',
                 slope=1.0, tie=None, **kw):
        self.name, self.n_x, self.n_u, self.n_w = name, int(n_x), n_u, int(n_w)
        self.lanes, self.by, self.chain, self.pow2, self.usable = int(lanes), by, int(chain), bool(pow2), bool(usable)
        self.collapsed, self.model, self.slope, self.tie, self.kw = int(collapsed), model, float(slope), tie, kw

    def __repr__(self):
        return self.name

    @property
    def input_names(self):
        return INPUTS + (('tied pair',) if self.tie is not None else ())

    @property
    def controls(self):
        return int(np.prod(self.n_u))

    @property
    def cells(self):
        return self.n_x * self.controls * self.n_w

    @property
    def npw(self):
        return 64 // self.lanes

    @property
    def tiles(self):
        return -(-self.n_x // self.npw)

    def solver(self, kernel='line', debug=None):
        if self.model == 'two orders':
            s = two_orders(self.n_x, (4. / (self.n_u[0] - 1), 6. / (self.n_u[1] - 1)), n_w=self.n_w, **self.kw)
        else:
            s = shop(self.n_x, self.n_u, self.n_w, **self.kw)
        s.kernel = kernel
        s.debug_defines = debug
        return s

    def inputs(self):
        """{name: V0} on the case's own axis (seeded by the shape: the same arrays in every process)"""
        x = np.asarray(self.solver().state_grid[0], dtype=float)
        n = x.size
        rng = np.random.default_rng(1000 * self.lanes + n)
        out = {k: np.asarray(V_OF[k](x, rng), dtype=float) for k in ('zeros', 'smooth', 'random', 'kinked')}
        out['flat'] = -self.slope * x
        V = out['smooth'].copy()
        V[n // 3], V[0], V[n - 1] = np.nan, np.inf, -np.inf
        if n >= 16:
            V[n // 2:n // 2 + 2] = np.nan
            V[(2 * n) // 3] = np.inf
        out['special'] = V
        if self.tie is not None:
            out['tied pair'] = 3. * np.maximum(self.tie - x, 0.) + np.maximum(x - self.tie, 0.)
        return out

    def sample_nodes(self):
        """the nodes compared with the oracle: all of them up to 2e6 cells per sweep; beyond that node 0, the last
        node, both sides of every boundary of the first and the last tile and of the eight shares of the tile walk
        (sdp_sweep: per_xcd tiles each), and a few seeded ones"""
        n, npw = self.n_x, self.npw
        if self.cells <= 2e6:
            return np.arange(n)
        per = -(-self.tiles // 8)
        last = (self.tiles - 1) * npw
        picked = {0, n - 1, npw - 1, npw, last - 1, last}
        for share in range(1, 8):
            picked.update((share * per * npw - 1, share * per * npw))
        picked.update(np.random.default_rng(n).integers(0, n, size=8).tolist())
        return np.array(sorted(p for p in picked if 0 <= p < n), dtype=np.int64)


def macro(source, name):
    """value of `#define name value` in a generated source, or None"""
    m = re.search(r'^#define {} (\S+)'.format(re.escape(name)), source, re.M)
    return m.group(1) if m else None


def planned(source):
    """(lanes, SDP_LINE_W, SDP_LINE_CHAIN) of a generated source; None where it is not the line kernel's"""
    if '#define SDP_LINE 1' not in source:
        return None
    return tuple(int(macro(source, k)) for k in ('SDP_LANES', 'SDP_LINE_W', 'SDP_LINE_CHAIN'))


def lattice_usable(s):
    """c.ok of sdp_line_setup for the shop's `x + u - w` family, restated: the whole shifts of the perturbation points
    (b = -w and its regroupings; floor(b / span (n - 1))) leave a lattice of at most 2 S + 64 rows"""
    g = np.asarray(s.state_grid[0], dtype=float)
    n = g.size
    q = np.floor(-np.asarray(s.perturb_grid[0], dtype=float) / (g[-1] - g[0]) * (n - 1))
    rows = n + int(q.max()) + int((-q).max()) + 1
    return n >= 3 and 2 <= rows <= 2 * n + 64


def control_counts(s):
    """controls of every node, from the box plan (what the long way of a bad node must visit exactly once)"""
    bp = s._box_plan(None)
    per = np.prod(np.asarray(bp['n'], dtype=np.int64), axis=0).ravel()
    return per if per.size == s._state_grid_shape[0] else np.full(s._state_grid_shape[0], int(per[0]), dtype=np.int64)


# a per-node box: the first and the last node (x = -8: [8, 8]; x = 24: [0, 0]) collapse to one control point -- a
# wave that holds one of them next to ordinary nodes fails __all(plain) and takes the general first pass
def _box_pow2(x):
    return ((np.max((0., -x)), np.min((8., 24. - x))),)


# (on the axis [-3, 6]: only the last node, x = 6, collapses)
def _box_odd(x):
    return ((0., np.min((8., 6. - x))),)


# the shapes at which the forms below run: lanes 1 (want's floor), 32 and 64 (want, on few nodes)
_AT = {1: (200, 33), 32: (130, 1025), 64: (65, 2049)}

CASES = [
    # ---- the shapes: every lane count, both branches of the formula, the ends of W, few tiles, a ragged tile
    Case('40x17x1', 40, 17, 1, 1, 'floor'),                               # W = 1; one tile of 64 with 40 nodes
    Case('200x2x9', 200, 2, 9, 1, 'floor'),                               # two controls: only `stop` outside the main loop
    Case('5000x33x5', 5000, 33, 5, 1, 'floor'),                           # NPW = 64, 5000 = 78 x 64 + 8: a ragged last tile
    Case('300x65x64', 300, 65, 64, 2, 'both'),                            # need = want = 2
    Case('300x65x65', 300, 65, 65, 4, 'need'),                            # W just past 64
    Case('130x33x128', 130, 33, 128, 4, 'need'),
    Case('600x257x16', 600, 257, 16, 8, 'want'),
    Case('3000x513x32', 3000, 513, 32, 16, 'want'),
    Case('70x33x1024', 70, 33, 1024, 32, 'need'),                         # 128 slices share 33 controls: most are empty
    Case('4000x1025x9', 4000, 1025, 9, 32, 'want'),
    Case('2000x2049x9', 2000, 2049, 9, 64, 'want'),
    Case('65x2049x64', 65, 2049, 64, 64, 'want'),                         # (need = 2)
    Case('7x8001x5', 7, 8001, 5, 64, 'want'),                             # 7 tiles: an empty share of the tile walk
]
for _l, (_n, _u) in sorted(_AT.items()):
    _by = 'floor' if _l == 1 else 'want'
    _t = '@{}'.format(_l)
    CASES += [
        # ---- a regrouped chain of sums (SDP_LINE_CHAIN 2), and two perturbation terms in the final-sum form (0)
        Case('x+(-w+u)' + _t, _n, _u, 9, _l, _by, chain=2, dyn=lambda x, u, w: (x + (-w + u),)),
        Case('(x-w)+u' + _t, _n, _u, 9, _l, _by, chain=2, dyn=lambda x, u, w: ((x - w) + u,)),
        Case('two terms' + _t, _n, _u, 9, _l, _by, dyn=lambda x, u, w: (x + u - 0.5 * w - 0.25 * w * w,)),
        # ---- a span that is no power of two (sdp_line_pass1<.., 0>), with an ordinary and with a per-node box
        Case('span 9' + _t, _n, _u, 9, _l, _by, pow2=False, grid=(-3., 6.)),
        Case('node box' + _t, _n, _u, 9, _l, _by, collapsed=2, box=_box_pow2),
        Case('node box span 9' + _t, _n, _u, 9, _l, _by, pow2=False, collapsed=1, grid=(-3., 6.), box=_box_odd),
        # ---- a stock that leaves the grid on both sides
        Case('leaves the grid' + _t, _n, _u, 9, _l, _by, grid=(0., 4.), box=lambda x: ((-6., 6.),), steps=(12. / (_u - 1),)),
        # ---- shifts of more rows than 2 S + 64: the lattice is not usable, every node is bad
        Case('wide shifts' + _t, _n, _u, 12, _l, _by, usable=False, wgrid=(-64., 96.)),
        # ---- three rows: the shortest axis the lattice takes
        Case('three rows' + _t, 3, _u, 9, _l, _by),
        # ---- the flat objective of test_flat_objective_near_ties: every control of a node ties up to rounding
        Case('flat cost' + _t, _n, _u, 5, _l, _by, slope=2.0, cost=lambda x, u, w: u * 2.0 + 0. * x,
             box=lambda x: ((0., 4.),), steps=(4. / (_u - 1),), wgrid=(0., 2.)),
    ]
# ---- two controls (SDP_NU = 2, never PLAIN): 5 x 5, 33 x 33 and 49 x 49 points
CASES += [
    Case('two controls@1', 200, (5, 5), 9, 1, 'floor', model='two orders'),
    Case('two controls@32', 130, (33, 33), 9, 32, 'want', model='two orders'),
    Case('two controls@64', 65, (49, 49), 9, 64, 'want', model='two orders'),
]

# ---- two survivors at the SECOND level.  One perturbation point w, rows h apart, controls du = h / 4 apart, w = du / 2,
# everything a small multiple of a power of two (no rounding anywhere); the 'tied pair' input is piecewise linear with
# slopes -3 and +1 around a kink at the node `tie`.  With the cost's slope 1 in the control, the two controls whose next
# stocks lie du / 2 on either side of the kink give the same value exactly, their neighbours one that is du / 2 ... larger.
# The shift of w is an eighth of a row, so the chord bound of the cell that holds the kink (7 / 64 of the kink's second
# difference, 4 h) covers three of the cell's four controls at the first level; the second level, which has no chord,
# keeps exactly the two that tie.  At every node from which the controls reach the kink.
CASES += [
    Case('tied pair@1', 129, 49, 1, 1, 'floor', tie=4., box=lambda x: ((0., 3.),), steps=(1. / 16,), wgrid=(1. / 32, 1.)),
    Case('tied pair@32', 1025, 1025, 1, 32, 'want', tie=4., steps=(1. / 128,), wgrid=(1. / 256, 1.)),
    Case('tied pair@64', 513, 2049, 1, 64, 'want', tie=6., grid=(0., 8.), steps=(1. / 256,), wgrid=(1. / 512, 1.)),
]

BY_NAME = {c.name: c for c in CASES}


def runs_wide(case):
    """whether the case also runs under DIAG_WIDE: the lane counts whose merges had no test before this table"""
    return case.lanes >= 32


def unit_sources(case):
    """{what: generated source} of every unit tests/test_gpu_line_forms.py runs for the case"""
    out = {'line': case.solver()._kernel_plan()['source'],
           'generic': case.solver('generic')._kernel_plan()['source'],
           'diag': case.solver(debug=DIAG)._kernel_plan()['source']}
    if runs_wide(case):
        out['diag wide'] = case.solver(debug=DIAG_WIDE)._kernel_plan()['source']
    return out

# ---- which counters each case makes non-zero in one SDP_LINE_DIAG sweep from each input: {case: {input: counters}}.
# Read off an MI355X (the counters exist only on the device); tests/test_gpu_line_forms.py asserts every one of them.
# (A counter is claimed where it counted at least three times or for a tenth of the nodes: a path that one node of
# thousands happens to take is no coverage anyone planned.)
PATHS = {
    '40x17x1': {'zeros': 'single1', 'smooth': 'single1', 'random': 'single1', 'kinked': 'single1',
        'flat': 'undecided1,left2,evals2,long way', 'special': 'bad,long way'},
    '200x2x9': {'zeros': 'single1', 'smooth': 'single1', 'random': 'single1,pair1', 'kinked': 'single1',
        'flat': 'pair1', 'special': 'bad,long way'},
    '5000x33x5': {'zeros': 'single1', 'smooth': 'single1', 'random': 'single1,pair1,undecided1,single2,evals2',
        'kinked': 'single1,pair1', 'flat': 'undecided1,left2,evals2,long way', 'special': 'bad,long way'},
    '300x65x64': {'zeros': 'single1', 'smooth': 'single1,pair1', 'random': 'single1,pair1,undecided1,single2,evals2',
        'kinked': 'single1,pair1', 'flat': 'undecided1,left2,evals2,long way', 'special': 'bad,long way'},
    '300x65x65': {'zeros': 'single1', 'smooth': 'single1,pair1', 'random': 'single1,pair1,undecided1,single2,evals2',
        'kinked': 'single1,pair1', 'flat': 'undecided1,left2,evals2,long way', 'special': 'bad,long way'},
    '130x33x128': {'zeros': 'single1', 'smooth': 'single1,pair1',
        'random': 'single1,pair1,undecided1,single2,evals2', 'kinked': 'single1,pair1',
        'flat': 'undecided1,left2,evals2,long way', 'special': 'bad,long way'},
    '600x257x16': {'zeros': 'single1', 'smooth': 'single1,pair1,undecided1,single2,evals2',
        'random': 'single1,pair1,undecided1,single2,evals2', 'kinked': 'single1,pair1,undecided1,single2,evals2',
        'flat': 'undecided1,left2,evals2,long way', 'special': 'bad,long way'},
    '3000x513x32': {'zeros': 'single1', 'smooth': 'single1,pair1', 'random': 'undecided1,single2,evals2',
        'kinked': 'single1,pair1', 'flat': 'undecided1,left2,evals2,long way', 'special': 'bad,long way'},
    '70x33x1024': {'zeros': 'single1', 'smooth': 'single1,undecided1,single2,evals2',
        'random': 'single1,pair1,undecided1,single2,evals2', 'kinked': 'single1,pair1,undecided1,single2,evals2',
        'flat': 'undecided1,left2,evals2,long way', 'special': 'bad,long way'},
    '4000x1025x9': {'zeros': 'single1', 'smooth': 'single1,pair1',
        'random': 'single1,pair1,undecided1,single2,evals2', 'kinked': 'single1,pair1,undecided1,single2,evals2',
        'flat': 'undecided1,left2,evals2,long way', 'special': 'bad,long way'},
    '2000x2049x9': {'zeros': 'single1', 'smooth': 'single1,undecided1,single2,evals2',
        'random': 'single1,pair1,undecided1,single2,evals2', 'kinked': 'single1,undecided1,single2,evals2',
        'flat': 'undecided1,left2,evals2,long way', 'special': 'bad,long way'},
    '65x2049x64': {'zeros': 'single1', 'smooth': 'single1,pair1,undecided1,single2,evals2',
        'random': 'undecided1,single2,evals2', 'kinked': 'single1,pair1,undecided1,single2,evals2',
        'flat': 'undecided1,left2,evals2,long way', 'special': 'bad,long way'},
    '7x8001x5': {'zeros': 'single1', 'smooth': 'single1,undecided1,single2,evals2',
        'random': 'single1,undecided1,single2,evals2', 'kinked': 'single1,undecided1,single2,evals2',
        'flat': 'undecided1,left2,evals2,long way', 'special': 'bad,long way'},
    'x+(-w+u)@1': {'zeros': 'single1', 'smooth': 'single1,pair1',
        'random': 'single1,pair1,undecided1,single2,evals2', 'kinked': 'single1,pair1',
        'flat': 'undecided1,left2,evals2,long way', 'special': 'bad,long way'},
    '(x-w)+u@1': {'zeros': 'single1', 'smooth': 'single1,pair1', 'random': 'single1,pair1,undecided1,single2,evals2',
        'kinked': 'single1,pair1', 'flat': 'undecided1,left2,evals2,long way', 'special': 'bad,long way'},
    'two terms@1': {'zeros': 'single1', 'smooth': 'single1,pair1,undecided1,single2,evals2',
        'random': 'single1,pair1,undecided1,single2,evals2', 'kinked': 'single1,pair1',
        'flat': 'undecided1,left2,evals2,long way', 'special': 'bad,long way'},
    'span 9@1': {'zeros': 'single1', 'smooth': 'single1,pair1', 'random': 'single1,pair1,undecided1,single2,evals2',
        'kinked': 'single1', 'flat': 'undecided1,left2,evals2,long way', 'special': 'bad,long way'},
    'node box@1': {'zeros': 'single1', 'smooth': 'single1,pair1',
        'random': 'single1,pair1,undecided1,single2,evals2', 'kinked': 'single1,pair1',
        'flat': 'undecided1,left2,evals2,long way', 'special': 'bad,long way'},
    'node box span 9@1': {'zeros': 'single1', 'smooth': 'single1,pair1',
        'random': 'single1,pair1,undecided1,single2,evals2', 'kinked': 'single1',
        'flat': 'pair1,undecided1,left2,evals2,long way', 'special': 'bad,long way'},
    'leaves the grid@1': {'zeros': 'single1', 'smooth': 'single1', 'random': 'single1', 'kinked': 'single1',
        'flat': 'undecided1,left2,evals2,long way', 'special': 'bad,long way'},
    'wide shifts@1': {'zeros': 'bad,long way', 'smooth': 'bad,long way', 'random': 'bad,long way',
        'kinked': 'bad,long way', 'flat': 'bad,long way', 'special': 'bad,long way'},
    'three rows@1': {'zeros': 'single1', 'smooth': 'single1,undecided1,single2,evals2',
        'random': 'single1,undecided1,single2,evals2', 'kinked': 'single1,undecided1,single2,evals2',
        'flat': 'undecided1,left2,evals2,long way', 'special': 'bad,long way'},
    'flat cost@1': {'zeros': 'single1', 'smooth': 'single1,pair1,undecided1,single2,evals2',
        'random': 'single1,pair1,undecided1,single2,evals2', 'kinked': 'single1,undecided1,left2,evals2,long way',
        'flat': 'undecided1,left2,evals2,long way', 'special': 'bad,long way'},
    'x+(-w+u)@32': {'zeros': 'single1', 'smooth': 'single1,pair1,undecided1,single2,evals2',
        'random': 'undecided1,single2,evals2', 'kinked': 'single1,pair1,undecided1,single2,evals2',
        'flat': 'undecided1,left2,evals2,long way', 'special': 'bad,long way'},
    '(x-w)+u@32': {'zeros': 'single1', 'smooth': 'single1,pair1,undecided1,single2,evals2',
        'random': 'undecided1,single2,evals2', 'kinked': 'single1,pair1,undecided1,single2,evals2',
        'flat': 'undecided1,left2,evals2,long way', 'special': 'bad,long way'},
    'two terms@32': {'zeros': 'single1', 'smooth': 'single1,pair1,undecided1,single2,evals2',
        'random': 'undecided1,single2,evals2', 'kinked': 'single1,pair1,undecided1,single2,evals2',
        'flat': 'undecided1,left2,evals2,long way', 'special': 'bad,long way'},
    'span 9@32': {'zeros': 'single1', 'smooth': 'single1,undecided1,single2,evals2',
        'random': 'undecided1,single2,evals2', 'kinked': 'single1,pair1,undecided1,single2,evals2',
        'flat': 'undecided1,left2,evals2,long way', 'special': 'bad,long way'},
    'node box@32': {'zeros': 'single1', 'smooth': 'single1,pair1,undecided1,single2,evals2',
        'random': 'undecided1,single2,evals2', 'kinked': 'single1,pair1,undecided1,single2,evals2',
        'flat': 'undecided1,left2,evals2,long way', 'special': 'bad,long way'},
    'node box span 9@32': {'zeros': 'single1', 'smooth': 'single1,undecided1,single2,evals2',
        'random': 'undecided1,single2,evals2', 'kinked': 'single1,pair1,undecided1,single2,evals2',
        'flat': 'undecided1,left2,evals2,long way', 'special': 'bad,long way'},
    'leaves the grid@32': {'zeros': 'single1', 'smooth': 'single1', 'random': 'undecided1,single2,evals2',
        'kinked': 'undecided1,single2,evals2', 'flat': 'undecided1,left2,evals2,long way', 'special': 'bad,long way'},
    'wide shifts@32': {'zeros': 'bad,long way', 'smooth': 'bad,long way', 'random': 'bad,long way',
        'kinked': 'bad,long way', 'flat': 'bad,long way', 'special': 'bad,long way'},
    'three rows@32': {'zeros': 'single1', 'smooth': 'single1,undecided1,single2,evals2', 'random': 'single1',
        'kinked': 'single1,undecided1,single2,evals2', 'flat': 'undecided1,left2,evals2,long way',
        'special': 'bad,long way'},
    'flat cost@32': {'zeros': 'single1', 'smooth': 'single1,pair1,undecided1,single2,evals2',
        'random': 'undecided1,single2,evals2', 'kinked': 'single1,pair1,undecided1,left2,evals2,long way',
        'flat': 'undecided1,left2,evals2,long way', 'special': 'bad,long way'},
    'x+(-w+u)@64': {'zeros': 'single1', 'smooth': 'single1', 'random': 'single1', 'kinked': 'single1',
        'flat': 'undecided1,left2,evals2,long way', 'special': 'bad,long way'},
    '(x-w)+u@64': {'zeros': 'single1', 'smooth': 'single1', 'random': 'single1', 'kinked': 'single1',
        'flat': 'undecided1,left2,evals2,long way', 'special': 'bad,long way'},
    'two terms@64': {'zeros': 'single1', 'smooth': 'pair1,undecided1,single2,evals2',
        'random': 'undecided1,single2,evals2', 'kinked': 'single1,pair1,undecided1,single2,evals2',
        'flat': 'undecided1,left2,evals2,long way', 'special': 'bad,long way'},
    'span 9@64': {'zeros': 'single1', 'smooth': 'undecided1,single2,evals2',
        'random': 'single1,pair1,undecided1,single2,evals2', 'kinked': 'single1,undecided1,single2,evals2',
        'flat': 'undecided1,left2,evals2,long way', 'special': 'bad,long way'},
    'node box@64': {'zeros': 'single1', 'smooth': 'single1', 'random': 'single1', 'kinked': 'single1',
        'flat': 'undecided1,left2,evals2,long way', 'special': 'bad,long way'},
    'node box span 9@64': {'zeros': 'single1', 'smooth': 'undecided1,single2,evals2',
        'random': 'single1,pair1,undecided1,single2,evals2', 'kinked': 'single1,undecided1,single2,evals2',
        'flat': 'undecided1,left2,evals2,long way', 'special': 'bad,long way'},
    'leaves the grid@64': {'zeros': 'single1', 'smooth': 'single1', 'random': 'single1', 'kinked': 'single1',
        'flat': 'undecided1,left2,evals2,long way', 'special': 'bad,long way'},
    'wide shifts@64': {'zeros': 'bad,long way', 'smooth': 'bad,long way', 'random': 'bad,long way',
        'kinked': 'bad,long way', 'flat': 'bad,long way', 'special': 'bad,long way'},
    'three rows@64': {'zeros': 'single1', 'smooth': 'single1,undecided1,single2,evals2',
        'random': 'single1,undecided1,single2,evals2', 'kinked': 'single1,undecided1,single2,evals2',
        'flat': 'undecided1,left2,evals2,long way', 'special': 'bad,long way'},
    'flat cost@64': {'zeros': 'single1', 'smooth': 'single1', 'random': 'single1',
        'kinked': 'single1,undecided1,left2,evals2,long way', 'flat': 'undecided1,left2,evals2,long way',
        'special': 'bad,long way'},
    'two controls@1': {'zeros': 'single1', 'smooth': 'single1,pair1',
        'random': 'single1,pair1,undecided1,single2,evals2', 'kinked': 'single1,pair1,evals2',
        'flat': 'undecided1,left2,evals2,long way', 'special': 'bad,long way'},
    'two controls@32': {'zeros': 'single1', 'smooth': 'single1,pair1,undecided1,single2,evals2',
        'random': 'single1,pair1,undecided1,single2,evals2', 'kinked': 'single1,undecided1,single2,evals2',
        'flat': 'undecided1,left2,evals2,long way', 'special': 'bad,long way'},
    'two controls@64': {'zeros': 'single1', 'smooth': 'single1', 'random': 'single1', 'kinked': 'single1',
        'flat': 'undecided1,left2,evals2,long way', 'special': 'bad,long way'},
    'tied pair@1': {'zeros': 'single1', 'smooth': 'single1,undecided1,single2,evals2',
        'random': 'single1,pair1,undecided1,single2,evals2', 'kinked': 'single1,undecided1,single2,evals2',
        'flat': 'undecided1,left2,evals2,long way', 'special': 'bad,long way',
        'tied pair': 'single1,undecided1,pair2,evals2'},
    'tied pair@32': {'zeros': 'single1', 'smooth': 'single1,undecided1,single2,evals2',
        'random': 'single1,pair1,undecided1,single2,evals2', 'kinked': 'single1,undecided1,single2,evals2',
        'flat': 'undecided1,left2,evals2,long way', 'special': 'bad,long way',
        'tied pair': 'single1,undecided1,pair2,evals2'},
    'tied pair@64': {'zeros': 'single1', 'smooth': 'single1,undecided1,single2,evals2',
        'random': 'single1,undecided1,single2,evals2', 'kinked': 'single1,undecided1,single2,evals2',
        'flat': 'undecided1,left2,evals2,long way', 'special': 'bad,long way',
        'tied pair': 'single1,undecided1,pair2,evals2'},
}

# counters that no case reaches at some lane count, with the reason: {counter: {lanes: why}}
UNREACHED = {}


def claimed(case, vname):
    return tuple(k for k in PATHS.get(case.name, {}).get(vname, '').split(',') if k)
