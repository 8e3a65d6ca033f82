"""The unit sizes of the column kernel with a ROW WINDOW (codegen.column_window_unit; phase B of
csrc/sdp_colfull_kernel.h, the window itself in csrc/sdp_column_kernel.h) as a table of cases (test infrastructure,
like tests/percontrol_forms.py, from which it takes the split rule, the inputs and the node sample; not a test file,
and no GPU code).

The unit is compiled per (rows of axis 0, W, real type, rows a node's controls span): SDP_COL_ROWS rows of table and
segments of `seg_nodes` nodes.  What phase B does with a unit is decided at run time, by the rows column_grid
(csrc/sdp_hip.hip) gives it: the 64-node groups of a unit are dealt to the 8 waves; with fewer groups than waves the
control lattice is cut into `chunks = waves // groups` ranges whose partial minima meet in LDS; with more groups than
waves the item loop makes a second trip.  Every run of the suite before this table had 9 to 120 columns, hence units of
64 to 227 rows: chunks of 8, 4 and 2, never 1, never a second trip, never a unit of the planned segment length, never
an empty chunk on purpose, and every input was white noise, on which a tie never happens.

A case is a model (`long_lead`: the benchmark model on a long leading axis, table built in order (2, 64); `storage`:
per-node boxes and a perturbed stock, table built round-robin -- both from tests/test_gpu_window.py), the real type,
the macros its unit must define and per geometry what its units must look like on the device (`units`: {geometry:
{rows: (groups, chunks, second trip)}}).  Geometries, sized from the compute units of the chip:

  'many'    at least 4 * cus columns in one launch (DPSolver.host_overlap off, see percontrol_forms.launch_columns):
            units of the planned segment length, or the nearest equal parts below it
  'few'     9 columns: columns are split down to units of 64 to 127 rows
  'some'    the 12 x 10 (or 7 x 9) columns of tests/test_gpu_window.py

tests/test_window_forms_plan.py and tests/test_gpu_window_forms.py are to this table what
tests/test_percontrol_forms_plan.py and tests/test_gpu_percontrol_forms.py are to the other."""
import numpy as np

from stodynprog_amd import models, SysDescription, DPSolver
from stodynprog_amd.models import NormalLaw

from percontrol_forms import (CUS, INPUTS, splits, unit_bounds, unit_rows, launch_columns, sweep_bounds, inputs,   # noqa: F401
                              sample_nodes, macro, missing_claims)

WAVES = 8                      # of the 512 threads of a row-window unit


def phase_b(rows, waves=WAVES):
    """(groups, chunks, second trip) of a unit of `rows` nodes: phase B of csrc/sdp_colfull_kernel.h"""
    groups = (rows + 63) >> 6
    chunks = waves // groups if groups < waves else 1
    return groups, chunks, groups * chunks > waves


def chunk_range(total, chunk, chunks):
    """[c_lo, c_hi) of the controls of one chunk of a lattice of `total` controls"""
    return total * chunk // chunks, total * (chunk + 1) // chunks


def long_lead(N0, dtype=np.float64):
    def make(trailing):
        _, s = models.synthetic3d(N=16)
        s.dtype = np.dtype(dtype)
        s.discretize_state(0, 1, N0, 0, 1, trailing[0], 0, 1, trailing[1])
        return s
    return make


def storage(n_E, n_w=11, p_max=0.35, step=0.05):
    def make(trailing):
        sysd = SysDescription((2, 1, 1), name='long storage')
        sysd.dyn = lambda E, P, u, w: (E + u - 0.05 * abs(u) + 0.02 * w, 0.8 * P + w)
        sysd.cost = lambda E, P, u, w: (P - u) ** 2 + 0.01 * E
        sysd.control_box = lambda E, P: ((np.max((-E, -p_max)), np.min((10 - E, p_max))),)
        sysd.perturb_laws = [NormalLaw(0, 0.5)]
        s = DPSolver(sysd)
        s.discretize_state(0, 10, n_E, -2, 2, trailing[0])
        s.discretize_perturb(-1.5, 1.5, n_w)
        s.control_steps = (step,)
        return s
    return make


_LINE = {'many': lambda cus: (4 * cus,), 'few': lambda cus: (9,)}
_PLANE = {'many': lambda cus: (32 * -(-cus // 256), 32), 'some': lambda cus: (12, 10)}
_RAGGED = {'some': lambda cus: (7, 9)}


class Case(object):
    """name; make(trailing axes) -> solver; n0; dtype; claims {macro: value or None}; seg_nodes; order: the table
    build ('order 2' / 'round robin'); units {geometry: {rows: (groups, chunks, second trip)}}; reach: None, or what
    DPSolver._lead_reach_rows answers for the case's solvers (a window planned narrower than the controls need)"""

    def __init__(self, name, make, n0, claims, seg_nodes, order, units, dtype=np.float64, trailing=_LINE, reach=None):
        self.name, self.make, self.n0, self.seg_nodes, self.order, self.reach = name, make, int(n0), int(seg_nodes), order, reach
        self.dtype, self.claims, self.trailing = np.dtype(dtype), dict(claims), dict(trailing)
        self.units = {g: dict(u) for g, u in units.items()}
        self.geometries = tuple(g for g in ('many', 'few', 'some') if g in self.units)
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
        if self.reach is not None:
            reach = int(self.reach)
            s._lead_reach_rows = lambda model, bp, box_t=None, **kw: reach
        return s


def _unit(n0, W, rows, order2, lead_w):
    return {'SDP_TRAIL_HAS_U': '0', 'SDP_COL_N0': str(n0), 'SDP_COL_W': str(W), 'SDP_COL_THREADS': '512',
            'SDP_COL_ROWS': str(rows), 'SDP_COL_A_ORDER': '2' if order2 else None, 'SDP_LEAD_HAS_W': str(lead_w),
            'SDP_COL_FILTER': None, 'SDP_COL_WCHUNK': None, 'SDP_COL_WPAIR': '0'}


def _st(name, n_E, n_w, rows, seg, units, **kw):
    reach = kw.pop('reach', None)
    return Case(name, storage(n_E, n_w, **kw), n_E, _unit(n_E, n_w, rows, False, 1), seg, 'round robin', units, reach=reach)


CASES = [
    # ---- per-node boxes, a perturbed stock, the table dealt round-robin
    _st('storage_2048', 2048, 11, 832, 640, {'many': {512: (8, 1, False)}, 'few': {64: (1, 8, False)}}),
    _st('storage_1900_two_trips', 1900, 11, 832, 640, {'many': {633: (10, 1, True), 634: (10, 1, True)}}),
    _st('storage_1900_w33_seg64', 1900, 33, 256, 64, {'few': {63: (1, 8, False), 64: (1, 8, False)}}),
    _st('storage_1100_w33_seg128', 1100, 33, 256, 128, {'many': {122: (2, 4, False), 123: (2, 4, False)}}),
    # (boxes of 3 to 5 controls: with 8 chunks some are empty -- the first one too --, and no chunk has a whole pair)
    _st('storage_2048_coarse_controls', 2048, 11, 832, 640,
        {'many': {512: (8, 1, False)}, 'few': {64: (1, 8, False)}}, step=0.2),
    # (a reach of 287 rows planned as 1: segments as long as the window, controls outside it are recomputed)
    _st('storage_2048_narrow_window', 2048, 11, 832, 768, {'many': {682: (11, 1, True), 683: (11, 1, True)}},
        p_max=0.7, reach=1),
    # ---- the benchmark model on a long leading axis, the table built in order (2, 64)
    Case('long_lead_1024', long_lead(1024), 1024, _unit(1024, 32, 288, True, 0), 192, 'order 2',
         {'many': {170: (3, 2, False), 171: (3, 2, False)}, 'some': {113: (2, 4, False), 114: (2, 4, False)}},
         trailing=_PLANE),
    Case('long_lead_2048_f32', long_lead(2048, np.float32), 2048, _unit(2048, 32, 576, True, 0), 384, 'order 2',
         {'many': {341: (6, 1, False), 342: (6, 1, False)}}, dtype=np.float32, trailing=_PLANE),
    Case('long_lead_1000_ragged', long_lead(1000), 1000, _unit(1000, 32, 288, True, 0), 192, 'order 2',
         {'some': {66: (2, 4, False), 67: (2, 4, False)}}, trailing=_RAGGED),
]
BY_NAME = {c.name: c for c in CASES}
PAIRS = [(c, g) for c in CASES for g in c.geometries]
RUNS = [(c, g, v) for c, g in PAIRS for v in INPUTS]


def box_sizes(solver):
    """controls per node of the solver's box table, on the grid's shape"""
    plan = solver._kernel_plan()
    assert plan['per_node']
    return np.prod(plan['n'].astype(np.int64), axis=0).reshape(solver._shape())


def empty_chunks(case, geometry, cus=CUS):
    """(node, chunk) pairs of the case at `geometry` whose chunk of the control lattice is empty"""
    s = case.solver(geometry, cus=cus)
    total = box_sizes(s)
    count = 0
    for lo, hi in sweep_bounds(s, cus, case.seg_nodes):
        _, chunks, _ = phase_b(hi - lo)
        t = total[lo:hi]
        for chunk in range(chunks):
            count += int((t * chunk // chunks == t * (chunk + 1) // chunks).sum())
    return count


def unit_sources(case, cus=CUS):
    """{what: generated source} of every unit tests/test_gpu_window_forms.py runs for the case on a chip of `cus`
    compute units: the row window and the direct kernel, per geometry"""
    out = {}
    for g in case.geometries:
        for kernel in ('column', 'generic'):
            out['{}, {}'.format(g, kernel)] = case.solver(g, kernel, cus)._kernel_plan()['source']
    return out
