"""The cases of tests/test_gpu_fp32_oracle.py as a table (test infrastructure, like tests/column_forms.py; not a
test file): problems in 4-byte reals, each with the kernels it runs in and the family each of them must plan.

Every other 4-byte test of the suite compares the project with itself (another kernel of the same headers) or with the
8-byte oracle under a max-norm bar.  Here the yardstick is oracle/vi_numpy.value_iteration(.., dtype=np.float32): the
direct kernel's definition restated in numpy float32, operation by operation.  The cases sit where 4-byte code differs
from 8-byte code, or where a float rounding moves a decision:

- the table of pairs of perturbation points (SDP_COL_WPAIR): even and odd W, W = 1, cost with and without w, per-node
  boxes with single-point lattices;
- the 4-byte rows of tests/column_forms.py (wide short first pass, SDP_COL_WIDE2, the 1024-thread split);
- the table per control and the staged tiles in 4 bytes; the lead and line kernels are 8-byte only: their problems
  must plan the direct kernel in 4 bytes and say so when asked for by name;
- four state axes without a perturbation and two controls; power-of-two spans next to others; an axis of two points,
  next states exactly on nodes, on the last node and three cells outside on both sides;
- the 512^3 problem of the benchmark's fifth configuration.

tests/test_fp32_cases_plan.py checks on the CPU that every case plans what it claims."""
import numpy as np

import column_forms as cf
import policies
from stodynprog_amd import SysDescription, DPSolver, models
from test_gpu_sweep import _priced_storage_problem

WHOLE_GRID_MAX = 20000          # the oracle runs on every node up to this many, on a sample above


class Run(object):
    """one kernel a case runs in: the `kernel` setting, with or without the certified filter, the family the plan
    must be (policies.family_of) and macros its unit must define ({name: value, or None for 'not defined'})"""

    def __init__(self, kernel, family, certified_filter=True, filtered=None, macros=None):
        self.kernel, self.family, self.certified_filter = kernel, family, certified_filter
        self.filtered = filtered            # what the plan says about the filter (None: not claimed)
        self.macros = dict(macros or {})

    def __repr__(self):
        return '{}{}'.format(self.kernel, '' if self.certified_filter else ' without filter')


GENERIC = Run('generic', 'generic')


def _column(first_pass=None, **macros):
    """the column family as 'auto' plans it, with and without its filter (`first_pass`: macros of the filter's own)"""
    return [GENERIC, Run('auto', 'column', True, True, dict(macros, **(first_pass or {}))),
            Run('auto', 'column', False, False, macros)]


class Case(object):
    def __init__(self, name, make, runs, chain=False, policies=(), refused=()):
        self.name, self._make, self.runs = name, make, list(runs)
        self.chain = chain              # value_iterations(V, 3) against three oracle sweeps
        self.policies = tuple(policies)  # kinds of tests/policies.py for eval_policy
        self.refused = tuple(refused)   # kernel names that must refuse 4-byte reals

    def __repr__(self):
        return self.name

    def reference(self):
        """the problem in 8-byte reals (the oracle's spec reads its discretisation)"""
        return self._make()

    def solver(self, run):
        s = policies.as_dtype(self.reference(), np.float32)
        s.kernel, s.certified_filter = run.kernel, run.certified_filter
        return s


def _model(name, **kw):
    def make():
        s = getattr(models, name)(**kw)[1]
        if len(s.state_grid) == 1:
            s.LINE_MIN_CELLS = 0        # (tests/policies.py: the line kernel would take the problem at this size)
        return s
    return make


def _form(case, geometry):
    return lambda: case.solver(geometry, dtype=np.float64)


def four_axes_deterministic():
    """four state axes, no perturbation (W = 0), two controls (C-order lattice, control 0 slowest)"""
    s = SysDescription((4, 2), name='four axes, deterministic')

    def dyn(a, b, c, d, u, v):
        return (a + 0.2 * u - 0.1 * v, 0.9 * b + 0.05 * c, 0.8 * c - 0.1 * b + 0.02, 0.7 * d + 0.2 * c)

    def cost(a, b, c, d, u, v):
        return (a - 0.1) * (a - 0.1) + 0.2 * u * u + 0.3 * abs(v) + 0.05 * u * v + 0.01 * b * d

    def box(a, b, c, d):
        return ((-1., 1.), (0., 0.5 + 0.5 * (a > 0)))
    s.dyn, s.cost, s.control_box = dyn, cost, box
    solver = DPSolver(s)
    solver.discretize_state(-1, 1, 9, -1, 1, 5, -1, 1, 4, -1, 1, 3)
    solver.control_steps = (0.25, 0.2)
    return solver


def spans(lo0, hi0, lo1, hi1):
    """a stock and an exogenous process on [lo0, hi0] x [lo1, hi1]: with power-of-two spans the position is a product
    with the reciprocal (csrc/sdp_device.h:sdp_div_span), with others the true division"""
    def make():
        s = SysDescription((2, 1, 1), name='spans')
        w0, w1 = hi0 - lo0, hi1 - lo1

        def dyn(e, p, u, w):
            return (e + 0.13 * w0 * u, (lo1 + 0.5 * w1) + 0.7 * (p - (lo1 + 0.5 * w1)) + w1 * w)

        def cost(e, p, u, w):
            return (p - u) * (p - u) + 0.15 * u * u + 0.01 * e
        s.dyn, s.cost = dyn, cost
        s.control_box = lambda e, p: ((-1., 1.),)
        s.perturb_laws = [models.NormalLaw(0, 0.1)]
        solver = DPSolver(s)
        solver.discretize_state(lo0, hi0, 23, lo1, hi1, 14)
        solver.discretize_perturb(-0.3, 0.3, 6)
        solver.control_steps = (0.11,)
        return solver
    return make


def edges():
    """Next states exactly on nodes, on the last node, and three cells and more outside on both sides; a second axis of
    two points (order - 2 = 0: the cell index is clamped to 0 whatever the position, lam is not clamped).

    Axis 0: 9 nodes on [0, 4], half a unit apart; the control lattice is k / 2 - 5.5 (exact in 4 bytes), so
    a' = a + u is a multiple of 0.5 between -5.5 and 9.5: every node, the last node (a' = 4: cell 7 with lam = 1, not
    a cell 8), and up to 11 cells outside.  Axis 1: the nodes 0 and 0.7; b' = 0.5 b + w with w up to 3 cells outside."""
    s = SysDescription((2, 1, 1), name='edges')

    def dyn(a, b, u, w):
        return (a + u, 0.5 * b + w)

    def cost(a, b, u, w):
        return 0.05 * u * u + 0.1 * (a - 1.5) * (a - 1.5) + 0.3 * b * w
    s.dyn, s.cost = dyn, cost
    s.control_box = lambda a, b: ((-5.5, 5.5),)
    s.perturb_laws = [models.NormalLaw(0, 1.0)]
    solver = DPSolver(s)
    solver.discretize_state(0, 4, 9, 0, 0.7, 2)
    solver.discretize_perturb(-2.1, 2.45, 14)
    solver.control_steps = (0.5,)
    return solver


_WPAIR = dict(SDP_COL_WPAIR='1')
_ALL = ('lattice', 'smooth', 'outside', 'special')
_F32 = [c for c in cf.CASES if c.dtype.itemsize == 4]

CASES = [
    # ---- the table of pairs of perturbation points
    Case('ar1_33x20', _model('storage_ar1', n_E=33, n_P=20, steps=(0.05, 0.1)), _column(**_WPAIR), chain=True,
         policies=_ALL),
    Case('searev_17x12x9', _model('searev', n_E=17, n_S=12, n_A=9, step=0.01), _column(**_WPAIR), policies=_ALL),
    Case('synthetic3d_24', _model('synthetic3d', N=24), _column(dict(SDP_COL_WIDE2='1'), **_WPAIR),
         policies=('smooth', 'special')),
    Case('priced_8', lambda: _priced_storage_problem(8)[1], _column(**_WPAIR), chain=True, policies=_ALL),
    Case('priced_7', lambda: _priced_storage_problem(7)[1], _column(**_WPAIR), chain=True, policies=('smooth',)),
    Case('priced_1', lambda: _priced_storage_problem(1)[1], _column(**_WPAIR), chain=True, policies=('outside',)),
    # ---- the 4-byte rows of tests/column_forms.py, at the geometries they run at there
] + [
    Case('{}-{}'.format(c.name, g), _form(c, g),
         [GENERIC, Run('auto', 'column', True, True, cf.claims(c, g)), Run('auto', 'column', False, False)])
    for c in _F32 for g in c.geometries
] + [
    # ---- the other families.  Two controlled stocks: the reduced-array sweep is 8-byte only
    Case('two_reservoirs', _model('two_reservoirs', n_a=12, n_b=10, n_y=8),
         [Run('auto', 'generic'), Run('column', 'table per control', macros=dict(SDP_COL_WPAIR='0')),
          Run('staged', 'staged')], chain=True, policies=_ALL, refused=('lead',)),
    Case('coupled_24', _model('synthetic3d_coupled', N=24),
         [GENERIC, Run('column', 'table per control', macros=dict(SDP_COL_WPAIR='0')), Run('staged', 'staged')],
         policies=('smooth', 'outside')),
    Case('coupled_48', _model('synthetic3d_coupled', N=48),
         [GENERIC, Run('auto', 'table per control', macros=dict(SDP_COL_WPAIR='0')), Run('staged', 'staged')]),
    # ---- one state variable: the line kernel is 8-byte only
    Case('inventory', _model('inventory'), [Run('auto', 'generic'), Run('staged', 'staged')], chain=True,
         policies=_ALL, refused=('line',)),
    Case('inventory_fine', _model('inventory_fine', n_x=200, n_u=33, n_w=8),
         [Run('auto', 'generic'), Run('staged', 'staged')], chain=True, policies=_ALL, refused=('line',)),
    # ---- shapes
    Case('four_axes_deterministic', four_axes_deterministic, [GENERIC, Run('auto', 'column', filtered=False)],
         chain=True, policies=('smooth', 'outside')),
    Case('spans_pow2', spans(0., 1., -4., 4.), _column(**_WPAIR), chain=True, policies=('smooth', 'outside')),
    Case('spans_other', spans(0., 0.7, -1., 2.), _column(**_WPAIR), chain=True, policies=('smooth', 'outside')),
    Case('edges', edges, _column(**_WPAIR), chain=True, policies=_ALL),
]

# the benchmark's fifth configuration at full size (its own test: sampled nodes, a time limit)
CONFIG5 = Case('config5_512', _model('synthetic3d', N=512),
               [GENERIC, Run('auto', 'column', True, True, dict(SDP_COL_WPAIR='1', SDP_COL_WIDE2='1'))])


def plan_of(solver):
    t = None if solver.sys.stationnary else 0
    return solver._kernel_plan() if t is None else solver._kernel_plan(t, solver._trace_now(t))


def unmet(case, run, plan):
    """what `plan` (of case.solver(run)) does not meet of the run's claims: a list of strings, empty when all is met"""
    out = []
    if policies.family_of(plan) != run.family:
        out.append('family {} (claimed {})'.format(policies.family_of(plan), run.family))
    if run.filtered is not None and bool(plan.get('filtered')) != run.filtered:
        out.append('filtered {} (claimed {})'.format(bool(plan.get('filtered')), run.filtered))
    if '#define SDP_REAL float' not in plan['source']:
        out.append('not a unit of 4-byte reals')
    for k, v in sorted(run.macros.items()):
        if cf.macro(plan['source'], k) != v:
            out.append('{} = {} (claimed {})'.format(k, cf.macro(plan['source'], k), v))
    return out


def nodes_of(shape, seed=0):
    """None (every node) up to WHOLE_GRID_MAX nodes; else column_forms.sample_nodes (boundaries and split rows) and
    2000 random nodes, sorted flat C-order ids"""
    S = int(np.prod(shape))
    if S <= WHOLE_GRID_MAX:
        return None
    extra = np.random.default_rng(77 + seed).choice(S, size=2000, replace=False)
    base = cf.sample_nodes(shape, seed=seed) if len(shape) == 3 else np.array([0, S - 1])
    return np.unique(np.concatenate([base, extra]))


def special_values(V):
    """NaN and +-inf inside V: the pattern of test_gpu_column_forms._special_values on three axes; on other shapes a
    NaN run, single NaN, +inf and -inf entries at the ends and inside"""
    V = np.array(V)
    if V.ndim == 3 and min(V.shape) >= 4:
        from test_gpu_column_forms import _special_values
        return _special_values(V)
    flat = V.reshape(-1)
    S = flat.size
    flat[S // 3:S // 3 + max(1, S // 40)] = np.nan
    flat[S - 1] = np.nan
    flat[(3 * S) // 4] = np.inf
    flat[0] = np.inf
    flat[S // 2] = -np.inf
    return V
