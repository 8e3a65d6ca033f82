"""The cases of tests/test_forward_plan.py (CPU) and tests/test_gpu_forward.py (GPU) as a table (test infrastructure,
like tests/multi_perturb.py; not a test file): models and policies whose transition operator
(DPSolver.transition_operator, stodynprog_amd/forward.py) is built on the device and compared with the definition.

  inventory      the tutorial's shop, d = 1: 2 vertices per cell, 4 law points, next states below the grid
  storage_ar1    models.storage_ar1(13, 9, 5): d = 2, two controls, a column unit; the AR(1) axis leaves the grid
  searev         models.searev(7, 9, 9, 5): d = 3, a column unit
  four_d         hand-written, 4 x 3 x 3 x 3: 16 vertices per cell
  two_inflows    models.two_inflows small: TWO perturbation variables, laws of 3 and 2 points (the flat law of 6)
  deterministic  no perturbation: W = 1, P = [1]
  leaves_grid    an expanding map: next states far outside on both sides, weights well below 0 and above 1
  nan_state      sqrt of a state variable that is negative at some nodes: NaN next states and NaN costs there
  horizon        models.finite_horizon, non-stationary with a symbolic time index, at t_k = 0 and 3
  lookup         non-stationary with constants looked up as DATA[k]: traced for the one step with a concrete int index
                 (time-lifted parameters), at t_k = 1 and 3; the definition then hands the callables the int too
  untraceable    the storage model behind a callable the tracer refuses: entries made on the host (from_coo); its
                 traced twin is `storage_ar1`

  long_line      (`long_line(cus)`, not in CASES) one state on cus * 8 * 256 + 129 nodes, a two-point law and steps of a
                 few nodes: past the launch caps of sdp_transitions, of the stream kernels of the CSR build, of k_push,
                 of k_push_group<16> once every row is listed, and (8-byte reals) of push_until's k_diff_stats

Policies are smooth functions of the state between bounds given per case, off every lattice: what a user may hand
to eval_policy.  The grids of CASES are small: every workgroup of theirs makes one trip through its grid-stride loop;
`long_line` is the case whose workgroups make a second one."""
import numpy as np

from stodynprog_amd import SysDescription, DPSolver, models
from stodynprog_amd.trace import TraceError

DTYPES = {'f64': np.float64, 'f32': np.float32}


def as_dtype(solver, dtype):
    """the same problem in other reals"""
    s = DPSolver(solver.sys, dtype=dtype)
    s.state_grid, s.perturb_grid = solver.state_grid, solver.perturb_grid
    s.perturb_proba, s.control_steps = solver.perturb_proba, solver.control_steps
    s._state_grid_shape, s._state_ref_ind = solver._state_grid_shape, solver._state_ref_ind
    return s


def wave_policy(solver, bounds, seed=0):
    """shape state_dims + (nu,): control c = lo_c + (hi_c - lo_c) (0.5 + 0.45 sin(phase + sum_k a_k z_k)), z the
    state scaled to [0, 1] per axis"""
    dims = tuple(len(g) for g in solver.state_grid)
    pol = np.empty(dims + (len(bounds),))
    for c, (lo, hi) in enumerate(bounds):
        rng = np.random.default_rng(1000 * seed + c)
        arg = np.full(dims, rng.uniform(0, 2 * np.pi))
        for k, g in enumerate(solver.state_grid):
            g = np.asarray(g, dtype=float)
            shape = [1] * len(dims)
            shape[k] = -1
            arg = arg + rng.uniform(1.5, 7.0) * rng.choice([-1, 1]) * ((g - g[0]) / (g[-1] - g[0])).reshape(shape)
        pol[..., c] = lo + (hi - lo) * (0.5 + 0.45 * np.sin(arg))
    return pol


class Case(object):
    """name; make() -> float64 solver; bounds of the policy per control; times: the t_k the operator is built at; host:
    the callables cannot be traced"""

    def __init__(self, name, make, bounds, times=(None,), host=False, time_index='real'):
        self.name, self._make, self.bounds, self.times, self.host = name, make, bounds, times, host
        self.time_index = time_index        # forward.entries(time_index=): how the definition hands t_k to the callables

    def __repr__(self):
        return self.name

    def solver(self, dtype=np.float64, kernel=None):
        s = as_dtype(self._make(), dtype)
        if kernel is not None:
            s.kernel = kernel
        return s

    def policy(self, solver):
        return wave_policy(solver, self.bounds)


def _four_d():
    s = SysDescription((4, 1, 1), name='four_d')
    s.dyn = lambda a, b, c, e, u, w: ((0.8 * a + 0.5 * u) + w, 0.5 * b + 0.3 * a, (0.6 * c + 0.5 * w) + 0.1 * e,
                                     0.9 * e - 0.2 * u)
    s.cost = lambda a, b, c, e, u, w: ((a - 0.5) * (a - 0.5) + u * u) + (b * c + e * w)
    s.control_box = lambda a, b, c, e: ((0., 1.),)
    solver = DPSolver(s)
    solver.discretize_state(0, 1, 4, 0, 1, 3, -1, 1, 3, 0, 2, 3)
    solver.perturb_grid = [np.array([-0.2, 0.05, 0.3])]
    solver.perturb_proba = [np.array([0.25, 0.5, 0.25])]
    solver.control_steps = (0.5,)
    return solver


def _deterministic():
    s = SysDescription((2, 1, 0), name='deterministic')
    s.dyn = lambda x, y, u: (0.9 * x + u, 0.5 * y + 0.25 * x)
    s.cost = lambda x, y, u: x * x + (y - u) * (y - u)
    s.control_box = lambda x, y: ((-0.5, 0.5),)
    solver = DPSolver(s)
    solver.discretize_state(-1, 1, 6, -1, 1, 5)
    solver.perturb_grid, solver.perturb_proba = [], []
    solver.control_steps = (0.25,)
    return solver


def _leaves_grid():
    s = SysDescription((2, 1, 1), name='leaves_grid')
    s.dyn = lambda x, y, u, w: ((2.5 * x + u) + w, 1.75 * y - w)
    s.cost = lambda x, y, u, w: (x * x + y * y) + u * w
    s.control_box = lambda x, y: ((-1., 1.),)
    solver = DPSolver(s)
    solver.discretize_state(-1, 1, 5, -1, 1, 4)
    solver.perturb_grid = [np.array([-0.5, 0.0, 0.75])]
    solver.perturb_proba = [np.array([0.3, 0.5, 0.2])]
    solver.control_steps = (0.5,)
    return solver


def _nan_state():
    s = SysDescription((1, 1, 1), name='nan_state')
    s.dyn = lambda x, u, w: ((np.sqrt(x) + u) + w,)
    s.cost = lambda x, u, w: 0.5 * np.sqrt(x) + u * u
    s.control_box = lambda x: ((0., 1.),)
    solver = DPSolver(s)
    solver.discretize_state(-1, 2, 7)                  # two nodes below zero
    solver.perturb_grid = [np.array([-0.25, 0.25])]
    solver.perturb_proba = [np.array([0.5, 0.5])]
    solver.control_steps = (0.5,)
    return solver


DATA = (0.3, -0.2, 0.0, 0.15)           # lookup: constants of step k


def _lookup():
    s = SysDescription((1, 1, 1), stationnary=False, name='lookup')
    s.dyn = lambda k, x, u, w: ((0.9 * x + u) + w * DATA[k],)
    s.cost = lambda k, x, u, w: (x - DATA[k]) * (x - DATA[k]) + 0.1 * u * u
    s.control_box = lambda k, x: ((-1., 1.),)
    solver = DPSolver(s)
    solver.discretize_state(-2, 2, 9)
    solver.perturb_grid = [np.array([-1.0, 0.5, 0.25])]
    solver.perturb_proba = [np.array([0.5, 0.125, 0.375])]
    solver.control_steps = (0.5,)
    return solver


def _untraceable():
    ref = models.storage_ar1(n_E=13, n_P=9, n_w=5)[1]
    s = SysDescription((2, 2, 1), name='untraceable')

    def dyn(E, P_mis, P_sto, P_cur, innov):
        shape = np.shape(P_sto)                         # needs a concrete array
        return ref.sys.dyn(E, P_mis, np.asarray(P_sto).reshape(shape), P_cur, innov)
    s.dyn = dyn
    s.cost = ref.sys.cost
    s.control_box = ref.sys.control_box
    solver = DPSolver(s)
    solver.discretize_state(0, 10., 13, -4., 4., 9)
    solver.perturb_grid, solver.perturb_proba = ref.perturb_grid, ref.perturb_proba
    solver.control_steps = ref.control_steps
    assert isinstance(solver._traced(), TraceError)
    return solver


def long_line_nodes(cus, per_cu=8):
    return cus * per_cu * 256 + 129


def long_line(cus, per_cu=8):
    """the Case on long_line_nodes(cus, per_cu) nodes of [0, 1]: x + u + w with |u| <= 1.5 and w = -2.5 or 3.25 node
    spacings, so rows are short (the lane path) and a vector that starts near the end of the grid stays there for a
    few pushes.  per_cu = 16: past the caps of the direct kernel's eval_policy and of k_shift (tests/test_gpu_policy_forms.py)"""
    S = long_line_nodes(cus, per_cu)
    h = 1.0 / (S - 1)

    def make():
        s = SysDescription((1, 1, 1), name='long_line')
        s.dyn = lambda x, u, w: ((x + u) + w,)
        s.cost = lambda x, u, w: (x - 0.5) * (x - 0.5) + u * w
        s.control_box = lambda x: ((-1., 1.),)
        solver = DPSolver(s)
        solver.discretize_state(0, 1, S)
        solver.perturb_grid = [np.array([-2.5 * h, 3.25 * h])]
        solver.perturb_proba = [np.array([0.375, 0.625])]
        solver.control_steps = (0.5,)
        return solver
    return Case('long_line', make, [(-1.5 * h, 1.5 * h)])


def long_line_caps(S, nnz, row_lengths, cus, itemsize):
    """the launches of csrc/sdp_hip.hip a long_line operator goes through, restated: name -> (workgroups wanted for
    one trip, the cap).  row_lengths: entries per row of P^T."""
    short = int((row_lengths < 8).sum())
    listed = int(((row_lengths >= 1) & (row_lengths < 256)).sum())         # set_long_rows(1): the rows of k_push_group<16>
    vec = 16 // itemsize
    return {'sdp_transitions': (-(-S * 2 // 256), cus * 8), 'k_iota, k_trans_gather, k_trans_count': (-(-nnz // 256), cus * 8),
            'k_push': (-(-S // 256) if short else 0, cus * 8), 'k_push_group<16>': (-(-listed // 16), cus * 64),
            'k_diff_stats': (-(-(S // vec) // 256), cus * 4)}


CASES = [
    Case('inventory', lambda: models.inventory()[1], [(0., 10.)]),
    Case('storage_ar1', lambda: models.storage_ar1(n_E=13, n_P=9, n_w=5)[1], [(-4., 4.), (0., 0.)]),
    Case('searev', lambda: models.searev(n_E=7, n_S=9, n_A=9, n_w=5)[1], [(-1.1, 1.1)]),
    Case('four_d', _four_d, [(0., 1.)]),
    Case('two_inflows', lambda: models.two_inflows(n_a=4, n_b=3, n_y=3, n_w=(3, 2))[1], [(0., 1.), (0., 1.)]),
    Case('deterministic', _deterministic, [(-0.5, 0.5)]),
    Case('leaves_grid', _leaves_grid, [(-1., 1.)]),
    Case('nan_state', _nan_state, [(0., 1.)]),
    Case('horizon', lambda: models.finite_horizon(n_x=9)[1], [(-1., 1.)], times=(0, 3)),
    Case('lookup', _lookup, [(-1., 1.)], times=(1, 3), time_index='int'),
    Case('untraceable', _untraceable, [(-4., 4.), (0., 0.)], host=True),
]
BY_NAME = {c.name: c for c in CASES}
DEVICE_CASES = [c for c in CASES if not c.host]


def plan_of(solver, t_k=None):
    """the plan of a case's solver (a time-dependent one: traced with its symbolic time index)"""
    if solver.sys.stationnary:
        return solver._kernel_plan()
    return solver._kernel_plan(t_k, solver._trace_now(t_k))


def unit_sources():
    """every generated unit the GPU tests run: each traced case in both reals, as planned and with the direct kernel"""
    out = []
    for dt in DTYPES.values():
        for case in DEVICE_CASES:
            for kernel in (None, 'generic'):
                s = case.solver(dt, kernel)
                out += [plan_of(s, t)['source'] for t in case.times]
        # long_line as an MI355X's 256 CUs size it (the source does not depend on the number of nodes)
        out += [plan_of(long_line(256).solver(dt, kernel))['source'] for kernel in (None, 'generic')]
    return list(dict.fromkeys(out))


def vectors(S, dtype):
    """the distributions pushed: uniform, random (signed), a single delta, and one with a NaN and an inf entry"""
    rng = np.random.default_rng(5 + S)
    delta = np.zeros(S)
    delta[S // 2] = 1.0
    bad = rng.random(S)
    bad[S // 3], bad[S - 1] = np.nan, np.inf
    return {'uniform': np.full(S, 1.0 / S).astype(dtype), 'random': rng.standard_normal(S).astype(dtype),
            'delta': delta.astype(dtype), 'non-finite': bad.astype(dtype)}


def same(a, b):
    """np.array_equal that also tells zeros of opposite sign apart and takes NaNs at the same places as equal"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != 'f':
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na], b[~nb])
                and np.array_equal(np.signbit(a[~na]), np.signbit(b[~nb])))
