"""The cases of tests/test_multi_perturb_plan.py (CPU) and tests/test_gpu_multi_perturb.py (GPU) as a table (test
infrastructure, like tests/fp32_cases.py; not a test file): systems with SEVERAL perturbation variables, which run the
node-order kernels of csrc/sdp_multiw_kernel.h on the flat law of stodynprog_amd/perturb.py.

The yardstick is the pinned oracle, unchanged: oracle/vi_numpy.py takes arbitrary callables and ONE law, so it is
given the flat law -- perturb_grid = [arange(W)], perturb_proba = [P] -- and callables wrapped by `flat_spec`'s
adapter, which turns the last argument j into the values wtab[i][j] of every variable.  Every grid is the smallest at
which the kernel can still go wrong:

  order       d = 1, 7 nodes, ONE control point, W = (3, 2), law and model asymmetric in the variables: the flat order
              and P (one lane per node)
  ragged      d = 2, 5 x 7 nodes, a traced box per node, W = (3, 2): several lanes per node, dead lanes, the box table,
              a last tile that is not full
  wide        d = 3, 5 x 4 x 3, two controls, W = (2, 3, 2): three variables
  one_lane    a control lattice of 2 points: ONE control per lane (codegen.lanes_for(2) = 2, the least number of lanes
              a lattice of more than one point is given; the single lane per node is `order`)
  full_wave   a lattice of 41 controls: 64 lanes per node, one node per wave
  degenerate  W = (5, 1): the second variable has one point -- the same bits as the ONE-variable system with that point
              written into the callables as a constant (`degenerate_twin`), which ties the new kernels to the pinned ones
  horizon     non-stationary, constants looked up as DATA[k], 4 steps: time-lifted parameters

The second variable of every model enters through operations with a NON-constant operand only: a product of two
constants would be folded in float64 by Python before a 4-byte problem rounds it, where the kernel multiplies two
float32 table entries."""
import numpy as np

from oracle import vi_numpy
from stodynprog_amd import SysDescription, DPSolver, perturb

DATA = (0.3, -0.2, 0.0, 0.15)           # horizon: constants of step k
HORIZON = len(DATA)
DEGENERATE_POINT = 0.7                  # degenerate: the single point of the second variable


class Case(object):
    """name; make(dtype) -> solver; m perturbation variables with `dims` points; `lanes` per node the plan must give"""

    def __init__(self, name, make, dims, lanes, horizon=None):
        self.name, self._make, self.dims, self.lanes, self.horizon = name, make, tuple(dims), lanes, horizon
        self.m = len(self.dims)

    def __repr__(self):
        return self.name

    def solver(self, dtype=np.float64):
        return self._make(dtype)


# asymmetric laws (probabilities that sum to 1 in float64; no two products equal)
LAW_3A = ([0.0, 0.4, 0.8], [0.2, 0.3, 0.5])
LAW_3B = ([-1.0, 0.5, 0.25], [0.5, 0.125, 0.375])
LAW_5 = ([-0.5, -0.2, 0.0, 0.3, 0.6], [0.1, 0.15, 0.4, 0.25, 0.1])
LAW_1 = ([DEGENERATE_POINT], [1.0])
LAW_2B = ([-1.0, 0.5], [0.4, 0.6])


def _finish(s, dtype, state, laws, steps):
    solver = DPSolver(s, dtype=dtype)
    solver.discretize_state(*state)
    solver.perturb_grid = [np.array(g, dtype=float) for g, _ in laws]
    solver.perturb_proba = [np.array(p, dtype=float) for _, p in laws]
    solver.control_steps = tuple(steps)
    return solver


def _order(dtype):
    s = SysDescription((1, 1, 2), name='order')
    s.dyn = lambda x, u, w1, w2: ((x + u) - w1 + 0.5 * x * w2,)
    s.cost = lambda x, u, w1, w2: (x * x + 2.0 * u * w2) + w1 * w1 * x
    s.control_box = lambda x: ((0.5, 0.5),)
    return _finish(s, dtype, (0, 3, 7), [LAW_3A, LAW_2B], (0.25,))


def _ragged(dtype):
    s = SysDescription((2, 1, 2), name='ragged')
    s.dyn = lambda a, y, u, w1, w2: ((a + u) - 0.3 * w1, (0.6 * y + w2 * u) + 0.1 * w1)
    s.cost = lambda a, y, u, w1, w2: ((u - y) * (u - y) + 0.2 * a * w2) + abs(a - 1.0) * w1
    s.control_box = lambda a, y: ((-0.25 * a, 0.5 + 0.125 * y),)
    return _finish(s, dtype, (0, 2, 5, -1, 1, 7), [LAW_3B, LAW_2B], (0.125,))


def _wide(dtype):
    s = SysDescription((3, 2, 3), name='wide')
    s.dyn = lambda a, b, y, u, v, w1, w2, w3: ((a + u) - w1 * v, (b + v) - 0.5 * u * w3, (0.7 * y + w2) + 0.1 * w3 * a)
    s.cost = lambda a, b, y, u, v, w1, w2, w3: ((u - 0.3) * (u - 0.3) + (v + y) * (v + y)) + (w1 * a + w2 * b * w3)
    s.control_box = lambda a, b, y: ((0., 1.), (-0.5, 0.5))
    return _finish(s, dtype, (0, 2, 5, 0, 1.5, 4, -1, 1, 3), [LAW_2B, LAW_3B, ([0.2, -0.4], [0.7, 0.3])], (0.5, 0.5))


def _one_control_per_lane(dtype):
    s = SysDescription((1, 1, 2), name='one_lane')
    s.dyn = lambda x, u, w1, w2: ((0.8 * x + u) + w1 * w2,)
    s.cost = lambda x, u, w1, w2: (x - 1.0) * (x - 1.0) + u * (w1 - w2)
    s.control_box = lambda x: ((0., 1.),)
    return _finish(s, dtype, (0, 2, 6), [LAW_3B, LAW_2B], (1.0,))


def _full_wave(dtype, n_x=9):
    """(n_x: tests/test_gpu_multi_perturb.py also runs it on a grid past the sweep's launch cap; the unit is the same)"""
    s = SysDescription((1, 1, 2), name='full_wave')
    s.dyn = lambda x, u, w1, w2: ((x + u) - w1 + 0.25 * u * w2,)
    s.cost = lambda x, u, w1, w2: (x * x + 0.5 * u * u) + (w2 * u + w1 * x)
    s.control_box = lambda x: ((-1., 1.),)
    return _finish(s, dtype, (-2, 2, n_x), [LAW_3B, LAW_2B], (0.05,))


def _degenerate_callables(second):
    """dyn and cost of `degenerate`; second(w2) is how the second variable is read: itself, or the constant"""
    def dyn(a, y, u, w1, w2):
        w2 = second(w2)
        return ((a + u) - w1 * w2, 0.5 * y + (w1 + w2 * u))

    def cost(a, y, u, w1, w2):
        w2 = second(w2)
        return ((u - y) * (u - y) + a * w2) + 0.3 * w1 * w1
    return dyn, cost


def _degenerate(dtype):
    s = SysDescription((2, 1, 2), name='degenerate')
    s.dyn, s.cost = _degenerate_callables(lambda w2: w2)
    s.control_box = lambda a, y: ((-0.5, 0.5),)
    return _finish(s, dtype, (0, 2, 4, -1, 1, 5), [LAW_5, LAW_1], (0.25,))


def degenerate_twin(dtype=np.float64):
    """`degenerate` as a system of ONE perturbation variable: the second variable's point a constant of the callables"""
    dyn2, cost2 = _degenerate_callables(lambda w2: DEGENERATE_POINT)
    s = SysDescription((2, 1, 1), name='degenerate twin')
    s.dyn = lambda a, y, u, w1: dyn2(a, y, u, w1, None)
    s.cost = lambda a, y, u, w1: cost2(a, y, u, w1, None)
    s.control_box = lambda a, y: ((-0.5, 0.5),)
    solver = _finish(s, dtype, (0, 2, 4, -1, 1, 5), [LAW_5], (0.25,))
    solver.kernel = 'generic'
    return solver


def _horizon(dtype):
    s = SysDescription((1, 1, 2), stationnary=False, name='horizon')
    s.dyn = lambda k, x, u, w1, w2: ((0.9 * x + u) + w1 * DATA[k] + w2 * x,)
    s.cost = lambda k, x, u, w1, w2: ((x - 0.1 * k) * (x - 0.1 * k) + 0.1 * u * u) + DATA[k] * u * w2
    s.control_box = lambda k, x: ((-1., 1.),)
    return _finish(s, dtype, (-2, 2, 9), [LAW_3B, LAW_2B], (0.5,))


CASES = [
    Case('order', _order, (3, 2), 1),
    Case('ragged', _ragged, (3, 2), 16),
    Case('wide', _wide, (2, 3, 2), 16),
    Case('one_lane', _one_control_per_lane, (3, 2), 2),
    Case('full_wave', _full_wave, (3, 2), 64),
    Case('degenerate', _degenerate, (5, 1), 8),
    Case('horizon', _horizon, (3, 2), 8, horizon=HORIZON),
]
BY_NAME = {c.name: c for c in CASES}
DTYPES = {'f64': np.float64, 'f32': np.float32}


def plan_of(solver, t_k=None):
    """the plan of a case's solver (a time-dependent one: of step t_k, traced for that step)"""
    if solver.sys.stationnary:
        return solver._kernel_plan()
    return solver._kernel_plan(t_k, solver._trace_now(t_k))


def unit_sources():
    """every generated unit the GPU tests run: each case in both reals (every step of the horizon), and the twin"""
    out = []
    for dt in DTYPES.values():
        for case in CASES:
            s = case.solver(dt)
            out += [plan_of(s, t)['source'] for t in (range(case.horizon) if case.horizon else (None,))]
        out.append(degenerate_twin(dt)._kernel_plan()['source'])
    return out


def flat_spec(solver, wtab=None, P=None):
    """The oracle's spec of `solver` on the FLAT law: one perturbation 'variable' j = 0..W-1 with probabilities P, dyn
    and cost behind an adapter that turns the last argument j into wtab[i].astype(j.dtype)[j] for every variable i (a
    4-byte run thereby reads the table rounded once to float32, as the kernel does).  A time index that the oracle's
    4-byte path hands over as a float32 scalar is made the int it stands for (the models index DATA with it)."""
    if wtab is None:
        wtab, P = perturb.product_law(solver.perturb_grid, solver.perturb_proba)
    s = solver.sys
    m = len(wtab)

    def adapt(f):
        def g(*args, **kw):
            j = np.asarray(args[-1])
            head = args[:-1]
            if not s.stationnary and isinstance(head[0], np.floating):
                assert float(head[0]) == int(head[0])
                head = (int(head[0]),) + tuple(head[1:])
            ws = tuple(wtab[i].astype(j.dtype)[j.astype(np.int64)] for i in range(m))
            return f(*(tuple(head) + ws), **kw)
        return g

    return vi_numpy.Spec(adapt(s.dyn), adapt(s.cost), s.control_box, solver.state_grid,
                         [np.arange(len(P), dtype=float)], [P], solver.control_steps, s.params, s.stationnary)


def inputs(shape, dtype):
    """four cost-to-go arrays: zeros, smooth, seeded random, and one with NaN and +-inf entries"""
    S = int(np.prod(shape))
    x = np.linspace(0., 1., S).reshape(shape)
    rng = np.random.default_rng(20 + len(shape))
    rand = rng.standard_normal(shape)
    bad = rng.standard_normal(shape)
    flat = bad.reshape(-1)
    flat[1], flat[S // 3], flat[S - 1] = np.nan, np.inf, -np.inf          # (none of them the relative-DP reference node)
    return {'zeros': np.zeros(shape, dtype=dtype), 'smooth': (3.0 * x * x - x).astype(dtype),
            'random': rand.astype(dtype), 'non-finite': bad.astype(dtype)}
