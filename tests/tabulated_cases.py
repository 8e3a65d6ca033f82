"""Tabulated mode -- the two kernels of sdp_tab_backup (csrc/sdp_hip.hip: k_tab_cells<D>, k_tab_reduce) and the four host
drivers that feed them (DPSolver._backup_tabulated, _eval_policy_tabulated, _lookahead_tabulated,
_value_at_state_vect) -- as a table of cases (test infrastructure, like tests/percontrol_forms.py; not a test file, and
no GPU code).

Every model here is one the tracer refuses (the `np.shape(u)` idiom: the dynamics needs a concrete array), so its
callables run on the host and everything else on the device: k_tab_cells<D> adds the interpolated cost-to-go to the cost
of every lattice cell (D state variables: 1, 2, 3 and, through `default:`, 4), k_tab_reduce sums a control's cells over
the perturbation points in order (a deterministic system has one cell per control) and takes the first-occurrence argmin
of a node in one wavefront: lane l sees controls l, l + 64, l + 128, ... in turn ("lane trips") and a 64-lane butterfly
settles the rest.  What a case is there for is a matter of its LATTICE SIZES, so a case claims d, nu, W, the smallest and
the largest number of controls U of a node, and the lane trips ceil(max U / 64).

The quantised line (`line`): one state x on [0, 1], the box (0, width * x) -- or a constant one -- and

    q = floor(quant * |u - centre * hi| + 0.5),    x' = 0.5 x + 0.05 q + w,    g = 10 q + 0.3 x^2 + 0.1 w q

The control reaches the next state and the cost through q alone: the controls of a node with the same q have the same
expected cost BIT FOR BIT, on every cost-to-go, and the minimisers are a run of adjacent controls around the centre.
Where the run lies among the lanes and trips is the case: tests/test_tabulated_cases_plan.py asserts it from the
oracle's per-control vector.

`with_cost_marks` puts NaN, +inf or -inf into the cost at given control indices (or at every control of some nodes);
`mirrored` cases are the same problems with the state axes turned round in the box, so that the lattices SHRINK along the
sweep (what is left of a larger batch lies behind a smaller one in the handle's buffers).

tests/test_tabulated_cases_plan.py checks on the CPU that every case is what it claims;
tests/test_gpu_tabulated.py runs them on the GPU against oracle/vi_numpy.py, bit for bit on all nodes."""
import inspect
import itertools

import numpy as np

import percontrol_forms as pf
from percontrol_forms import INPUTS
from stodynprog_amd import SysDescription, DPSolver
from stodynprog_amd import lookahead as la
from stodynprog_amd.models import NormalLaw
from oracle import vi_numpy

LANES = 64


def inputs(shape):
    """the six cost-to-go arrays of the form tables (percontrol_forms.inputs: 'zeros', 'smooth', 'random', 'kinked',
    'flat', 'special' -- NaN, +inf and -inf entries), with 'flat' the constant 2^60 on the whole grid: the cost of a control
    is lost in its rounding and the interpolation weights of a next state inside the grid sum to one exactly, so the
    controls of a node tie bit for bit across all lanes and trips and index 0 must win"""
    V = pf.inputs(shape, 8)
    V['flat'] = np.full(tuple(int(n) for n in shape), 2.0 ** 60)
    return V


def trips(U):
    """controls a lane of k_tab_reduce sees at most at a node of U controls"""
    return -(-int(U) // LANES)


def _skew(solver):
    """weights that are not symmetric about the middle point (those of a discretised normal law are, bit for bit: a sum
    that took them in the opposite order would give the same bits): 1 : 2 : 3 : ... scaled to sum to one"""
    W = len(solver.perturb_grid[0])
    p = np.arange(1., W + 1.)
    solver.perturb_proba = [p / p.sum()]


def _concrete(u):
    """the idiom the tracer refuses: the shape of a concrete array"""
    return np.asarray(u).reshape(np.shape(u))


# ---------------------------------------------------------------------------------------------------------------------
# the models
# ---------------------------------------------------------------------------------------------------------------------
def line(centre=0.5, quant=4.0, width=3.2, step=0.025, n_x=33, constant=None, mirror=False, dtype=np.float64):
    """the quantised line of the module's docstring.  `constant`: a box (0, constant) at every node instead of
    (0, width * x); `mirror`: (0, width * (1 - x))"""
    def make():
        sysd = SysDescription((1, 1, 1), name='quantised line')

        def hi_of(x):
            return constant if constant is not None else width * ((1.0 - x) if mirror else x)

        def q_of(x, u):
            return np.floor(quant * np.abs(_concrete(u) - centre * hi_of(x)) + 0.5)

        def dyn(x, u, w):
            return (0.5 * x + 0.05 * q_of(x, u) + w,)

        def cost(x, u, w):
            q = q_of(x, u)
            return 10.0 * q + 0.3 * x * x + 0.1 * w * q
        sysd.dyn, sysd.cost = dyn, cost
        sysd.control_box = lambda x: ((0.0, hi_of(x)),)
        sysd.perturb_laws = [NormalLaw(0, 0.1)]
        s = DPSolver(sysd, dtype=dtype)
        s.discretize_state(0, 1, n_x)
        s.discretize_perturb(-0.3, 0.3, 3)
        _skew(s)
        s.control_steps = (step,)
        return s
    return make


def constant_line(U):
    """exactly U controls at every node: the box (0, (U - 1) / 4) in steps of 1 / 4 (exact in binary), the centre on the
    LAST control and q = 0 within three controls of it: U - 4 .. U - 1 tie, on either side of lane 63 / 0 for U = 65"""
    return line(centre=1.0, quant=0.5, step=0.25, n_x=9, constant=(U - 1) * 0.25)


NAN_A, INF_A, BIG_A = 0.3125, 0.4375, 0.5625         # off-grid states whose box has no lattice (lookahead: NaN, NaN, -1)


def _no_lattice(a, hi):
    """the box end `hi`, but NaN / +inf / 10^12 (a lattice of more than 2^31 points) at three states between the nodes"""
    if np.ndim(a) == 0:
        if a == NAN_A:
            return np.nan
        if a == INF_A:
            return np.inf
        if a == BIG_A:
            return 1e12
    return hi


def two_controls(n_a=7, n_b=6, mirror=False, dtype=np.float64):
    """two states on [0, 1]^2, two controls whose box ends all move with the state: (-a, a) in steps of 1 / 4 and
    (-2 b, 2 b) in steps of 1 / 4: 1 x 1 points at the origin, 1 x n along a == 0, n x 1 along b == 0, 9 x 17 at (1, 1)"""
    def make():
        sysd = SysDescription((2, 2, 1), name='two controls')

        def dyn(a, b, u, v, w):
            u, v = _concrete(u), _concrete(v)
            return (0.8 * a + 0.15 * u + 0.05 * v + 0.5 * w, 0.6 * b + 0.2 * v - 0.1 * u * w)
        sysd.dyn = dyn
        sysd.cost = lambda a, b, u, v, w: (u - 0.3) * (u - 0.3) + 0.5 * (v + 0.4 - b) * (v + 0.4 - b) + 0.2 * a * w + 0.1 * u * v

        def box(a, b):
            ra, rb = ((1.0 - a), (1.0 - b)) if mirror else (a, b)
            return ((-ra, _no_lattice(a, ra)), (-2.0 * rb, 2.0 * rb))
        sysd.control_box = box
        sysd.perturb_laws = [NormalLaw(0, 0.2)]
        s = DPSolver(sysd, dtype=dtype)
        s.discretize_state(0, 1, n_a, 0, 1, n_b)
        s.discretize_perturb(-0.4, 0.4, 5)
        _skew(s)
        s.control_steps = (0.25, 0.25)
        return s
    return make


def three_states(shape=(7, 6, 5), timed=False, dtype=np.float64):
    """three states, one control on (-1 - a, 1 + b) in steps of 1 / 20: 41 to 81 controls.  `timed`: a time-dependent
    system (the callables get the time index first; it drifts the dynamics, tilts the cost and widens the box)"""
    def make():
        sysd = SysDescription((3, 1, 1), stationnary=not timed, name='three states')

        def dyn3(t, a, b, c, u, w):
            u = _concrete(u)
            return (0.7 * a + 0.2 * u + 0.05 * t, 0.9 * b + 0.3 * w - 0.05 * u, 0.5 * c + 0.25 * a * u + 0.1 * w)

        def cost3(t, a, b, c, u, w):
            return (u - 0.4 * c - 0.1 * t - 1.2) * (u - 0.4 * c - 0.1 * t - 1.2) + 0.3 * b * w + 0.1 * a + 0.05 * u * w

        def box3(t, a, b, c):
            return ((-1.0 - a, _no_lattice(a, 1.0 + b + 0.25 * t)),)
        if timed:
            sysd.dyn, sysd.cost, sysd.control_box = dyn3, cost3, box3
        else:
            sysd.dyn = lambda a, b, c, u, w: dyn3(0.0, a, b, c, u, w)
            sysd.cost = lambda a, b, c, u, w: cost3(0.0, a, b, c, u, w)
            sysd.control_box = lambda a, b, c: box3(0.0, a, b, c)
        sysd.perturb_laws = [NormalLaw(0, 0.2)]
        s = DPSolver(sysd, dtype=dtype)
        s.discretize_state(0, 1, shape[0], 0, 1, shape[1], -1, 1, shape[2])
        s.discretize_perturb(-0.4, 0.4, 3)
        _skew(s)
        s.control_steps = (0.05,)
        return s
    return make


def four_states(shape=(5, 4, 4, 3), mirror=False):
    """four states, two controls, NO perturbation: the box ((-1, 1), (-0.5 - b, 0.5 + a)) in steps (1 / 4, 1 / 8): 9 x 9
    to 9 x 25 controls.  The cost is least near u = 0.75, the last but one of its nine points: index >= 64 at most nodes"""
    def make():
        sysd = SysDescription((4, 2), name='four states')

        def dyn(a, b, c, e, u, v):
            u, v = _concrete(u), _concrete(v)
            return (0.8 * a + 0.1 * u, 0.7 * b + 0.1 * v + 0.05, 0.9 * c + 0.05 * u * v, 0.5 * e + 0.3 * a - 0.1 * v)
        sysd.dyn = dyn
        sysd.cost = lambda a, b, c, e, u, v: (u - 0.8) * (u - 0.8) + 0.5 * (v - 0.3 * e) * (v - 0.3 * e) + 0.1 * c * u + 0.2 * b

        def box(a, b, c, e):
            ra, rb = ((1.0 - a), (1.0 - b)) if mirror else (a, b)
            return ((-1.0, 1.0), (-0.5 - rb, _no_lattice(a, 0.5 + ra)))
        sysd.control_box = box
        s = DPSolver(sysd)
        s.discretize_state(0, 1, shape[0], 0, 1, shape[1], -1, 1, shape[2], -1, 1, shape[3])
        s.control_steps = (0.25, 0.125)
        return s
    return make


WILD_NAN_ABOVE = 0.6


def wild():
    """two states on a 6 x 5 grid of [0, 1]^2, 17 controls on (-1, 1).  The next state leaves the grid by up to ten grid
    lengths along axis 0 (lam about +-50); along axis 1 it is exactly the last grid point at u == 0, 10^300 (beyond the
    range of an int: the cast that gives cell 0) at u == -0.5 of the nodes with b == 0 and +inf at u == -0.25 of the node
    (0, 1); at the nodes with a > 0.7 (past the reference node of the relative form) the controls above 0.6 send axis 0 to
    NaN (cell 0, lam NaN)"""
    def make():
        sysd = SysDescription((2, 1, 1), name='wild next state')

        def dyn(a, b, u, w):
            u = _concrete(u)
            far = a + 10.0 * u + 0.0 * w
            b1 = b + 0.5 * w + 0.0 * u
            b1 = np.where(u == 0.0, 1.0, np.where((u == -0.5) & (b == 0.0), 1e300,
                                                  np.where((u == -0.25) & (b == 1.0) & (a == 0.0), np.inf, b1)))
            return (np.where((u > WILD_NAN_ABOVE) & (a > 0.7), np.nan, far), b1)
        sysd.dyn = dyn
        sysd.cost = lambda a, b, u, w: 0.2 * (u + 0.3) * (u + 0.3) + 0.1 * a * w + b
        sysd.control_box = lambda a, b: ((-1.0, 1.0),)
        sysd.perturb_laws = [NormalLaw(0, 0.2)]
        s = DPSolver(sysd)
        s.discretize_state(0, 1, 6, 0, 1, 5)
        s.discretize_perturb(-0.4, 0.4, 3)
        _skew(s)
        s.control_steps = (0.125,)
        return s
    return make


# ---------------------------------------------------------------------------------------------------------------------
# cost variants: NaN, +inf and -inf at chosen controls
# ---------------------------------------------------------------------------------------------------------------------
# name -> ([(control index, value)] put at every node that has the control, every how many nodes along axis 0 ALL
# controls get +inf, the one control that keeps its cost where all others get +inf).  numpy.argmin takes the first NaN,
# else the first of the smallest.
MARKS = {
    'inf nodes': ([], 2, None),                                       # index 0, J = +inf
    'nan 37 and 100': ([(37, np.nan), (100, np.nan)], 0, None),       # 37 wins: lane 36 meets its NaN on its second trip
    'nan past 64': ([(70, np.nan)], 0, None),                         # the only NaN on a second trip
    'minus inf twice': ([(69, -np.inf), (5, -np.inf)], 0, None),      # two trips: 5 wins
    # +inf at every control but number 70 (at all of them where the node has no such control): the one finite value of
    # a node comes on lane 6's second trip, against 63 lanes that hold +inf from their first
    'finite at 70 alone': ([], 0, 70),
}


def with_cost_marks(solver, name):
    """`solver` with the cost variant `name` (node-by-node calls only: the state is a scalar)"""
    marks, every, only = MARKS[name]
    base = solver.sys.cost
    d = len(solver.sys.state)
    W = solver._law_points()
    rows = set(np.asarray(solver.state_grid[0])[::every].tolist()) if every else ()
    lead = 0 if solver.sys.stationnary else 1

    def cost(*args):
        g = base(*args)
        tail = args[lead + d:]
        g = np.array(np.broadcast_to(np.asarray(g, dtype=float), np.broadcast(*tail).shape))
        per_control = g.reshape(-1, W) if W else g.reshape(-1, 1)
        for c, val in marks:
            if c < per_control.shape[0]:
                per_control[c] = val
        if float(args[lead]) in rows:
            per_control[:] = np.inf
        if only is not None:
            kept = per_control[only].copy() if only < per_control.shape[0] else None
            per_control[:] = np.inf
            if kept is not None:
                per_control[only] = kept
        return g
    # (SysDescription checks the positional names of a callable: the wrapper carries those of the cost it wraps)
    cost.__signature__ = inspect.signature(base)
    solver.sys.cost = cost
    return solver


# ---------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------
class Case(object):
    """name; make() -> solver; d, nu, W; U: (smallest, largest) number of controls of a node; trips; t_fin: steps of
    the finite horizon the case is swept through (0: a stationary case, value_iteration); ties: what the plan test asserts
    of the oracle's per-control vector at the node with the most controls, on the 'random' input --
    (first tied control, last tied control, winner); why: what the case is there for"""

    def __init__(self, name, make, d, nu, W, U, why, ties=None, t_fin=0, mirrored=None):
        self.name, self.make, self.d, self.nu, self.W, self.U = name, make, d, nu, W, tuple(U)
        self.trips, self.why, self.ties, self.t_fin, self.mirrored = trips(U[1]), why, ties, t_fin, mirrored

    def __repr__(self):
        return self.name

    def solver(self):
        return self.make()


CASES = [
    Case('line ragged', line(), 1, 1, 3, (1, 129),
         'U = 1, U on both sides of 64 and of 128, ragged cell_off, three lane trips; a tie of control 60 (lane 60, first '
         'trip) with 64 .. 68 (lanes 0 .. 4, second trip)', ties=(60, 68, 60), mirrored=line(mirror=True)),
    Case('line ties 0.75', line(centre=0.75), 1, 1, 3, (1, 129),
         'a tied run wholly on the second trip: the winner is past 64', ties=(92, 100, 92)),
    Case('line ties 0.99', line(centre=0.99), 1, 1, 3, (1, 129),
         'a tied run from the second trip into the third: the winner on lane 58, its rival 128 alone on lane 0',
         ties=(122, 128, 122)),
    Case('line last', line(centre=1.0, quant=64.0), 1, 1, 3, (1, 129),
         'the LAST control wins at every node: 128 where U = 129, the only control of the third trip',
         ties=(128, 128, 128)),
    Case('U = 63', constant_line(63), 1, 1, 3, (63, 63), 'one control short of a full wavefront', ties=(59, 62, 59)),
    Case('U = 64', constant_line(64), 1, 1, 3, (64, 64), 'exactly one trip of every lane', ties=(60, 63, 60)),
    Case('U = 65', constant_line(65), 1, 1, 3, (65, 65), 'one control on a second trip, tied with lanes 61 .. 63',
         ties=(61, 64, 61)),
    Case('two controls', two_controls(), 2, 2, 5, (1, 153),
         'unravel_index of the flat index on the dims of the node; a control that is a single point at some nodes',
         mirrored=two_controls(mirror=True)),
    Case('three states', three_states(), 3, 1, 3, (41, 81), 'k_tab_cells<3>'),
    Case('four states', four_states(), 4, 2, 0, (81, 225),
         'k_tab_cells<4> through default:, the W == 0 branch of k_tab_reduce, four lane trips',
         mirrored=four_states(mirror=True)),
    Case('time index', three_states((4, 4, 3), timed=True), 3, 1, 3, (41, 91),
         '(t_k,) + args with t_k != 0 in k_tab_cells<3>', t_fin=3),
    Case('wild next state', wild(), 2, 1, 3, (17, 17),
         'the cell clamp, the unclamped lam, the cast of a NaN and of a number beyond int to cell 0'),
]
BY_NAME = {c.name: c for c in CASES}
RUNS = [(c, v) for c in CASES for v in INPUTS]
MARK_RUNS = [(BY_NAME[c], m) for c in ('line ragged', 'two controls') for m in MARKS]
# the chunked sweeps: case -> chunk_cells of DPSolver._backup_tabulated (1: one node per call); every one is run on the
# case and on its mirrored twin
CHUNKS = {'line ragged': (1, 400, 1000), 'two controls': (1, 1500), 'four states': (1, 2000)}
FOUR_BYTE = ('line ragged', 'two controls')


# ---------------------------------------------------------------------------------------------------------------------
# what the plan test and the GPU test share
# ---------------------------------------------------------------------------------------------------------------------
def nodes_of(solver):
    """the grid nodes in sweep order (C order): a list of coordinate tuples"""
    return list(itertools.product(*solver.state_grid))


def lattice_sizes(solver, t_k=None):
    """controls U of every node in sweep order (int array)"""
    return np.array([int(np.prod(solver.control_grids(x, t_k)[1])) for x in nodes_of(solver)], dtype=np.int64)


def batches(cells, chunk_cells):
    """the flush rule of DPSolver._backup_tabulated, restated: a node joins the batch, and the batch goes to the device
    once it holds `chunk_cells` cells or more; the rest at the end.  cells: lattice cells per node (U * max(W, 1)).
    Returns [(nodes, cells)] per sdp_tab_backup call."""
    out, n, c = [], 0, 0
    for k in cells:
        n, c = n + 1, c + int(k)
        if c >= chunk_cells:
            out.append((n, c))
            n, c = 0, 0
    if n:
        out.append((n, c))
    return out


def chunked_runs(case):
    """[(chunk_cells, mirrored?, maker)] of the chunked sweeps of a case of CHUNKS"""
    return [(k, mirrored, case.mirrored if mirrored else case.make)
            for k in CHUNKS[case.name] for mirrored in (False, True)]


def alternating(U):
    """an order of the nodes that alternates small and large lattices: smallest, largest, second smallest, ..."""
    by_size = np.argsort(np.asarray(U), kind='stable')
    lo, hi, order = 0, len(by_size) - 1, []
    while lo <= hi:
        order.append(int(by_size[lo]))
        if hi != lo:
            order.append(int(by_size[hi]))
        lo, hi = lo + 1, hi - 1
    return order


def oracle_sweep(solver, V, t_k=None):
    """(J, policy, index) of the numpy oracle on ALL nodes"""
    spec = vi_numpy.Spec.from_solver(solver)
    with np.errstate(all='ignore'):
        J, pol, idx, _ = vi_numpy.value_iteration(spec, V, t_k=t_k)
    return J, pol, idx


def off_lattice_policy(solver, seed=3):
    """a policy no sweep returns (what tests/policies.py calls 'smooth' and 'outside' in one): per control a wave of the
    state between the box ends and, at every fifth node, up to a box width outside"""
    dims = solver._state_grid_shape
    nu = len(solver.sys.control)
    pol = np.empty(dims + (nu,))
    rng = np.random.default_rng(seed)
    for n, (ind, x) in enumerate(zip(itertools.product(*[range(k) for k in dims]), nodes_of(solver))):
        box = solver.sys.control_box(*x, **solver.sys.params)
        for c, (lo, hi) in enumerate(box):
            z = 0.5 + 0.45 * np.sin(3.0 * n / len(dims) + c)
            if n % 5 == 0:
                z = rng.uniform(-1., 2.)
            pol[ind + (c,)] = lo + (hi - lo) * z + 0.01
    return pol


def lookahead_states(solver, B, seed=0):
    """(B, d) states: grid nodes, points between the nodes, points outside the grid and -- every seventh -- a state
    whose box has no lattice (NAN_A, INF_A, BIG_A on axis 0, in turn)"""
    grid = [np.asarray(g, dtype=float) for g in solver.state_grid]
    d = len(grid)
    rng = np.random.default_rng(seed + B)
    lo, hi = np.array([g[0] for g in grid]), np.array([g[-1] for g in grid])
    nodes = np.array(nodes_of(solver))
    x = np.empty((B, d))
    for b in range(B):
        kind = b % 7
        if kind in (0, 1, 2):
            x[b] = nodes[rng.integers(len(nodes))]
        elif kind in (3, 4):
            x[b] = lo + (hi - lo) * rng.random(d)
        elif kind == 5:
            x[b] = lo + (hi - lo) * rng.random(d)
            k = (b // 7) % d                                   # outside the grid along one axis, on either side in turn
            x[b, k] = hi[k] + 0.2 * (hi[k] - lo[k]) * rng.random() if (b // 7) % 2 else lo[k] - 0.2 * (hi[k] - lo[k]) * rng.random()
        else:
            x[b] = lo + (hi - lo) * rng.random(d)
            x[b, 0] = (NAN_A, INF_A, BIG_A)[(b // 7) % 3]
    return x


def lookahead_rule(solver, J_next, x, t_k=None):
    """What DPSolver.lookahead gives for a model that does not trace, restated (stodynprog_amd/lookahead.py is this in
    8-byte reals): the state rounded ONCE to the solver's reals, the lattice rule of `lookahead.lattice` with its ONE
    rounding of the box ends to those reals, then -- whatever the reals -- the points, the callables, the oracle's
    interpolation and the sequential expectation in float64, first-occurrence argmin, and ONE rounding of J and u to
    the solver's reals.  No lattice: NaN, NaN, -1.

    How far this reference is independent: the lattice and the control points are `lookahead.lattice` and
    `lookahead.control_points`, the very functions the driver under test calls, so only the interpolation (the
    oracle's), the expectation and the argmin are a second opinion.  The lattice rule itself is checked where the
    tests compare a grid node with the oracle's sweep, which takes it from `vi_numpy.control_grids`; at states off the
    grid it has no check but the definition's own tests (tests/test_lookahead_definition.py)."""
    sd = solver.sys
    dt = np.dtype(solver.dtype)
    x = np.atleast_2d(np.asarray(x, dtype=float)).astype(dt).astype(float)
    B, nu = x.shape[0], len(sd.control)
    lo, hi, n = la.lattice(sd.control_box, sd.params, solver.control_steps, x, t_k, dt)
    lo, hi = lo.astype(float), hi.astype(float)
    interp = vi_numpy.Interp(*[np.asarray(g, dtype=float) for g in solver.state_grid])
    interp.set_values(np.asarray(J_next, dtype=float))
    w_args, proba, W = solver._flat_law()
    J, u, idx = np.full(B, np.nan), np.full((B, nu), np.nan), np.full(B, -1, dtype=np.int32)
    lead = () if t_k is None else (t_k,)
    with np.errstate(all='ignore'):
        for b in range(B):
            if n[0, b] == 0:
                continue
            dims = tuple(int(v) for v in n[:, b])
            grids = [la.control_points(lo[c, b], hi[c, b], n[c, b]) for c in range(nu)]
            mesh = [g.reshape((1,) * c + (-1,) + (1,) * (nu - c)) for c, g in enumerate(grids)]
            args = lead + tuple(x[b]) + tuple(mesh) + tuple(w_args)
            x_next = sd.dyn(*args, **sd.params)
            cell = sd.cost(*args, **sd.params) + interp(*x_next)
            full = np.broadcast_to(cell, dims + ((W,) if W else (1,)))
            if W:
                acc = np.zeros(dims)
                for j in range(W):
                    acc = acc + full[..., j] * proba[j]
            else:
                acc = np.array(full[..., 0])
            flat = int(acc.argmin())
            ind = np.unravel_index(flat, dims)
            J[b], idx[b] = acc[ind], flat
            u[b] = [grids[c][ind[c]] for c in range(nu)]
    return J.astype(dt), u.astype(dt), idx
