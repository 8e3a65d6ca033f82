"""Test infrastructure of the one-step lookahead at arbitrary states (DPSolver.lookahead / simulate_lookahead,
stodynprog_amd/lookahead.py, csrc/sdp_lookahead_kernel.h): small models with their state batches, the oracle's answer
at a batch, and the oracle chained step by step into a closed loop (in the manner of horizon_sim.simulate_indexed).

The yardstick is oracle/vi_numpy.py: `backup_node` (8-byte reals) and `backup_node_real` (4-byte reals) take any
state, not only nodes.  A 4-byte problem rounds its states once; the oracle is then asked at the rounded state
widened to float64, which is where the kernel evaluates the box.

States of a case: every node of the grid, cell interiors, points on the last node of an axis, points up to 20 %
outside each side, and per model the states `extra` names (a width below 0.1 step: the midpoint rule; hi < lo).
"""
import itertools

import numpy as np

import horizon_cases as hc
import horizon_sim as hs
from oracle import vi_numpy
from policies import as_dtype
from stodynprog_amd import SysDescription, DPSolver, models
from stodynprog_amd.models import NormalLaw

T_SIM = 6


# ----------------------------------------------------------------------------------------------------------------------
# models

def lanes_model(L, dtype=np.float64):
    """one state on [0, 1], one control on (-1, -1 + a + b x) with step 1: the lattice of every node has at most L
    points (and more than L / 2 where L > 1), so the unit has SDP_LANES = L; off the grid it has 1, L - 1, L and
    L + 1 points (`LANE_STATES`), a width below 0.1 step and a negative width"""
    a, b = {1: (0.02, 0.06), 8: (4.5, 2.5), 64: (36., 20.)}[L]
    s = SysDescription((1, 1, 1), name='lanes {}'.format(L))
    s.dyn = lambda x, u, w: (0.9 * x + 0.01 * u + w,)
    s.cost = lambda x, u, w: (0.02 * u - x) * (0.02 * u - x) + 0.001 * u
    s.control_box = lambda x: ((-1.0, (-1.0 + a) + b * x),)
    s.perturb_laws = [NormalLaw(0, 0.1)]
    solver = DPSolver(s, dtype=dtype)
    solver.discretize_state(0, 1, 9)
    solver.discretize_perturb(-0.3, 0.3, 3)
    solver.control_steps = (1.,)
    return solver


# states of lanes_model(L) whose lattice has 1 (midpoint rule), L - 1, L, L + 1 points, and one with hi < lo
LANE_STATES = {1: (0.5, 1.5, -2.0),                         # 1 point; 2 = L + 1 points; a negative width
               8: (-1.78, 0.5, 0.9, 1.2, -2.5),             # 1, 7, 8, 9 points; a negative width
               64: (-1.7975, 1.275, 1.325, 1.375, -2.5)}    # 1, 63, 64, 65 points; a negative width
LANE_TOTALS = {1: (1, 2, 1), 8: (1, 7, 8, 9, 1), 64: (1, 63, 64, 65, 1)}


def deterministic():
    s = SysDescription((1, 1, 0), name='deterministic')
    s.dyn = lambda x, u: (0.8 * x + 0.3 * u,)
    s.cost = lambda x, u: (x - 0.4) * (x - 0.4) + 0.1 * u * u
    s.control_box = lambda x: ((-0.5 - 0.25 * x, 0.5),)
    solver = DPSolver(s)
    solver.discretize_state(-1, 1, 11)
    solver.control_steps = (0.125,)
    return solver


def symbolic_time():
    """time-dependent: the box and the drift use the time index as a number"""
    s = SysDescription((2, 1, 1), stationnary=False, name='symbolic time')
    s.dyn = lambda k, e, p, u, w: ((e + 0.15 * (k - 3)) + (1.1 * u - 0.02 * abs(u)), (0.75 * p + 0.05 * k) + w)
    s.cost = lambda k, e, p, u, w: 0.01 * e + (((p - u) * (p - u) + 0.15 * u * u) + (0.1 * k - 0.35) * u)
    s.control_box = lambda k, e, p: ((np.maximum(-e, -1.0), (0.25 + 0.125 * k) + 0.1 * e),)
    s.perturb_laws = [NormalLaw(0, 0.3)]
    solver = DPSolver(s)
    solver.discretize_state(0, 4, 7, -2, 2, 5)
    solver.discretize_perturb(-0.9, 0.9, 3)
    solver.control_steps = (0.125,)
    return solver


def data_time():
    """time-dependent: the box (and the model) look data up with the time index, `data[k]` -- the host path"""
    return hc.storage(n_E=7, n_P=5, n_w=3, data=True)


def branching_box():
    """a Python `if` on the state in control_box: the tracer merges the two paths into a select"""
    s = SysDescription((1, 1, 1), name='branching box')
    s.dyn = lambda x, u, w: (0.9 * x + 0.2 * u + w,)
    s.cost = lambda x, u, w: (x - 0.3) * (x - 0.3) + 0.1 * u * u

    def box(x):
        if x > 0.5:
            return ((-1.0, 0.25 * x),)
        return ((-0.5, 1.0 - x),)
    s.control_box = box
    s.perturb_laws = [NormalLaw(0, 0.1)]
    solver = DPSolver(s)
    solver.discretize_state(0, 1, 9)
    solver.discretize_perturb(-0.3, 0.3, 3)
    solver.control_steps = (0.125,)
    return solver


def untraceable():
    """a dynamics that needs a concrete array (np.shape): the tabulated host path"""
    solver = branching_box()

    def dyn(x, u, w):
        shape = np.shape(u)
        return (0.9 * x + 0.2 * np.asarray(u).reshape(shape) + w,)
    solver.sys.dyn = dyn
    return solver


def flat_cost():
    """neither the cost nor the next state sees the control: every lattice point has the same value, idx == 0"""
    s = SysDescription((1, 1, 1), name='flat')
    s.dyn = lambda x, u, w: (0.9 * x + w + 0.0 * u,)
    s.cost = lambda x, u, w: x * x + 0.0 * u
    s.control_box = lambda x: ((-1.0, 1.0 + x),)
    s.perturb_laws = [NormalLaw(0, 0.1)]
    solver = DPSolver(s)
    solver.discretize_state(0, 1, 9)
    solver.discretize_perturb(-0.3, 0.3, 3)
    solver.control_steps = (0.125,)
    return solver


NAN_STATE = 0.25             # (the same number in 4-byte reals)


def nan_box(dtype=np.float64):
    """the upper end is NaN at the one state x == NAN_STATE (0 * inf) and 1 everywhere else"""
    s = SysDescription((1, 1, 1), name='nan box')
    s.dyn = lambda x, u, w: (0.9 * x + 0.2 * u + w,)
    s.cost = lambda x, u, w: (x - 0.3) * (x - 0.3) + 0.1 * u * u
    s.control_box = lambda x: ((-1.0, 1.0 + 0.0 * (1.0 / (x - NAN_STATE))),)
    s.perturb_laws = [NormalLaw(0, 0.1)]
    solver = DPSolver(s, dtype=dtype)
    solver.discretize_state(0, 1, 10)
    solver.discretize_perturb(-0.3, 0.3, 3)
    solver.control_steps = (0.25,)
    return solver


class Case(object):
    """name, how to build the solver, what lookahead_path simulate_lookahead must report, the time indices the
    lookahead is checked at (None: stationary), more states, the batch sizes of the lane count"""

    def __init__(self, name, make, path='device', times=(None,), extra=(), batches=(1, 2, 3), int_time=False, box='device'):
        self.name, self.make, self.path, self.times = name, make, path, tuple(times)
        self.extra, self.batches, self.int_time, self.box = tuple(extra), tuple(batches), int_time, box

    def __repr__(self):
        return self.name

    def solver(self):
        return self.make()


def _col(values):
    return [(v,) for v in values]


B_1, B_8, B_64 = (1, 63, 64, 65), (7, 8, 9), (1, 2, 3)

CASES = [
    Case('inventory', lambda: models.inventory()[1], batches=B_8),
    # (the box is min / max of the state; the second control is a single point)
    Case('storage_ar1', lambda: models.storage_ar1(n_E=11, n_P=9, n_w=5, steps=(0.25, 0.1))[1], batches=B_64,
         extra=[(0.005, 0.3), (9.995, -0.2), (-0.5, 0.1), (10.5, 0.)]),
    # (3-D; the lattice falls to 1 point near the ends of the stock axis)
    Case('searev', lambda: models.searev(n_E=5, n_S=7, n_A=7, n_w=3, step=0.05)[1], batches=B_64,
         extra=[(0.0005, 0.1, 0.1), (9.9995, -0.1, 0.2), (-0.3, 0., 0.), (10.4, 0.1, -0.1)]),
    # (two controls, 81 points: a second trip of 17 lanes)
    Case('two_reservoirs', lambda: models.two_reservoirs(n_a=6, n_b=6, n_y=4, n_w=3)[1], batches=B_64),
    # (two perturbation variables)
    Case('two_inflows', lambda: models.two_inflows(n_a=5, n_b=5, n_y=4, n_w=(3, 2))[1], batches=B_64),
    Case('deterministic', deterministic, batches=B_8),
    Case('symbolic time', symbolic_time, times=(0, 5), batches=B_8),
    Case('data[k]', data_time, path='host', times=(1, 6), batches=B_64, int_time=True, box='host'),
    Case('branching box', branching_box, batches=B_8),
    Case('untraceable', untraceable, path='host', batches=B_8, box='host'),
    Case('lanes 1', lambda: lanes_model(1), batches=B_1, extra=_col(LANE_STATES[1])),
    Case('lanes 8', lambda: lanes_model(8), batches=B_8, extra=_col(LANE_STATES[8])),
    Case('lanes 64', lambda: lanes_model(64), batches=B_64, extra=_col(LANE_STATES[64])),
    Case('flat', flat_cost, batches=B_8),
    # 4-byte twins
    Case('searev f32', lambda: as_dtype(models.searev(n_E=5, n_S=7, n_A=7, n_w=3, step=0.05)[1], np.float32), batches=B_64,
         extra=[(0.0005, 0.1, 0.1), (9.9995, -0.1, 0.2), (-0.3, 0., 0.), (10.4, 0.1, -0.1)]),
    Case('lanes 8 f32', lambda: lanes_model(8, np.float32), batches=B_8, extra=_col(LANE_STATES[8])),
]
BY_NAME = {c.name: c for c in CASES}
TRACED = [c for c in CASES if c.name != 'untraceable']


# ----------------------------------------------------------------------------------------------------------------------
# states and inputs

def states(case, solver, seed=0):
    """(B, d) float64: every node, cell interiors, points on the last node of an axis, points up to 20 % outside each
    side of every axis, and the case's own"""
    grid = [np.asarray(g, dtype=float) for g in solver.state_grid]
    d = len(grid)
    rng = np.random.default_rng(100 + seed + d)
    lo = np.array([g[0] for g in grid])
    hi = np.array([g[-1] for g in grid])
    out = [np.array(list(itertools.product(*grid)))]
    out.append(lo + (hi - lo) * rng.random((12, d)))                                 # cell interiors
    last = lo + (hi - lo) * rng.random((2 * d, d))
    for k in range(d):
        last[2 * k:2 * k + 2, k] = hi[k]                                             # on the last node of axis k
    out.append(last)
    outside = lo + (hi - lo) * rng.random((4 * d, d))
    for k in range(d):
        outside[4 * k:4 * k + 2, k] = lo[k] - (hi[k] - lo[k]) * 0.2 * rng.random(2)
        outside[4 * k + 2:4 * k + 4, k] = hi[k] + (hi[k] - lo[k]) * 0.2 * rng.random(2)
    out.append(outside)
    if case.extra:
        out.append(np.array(case.extra, dtype=float).reshape(-1, d))
    return np.concatenate(out)


def n_nodes(solver):
    return int(np.prod([len(g) for g in solver.state_grid]))


def cost_to_go(solver, seed=0):
    """a smooth cost-to-go with a seeded ripple on the state grid (float64)"""
    shape = tuple(len(g) for g in solver.state_grid)
    rng = np.random.default_rng(7 + seed)
    mesh = np.meshgrid(*[np.linspace(-1., 1., n) for n in shape], indexing='ij')
    J = sum((k + 1) * 0.3 * m * m for k, m in enumerate(mesh)) + 0.05 * rng.standard_normal(shape)
    return np.ascontiguousarray(J)


# ----------------------------------------------------------------------------------------------------------------------
# the oracle

def spec_of(case, solver):
    return hs.spec_of(solver, int_time=case.int_time)


def oracle_interp(solver, spec, J_next):
    dt = np.dtype(solver.dtype)
    if dt == np.float64:
        interp = vi_numpy.Interp(*spec.state_grid)
        interp.set_values(np.asarray(J_next, dtype=float))
        return interp
    return vi_numpy.InterpReal(spec, np.asarray(J_next).astype(dt.type), dt.type)


def oracle_lookahead(solver, spec, J_next, x, t_k=None):
    """(J_opt (B,), u_opt (B, nu), idx (B,)) of the oracle's backup at every state of x (B, d): `backup_node` for
    8-byte reals, `backup_node_real` for 4-byte reals at the state rounded once and widened"""
    dt = np.dtype(solver.dtype)
    interp = oracle_interp(solver, spec, J_next)
    x = np.atleast_2d(np.asarray(x, dtype=float)).astype(dt).astype(float)
    nu = len(spec.control_steps)
    J = np.zeros(len(x), dtype=dt)
    u = np.zeros((len(x), nu), dtype=dt)
    idx = np.zeros(len(x), dtype=np.int32)
    with np.errstate(all='ignore'):
        for b, x_k in enumerate(x):
            if dt == np.float64:
                J[b], u[b], idx[b], _ = vi_numpy.backup_node(spec, tuple(x_k), interp, t_k)
            else:
                J[b], u[b], idx[b], _ = vi_numpy.backup_node_real(spec, tuple(x_k), interp, t_k)
    return J, u, idx


def oracle_closed_loop(solver, spec, J_next, x0, w, T, t0=0):
    """(x (T+1, B, d), u (T, B, nu), g (T, B), q (T, B)) of the oracle chained step by step: `backup_node` at the
    carried state, then spec.dyn / spec.cost at the optimal control, one element per trajectory, in the problem's
    reals.  J_next: one cost-to-go, or (T_J,) + dims (step k reads J_next[t0 + k]).  w: (T, B), for several
    perturbation variables indices into the flat law (`multi_perturb.flat_spec`), or None."""
    dt = np.dtype(solver.dtype)
    shape = tuple(len(g) for g in solver.state_grid)
    J_next = np.asarray(J_next)
    timed = J_next.ndim == len(shape) + 1
    x0 = np.atleast_2d(np.asarray(x0, dtype=float))
    B, d = x0.shape
    nu = len(spec.control_steps)
    x = np.zeros((T + 1, B, d), dtype=dt)
    u = np.zeros((T, B, nu), dtype=dt)
    g = np.zeros((T, B), dtype=dt)
    q = np.zeros((T, B), dtype=dt)
    x[0] = x0.astype(dt)
    with np.errstate(all='ignore'):
        for k in range(T):
            t_k = None if spec.stationnary else t0 + k
            q[k], u[k], _ = oracle_lookahead(solver, spec, J_next[t0 + k] if timed else J_next, x[k], t_k)
            args = tuple(x[k, :, i] for i in range(d)) + tuple(u[k, :, c] for c in range(nu))
            if w is not None:
                args = args + (np.asarray(w[k], dtype=dt),)
            if t_k is not None:
                args = ((t_k if dt == np.float64 else dt.type(t_k)),) + args
            xn = spec.dyn(*args, **spec.params)
            gk = spec.cost(*args, **spec.params)
            for i in range(d):
                x[k + 1, :, i] = xn[i]
            g[k] = gk
    return x, u, g, q


def draws(solver, T, B, seed=3):
    """(w for simulate_lookahead, w for the oracle's closed loop): (T, B) values of the solver's perturbation grid;
    several variables: (T, m, B) values and (T, B) indices into the flat law; (None, None) for a deterministic system"""
    m = len(solver.perturb_grid)
    if m == 0:
        return None, None
    rng = np.random.default_rng(seed)
    if m == 1:
        grid = np.asarray(solver.perturb_grid[0], dtype=float)
        w = grid[rng.integers(0, len(grid), size=(T, B))]
        return w, w
    from stodynprog_amd import perturb
    wtab, P = perturb.product_law(solver.perturb_grid, solver.perturb_proba)
    j = rng.integers(0, len(P), size=(T, B))
    return np.ascontiguousarray(np.moveaxis(wtab[:, j], 0, 1)), j.astype(float)


def start_states(case, solver, B, seed=5):
    """B start states inside the grid (the first one a node)"""
    grid = [np.asarray(g, dtype=float) for g in solver.state_grid]
    rng = np.random.default_rng(seed)
    lo = np.array([g[0] for g in grid])
    hi = np.array([g[-1] for g in grid])
    x0 = lo + (hi - lo) * (0.2 + 0.6 * rng.random((B, len(grid))))
    x0[0] = [g[len(g) // 2] for g in grid]
    return x0


# ----------------------------------------------------------------------------------------------------------------------
# batches past the launch caps of sdp_lookahead and sdp_simulate_lookahead (csrc/sdp_hip.hip, restated)

def cap_batch(lanes, cus):
    """the smallest batch shape past both caps: cus * 8 workgroups of (64 / lanes) * 4 states, and a ragged tile more"""
    return cus * 8 * (64 // lanes) * 4 + 33


def lookahead_grid(B, lanes, cus):
    """sdp_problem_lookahead launches sweep_blocks(p, B) workgroups: (tiles, workgroups)"""
    tile = (64 // lanes) * 4
    tiles = -(-B // tile)
    return tiles, max(8, -(-min(cus * 8, tiles) // 8) * 8)


def lookahead_later_trips(B, lanes, cus):
    """the rows of a batch that kernel sdp_lookahead reaches after a workgroup's first tile: XCD x walks the x-th
    contiguous eighth of the tiles with a stride of workgroups / 8"""
    tile = (64 // lanes) * 4
    tiles, blocks = lookahead_grid(B, lanes, cus)
    per_xcd, stride = -(-tiles // 8), blocks // 8
    rows = []
    for xcd in range(8):
        for t in range(xcd * per_xcd + stride, min((xcd + 1) * per_xcd, tiles)):
            rows += range(t * tile, min((t + 1) * tile, B))
    return np.array(rows, dtype=np.int64)


def simulate_grid(B, lanes, cus):
    """sdp_problem_simulate_lookahead: (tiles, workgroups); workgroup b takes the tiles b, b + workgroups, .."""
    tiles = -(-B // ((64 // lanes) * 4))
    return tiles, min(tiles, cus * 8)


def repeated_rows(B, distinct, seed=11):
    """which of `distinct` inputs every row of a batch of B carries, drawn at random: the definition is a function of a
    row's own inputs, so its answer on the distinct inputs, gathered, is its answer on the whole batch"""
    pick = np.random.default_rng(seed).integers(0, distinct, size=B)
    pick[:distinct] = np.arange(distinct)
    return pick


def unit_source(solver, t_k=None):
    """the generated source of the solver's lookahead unit (no GPU)"""
    from stodynprog_amd import codegen
    from stodynprog_amd.trace import TraceError
    box_t = None if solver.sys.stationnary else t_k
    model = solver._trace_now(t_k)
    tb = solver._trace_box_now(box_t)
    box = tb if (not isinstance(tb, TraceError) and tb.t_value is None) else None
    return codegen.lookahead_unit(model, solver.dtype, solver._box_plan(box_t)['lanes'], box)


def unit_sources():
    """the lookahead units of every traced case (the build compiles them ahead)"""
    out = []
    for case in TRACED + [Case('nan box', nan_box)]:
        s = case.solver()
        if case.name == 'data[k]':
            out += [unit_source(s, t) for t in range(hc.T)]
        else:
            out.append(unit_source(s, case.times[0]))
        for kernel in ('generic', 'auto'):
            if s.sys.stationnary and case.name in VI_CASES:
                s2 = case.solver()
                s2.kernel = kernel
                out.append(s2._kernel_plan()['source'])
    return out


# cases whose nodes are also compared with value_iteration of the same solver
VI_CASES = ('inventory', 'storage_ar1', 'searev', 'two_reservoirs', 'two_inflows', 'lanes 8', 'searev f32')
