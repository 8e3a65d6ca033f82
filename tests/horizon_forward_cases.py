"""The rows of tests/test_gpu_horizon_forward.py (GPU) and tests/test_horizon_forward_plan.py (CPU) as a table (test
infrastructure, like tests/forward_cases.py; not a test file): models and TIME-INDEXED policies whose chain of
transition operators (DPSolver.horizon_operator, stodynprog_amd/forward.py: chain_entries, propagate) is built on the
device in one call and compared with the definition.  The shapes are the smallest that reach each path of kernel
sdp_transitions_h (csrc/sdp_trans_horizon_kernel.h: a tile of 256 >> d nodes of one step is a workgroup):

  line            horizon_cases.line(): d = 1, 65 nodes, under one tile of 128; symbolic time, the model drifts off the grid
  line_ragged     the same model on 129 + 5 nodes: a ragged second tile
  storage         horizon_cases.storage(n_E=7, n_P=5): d = 2, 35 nodes, under one tile of 64; symbolic time
  storage_ragged  the same at 21 x 13 = 273 nodes: 4 tiles and 17 nodes
  storage_data    horizon_cases.storage(data=True): constants looked up as data[k], a row per step (steps equal to a
                  literal, 0.0 and -0.0 among them)
  reservoirs      horizon_cases.reservoirs() cut to 5 x 4 x 3 nodes: d = 3, two controls, a ragged second tile of 32
  two_variables   the `horizon` case of tests/multi_perturb.py: SDP_NW = 2, data[k], 4 steps
  deterministic   models.pv_storage(T=6, N_E=9, u_step=0.05): W = 1, data[k]
  inventory       models.inventory: a STATIONARY model under a time-indexed policy, 4 steps of bellman_recursion
  untraceable     forward_cases' storage model behind a callable the tracer refuses: the host path

Policies are smooth functions of the state (forward_cases.wave_policy), another one at every step; `inventory` takes what
bellman_recursion returns.  `long_line(cus)` is the d = 1 line model past the launch caps of the build and of the push."""
import numpy as np

import forward_cases as fc
import horizon_cases as hc
import multi_perturb as mp
from stodynprog_amd import models

DTYPES = fc.DTYPES
THREADS = 256                    # SDP_TRANSH_THREADS
PUSH_LONG, PUSH_WIDE = 8, 256    # SDP_PUSH_LONG, SDP_PUSH_WIDE of csrc/sdp_hip.hip
BUILD_PER_CU = 8                 # workgroups per compute unit of the build's and the short rows' launches
GROUP_PER_CU = 64                # .. of the long rows' launches


def tile(d):
    """nodes of a workgroup's tile: SDP_TRANSH_TILE"""
    return THREADS >> d


def units(n_steps, S, d):
    """(step, tile) units of one launch of sdp_transitions_h"""
    return n_steps * (-(-S // tile(d)))


def build_blocks(n_steps, S, d, cus):
    """the grid of sdp_chainop_create, restated"""
    return min(units(n_steps, S, d), cus * BUILD_PER_CU)


def push_blocks(n, per, cap, B):
    """chain_blocks of csrc/sdp_hip.hip, restated: workgroups of one launch over n rows, `per` to a workgroup, for B
    vectors on the grid's second dimension"""
    return max(1, min(-(-n // per), cap // B))


class Row(object):
    """name; make() -> float64 solver; bounds of the policy per control; T steps; time_index: how the definition hands
    the time index to the callables; host: the horizon kernels do not run the model; t0s: the time indices operators are
    built at, solo ones included (each plans its own unit where the control lattice changes with the time index)"""

    def __init__(self, name, make, bounds, T, time_index='real', host=False, t0s=(0,)):
        self.name, self._make, self.bounds, self.T, self.time_index, self.host, self.t0s = (
            name, make, bounds, T, time_index, host, tuple(t0s))

    def __repr__(self):
        return self.name

    def solver(self, dtype=np.float64):
        return fc.as_dtype(self._make(), dtype)

    def policy(self, solver):
        """(T,) + dims + (nu,): a smooth policy per step"""
        return np.stack([fc.wave_policy(solver, self.bounds, seed=k) for k in range(self.T)])


def _line(n=65):
    s = hc.line()
    s.discretize_state(-4, 4, n)
    return s


def _reservoirs():
    s = hc.reservoirs()
    s.discretize_state(0., 2., 5, 0., 2., 4, -0.4, 0.8, 3)
    return s


# The two models below look their constants up in a float64 ARRAY (`d[k]` is a numpy.float64).  Next to 4-byte arrays such
# a scalar makes numpy compute in 8-byte reals, so the definition in 4-byte reals would not round what the kernels round
# (their constants are lifted and rounded once).  The rows take the same callables with the constants as Python floats:
# bit for bit the same model in 8-byte reals (tests/test_horizon_forward_plan.py checks that), and one whose callables
# compute in the reals of their arguments.

def _storage_data():
    """horizon_cases.storage(data=True) with TIME_DATA[k] read from the tuple"""
    s = hc.storage(data=True)
    d = hc.TIME_DATA
    s.sys.dyn = lambda k, e, p, u, w: ((e + d[k]) + (1.1 * u - 0.02 * abs(u)), (0.75 * p + 0.05 * k) + w)
    s.sys.cost = lambda k, e, p, u, w: 0.01 * e + (((p - u) * (p - u) + 0.15 * u * u) + d[k] * u)
    return s


def _pv():
    """models.pv_storage(T=6, N_E=9, u_step=0.05) with the production of step k a Python float"""
    s = models.pv_storage(T=6, N_E=9, u_step=0.05)[1]
    prod = [float(x) for x in s.P_prod_data]

    def cost(k, E_sto, P_sto):
        P_grid = prod[k] - P_sto
        over = np.where(P_grid > 0.4, P_grid - 0.4, 0)
        neg = np.where(P_grid < 0, P_grid, 0)
        return over ** 2 + neg ** 2 + 0 * P_sto ** 2
    s.sys.cost = cost
    return s


ROWS = [
    Row('line', _line, [(-1., 1.)], hc.T, t0s=(0, 1, 2)),
    Row('line_ragged', lambda: _line(129 + 5), [(-1., 1.)], hc.T),
    Row('storage', lambda: hc.storage(n_E=7, n_P=5), [(-1., 1.)], hc.T, t0s=(0, 1, 2, 4)),
    Row('storage_ragged', hc.storage, [(-1., 1.)], hc.T, t0s=range(hc.T)),
    Row('storage_data', _storage_data, [(-1., 1.)], hc.T, time_index='int', t0s=range(hc.T)),
    Row('reservoirs', _reservoirs, [(0., 1.), (0., 1.)], hc.T),
    Row('two_variables', lambda: mp.BY_NAME['horizon'].solver(), [(-1., 1.)], mp.HORIZON, time_index='int'),
    Row('deterministic', _pv, [(-1., 1.)], 6, time_index='int', t0s=range(6)),
    Row('inventory', lambda: models.inventory()[1], [(0., 10.)], 4),
    Row('untraceable', fc.BY_NAME['untraceable'].solver, [(-4., 4.), (0., 0.)], 3, host=True),
]
BY_NAME = {r.name: r for r in ROWS}
DEVICE_ROWS = [r for r in ROWS if not r.host]


def long_line_nodes(cus, B=2):
    """the smallest grid of the line model, plus a ragged tile, on which a step's rows are more than one trip of the
    push's grid for B vectors covers -- and two steps of it more (step, tile) units than one trip of the build's"""
    return (cus * BUILD_PER_CU // B) * THREADS + 129 + 5


def long_line(cus, B=2):
    """two steps of the line model on long_line_nodes(cus, B) nodes.  Controls below zero: the model drifts downwards, so
    the rows at the upper end of the grid -- those of the push's second trip -- are short or empty (the lane path), the
    others hold 8 entries or more (a group of lanes each) and the two at the ends far more than SDP_PUSH_WIDE (a wave)"""
    return Row('long_line', lambda: _line(long_line_nodes(cus, B)), [(-1., 0.)], 2)


def plan_of(solver, t_k=None):
    """the plan of a row's solver (a time-dependent one: traced at its first step)"""
    if solver.sys.stationnary:
        return solver._kernel_plan()
    return solver._kernel_plan(t_k, solver._trace_now(t_k))


def unit_sources():
    """every generated unit the GPU tests run: each device row in both reals at the first steps it is built at, and the
    long line as an MI355X's 256 compute units size it"""
    out = []
    for dt in DTYPES.values():
        for row in DEVICE_ROWS:
            s = row.solver(dt)
            out += [plan_of(s, t0)['source'] for t0 in row.t0s]
    out.append(plan_of(long_line(256).solver(), 0)['source'])
    return list(dict.fromkeys(out))
