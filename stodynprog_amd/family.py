"""A family of same-shaped problems solved in one device call: `SolverFamily`.

The reference's own studies are loops over small problems -- a range of storage capacities, of rated powers, of
correlations -- and a grid of a few thousand nodes fills a small fraction of the GPU: a loop of solo calls pays the
launch and call costs once per member and sweep.  A SolverFamily takes P `DPSolver` objects, each set up exactly as
for a solo call, and runs their sweeps together: one launch of kernel `sdp_family_sweep`
(csrc/sdp_family_kernel.h) backs up every member.

`eval_policy` and `policy_iteration` evaluate the members' policies together as well (csrc/sdp_family_policy_kernel.h):
one launch of `sdp_family_evalpol` per step, or all steps of a member in one workgroup with its values in LDS
(`sdp_family_evalpol_resident`); the improvement of policy iteration is the family sweep.

`monte_carlo` scores the members' policies in closed loop together (csrc/sdp_family_mc_kernel.h): one launch of
`sdp_family_montecarlo` per cut of the steps runs every member's trajectories, a tile of 256 of one member a workgroup;
with one seed the members see the same draws (common random numbers, `FamilyMonteCarloResult.paired`).

`lookahead` and `monte_carlo_lookahead` decide at arbitrary states, and score the members in closed loop under those
decisions -- the controller that would run -- together (csrc/sdp_family_lookahead_kernel.h): kernels
`sdp_family_lookahead` and `sdp_family_montecarlo_lookahead`, a tile of (64 / lanes) x 4 states of one member a
workgroup, every lattice made on the device from the member's traced control_box with its constants lifted.

`simulate` and `monte_carlo_horizon` run the members' policies forward over a horizon together -- the policies
`bellman_recursion` returns, time-indexed per member, or stationary ones -- also for members whose model looks data up as
`data[k]` (csrc/sdp_family_horizon_kernel.h): kernels `sdp_family_simulate`, a tile of 64 trajectories of one member a
workgroup, and `sdp_family_montecarlo_h`, a tile of 256, each step with the member's policy slice and row of constants
of that step.

`simulate_lookahead` and `monte_carlo_lookahead_horizon` run the members forward over a horizon under lookahead controls
-- step k looks ahead into the member's cost-to-go of that step, `J_next[p, t0 + k]`, what `bellman_recursion` returns --
also for members whose model looks data up as `data[k]` (csrc/sdp_family_lookahead_horizon_kernel.h): kernels
`sdp_family_simulate_lookahead` and `sdp_family_montecarlo_lookahead_h`, the tile and the lattice of the lookahead kernels
with the cost-to-go slice and the row of constants of the step.

`transition_operator` and `stationary_distribution` build the transition operators of the members' policies together
(csrc/sdp_family_trans_kernel.h): one launch of `sdp_family_transitions`, a tile of 256 >> d nodes of one member a
workgroup, and one stable sort make a block-diagonal CSR per chunk of members (`FamilyTransitionOperator`), which one
launch per push moves forward for all members; in `stationary` every member stops at its own checked push.

The definition is the solo call: member p of every result equals, bit for bit, what `solvers[p]` returns from the
same method with `kernel = 'generic'` (`monte_carlo`, `lookahead`, `monte_carlo_lookahead`, `simulate`,
`monte_carlo_horizon` -- against `solvers[p].monte_carlo` -- and `transition_operator`: on its device path, whatever its
kernel).

Members may differ in every real constant of dyn / cost, in the ends of the state grid, in the perturbation grid
and weights, in control_steps and control_box.  They must agree in the grid's shape, the dtype, the number of
controls, the `stationnary` flag, the number of perturbation points and the structure of the traced model
(`TracedModel.structure_key`): the constants are always lifted, and the members share one code object that reads
row p of a table of constants for member p.  NOT in the reference API.
"""
from __future__ import division, print_function
import ctypes as C
import hashlib

import numpy as np

from . import _native as nat
from . import codegen
from . import convergence as conv
from . import forward
from . import montecarlo as mc
from .solver import DPSolver
from .trace import TraceError, trace_model

__all__ = ['SolverFamily', 'FamilyTransitionOperator']


class _FamilyProblem(object):
    """Owner of one sdp_family handle (include/sdp_hip.h): the members [first, last) of a family."""

    def __init__(self, tabs, first, last, module, dtype, shape, nu, W):
        self.P = last - first
        self.dtype = np.dtype(dtype)
        self.shape = tuple(shape)
        self.S = int(np.prod(shape))
        self.nu = nu
        # host arrays the descriptor points to, cut to the members of this handle
        keep = {k: np.ascontiguousarray(tabs[k][first:last]) for k in ('axes', 'wgrid', 'proba', 'lo', 'hi', 'n')
                if tabs[k] is not None}
        d = nat.sdp_family_desc()
        d.dtype = nat.np_real(dtype)
        d.d, d.nu, d.W, d.P = len(shape), nu, W, self.P
        d.n_params = tabs['prm'].shape[1]
        d.box_per_node = int(tabs['per_node'])
        d.lanes_per_node = int(tabs['lanes'])
        for k, n in enumerate(shape):
            d.orders[k] = n
        d.axes = keep['axes'].ctypes.data
        if W > 0:
            d.wgrid = keep['wgrid'].ctypes.data
            d.proba = keep['proba'].ctypes.data
        d.box_lo = keep['lo'].ctypes.data
        d.box_hi = keep['hi'].ctypes.data
        d.box_n = keep['n'].ctypes.data
        d.module_path = module.encode()
        h = C.c_void_p()
        nat.check(nat.lib().sdp_family_create(C.byref(d), C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, 'h', None):
            nat.lib().sdp_family_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_value(self, V):
        V = np.ascontiguousarray(V, dtype=self.dtype)
        assert V.size == self.P * self.S
        nat.check(nat.lib().sdp_family_set_value(self.h, nat.ptr(V)))

    def set_params(self, values):
        values = np.ascontiguousarray(values, dtype=self.dtype)
        assert values.shape[0] == self.P
        nat.check(nat.lib().sdp_family_set_params(self.h, nat.ptr(values), int(values.shape[1])))

    def sweep(self, t_k=0.0, rel_dp=False, ref_index=0):
        refs = np.zeros(self.P)
        nat.check(nat.lib().sdp_family_vi_sweep(self.h, float(t_k), int(bool(rel_dp)), int(ref_index), nat.ptr(refs)))
        return refs

    def sweeps(self, n_iter, rel_dp=False, ref_index=0):
        refs = np.zeros((int(n_iter), self.P))
        nat.check(nat.lib().sdp_family_vi_sweeps(self.h, int(n_iter), int(bool(rel_dp)), int(ref_index), nat.ptr(refs)))
        return refs

    def until(self, n_max, rel_dp, ref_index, check_every, tol):
        """(sweeps done [P], [n_checks][P][2] dmin / dmax -- NaN where a member did not run the check --,
        reference costs [n_max][P])"""
        schedule = conv.check_schedule(int(n_max), int(check_every))
        stats = np.full((len(schedule), self.P, 2), np.nan)
        refs = np.zeros((int(n_max), self.P))
        n_done = np.zeros(self.P, dtype=np.int32)
        nat.check(nat.lib().sdp_family_vi_until(self.h, int(n_max), int(bool(rel_dp)), int(ref_index), int(check_every),
                                                float(tol), nat.ptr(n_done), nat.ptr(stats), nat.ptr(refs)))
        return n_done, stats, refs

    # ---- policy evaluation (csrc/sdp_family_policy_kernel.h)
    def load_policy_unit(self, module):
        nat.check(nat.lib().sdp_family_load_policy_unit(self.h, module.encode()))

    def set_policy(self, pol):
        pol = np.ascontiguousarray(pol, dtype=self.dtype)
        assert pol.size == self.P * self.S * self.nu
        nat.check(nat.lib().sdp_family_set_policy(self.h, nat.ptr(pol)))

    def take_policy(self):
        nat.check(nat.lib().sdp_family_take_policy(self.h))

    def compare_policy(self):
        """[P] bool: the policy of the last sweep equals the prescribed one, value by value"""
        same = np.zeros(self.P, dtype=np.int32)
        nat.check(nat.lib().sdp_family_compare_policy(self.h, nat.ptr(same)))
        return same != 0

    def set_members(self, members):
        members = np.ascontiguousarray(members, dtype=np.int32)
        nat.check(nat.lib().sdp_family_set_members(self.h, nat.ptr(members), int(members.size)))

    def eval_policy(self, n_iter, rel_dp, ref_index, resident):
        refs = np.zeros((max(int(n_iter), 1), self.P))
        nat.check(nat.lib().sdp_family_eval_policy(self.h, int(n_iter), int(bool(rel_dp)), int(ref_index),
                                                   int(bool(resident)), nat.ptr(refs)))
        return refs[:int(n_iter)]

    def eval_policy_until(self, n_max, rel_dp, ref_index, check_every, tol, resident):
        """as `until`, for the members listed (the entries of the others stay 0 / NaN)"""
        schedule = conv.check_schedule(int(n_max), int(check_every))
        stats = np.full((len(schedule), self.P, 2), np.nan)
        refs = np.zeros((int(n_max), self.P))
        n_done = np.zeros(self.P, dtype=np.int32)
        nat.check(nat.lib().sdp_family_eval_policy_until(self.h, int(n_max), int(bool(rel_dp)), int(ref_index),
                                                         int(check_every), float(tol), int(bool(resident)),
                                                         nat.ptr(n_done), nat.ptr(stats), nat.ptr(refs)))
        return n_done, stats, refs

    # ---- Monte Carlo evaluation (csrc/sdp_family_mc_kernel.h)
    def load_mc_unit(self, module):
        nat.check(nat.lib().sdp_family_load_mc_unit(self.h, module.encode()))

    def montecarlo(self, pol, x0, n_steps, n_burn, seeds, traj_offset, cum, law_grid, t0, steps_per_launch, occupancy):
        """pol [P][nu][S], x0 [P][d][B], cum / law_grid [P][n_law], seeds [P]: (cost_sum [P][B], n_outside [P][B],
        x_final [P][d][B], occupancy [P][S] uint64 or None)"""
        d, B = x0.shape[1], x0.shape[2]
        assert pol.shape == (self.P, self.nu, self.S) and x0.shape[0] == self.P and cum.shape == law_grid.shape
        assert all(a.flags.c_contiguous for a in (pol, x0, cum, law_grid, seeds))
        cost_sum = np.empty((self.P, B), dtype=self.dtype)
        n_out = np.empty((self.P, B), dtype=np.int64)
        x_final = np.empty((self.P, d, B), dtype=self.dtype)
        occ = np.empty((self.P, self.S), dtype=np.uint64) if occupancy else None
        nat.check(nat.lib().sdp_family_montecarlo(
            self.h, nat.ptr(pol), B, int(n_steps), int(n_burn), nat.ptr(seeds), int(traj_offset), nat.ptr(x0),
            nat.ptr(cum), int(cum.shape[1]), nat.ptr(law_grid), float(t0), int(steps_per_launch), nat.ptr(cost_sum),
            nat.ptr(n_out), nat.ptr(x_final), nat.ptr(occ)))
        return cost_sum, n_out, x_final, occ

    # ---- closed loops over a horizon (csrc/sdp_family_horizon_kernel.h)
    def load_horizon_unit(self, module):
        nat.check(nat.lib().sdp_family_load_horizon_unit(self.h, module.encode()))

    def simulate_h(self, pol, pol_timed, table, prm_timed, chunk_bytes, x0, w, n_steps, t0):
        """pol [P][T or 1][nu][S], table [P][T or 1][n_prm], x0 [P][d][B], w [P][T][B] or None: (x [P][T+1][d][B],
        u [P][T][nu][B], g [P][T][B])"""
        d, B, T = x0.shape[1], x0.shape[2], int(n_steps)
        assert pol.shape[0] == table.shape[0] == x0.shape[0] == self.P and pol.shape[2:] == (self.nu, self.S)
        assert w is None or w.shape == (self.P, T, B)
        assert all(a.flags.c_contiguous for a in (pol, table, x0) + (() if w is None else (w,)))
        x = np.empty((self.P, T + 1, d, B), dtype=self.dtype)
        u = np.empty((self.P, T, self.nu, B), dtype=self.dtype)
        g = np.empty((self.P, T, B), dtype=self.dtype)
        nat.check(nat.lib().sdp_family_simulate(
            self.h, nat.ptr(pol), int(pol.shape[1]), int(bool(pol_timed)), nat.ptr(table) if table.size else None,
            int(table.shape[2]), int(bool(prm_timed)), int(chunk_bytes), B, T, nat.ptr(x0), nat.ptr(w), float(t0),
            nat.ptr(x), nat.ptr(u), nat.ptr(g)))
        return x, u, g

    def montecarlo_h(self, pol, pol_timed, table, prm_timed, chunk_bytes, x0, n_steps, n_burn, seeds, traj_offset, cum,
                     law_grid, t0, steps_per_launch, occupancy):
        """pol and table as in `simulate_h`, the rest as in `montecarlo`: what `montecarlo` returns"""
        d, B = x0.shape[1], x0.shape[2]
        assert pol.shape[0] == table.shape[0] == x0.shape[0] == self.P and pol.shape[2:] == (self.nu, self.S)
        assert cum.shape == law_grid.shape and all(a.flags.c_contiguous for a in (pol, table, x0, cum, law_grid, seeds))
        cost_sum = np.empty((self.P, B), dtype=self.dtype)
        n_out = np.empty((self.P, B), dtype=np.int64)
        x_final = np.empty((self.P, d, B), dtype=self.dtype)
        occ = np.empty((self.P, self.S), dtype=np.uint64) if occupancy else None
        nat.check(nat.lib().sdp_family_montecarlo_h(
            self.h, nat.ptr(pol), int(pol.shape[1]), int(bool(pol_timed)), nat.ptr(table) if table.size else None,
            int(table.shape[2]), int(bool(prm_timed)), int(chunk_bytes), B, int(n_steps), int(n_burn), nat.ptr(seeds),
            int(traj_offset), nat.ptr(x0), nat.ptr(cum), int(cum.shape[1]), nat.ptr(law_grid), float(t0),
            int(steps_per_launch), nat.ptr(cost_sum), nat.ptr(n_out), nat.ptr(x_final), nat.ptr(occ)))
        return cost_sum, n_out, x_final, occ

    # ---- lookahead at arbitrary states (csrc/sdp_family_lookahead_kernel.h)
    def load_lookahead_unit(self, module):
        nat.check(nat.lib().sdp_family_load_lookahead_unit(self.h, module.encode()))

    def set_lookahead_box(self, bprm, steps):
        """bprm [P][n_box] float64, the constants of every member's box; steps [P][nu] float64, its control steps"""
        bprm = np.ascontiguousarray(bprm, dtype=np.float64)
        steps = np.ascontiguousarray(steps, dtype=np.float64)
        assert bprm.shape[0] == self.P and steps.shape == (self.P, self.nu)
        nat.check(nat.lib().sdp_family_set_lookahead_box(self.h, nat.ptr(bprm) if bprm.size else None, int(bprm.shape[1]),
                                                         nat.ptr(steps)))

    def lookahead(self, x, t_k):
        """x [P][d][B] at the values set: (J [P][B], u [P][nu][B], idx [P][B])"""
        B = x.shape[2]
        assert x.shape[0] == self.P and x.flags.c_contiguous and x.dtype == self.dtype
        J = np.empty((self.P, B), dtype=self.dtype)
        u = np.empty((self.P, self.nu, B), dtype=self.dtype)
        idx = np.empty((self.P, B), dtype=np.int32)
        nat.check(nat.lib().sdp_family_lookahead(self.h, B, nat.ptr(x), float(t_k), nat.ptr(J), nat.ptr(u), nat.ptr(idx)))
        return J, u, idx

    def montecarlo_lookahead(self, x0, n_steps, n_burn, seeds, traj_offset, cum, law_grid, t0, steps_per_launch, occupancy):
        """x0 [P][d][B], cum / law_grid [P][n_law], seeds [P], at the values set: what `montecarlo` returns"""
        d, B = x0.shape[1], x0.shape[2]
        assert x0.shape[0] == self.P and cum.shape == law_grid.shape
        assert all(a.flags.c_contiguous for a in (x0, cum, law_grid, seeds))
        cost_sum = np.empty((self.P, B), dtype=self.dtype)
        n_out = np.empty((self.P, B), dtype=np.int64)
        x_final = np.empty((self.P, d, B), dtype=self.dtype)
        occ = np.empty((self.P, self.S), dtype=np.uint64) if occupancy else None
        nat.check(nat.lib().sdp_family_montecarlo_lookahead(
            self.h, B, int(n_steps), int(n_burn), nat.ptr(seeds), int(traj_offset), nat.ptr(x0), nat.ptr(cum),
            int(cum.shape[1]), nat.ptr(law_grid), float(t0), int(steps_per_launch), nat.ptr(cost_sum), nat.ptr(n_out),
            nat.ptr(x_final), nat.ptr(occ)))
        return cost_sum, n_out, x_final, occ

    # ---- closed loops under lookahead controls over a horizon (csrc/sdp_family_lookahead_horizon_kernel.h)
    def load_lookahead_horizon_unit(self, module):
        nat.check(nat.lib().sdp_family_load_lookahead_horizon_unit(self.h, module.encode()))

    def simulate_lookahead_h(self, V, V_timed, table, prm_timed, chunk_bytes, x0, w, n_steps, t0):
        """V [P][T or 1][S], table [P][T or 1][n_prm], x0 [P][d][B], w [P][T][B] or None, at the box set: (x [P][T+1][d][B],
        u [P][T][nu][B], g [P][T][B], q [P][T][B])"""
        d, B, T = x0.shape[1], x0.shape[2], int(n_steps)
        assert V.shape[0] == table.shape[0] == x0.shape[0] == self.P and V.shape[2:] == (self.S,)
        assert w is None or w.shape == (self.P, T, B)
        assert all(a.flags.c_contiguous and a.dtype == self.dtype for a in (V, table, x0) + (() if w is None else (w,)))
        x = np.empty((self.P, T + 1, d, B), dtype=self.dtype)
        u = np.empty((self.P, T, self.nu, B), dtype=self.dtype)
        g = np.empty((self.P, T, B), dtype=self.dtype)
        q = np.empty((self.P, T, B), dtype=self.dtype)
        nat.check(nat.lib().sdp_family_simulate_lookahead(
            self.h, nat.ptr(V), int(V.shape[1]), int(bool(V_timed)), nat.ptr(table) if table.size else None,
            int(table.shape[2]), int(bool(prm_timed)), int(chunk_bytes), B, T, nat.ptr(x0), nat.ptr(w), float(t0),
            nat.ptr(x), nat.ptr(u), nat.ptr(g), nat.ptr(q)))
        return x, u, g, q

    def montecarlo_lookahead_h(self, V, V_timed, table, prm_timed, chunk_bytes, x0, n_steps, n_burn, seeds, traj_offset,
                               cum, law_grid, t0, steps_per_launch, occupancy):
        """V and table as in `simulate_lookahead_h`, the rest as in `montecarlo_lookahead`: what `montecarlo` returns"""
        d, B = x0.shape[1], x0.shape[2]
        assert V.shape[0] == table.shape[0] == x0.shape[0] == self.P and V.shape[2:] == (self.S,)
        assert cum.shape == law_grid.shape and all(a.flags.c_contiguous for a in (V, table, x0, cum, law_grid, seeds))
        assert all(a.dtype == self.dtype for a in (V, table, x0, law_grid))
        cost_sum = np.empty((self.P, B), dtype=self.dtype)
        n_out = np.empty((self.P, B), dtype=np.int64)
        x_final = np.empty((self.P, d, B), dtype=self.dtype)
        occ = np.empty((self.P, self.S), dtype=np.uint64) if occupancy else None
        nat.check(nat.lib().sdp_family_montecarlo_lookahead_h(
            self.h, nat.ptr(V), int(V.shape[1]), int(bool(V_timed)), nat.ptr(table) if table.size else None,
            int(table.shape[2]), int(bool(prm_timed)), int(chunk_bytes), B, int(n_steps), int(n_burn), nat.ptr(seeds),
            int(traj_offset), nat.ptr(x0), nat.ptr(cum), int(cum.shape[1]), nat.ptr(law_grid), float(t0),
            int(steps_per_launch), nat.ptr(cost_sum), nat.ptr(n_out), nat.ptr(x_final), nat.ptr(occ)))
        return cost_sum, n_out, x_final, occ

    # ---- transition operators (csrc/sdp_family_trans_kernel.h)
    def load_trans_unit(self, module):
        nat.check(nat.lib().sdp_family_load_trans_unit(self.h, module.encode()))

    def transop_create(self, pol, t_k):
        """pol [P][S][nu] at the constants set: the sdp_transop handle of the members' block-diagonal operator (the
        caller owns it; it does not refer to this handle afterwards)"""
        assert pol.shape == (self.P, self.S, self.nu) and pol.flags.c_contiguous and pol.dtype == self.dtype
        h = C.c_void_p()
        nat.check(nat.lib().sdp_family_transop_create(self.h, nat.ptr(pol), float(t_k), C.byref(h)))
        return h

    def get_value(self):
        J = np.empty((self.P,) + self.shape, dtype=self.dtype)
        nat.check(nat.lib().sdp_family_get_value(self.h, nat.ptr(J)))
        return J

    def get_policy(self):
        pol = np.empty((self.P,) + self.shape + (self.nu,), dtype=self.dtype)
        idx = np.empty((self.P,) + self.shape, dtype=np.int32)
        nat.check(nat.lib().sdp_family_get_policy(self.h, nat.ptr(pol), nat.ptr(idx)))
        return pol, idx

    def last_kernel_ms(self):
        ms = C.c_double(0.0)
        nat.check(nat.lib().sdp_family_last_kernel_ms(self.h, C.byref(ms)))
        return ms.value


def _trace_member(s, t_k=None):
    """dyn and cost of one member, traced for one call and with EVERY real constant lifted (a family always lifts,
    also where all members' constants are equal).  A time-dependent system whose callables need a concrete time
    index (`data[k]`) is traced for the step t_k alone, as DPSolver._trace_now does.  A TracedModel or a TraceError."""
    sd = s.sys
    args = (sd.dyn, sd.cost, len(sd.state), len(sd.control), len(sd.perturb), sd.params, sd.stationnary)
    try:
        model = trace_model(*args)
    except TraceError as e:
        if sd.stationnary or t_k is None:
            return e
        try:
            model = trace_model(*args, t_value=int(t_k))
        except TraceError:
            return e
    model.lift_constants()
    return model


def _structure_message(p, model, first, where='', what=('model', 'dyn / cost')):
    """why member p cannot share member 0's code object (`what`: how the message names the trace -- the model's, or
    that of control_box, a TracedBox)"""
    n_p, n_0 = len(model.param_values()), len(first.param_values())
    ops = lambda m: [n.op for n in m.live_nodes() if n.op != 'const']
    if n_p != n_0 and ops(model) == ops(first):
        # the trace shares equal constants (one node for h and for c where h == c): the DAG has another shape
        few = p if n_p < n_0 else 0
        return ('member {}{}: constants that coincide in member {} make its traced {} another structure ({} distinct '
                'constants against {}): equal values are one node of the trace.  Give the coinciding constants '
                'different values, or solve that member alone'.format(p, where, few, what[0], min(n_p, n_0), max(n_p, n_0)))
    return ('member {}{}: the structure of the traced {} differs from member 0\'s (another expression, another '
            'np.interp table, or a different time dependence)'.format(p, where, what[1]))


_BOX = ('control_box', 'control_box')


class FamilyTransitionOperator(object):
    """The transition operators of a family's policies on the device (`SolverFamily.transition_operator`): per chunk of
    members ONE block-diagonal CSR matrix in device memory -- member p's node s is row p_local * S + s -- owner of
    one sdp_transop handle per chunk (include/sdp_hip.h: sdp_family_transop_create).  Member p of everything it returns
    equals, bit for bit, what `solvers[p].transition_operator(pol[p], t_k)` returns on the device:
    `stodynprog_amd.forward` on member p is the definition.  NOT in the reference API.

    shape     : the members' state grid's
    P         : members
    nnz       : entries of all members, P S W 2^d
    mean_cost : gbar of every member, (P,) + shape
    info      : entries, bytes, members, chunks, build_ms (entries_ms + sort_ms) and, once used, push_ms and pushes"""

    def __init__(self, parts, shape, dtype, nnz_member):
        self.parts = [(int(a), int(b), h) for a, b, h in parts]      # [(first, last, sdp_transop handle)]
        self.shape = tuple(shape)
        self.dtype = np.dtype(dtype)
        self.S = int(np.prod(self.shape))
        self.P = self.parts[-1][1]
        self.nnz_member = int(nnz_member)
        self.nnz = self.P * self.nnz_member
        self.nbytes = sum(forward.operator_bytes((b - a) * self.nnz_member, (b - a) * self.S, self.dtype.itemsize)
                          for a, b, _ in self.parts)
        self._csr = None                   # (chunk, its CSR on the host): the chunk `tocsr` read last
        self.mean_cost = np.empty((self.P,) + self.shape, dtype=self.dtype)
        entries_ms = sort_ms = 0.0
        for a, b, h in self.parts:
            gbar = np.empty((b - a,) + self.shape, dtype=self.dtype)
            nat.check(nat.lib().sdp_transop_get_mean_cost(h, nat.ptr(gbar)))
            self.mean_cost[a:b] = gbar
            e_ms, s_ms = C.c_double(0.0), C.c_double(0.0)
            nat.check(nat.lib().sdp_transop_build_ms(h, C.byref(e_ms), C.byref(s_ms)))
            entries_ms, sort_ms = entries_ms + e_ms.value, sort_ms + s_ms.value
        self.info = dict(entries=self.nnz, bytes=self.nbytes, members=self.P, chunks=len(self.parts), path='device',
                         build_ms=entries_ms + sort_ms, entries_ms=entries_ms, sort_ms=sort_ms)

    def close(self):
        for _, _, h in getattr(self, 'parts', ()):
            nat.lib().sdp_transop_destroy(h)
        self.parts = []
        self._csr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return self.P

    def _parts(self):
        if not self.parts:
            raise ValueError('the operator is closed')
        return self.parts

    def _vectors(self, mu):
        """[P][S] in the operator's reals, from an array of the grid's shape (every member's) or (P,) + shape"""
        mu = np.asarray(mu)
        one, each = self.shape, (self.P,) + self.shape
        if mu.shape == one and one != each:
            mu = np.broadcast_to(mu, each)
        elif mu.shape != each:
            raise ValueError('mu must have shape {} (the same for all {} members) or {} (member p from mu[p]), not {}'.format(
                one, self.P, each, mu.shape))
        return np.ascontiguousarray(mu, dtype=self.dtype).reshape(self.P, self.S)

    def _kernel_ms(self, h):
        ms = C.c_double(0.0)
        nat.check(nat.lib().sdp_transop_last_kernel_ms(h, C.byref(ms)))
        return ms.value

    def _get(self, h, a, b, out):
        part = np.empty((b - a, self.S), dtype=self.dtype)
        nat.check(nat.lib().sdp_transop_get(h, nat.ptr(part)))
        out[a:b] = part.reshape((b - a,) + self.shape)

    def push(self, mu, n_steps=1):
        """every member's mu after n_steps steps under its policy, (P_p^T)^n mu_p: (P,) + shape.  mu: (P,) + shape,
        or the grid's shape for all members.  One launch per step pushes all members of a chunk."""
        n_steps = int(n_steps)
        if n_steps < 0:
            raise ValueError('n_steps must not be negative')
        mu = self._vectors(mu)
        out = np.empty((self.P,) + self.shape, dtype=self.dtype)
        ms = 0.0
        for a, b, h in self._parts():
            nat.check(nat.lib().sdp_transop_push(h, nat.ptr(np.ascontiguousarray(mu[a:b])), n_steps))
            ms += self._kernel_ms(h)
            self._get(h, a, b, out)
        self.info.update(push_ms=ms, pushes=n_steps)
        return out

    def stationary(self, mu0=None, tol=1e-12, n_max=10000, check_every=10):
        """The power iteration of `TransitionOperator.stationary` on every member, one launch per push for all members
        still running: member p stops at its own first checked push with max |mu_{k+1} - mu_k| <= tol over its slice,
        or at n_max, and is computed no more.  mu0: (P,) + shape, the grid's shape for all members, or None (uniform).
        Returns a `forward.FamilyStationary` record (mu, n_done, converged, delta, average_cost, mass, each stacked over
        the members; res[p] is the solo `forward.Stationary` of member p)."""
        tol, check_every = conv.validate(tol, check_every)
        n_max = int(n_max)
        if n_max < 1:
            raise ValueError('n_max must be at least 1')
        if mu0 is None:
            mu0 = np.broadcast_to(forward.uniform(self.S, self.dtype), (self.P, self.S))
        else:
            mu0 = self._vectors(mu0)
        mu = np.empty((self.P,) + self.shape, dtype=self.dtype)
        n_done = np.zeros(self.P, dtype=np.int32)
        delta = np.full(self.P, np.nan)
        ms = 0.0
        for a, b, h in self._parts():
            nat.check(nat.lib().sdp_transop_push(h, nat.ptr(np.ascontiguousarray(mu0[a:b])), 0))
            done, d = np.zeros(b - a, dtype=np.int32), np.full(b - a, np.nan)
            nat.check(nat.lib().sdp_transop_push_until_members(h, n_max, check_every, tol, nat.ptr(done), nat.ptr(d)))
            n_done[a:b], delta[a:b] = done, d
            ms += self._kernel_ms(h)
            self._get(h, a, b, mu)
        self.info.update(push_ms=ms, pushes=int(n_done.max()))
        return forward.FamilyStationary(mu, n_done, delta, tol, self.mean_cost)

    def set_long_rows(self, min_entries):
        """`TransitionOperator.set_long_rows` on every chunk: no result depends on it"""
        for _, _, h in self._parts():
            nat.check(nat.lib().sdp_transop_set_long_rows(h, int(min_entries)))
        self.info['long_rows_from'] = int(min_entries)

    def tocsr(self, p):
        """(indptr int64 [S + 1], indices int32, data) of member p's P^T, in the member's own node ids"""
        p = int(p)
        if not 0 <= p < self.P:
            raise IndexError('member {} of {}'.format(p, self.P))
        c = next(i for i, (a, b, _) in enumerate(self._parts()) if a <= p < b)
        a, b, h = self.parts[c]
        if self._csr is None or self._csr[0] != c:
            rows, nnz = (b - a) * self.S, (b - a) * self.nnz_member
            indptr = np.empty(rows + 1, dtype=np.int64)
            indices = np.empty(nnz, dtype=np.int32)
            data = np.empty(nnz, dtype=self.dtype)
            nat.check(nat.lib().sdp_transop_get_csr(h, nat.ptr(indptr), nat.ptr(indices), nat.ptr(data)))
            self._csr = (c, (indptr, indices, data))
        indptr, indices, data = self._csr[1]
        first = (p - a) * self.S
        lo, hi = int(indptr[first]), int(indptr[first + self.S])
        return indptr[first:first + self.S + 1] - lo, indices[lo:hi] - np.int32(first), data[lo:hi].copy()


class SolverFamily(object):
    """P >= 1 DPSolver objects, each set up exactly as for a solo call, solved together (module docstring)."""

    # members are processed in chunks of at most this many bytes of device arrays (a member larger than that runs
    # alone); every chunk is an independent call, so no cut changes a bit
    chunk_bytes = DPSolver.horizon_chunk_bytes

    def __init__(self, solvers):
        solvers = list(solvers)
        if not solvers:
            raise ValueError('a family has at least one member')
        for p, s in enumerate(solvers):
            if not isinstance(s, DPSolver):
                raise TypeError('member {} is not a DPSolver'.format(p))
        # what no family runs (checked for every member before anything else, and before a device is touched)
        models = []
        for p, s in enumerate(solvers):
            if s.comm is not None:
                raise NotImplementedError('member {} has a communicator: a family runs on one GPU'.format(p))
            if len(s.sys.perturb) >= 2:
                raise NotImplementedError('member {} has {} perturbation variables: a family takes one at most'.format(
                    p, len(s.sys.perturb)))
            if len(s.state_grid) > 4:
                raise NotImplementedError('member {} has {} state variables: interpolation stops at 4'.format(
                    p, len(s.state_grid)))
            model = _trace_member(s, None if s.sys.stationnary else 0)
            if isinstance(model, TraceError):
                raise NotImplementedError('member {}: dyn / cost do not trace ({}): a family runs traced models only'.format(p, model))
            models.append(model)
        first = solvers[0]
        self.dims = first._shape()
        self.dtype = first.dtype
        self.nu = len(first.sys.control)
        self.stationnary = bool(first.sys.stationnary)
        self.W = self._law_points(first)
        for p, s in enumerate(solvers[1:], 1):
            for what, mine, ref in (('dims', s._shape(), self.dims), ('dtype', s.dtype, self.dtype),
                                    ('number of controls', len(s.sys.control), self.nu),
                                    ('stationnary flag', bool(s.sys.stationnary), self.stationnary),
                                    ('number of perturbation points', self._law_points(s), self.W)):
                if mine != ref:
                    raise ValueError('member {}: {} {} differs from member 0\'s {}'.format(p, what, mine, ref))
            if models[p].structure_key() != models[0].structure_key():
                raise ValueError(_structure_message(p, models[p], models[0]))
        self.solvers = solvers
        self.P = len(solvers)
        self._handle = None                # (key, _FamilyProblem) of a family that runs as one chunk
        self.last_policy_index = None
        self.last_convergence = None
        self.backend_info = {}

    @staticmethod
    def _law_points(s):
        return len(s.perturb_grid[0]) if s.sys.perturb else 0

    def __len__(self):
        return self.P

    # ------------------------------------------------------------------ host side
    def _tables(self, t_k=None):
        """Everything the device needs for one call or time step, member-major (no GPU needed): the table of
        lifted constants, the axes, the laws, the box tables, the lane count and the generated source."""
        dt = self.dtype
        box_t = None if self.stationnary else t_k
        where = '' if t_k is None else ' at step {}'.format(t_k)
        models, plans = [], []
        for p, s in enumerate(self.solvers):
            s._check_supported()
            model = _trace_member(s, t_k)
            if isinstance(model, TraceError):
                raise model
            if p and model.structure_key() != models[0].structure_key():
                raise ValueError(_structure_message(p, model, models[0], where))
            if s._shape() != self.dims or self._law_points(s) != self.W:
                raise ValueError('member {}: its discretisation changed since the family was made'.format(p))
            models.append(model)
            plans.append(s._box_plan(box_t))
        S = int(np.prod(self.dims))
        per_node = any(bp['per_node'] for bp in plans)
        cols = S if per_node else 1
        wide = lambda a, t: np.ascontiguousarray(np.broadcast_to(a, (self.nu, cols)), dtype=t)
        tabs = dict(
            model=models[0], per_node=per_node, lanes=max(bp['lanes'] for bp in plans),
            prm=np.ascontiguousarray([m.param_values() for m in models], dtype=dt).reshape(self.P, -1),
            axes=np.ascontiguousarray([np.concatenate([np.asarray(g, dtype=dt) for g in s.state_grid])
                                       for s in self.solvers], dtype=dt),
            wgrid=np.ascontiguousarray([s.perturb_grid[0] for s in self.solvers], dtype=dt) if self.W else None,
            proba=np.ascontiguousarray([s.perturb_proba[0] for s in self.solvers], dtype=dt) if self.W else None,
            lo=np.stack([wide(bp['lo'], dt) for bp in plans]),
            hi=np.stack([wide(bp['hi'], dt) for bp in plans]),
            n=np.stack([wide(bp['n'], np.int32) for bp in plans]),
            time_specialized=models[0].t_value is not None)
        tabs['source'] = codegen.family_unit(models[0], dt, tabs['lanes'])
        return tabs

    def _member_bytes(self, tabs):
        """bytes of device arrays one member takes: two value arrays, policy, indices, box table, its rows of the
        small tables"""
        S = int(np.prod(self.dims))
        rs = self.dtype.itemsize
        cols = S if tabs['per_node'] else 1
        return (S * rs * (2 + self.nu) + S * 4 + self.nu * cols * (2 * rs + 4)
                + rs * (tabs['axes'].shape[1] + 2 * self.W + tabs['prm'].shape[1]) + 4 + 24)

    def _policy_bytes(self):
        """what a member takes on top of _member_bytes in eval_policy and policy_iteration: the prescribed policy
        (allocated at the first evaluation), its flag of the policy compare and its word of the resident kernel"""
        return int(np.prod(self.dims)) * self.nu * self.dtype.itemsize + 8

    def _chunks(self, tabs, extra=0, most=None):
        """[(first, last), ...]: members whose device arrays take at most chunk_bytes together (`extra`: bytes a
        member takes beside _member_bytes in this call; `most`: the most members a chunk may hold whatever their bytes)"""
        step = max(1, int(self.chunk_bytes) // (self._member_bytes(tabs) + extra))
        if most is not None:
            step = max(1, min(step, int(most)))
        return [(a, min(a + step, self.P)) for a in range(0, self.P, step)]

    def _run(self, tabs, J0, work, evaluation=False, mc_bytes=None, look=None, horizon=None, trans=None, look_horizon=None):
        """work(prob, first, last) on every chunk, each with its values set from J0 [P] + dims.  evaluation: the
        call evaluates policies, so every handle also loads the family's evaluation unit and the chunks leave room
        for the prescribed policy.  mc_bytes: the call is a Monte Carlo run whose arrays take that many bytes a
        member beside the handle's, so every handle also loads the family's Monte Carlo unit (J0 is None then: the
        values of a handle that is reused stay what they were).  look: the call is a lookahead (`_lookahead_tables`:
        source, bprm, steps, bytes a member takes beside the handle's), so every handle also loads the family's
        lookahead unit and is given its members' box constants and control steps.  horizon: the call is a closed loop over
        a horizon (dict(source, bytes): the horizon unit and the bytes a member takes beside the handle's), so every
        handle also loads the family's horizon unit (J0 is None then).  trans: the call builds transition operators
        (dict(bytes, most): the bytes a member takes beside the handle's and the most members of a chunk), so every handle
        also loads the family's transition unit (J0 is None then).  look_horizon: the call is a closed loop under lookahead
        controls over a horizon (what `look` takes, from `_lookahead_horizon_tables`: the bytes count the member's
        cost-to-go slices, table rows, states and outputs), so every handle also loads that unit and is given its members'
        box constants and control steps (J0 is None then).  Returns the chunks [(first, last), ...] it ran in"""
        nat.require_gpu()
        module = nat.compile_model(tabs['source'])
        look_module = nat.compile_model(look['source']) if look is not None else None
        look_horizon_module = nat.compile_model(look_horizon['source']) if look_horizon is not None else None
        policy_module = nat.compile_model(codegen.family_policy_unit(tabs['model'], self.dtype)) if evaluation else None
        mc_module = nat.compile_model(codegen.family_mc_unit(tabs['model'], self.dtype)) if mc_bytes is not None else None
        horizon_module = nat.compile_model(horizon['source']) if horizon is not None else None
        trans_module = nat.compile_model(codegen.family_trans_unit(tabs['model'], self.dtype)) if trans is not None else None
        chunks = self._chunks(tabs, self._policy_bytes() if evaluation else
                              int(mc_bytes or 0) + (look['bytes'] if look else 0) + (horizon['bytes'] if horizon else 0)
                              + (trans['bytes'] if trans else 0) + (look_horizon['bytes'] if look_horizon else 0),
                              trans['most'] if trans else None)
        digest = hashlib.sha256()
        for k in ('axes', 'wgrid', 'proba', 'lo', 'hi', 'n'):
            if tabs[k] is not None:
                digest.update(tabs[k].tobytes())
        key = (module, tabs['lanes'], tabs['per_node'], tabs['prm'].shape[1], digest.hexdigest(), tuple(chunks))
        for first, last in chunks:
            if self._handle is not None and self._handle[0] == key and len(chunks) == 1:
                prob = self._handle[1]
            else:
                if self._handle is not None:
                    self._handle[1].close()
                    self._handle = None
                prob = _FamilyProblem(tabs, first, last, module, self.dtype, self.dims, self.nu, self.W)
                if len(chunks) == 1:
                    self._handle = (key, prob)
            try:
                if evaluation and getattr(prob, 'policy_module', None) != policy_module:
                    prob.load_policy_unit(policy_module)
                    prob.policy_module = policy_module
                if mc_module is not None and getattr(prob, 'mc_module', None) != mc_module:
                    prob.load_mc_unit(mc_module)
                    prob.mc_module = mc_module
                if horizon_module is not None and getattr(prob, 'horizon_module', None) != horizon_module:
                    prob.load_horizon_unit(horizon_module)
                    prob.horizon_module = horizon_module
                if trans_module is not None and getattr(prob, 'trans_module', None) != trans_module:
                    prob.load_trans_unit(trans_module)
                    prob.trans_module = trans_module
                for which, unit, load in (('look_module', look, prob.load_lookahead_unit),
                                          ('look_horizon_module', look_horizon, prob.load_lookahead_horizon_unit)):
                    if unit is None:
                        continue
                    # (the two units of a handle share the lanes and the box rows: the library drops the one of another plan)
                    plan = (tabs['lanes'], unit['bprm'].shape[1])
                    if getattr(prob, 'look_plan', plan) != plan:
                        prob.look_module = prob.look_horizon_module = None
                    prob.look_plan = plan
                    built = look_module if unit is look else look_horizon_module
                    if getattr(prob, which, None) != built:
                        load(built)
                        setattr(prob, which, built)
                    prob.set_lookahead_box(unit['bprm'][first:last], unit['steps'][first:last])
                prob.set_params(tabs['prm'][first:last])
                if J0 is not None:
                    prob.set_value(J0[first:last])
                work(prob, first, last)
            finally:
                if len(chunks) > 1:        # one chunk's arrays on the device at a time
                    prob.close()
        self.backend_info = dict(kernel='family', members=self.P, lanes=tabs['lanes'],
                                 lifted_constants=int(tabs['prm'].shape[1]), chunks=len(chunks), module=module,
                                 per_node=tabs['per_node'], time_specialized=tabs['time_specialized'])
        return chunks

    def _start(self, J_next, rel_dp, name='J_next'):
        """the start of every member, [P] + dims in the family's reals, from an array of shape dims or (P,) + dims"""
        J_next = np.asarray(J_next)
        if J_next.shape == self.dims:
            J_next = np.broadcast_to(J_next, (self.P,) + self.dims)
        elif J_next.shape != (self.P,) + self.dims:
            raise ValueError('array `{:s}` should be of shape {:s} or {:s}, not {:s}'.format(
                name, str(self.dims), str((self.P,) + self.dims), str(J_next.shape)))
        if rel_dp:
            # the cost-to-go must be a *differential* cost, zero at the reference state, for every member
            assert np.all(J_next[(slice(None),) + self.solvers[0]._state_ref_ind] == 0.)
        return np.ascontiguousarray(J_next, dtype=self.dtype)

    def _ref_flat(self, rel_dp):
        return self.solvers[0]._ref_flat() if rel_dp else 0

    # ------------------------------------------------------------------ the solo methods, stacked
    def value_iteration(self, J_next, rel_dp=False):
        """one DP step of every member: `DPSolver.value_iteration` of each, stacked on a new leading axis.
        J_next: shape dims (the same start for every member) or (P,) + dims; with rel_dp a (J, J_ref) tuple.
        Returns (J, pol) of shapes (P,) + dims and (P,) + dims + (nu,); J is (J_diff, J_ref [P]) with rel_dp."""
        if rel_dp:
            J_next, _ = J_next
        J0 = self._start(J_next, rel_dp)
        tabs = self._tables(None)
        out = self._empty()
        refs = np.zeros(self.P)

        def work(prob, a, b):
            refs[a:b] = prob.sweep(0.0, rel_dp, self._ref_flat(rel_dp))
            out[0][a:b] = prob.get_value()
            out[1][a:b], out[2][a:b] = prob.get_policy()
        self._run(tabs, J0, work)
        self.last_policy_index = out[2]
        self.last_convergence = None
        return ((out[0], refs) if rel_dp else out[0]), out[1]

    def _empty(self):
        return (np.empty((self.P,) + self.dims, dtype=self.dtype),
                np.empty((self.P,) + self.dims + (self.nu,), dtype=self.dtype),
                np.empty((self.P,) + self.dims, dtype=np.int32))

    def value_iterations(self, J_next, n_iter, rel_dp=False, J_ref_full=False, tol=None, check_every=1):
        """`DPSolver.value_iterations` of every member, stacked.  With `tol` a member stops at its own first
        checked sweep whose span is <= tol and the others go on: member p of the result equals the solo call with
        n_iter = the sweeps it ran, and last_convergence[p] is the solo record.  With rel_dp J is (J_diff, J_ref),
        J_ref of shape (P,), or with J_ref_full a list of P arrays (one reference cost per sweep the member ran)."""
        assert n_iter >= 1
        if tol is not None:
            tol, check_every = conv.validate(tol, check_every)
        self.last_convergence = None
        if rel_dp:
            J_next, _ = J_next
        J0 = self._start(J_next, rel_dp)
        tabs = self._tables(None)
        out = self._empty()
        refs = np.zeros((n_iter, self.P))
        n_done = np.full(self.P, n_iter, dtype=np.int32)
        schedule = conv.check_schedule(n_iter, check_every) if tol is not None else []
        stats = np.full((len(schedule), self.P, 2), np.nan)

        def work(prob, a, b):
            ref_flat = self._ref_flat(rel_dp)
            if tol is None:
                refs[:, a:b] = prob.sweeps(n_iter, rel_dp, ref_flat)
            else:
                n_done[a:b], stats[:, a:b], refs[:, a:b] = prob.until(n_iter, rel_dp, ref_flat, check_every, tol)
            out[0][a:b] = prob.get_value()
            out[1][a:b], out[2][a:b] = prob.get_policy()
        self._run(tabs, J0, work)
        self.last_policy_index = out[2]
        per_member = [refs[:n_done[p], p].copy() for p in range(self.P)]
        if tol is not None:
            records = []
            for p in range(self.P):
                checked = [k for k in schedule if k <= n_done[p]]
                checks = [(k, stats[c, p, 0], stats[c, p, 1]) for c, k in enumerate(checked)]
                records.append(DPSolver._sweep_record(tol, check_every, int(n_done[p]), checks, per_member[p], rel_dp))
            self.last_convergence = records
        if rel_dp:
            return (out[0], per_member if J_ref_full else np.array([r[-1] for r in per_member])), out[1]
        return out[0], out[1]

    def bellman_recursion(self, t_fin, J_fin, t_ini=0):
        """`DPSolver.bellman_recursion` of every member, stacked: (J, pol) of shapes (P, t_fin - t_ini) + dims and
        (P, t_fin - t_ini) + dims + (nu,).  The time index is stepped here, one family launch per step; a model that
        looks data up as data[k] is traced per member and step, and step k runs with the constants of that step."""
        assert t_ini == 0       # t_ini > 0 not tested (as in the reference)
        T = t_fin - t_ini
        J = np.zeros((self.P, T) + self.dims)
        pol = np.zeros((self.P, T) + self.dims + (self.nu,))
        J_fin = self._start(J_fin, False)
        idx = np.empty((self.P,) + self.dims, dtype=np.int32)
        for t_k in range(t_ini, t_fin)[::-1]:
            k = t_k - t_ini
            J_next = J_fin if t_k == t_fin - 1 else J[:, k + 1]
            tabs = self._tables(t_k)

            def work(prob, a, b):
                prob.sweep(t_k, False, 0)
                J[a:b, k] = prob.get_value()
                pol[a:b, k], idx[a:b] = prob.get_policy()
            self._run(tabs, np.ascontiguousarray(J_next, dtype=self.dtype), work)
        self.last_policy_index = idx
        self.last_convergence = None
        return J, pol

    # ------------------------------------------------------------------ policy evaluation and iteration
    # the form of an evaluation (csrc/sdp_family_policy_kernel.h): 'steps' is a launch per step (kernel
    # sdp_family_evalpol, any grid size); 'resident' runs all steps of a member in one workgroup with its values in
    # LDS (sdp_family_evalpol_resident), for a member that fits there (codegen.family_resident_nodes).  'auto' takes the
    # resident form for n_iter >= 2 steps of a member of at most one node per thread of the resident workgroup, the
    # steps form otherwise: as measured, a member of 651 nodes is 1.3 to 1.8 times faster resident at
    # every family size, one of 2501 nodes -- three trips of the workgroup a step, on one CU -- is not
    evaluation = 'auto'

    def _evaluation_form(self, n_iter):
        """'steps' or 'resident' for a call of n_iter steps, by `self.evaluation` and the fit rule
        (codegen.family_resident_nodes)"""
        if self.evaluation not in ('auto', 'steps', 'resident'):
            raise ValueError("evaluation should be 'auto', 'steps' or 'resident', not {!r}".format(self.evaluation))
        S, rs = int(np.prod(self.dims)), self.dtype.itemsize
        fits = S <= codegen.family_resident_nodes(self.dtype)
        if self.evaluation == 'resident' and not fits:
            raise ValueError('the resident evaluation holds two value buffers of a member in {} bytes of LDS: a member of '
                             '{} nodes needs {} bytes'.format(
                                 codegen.FAMILY_RESIDENT_LDS_BYTES - codegen.FAMILY_RESIDENT_REDUCTION_BYTES, S, 2 * S * rs))
        if self.evaluation == 'auto':
            return 'resident' if fits and S <= codegen.FAMILY_RESIDENT_THREADS and n_iter >= 2 else 'steps'
        return self.evaluation

    def _policy(self, pol, name='pol'):
        """the policy of every member, [P] + dims + (nu,) in the family's reals, from an array of shape
        dims + (nu,) (every member's policy) or (P,) + dims + (nu,)"""
        pol = np.asarray(pol)
        one, each = self.dims + (self.nu,), (self.P,) + self.dims + (self.nu,)
        if pol.shape == one and one != each:
            pol = np.broadcast_to(pol, each)
        elif pol.shape != each:
            raise ValueError('array `{:s}` should be of shape {:s} or {:s}, not {:s}'.format(name, str(one), str(each), str(pol.shape)))
        return np.ascontiguousarray(pol, dtype=self.dtype)

    def _evaluate(self, prob, n_iter, rel_dp, tol, check_every, form):
        """the evaluation of the members listed in `prob`, from the values set: (steps run [P], statistics
        [n_checks][P][2] or None, reference costs [n_iter][P])"""
        ref_flat = self._ref_flat(rel_dp)
        if tol is None:
            refs = prob.eval_policy(n_iter, rel_dp, ref_flat, form == 'resident')
            return np.full(prob.P, n_iter, dtype=np.int32), None, refs
        return prob.eval_policy_until(n_iter, rel_dp, ref_flat, check_every, tol, form == 'resident')

    def _records(self, members, n_done, stats, refs, n_iter, rel_dp, tol, check_every):
        """the solo SweepConvergence of every member of `members` (positions in the arrays of one chunk)"""
        schedule = conv.check_schedule(n_iter, check_every)
        out = []
        for p in members:
            checked = [k for k in schedule if k <= n_done[p]]
            checks = [(k, stats[c, p, 0], stats[c, p, 1]) for c, k in enumerate(checked)]
            out.append(DPSolver._sweep_record(tol, check_every, int(n_done[p]), checks, refs[:n_done[p], p].copy(), rel_dp))
        return out

    def _evaluation_info(self, form):
        S, rs = int(np.prod(self.dims)), self.dtype.itemsize
        self.backend_info['evaluation'] = form
        self.backend_info['evaluation_lds_bytes'] = (2 * S * rs + codegen.FAMILY_RESIDENT_REDUCTION_BYTES
                                                     if form == 'resident' else 0)

    def _check_evaluation(self, n_iter, rel_dp, tol, check_every, what):
        if tol is not None:
            tol, check_every = conv.validate(tol, check_every)
            if n_iter < 1:
                raise ValueError('{} with tol needs n_iter >= 1, not {!r}'.format(what, n_iter))
        if n_iter < (1 if rel_dp else 0):
            raise ValueError('{} needs n_iter >= {}, not {!r}'.format(what, 1 if rel_dp else 0, n_iter))
        return tol, check_every

    def eval_policy(self, pol, n_iter, rel_dp=False, J_zero=None, J_ref_full=False, tol=None, check_every=1):
        """`DPSolver.eval_policy` of every member, stacked, without its progress lines.  pol: shape dims + (nu,)
        (every member's policy) or (P,) + dims + (nu,); J_zero: dims or (P,) + dims, zeros by default.  Returns
        J_pol of shape (P,) + dims, or with rel_dp (J_pol, J_ref), J_ref of shape (P,) or with J_ref_full a list of
        P arrays (one reference cost per step the member ran).  With `tol` a member stops at its own first checked
        step whose span is <= tol: member p equals the solo call with n_iter = the steps it ran, and
        last_convergence[p] is the solo record.  A time-dependent system is evaluated at time index 0."""
        tol, check_every = self._check_evaluation(n_iter, rel_dp, tol, check_every, 'eval_policy')
        self.last_convergence = None
        pol = self._policy(pol)
        J0 = self._start(np.zeros(self.dims) if J_zero is None else J_zero, False, 'J_zero')
        form = self._evaluation_form(n_iter)
        tabs = self._tables(None if self.stationnary else 0)
        J = np.empty((self.P,) + self.dims, dtype=self.dtype)
        per_member, records = [None] * self.P, [None] * self.P

        def work(prob, a, b):
            prob.set_policy(pol[a:b])
            n_done, stats, refs = self._evaluate(prob, n_iter, rel_dp, tol, check_every, form)
            J[a:b] = prob.get_value()
            for p in range(b - a):
                per_member[a + p] = refs[:n_done[p], p].copy()
            if tol is not None:
                records[a:b] = self._records(range(b - a), n_done, stats, refs, n_iter, rel_dp, tol, check_every)
        self._run(tabs, J0, work, evaluation=True)
        self._evaluation_info(form)
        if tol is not None:
            self.last_convergence = records
        if rel_dp:
            return J, (per_member if J_ref_full else np.array([r[-1] for r in per_member]))
        return J

    def policy_iteration(self, pol_init, n_val, n_pol=1, rel_dp=False, tol=None, check_every=1):
        """`DPSolver.policy_iteration` of every member, stacked, without its progress lines: (J_pol, pol) of shapes
        (P,) + dims and (P,) + dims + (nu,); J_pol is (J_diff, J_ref) with rel_dp, J_ref of shape (P,).  With `tol`
        every evaluation stops per member as in `eval_policy`, a member whose improvement step returns exactly the
        policy it was given is stable and leaves the list of members still running, and last_convergence[p] is the
        solo PolicyIterationConvergence.  The improvement is a family sweep; the policy it writes becomes the next
        evaluation's input on the device (the two buffers swap), and `same policy` is decided there."""
        tol, check_every = self._check_evaluation(n_val, rel_dp, tol, check_every, 'policy_iteration')
        self.last_convergence = None
        pol0 = self._policy(pol_init, 'pol_init')
        form = self._evaluation_form(n_val)
        tabs = self._tables(None if self.stationnary else 0)
        ref_flat = self._ref_flat(rel_dp)
        J = np.zeros((self.P,) + self.dims, dtype=self.dtype)
        pol = pol0.copy()
        idx = np.zeros((self.P,) + self.dims, dtype=np.int32)
        J_ref = np.zeros(self.P)
        evaluations = [[] for _ in range(self.P)]
        n_improvements, stable = np.zeros(self.P, dtype=int), np.zeros(self.P, dtype=bool)
        zeros = np.zeros((self.P,) + self.dims, dtype=self.dtype)

        def work(prob, a, b):
            def evaluate(members):
                """the members listed (positions in the chunk) from zeros, under the prescribed policy"""
                prob.set_value(zeros[a:b])
                prob.set_members(members)
                n_done, stats, refs = self._evaluate(prob, n_val, rel_dp, tol, check_every, form)
                J[a + members] = prob.get_value()[members]
                if rel_dp:
                    J_ref[a + members] = [refs[n_done[p] - 1, p] for p in members]
                if tol is not None:
                    for p, rec in zip(members, self._records(members, n_done, stats, refs, n_val, rel_dp, tol, check_every)):
                        evaluations[a + p].append(rec)
            prob.set_policy(pol0[a:b])
            active = np.arange(b - a)
            evaluate(active)
            for k in range(n_pol):
                # the improvement: one family sweep of the members still running, from their evaluations
                prob.set_value(J[a:b])
                prob.set_members(active)
                prob.sweep(0.0, rel_dp, ref_flat)
                n_improvements[a + active] += 1
                same = prob.compare_policy()[active] if tol is not None else np.zeros(active.size, dtype=bool)
                last = k == n_pol - 1
                if same.any() or last:
                    # a member that ends here returns this sweep's policy (a stable one: equal to the one it was given)
                    pol_new, idx_new = prob.get_policy()
                    ends = active if last else active[same]
                    pol[a + ends], idx[a + ends] = pol_new[ends], idx_new[ends]
                stable[a + active[same]] = True          # (J is already the evaluation of this policy)
                active = active[~same]
                if active.size == 0:
                    break
                prob.take_policy()
                evaluate(active)
        self._run(tabs, zeros, work, evaluation=True)
        self._evaluation_info(form)
        self.last_policy_index = idx
        if tol is not None:
            self.last_convergence = [conv.PolicyIterationConvergence(evaluations[p], int(n_improvements[p]), bool(stable[p]))
                                     for p in range(self.P)]
        return ((J, J_ref) if rel_dp else J), pol

    # ------------------------------------------------------------------ Monte Carlo evaluation
    # a run is cut into launches of at most this many steps, as the solo call's; the state stays on the device
    steps_per_launch = DPSolver.steps_per_launch

    def _mc_seeds(self, seed):
        """the seed of every member: one integer for all of them (common random numbers) or a sequence of P"""
        if np.ndim(seed) == 0:
            return [mc.check_seed(seed)] * self.P
        seeds = list(seed)
        if len(seeds) != self.P:
            raise ValueError('seed: one integer or a sequence of {} (one per member), not {} values'.format(self.P, len(seeds)))
        return [mc.check_seed(s) for s in seeds]

    def _mc_laws(self, law):
        """[(grid, proba)] of every member in float64, checked as the solo call checks its law: None (each member's
        own), one (grid, proba) for all members, or a sequence of P of them.  All have the same number of points."""
        for p, s in enumerate(self.solvers):
            if self._law_points(s) == 0:
                raise NotImplementedError('member {}: a deterministic system has nothing to draw: use simulate(pol, x0, '
                                          'n_steps=...)'.format(p))
        if law is None:
            each = [None] * self.P
        else:
            try:
                shared = len(law) == 2 and np.ndim(law[0][0]) == 0      # (grid, proba): its first entry is a number
            except (TypeError, IndexError):
                raise ValueError('law must be (grid, proba), or a sequence of {} of them'.format(self.P))
            each = [law] * self.P if shared else list(law)
            if len(each) != self.P:
                raise ValueError('law: one (grid, proba) or a sequence of {} (one per member), not {}'.format(self.P, len(each)))
        laws = [s._mc_law(lw) for s, lw in zip(self.solvers, each)]
        n = len(laws[0][1])
        rs = self.dtype.itemsize
        for p, (grid, proba) in enumerate(laws):
            if len(proba) != n:
                raise ValueError('member {}: a law of {} points, member 0\'s has {}: the laws of a family have the same '
                                 'number of points'.format(p, len(proba), n))
        if (n - 1) * 8 + n * rs > 65536:
            raise ValueError('a law of {} points needs a draw table of {} bytes: at most 65536'.format(n, (n - 1) * 8 + n * rs))
        return laws

    def monte_carlo_draws(self, seed, n_traj, n_steps, law=None, traj_offset=0):
        """`DPSolver.monte_carlo_draws` of every member, stacked (numpy alone): (indices, w) of shapes
        (P, n_steps, n_traj).  seed and law as in `monte_carlo`."""
        seeds = self._mc_seeds(seed)
        laws = self._mc_laws(law)
        out = [s.monte_carlo_draws(seeds[p], n_traj, n_steps, law=laws[p], traj_offset=traj_offset)
               for p, s in enumerate(self.solvers)]
        return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])

    def _mc_member_bytes(self, B, n_law, occupancy):
        """bytes of device arrays one member takes in a Monte Carlo run beside _member_bytes (the value, index and
        box arrays of the handle are allocated with it, so they count): its policy, states and sums, the outside
        counts, the occupancy, its rows of the draw tables and its seed"""
        S, d, rs = int(np.prod(self.dims)), len(self.dims), self.dtype.itemsize
        return (self.nu * S + (d + 1) * B) * rs + 8 * B + (8 * S if occupancy else 0) + n_law * (8 + rs) + 8

    def _mc_inputs(self, x0, n_steps, n_burn, n_traj, seed, traj_offset):
        """what every Monte Carlo call checks of its start states, steps, seeds and trajectory ids: (x0 (P, B, d), B,
        n_steps, n_burn, the members' seeds, steps_per_launch)"""
        d = len(self.dims)
        x0 = np.asarray(x0, dtype=float)
        shapes = '({},) with n_traj, (B, {}) or ({}, B, {})'.format(d, d, self.P, d)
        if x0.ndim == 1:
            if x0.shape != (d,):
                raise ValueError('x0 must have shape {}, not {}'.format(shapes, x0.shape))
            if n_traj is None:
                raise ValueError('give n_traj with a single start state')
            if int(n_traj) < 1:
                raise ValueError('n_traj must be at least 1')
            x0 = np.broadcast_to(x0, (int(n_traj), d))
        elif x0.ndim not in (2, 3) or x0.shape[-1] != d or (x0.ndim == 3 and x0.shape[0] != self.P):
            raise ValueError('x0 must have shape {}, not {}'.format(shapes, x0.shape))
        elif n_traj is not None and int(n_traj) != x0.shape[-2]:
            raise ValueError('n_traj = {} but x0 holds {} start states'.format(n_traj, x0.shape[-2]))
        B = x0.shape[-2]
        if x0.ndim == 2:
            x0 = np.broadcast_to(x0, (self.P, B, d))
        n_steps, n_burn = int(n_steps), int(n_burn)
        if n_steps < 1 or not 0 <= n_burn < n_steps:
            raise ValueError('need n_steps >= 1 and 0 <= n_burn < n_steps')
        seeds = self._mc_seeds(seed)
        DPSolver._mc_ids(B, traj_offset)
        spl = int(self.steps_per_launch)
        if spl < 1:
            raise ValueError('steps_per_launch must be at least 1')
        return x0, B, n_steps, n_burn, seeds, spl

    def monte_carlo(self, pol, x0, n_steps, seed=0, n_burn=0, n_traj=None, law=None, occupancy=False, traj_offset=0, t0=0):
        """`DPSolver.monte_carlo` of every member in one device call per cut of the steps (kernel
        sdp_family_montecarlo, csrc/sdp_family_mc_kernel.h): a `montecarlo.FamilyMonteCarloResult`, member p of
        every field equal, bit for bit, to what `solvers[p].monte_carlo` returns on its device path.

        pol   : (P,) + dims + (nu,), what `policy_iteration` or `value_iteration` returns (or dims + (nu,): every
                member's policy)
        x0    : (d,) with n_traj given, (B, d) shared by all members, or (P, B, d)
        seed  : one integer -- every member then sees the same uniform draws (common random numbers: compare two
                members with `res.paired(p, q)`) -- or a sequence of P integers
        law   : None (each member's own law), one (grid, proba) for all members, or a sequence of P of them; all
                with the same number of points
        n_burn, occupancy, traj_offset, t0: as in the solo call.
        Not built here: time-indexed policies and models that look data up as data[k] (`monte_carlo_horizon` runs
        both); deterministic members (`simulate`)."""
        d = len(self.dims)
        # ---- everything that is refused, before a device is touched
        laws = self._mc_laws(law)
        pol = np.asarray(pol)
        one = self.dims + (self.nu,)
        if pol.ndim > len(one) + 1 and pol.shape[-len(one):] == one:
            raise NotImplementedError('pol of shape {}: a time-indexed policy (a leading axis beside the members\') is not '
                                      'what monte_carlo takes: use monte_carlo_horizon'.format(pol.shape))
        pol = self._policy(pol)
        x0, B, n_steps, n_burn, seeds, spl = self._mc_inputs(x0, n_steps, n_burn, n_traj, seed, traj_offset)
        tabs = self._tables(None if self.stationnary else 0)
        if tabs['time_specialized']:
            raise NotImplementedError('the members\' model looks data up at a concrete time index (data[k]): monte_carlo '
                                      'has no table of constants per step: use monte_carlo_horizon')
        # ---- member-major device arrays
        dt = self.dtype
        S, n_law = int(np.prod(self.dims)), len(laws[0][1])
        pol_d = np.ascontiguousarray(np.moveaxis(pol, -1, 1), dtype=dt).reshape(self.P, self.nu, S)       # [P][nu][S]
        x0_d = np.ascontiguousarray(np.moveaxis(x0, -1, 1), dtype=dt)                                     # [P][d][B]
        cum = np.ascontiguousarray([mc.cumulative(proba) for _, proba in laws])                           # [P][n_law]
        law_d = np.ascontiguousarray([grid for grid, _ in laws], dtype=dt)
        seeds_d = np.array(seeds, dtype=np.uint64)
        cost_sum = np.empty((self.P, B), dtype=dt)
        n_out = np.empty((self.P, B), dtype=np.int64)
        x_final = np.empty((self.P, B, d), dtype=dt)
        occ = np.empty((self.P,) + self.dims, dtype=np.int64) if occupancy else None

        def work(prob, a, b):
            c, n, xf, o = prob.montecarlo(pol_d[a:b], x0_d[a:b], n_steps, n_burn, seeds_d[a:b], traj_offset, cum[a:b],
                                          law_d[a:b], t0, spl, occupancy)
            cost_sum[a:b], n_out[a:b], x_final[a:b] = c, n, np.moveaxis(xf, 1, 2)
            if occupancy:
                occ[a:b] = o.astype(np.int64).reshape((b - a,) + self.dims)
        self._run(tabs, None, work, mc_bytes=self._mc_member_bytes(B, n_law, occupancy))
        self.backend_info['monte_carlo'] = dict(members=self.P, n_traj=B, chunks=self.backend_info['chunks'],
                                                launches=self.backend_info['chunks'] * (-(-n_steps // min(spl, 1 << 30))))
        return mc.FamilyMonteCarloResult(cost_sum, n_out, x_final, occ, n_steps, n_burn, seeds, int(traj_offset), t0, 'device')

    # ------------------------------------------------------------------ closed loops over a horizon
    # the policy of a time-indexed run goes up in cuts of whole steps of at most this many bytes (of all members of a
    # chunk together), as the solo calls cut theirs; the state stays on the device, so no cut changes a bit
    horizon_chunk_bytes = DPSolver.horizon_chunk_bytes

    def _horizon_policy(self, pol, n_steps, t0):
        """(the policy as [P][T_c][nu][S] in the family's reals, control axis first -- T_c = n_steps slices of a
        time-indexed policy, the steps t0 .. t0 + n_steps - 1, or the one slice of a stationary policy --, whether it is
        time-indexed): from dims + (nu,), (P,) + dims + (nu,) or (P, T_pol) + dims + (nu,)"""
        pol = np.asarray(pol)
        one = self.dims + (self.nu,)
        S = int(np.prod(self.dims))
        if pol.shape in (one, (self.P,) + one):
            each = np.broadcast_to(pol, (self.P,) + one)
            return np.ascontiguousarray(np.moveaxis(each, -1, 1), dtype=self.dtype).reshape(self.P, 1, self.nu, S), False
        if pol.ndim != len(one) + 2 or pol.shape[0] != self.P or pol.shape[2:] != one:
            raise ValueError('pol must have shape {} (one stationary policy), {} (one per member) or ({}, T_pol) + {} (a '
                             'time-indexed one per member), not {}'.format(one, (self.P,) + one, self.P, one, pol.shape))
        if int(t0) != t0:
            raise ValueError('t0 = {} must be an integer to index a time-indexed policy'.format(t0))
        if t0 < 0 or t0 + n_steps > pol.shape[1]:
            raise ValueError('t0 = {} and n_steps = {} need the policy steps {} .. {}: the policy has T_pol = {}'.format(
                t0, n_steps, t0, t0 + n_steps - 1, pol.shape[1]))
        part = np.moveaxis(pol[:, int(t0):int(t0) + n_steps], -1, 2)
        return np.ascontiguousarray(part, dtype=self.dtype).reshape(self.P, n_steps, self.nu, S), True

    def _horizon_tables(self, n_steps, t0):
        """(tabs, table, timed) of a run of the steps t0 .. t0 + n_steps - 1, no GPU needed: the tables of the family at
        the first step, and the lifted constants of every member and step in the family's reals, rounded once --
        [P][n_steps][n_params] for members whose model is traced per step (`data[k]`; timed), row (p, k) what row k
        of `solvers[p]._horizon_table` holds, or [P][1][n_params] for members whose model is symbolic in time: one row
        per member, read at every step.  A family has no host path: a step that does not trace is refused, and so are
        steps or members whose traces differ in structure."""
        symbolic = self.stationnary or all(not isinstance(_trace_member(s, None), TraceError) for s in self.solvers)
        if symbolic:
            tabs = self._tables(None if self.stationnary else t0)
            return tabs, np.ascontiguousarray(tabs['prm'].reshape(self.P, 1, -1)), False
        if int(t0) != t0:
            raise ValueError('t0 = {} must be an integer: the members\' model looks data up at a concrete time index '
                             '(data[k])'.format(t0))
        t0 = int(t0)
        rows, first = [], None
        for p, s in enumerate(self.solvers):
            mine = []
            for t in range(t0, t0 + n_steps):
                model = _trace_member(s, t)
                if isinstance(model, TraceError):
                    raise NotImplementedError('member {} at step {}: dyn / cost do not trace ({}): a family runs traced '
                                              'models only, there is no host path'.format(p, t, model))
                if first is None:
                    first = model
                elif model.structure_key() != first.structure_key():
                    raise ValueError(_structure_message(p, model, first, ' at step {}'.format(t)))
                mine.append(model.param_values())
            rows.append(mine)
        tabs = self._tables(t0)
        table = np.ascontiguousarray(np.asarray(rows, dtype=float).reshape(self.P, n_steps, -1), dtype=self.dtype)
        return tabs, table, True

    def _horizon_bytes(self, pol_d, table):
        """bytes of device arrays one member takes in a run over a horizon beside its states: its policy steps and its
        rows of the table of constants"""
        return (pol_d.shape[1] * pol_d.shape[2] * pol_d.shape[3] + table.shape[1] * table.shape[2]) * self.dtype.itemsize

    def _horizon_info(self, chunks, B, n_steps, pol_d, timed, prm_timed, spl):
        """backend_info['horizon'] of the call that just ran in the member chunks `chunks`: the cuts, restated from the
        library's rule"""
        slice_bytes = pol_d.shape[2] * pol_d.shape[3] * self.dtype.itemsize
        step_chunks = launches = 0
        for a, b in chunks:
            per = min(n_steps, max(1, int(self.horizon_chunk_bytes) // ((b - a) * slice_bytes))) if timed else n_steps
            for c in range(0, n_steps, per):
                step_chunks += 1
                launches += 1 if spl is None else -(-min(per, n_steps - c) // spl)
        self.backend_info['horizon'] = dict(members=self.P, n_traj=B, n_steps=n_steps, timed=bool(timed),
                                            time_specialized=bool(prm_timed), chunks=len(chunks), step_chunks=step_chunks,
                                            launches=launches)

    def _simulate_inputs(self, x0, w, n_steps):
        """what every closed loop with prescribed perturbations checks of its start states and sequences: (x0 (P, B, d),
        w (P, >= T, B) or None, B, T, whether x0 was a single state)"""
        d = len(self.dims)
        x0 = np.asarray(x0, dtype=float)
        single = x0.ndim == 1
        if single:
            x0 = x0[None]
        if x0.ndim not in (2, 3) or x0.shape[-1] != d or (x0.ndim == 3 and x0.shape[0] != self.P):
            raise ValueError('x0 must have shape ({0},), (B, {0}) or ({1}, B, {0}), not {2}'.format(
                d, self.P, x0.shape[1:] if single else x0.shape))
        B = x0.shape[-2]
        if B < 1:
            raise ValueError('x0 holds no start state')
        if x0.ndim == 2:
            x0 = np.broadcast_to(x0, (self.P, B, d))
        if self.W:
            if w is None:
                raise ValueError('stochastic members need the perturbation sequence(s) w')
            w = np.asarray(w, dtype=float)
            if w.ndim == 1:
                w = w.reshape(-1, 1)
            if w.ndim not in (2, 3) or w.shape[-1] != B or (w.ndim == 3 and w.shape[0] != self.P):
                raise ValueError('w must have shape (T,), (T, {0}) or ({1}, T, {0}), not {2}'.format(B, self.P, w.shape))
            T = w.shape[-2] if n_steps is None else int(n_steps)
            if w.shape[-2] < T:
                raise ValueError('w holds {} steps, n_steps = {}'.format(w.shape[-2], T))
            if w.ndim == 2:
                w = np.broadcast_to(w, (self.P,) + w.shape)
        else:
            if n_steps is None:
                raise ValueError('give n_steps for deterministic members')
            T, w = int(n_steps), None
        if T < 1:
            raise ValueError('need n_steps >= 1')
        return x0, w, B, T, single

    def simulate(self, pol, x0, w=None, n_steps=None, t0=0):
        """`DPSolver.simulate` of every member in one device call per cut of the steps (kernel sdp_family_simulate,
        csrc/sdp_family_horizon_kernel.h): (x (P, T+1, B, d), u (P, T, B, nu), g (P, T, B)), member p equal, bit for
        bit, to what `solvers[p].simulate(pol[p], x0[p], w[p], n_steps, t0)` returns on its device path.

        pol : dims + (nu,) (one stationary policy for all members), (P,) + dims + (nu,) (one per member), or
              (P, T_pol) + dims + (nu,), what `bellman_recursion` returns: step k then runs at time index t0 + k with
              the controls of pol[p, t0 + k].  A time-indexed policy always carries both leading axes.
        x0  : (d,) -- the results then have no B axis --, (B, d) shared by all members, or (P, B, d)
        w   : (T,), (T, B) shared by all members, or (P, T, B); None for deterministic members (then give n_steps)
        Models that are symbolic in time and models that look data up as data[k] (traced per member and step) both
        run; there is no host path."""
        d = len(self.dims)
        # ---- everything that is refused, before a device is touched
        x0, w, B, T, single = self._simulate_inputs(x0, w, n_steps)
        pol_d, timed = self._horizon_policy(pol, T, t0)
        tabs, table, prm_timed = self._horizon_tables(T, t0)
        # ---- member-major device arrays
        dt = self.dtype
        rs = dt.itemsize
        x0_d = np.ascontiguousarray(np.moveaxis(x0, -1, 1), dtype=dt)                                     # [P][d][B]
        w_d = np.ascontiguousarray(w[:, :T], dtype=dt) if w is not None else None                        # [P][T][B]
        x = np.empty((self.P, T + 1, B, d), dtype=dt)
        u = np.empty((self.P, T, B, self.nu), dtype=dt)
        g = np.empty((self.P, T, B), dtype=dt)

        def work(prob, a, b):
            xs, us, g[a:b] = prob.simulate_h(pol_d[a:b], timed, table[a:b], prm_timed, self.horizon_chunk_bytes, x0_d[a:b],
                                             None if w_d is None else w_d[a:b], T, t0)
            x[a:b], u[a:b] = np.moveaxis(xs, 2, 3), np.moveaxis(us, 2, 3)
        extra = self._horizon_bytes(pol_d, table) + (d * B + (1 if self.W else 0) * T * B + (T + 1) * d * B
                                                     + T * self.nu * B + T * B) * rs
        self._horizon_info(self._run_horizon(tabs, work, extra), B, T, pol_d, timed, prm_timed, None)
        if single:
            return x[:, :, 0], u[:, :, 0], g[:, :, 0]
        return x, u, g

    def _run_horizon(self, tabs, work, extra):
        """`_run` of a closed loop over a horizon whose arrays take `extra` bytes a member beside the handle's: the
        member chunks it ran in"""
        return self._run(tabs, None, work, horizon=dict(source=codegen.family_horizon_unit(tabs['model'], self.dtype), bytes=int(extra)))

    def monte_carlo_horizon(self, pol, x0, n_steps, seed=0, n_burn=0, n_traj=None, law=None, occupancy=False, traj_offset=0,
                            t0=0):
        """`DPSolver.monte_carlo` of every member under a policy of any of the three shapes `simulate` takes, in one
        device call per cut of the steps (kernel sdp_family_montecarlo_h, csrc/sdp_family_horizon_kernel.h): a
        `montecarlo.FamilyMonteCarloResult` with path 'device', member p of every field equal, bit for bit, to what
        `solvers[p].monte_carlo(pol[p], ...)` returns on its device path.  The other arguments are `monte_carlo`'s.
        Models that are symbolic in time and models that look data up as data[k] both run; a stationary policy on a
        symbolic model gives the bits of `monte_carlo`.  Launches are cut at the policy's uploads
        (horizon_chunk_bytes) and at steps_per_launch.  Not built: deterministic members (use `simulate`)."""
        d = len(self.dims)
        # ---- everything that is refused, before a device is touched
        laws = self._mc_laws(law)
        x0, B, n_steps, n_burn, seeds, spl = self._mc_inputs(x0, n_steps, n_burn, n_traj, seed, traj_offset)
        pol_d, timed = self._horizon_policy(pol, n_steps, t0)
        tabs, table, prm_timed = self._horizon_tables(n_steps, t0)
        # ---- member-major device arrays
        dt = self.dtype
        n_law = len(laws[0][1])
        x0_d = np.ascontiguousarray(np.moveaxis(x0, -1, 1), dtype=dt)                                     # [P][d][B]
        cum = np.ascontiguousarray([mc.cumulative(proba) for _, proba in laws])                           # [P][n_law]
        law_d = np.ascontiguousarray([grid for grid, _ in laws], dtype=dt)
        seeds_d = np.array(seeds, dtype=np.uint64)
        cost_sum = np.empty((self.P, B), dtype=dt)
        n_out = np.empty((self.P, B), dtype=np.int64)
        x_final = np.empty((self.P, B, d), dtype=dt)
        occ = np.empty((self.P,) + self.dims, dtype=np.int64) if occupancy else None

        def work(prob, a, b):
            c, n, xf, o = prob.montecarlo_h(pol_d[a:b], timed, table[a:b], prm_timed, self.horizon_chunk_bytes, x0_d[a:b],
                                            n_steps, n_burn, seeds_d[a:b], traj_offset, cum[a:b], law_d[a:b], t0, spl,
                                            occupancy)
            cost_sum[a:b], n_out[a:b], x_final[a:b] = c, n, np.moveaxis(xf, 1, 2)
            if occupancy:
                occ[a:b] = o.astype(np.int64).reshape((b - a,) + self.dims)
        # (_mc_member_bytes counts one policy slice: the others and the table are what the horizon adds)
        S = int(np.prod(self.dims))
        extra = self._mc_member_bytes(B, n_law, occupancy) + self._horizon_bytes(pol_d, table) - self.nu * S * dt.itemsize
        self._horizon_info(self._run_horizon(tabs, work, extra), B, n_steps, pol_d, timed, prm_timed, min(spl, 1 << 30))
        return mc.FamilyMonteCarloResult(cost_sum, n_out, x_final, occ, n_steps, n_burn, seeds, int(traj_offset), t0, 'device')

    # ------------------------------------------------------------------ lookahead at arbitrary states
    def _lookahead_boxes(self, t_k):
        """control_box of every member, traced with a symbolic time index and with EVERY constant lifted: a list of
        TracedBox of one structure.  There is no host fallback in a family: a box that does not trace, traces only at
        a concrete time index or uses inexact operations is refused, and so are boxes of different structures."""
        boxes = []
        for p, s in enumerate(self.solvers):
            tb = s._trace_box_now(None if self.stationnary else (0 if t_k is None else t_k))
            if isinstance(tb, TraceError):
                raise NotImplementedError('member {}: control_box does not trace ({}): a family makes every lattice on the '
                                          'device, there is no host path'.format(p, tb))
            if tb.t_value is not None:
                raise NotImplementedError('member {}: control_box traces only at a concrete time index (data[k]): a box '
                                          'function per step is not built for families'.format(p))
            tb.lift_constants()
            if p and tb.structure_key() != boxes[0].structure_key():
                raise ValueError(_structure_message(p, tb, boxes[0], what=_BOX))
            boxes.append(tb)
        return boxes

    def _lookahead_tables(self, t_k, extra_bytes):
        """(tabs, look) of a lookahead call at the time index t_k (None: stationary members), no GPU needed: the
        tables of the sweep, and for `_run` the source of the lookahead unit, the members' box constants [P][n_box]
        and control steps [P][nu] in float64 and the bytes a member takes beside the handle's"""
        for p, s in enumerate(self.solvers):
            if isinstance(_trace_member(s, None), TraceError):       # (it traces at a concrete step only: the constructor saw to that)
                raise NotImplementedError('member {}: its model looks data up at a concrete time index (data[k]): a table '
                                          'of constants per step is not built for families'.format(p))
        boxes = self._lookahead_boxes(t_k)
        tabs = self._tables(None if self.stationnary else t_k)
        bprm = np.ascontiguousarray([b.param_values() for b in boxes], dtype=np.float64).reshape(self.P, -1)
        steps = np.ascontiguousarray([s.control_steps for s in self.solvers], dtype=np.float64).reshape(self.P, self.nu)
        if np.isnan(steps).any():
            raise ValueError('member {}: a control step is NaN'.format(int(np.argwhere(np.isnan(steps))[0][0])))
        look = dict(source=codegen.family_lookahead_unit(tabs['model'], boxes[0], self.dtype, tabs['lanes']),
                    bprm=bprm, steps=steps, bytes=int(extra_bytes) + 8 * (bprm.shape[1] + self.nu))
        return tabs, look

    def _cost_to_go(self, J_next):
        """J_next of every member, (P,) + dims, from dims or (P,) + dims; a further leading axis is a time-indexed
        cost-to-go, which is not built"""
        J_next = np.asarray(J_next)
        if J_next.ndim > len(self.dims) + 1 and J_next.shape[-len(self.dims):] == self.dims:
            raise NotImplementedError('J_next of shape {}: a time-indexed cost-to-go (a leading axis beside the members\') is '
                                      'not built for families'.format(J_next.shape))
        return self._start(J_next, False)

    def lookahead(self, J_next, x, t_k=None):
        """`DPSolver.lookahead` of every member in one device call (kernel sdp_family_lookahead,
        csrc/sdp_family_lookahead_kernel.h): (J_opt (P, B), u_opt (P, B, nu), idx (P, B) int32), member p equal, bit for
        bit, to what `solvers[p].lookahead(J_next[p], x[p], t_k)` returns on its device path.

        J_next : dims (the same cost-to-go for every member) or (P,) + dims
        x      : (d,), (B, d) shared by all members, or (P, B, d); 4-byte members round them once
        t_k    : the time index (time-dependent members)
        A state without a valid lattice gives NaN, NaN, -1.  Every lattice is made on the device from the traced
        control_box of the member; there is no host path.  Not built: a time-indexed J_next, models that look data up
        as data[k]."""
        d = len(self.dims)
        J0 = self._cost_to_go(J_next)
        x = np.asarray(x, dtype=float)
        if x.ndim == 1:
            x = x[None]
        if x.ndim not in (2, 3) or x.shape[-1] != d or (x.ndim == 3 and x.shape[0] != self.P):
            raise ValueError('x must have shape ({0},), (B, {0}) or ({1}, B, {0}), not {2}'.format(d, self.P, x.shape))
        B = x.shape[-2]
        if x.ndim == 2:
            x = np.broadcast_to(x, (self.P, B, d))
        if self.stationnary:
            t_k = None
        elif t_k is None:
            raise ValueError('a time-dependent system needs the time index t_k')
        rs = self.dtype.itemsize
        tabs, look = self._lookahead_tables(t_k, (d + 1 + self.nu) * B * rs + 4 * B)
        J = np.empty((self.P, B), dtype=self.dtype)
        u = np.empty((self.P, B, self.nu), dtype=self.dtype)
        idx = np.empty((self.P, B), dtype=np.int32)
        if B == 0:
            return J, u, idx
        x_d = np.ascontiguousarray(np.moveaxis(x, -1, 1), dtype=self.dtype)                             # [P][d][B]

        def work(prob, a, b):
            J[a:b], u_d, idx[a:b] = prob.lookahead(x_d[a:b], 0.0 if t_k is None else t_k)
            u[a:b] = np.moveaxis(u_d, 1, 2)
        self._run(tabs, J0, work, look=look)
        self.backend_info.update(lookahead_path='device', lookahead_box='device', box_constants=int(look['bprm'].shape[1]))
        return J, u, idx

    def monte_carlo_lookahead(self, J_next, x0, n_steps, seed=0, n_burn=0, n_traj=None, law=None, occupancy=False,
                              traj_offset=0, t0=0):
        """`DPSolver.monte_carlo_lookahead` of every member in one device call per cut of the steps (kernel
        sdp_family_montecarlo_lookahead, csrc/sdp_family_lookahead_kernel.h): a `montecarlo.FamilyMonteCarloResult`,
        member p of every field equal, bit for bit, to what `solvers[p].monte_carlo_lookahead` returns on its device
        path -- the sizings of a study ranked under the controller that would run, not under the interpolated policy.

        J_next : dims or (P,) + dims, the cost-to-go every step looks ahead into
        x0, seed, law, n_burn, n_traj, occupancy, traj_offset, t0 : as in `monte_carlo`.  `law` is the law the PLANT
                 draws from; the expectation inside the backup always runs over member p's own discretised law.
        Not built: a time-indexed J_next, models that look data up as data[k], deterministic members."""
        d = len(self.dims)
        # ---- everything that is refused, before a device is touched
        for p, s in enumerate(self.solvers):
            if self._law_points(s) == 0:
                raise ValueError('member {}: a deterministic system has nothing to draw: use simulate_lookahead(J_next, x0, '
                                 'n_steps=...)'.format(p))
        laws = self._mc_laws(law)
        J0 = self._cost_to_go(J_next)
        x0, B, n_steps, n_burn, seeds, spl = self._mc_inputs(x0, n_steps, n_burn, n_traj, seed, traj_offset)
        dt = self.dtype
        S, n_law, rs = int(np.prod(self.dims)), len(laws[0][1]), self.dtype.itemsize
        extra = (d + 1) * B * rs + 8 * B + (8 * S if occupancy else 0) + n_law * (8 + rs) + 8
        tabs, look = self._lookahead_tables(None if self.stationnary else t0, extra)
        # ---- member-major device arrays
        x0_d = np.ascontiguousarray(np.moveaxis(x0, -1, 1), dtype=dt)                                     # [P][d][B]
        cum = np.ascontiguousarray([mc.cumulative(proba) for _, proba in laws])                           # [P][n_law]
        law_d = np.ascontiguousarray([grid for grid, _ in laws], dtype=dt)
        seeds_d = np.array(seeds, dtype=np.uint64)
        cost_sum = np.empty((self.P, B), dtype=dt)
        n_out = np.empty((self.P, B), dtype=np.int64)
        x_final = np.empty((self.P, B, d), dtype=dt)
        occ = np.empty((self.P,) + self.dims, dtype=np.int64) if occupancy else None

        def work(prob, a, b):
            c, n, xf, o = prob.montecarlo_lookahead(x0_d[a:b], n_steps, n_burn, seeds_d[a:b], traj_offset, cum[a:b],
                                                    law_d[a:b], t0, spl, occupancy)
            cost_sum[a:b], n_out[a:b], x_final[a:b] = c, n, np.moveaxis(xf, 1, 2)
            if occupancy:
                occ[a:b] = o.astype(np.int64).reshape((b - a,) + self.dims)
        self._run(tabs, J0, work, look=look)
        self.backend_info.update(lookahead_path='device', lookahead_box='device', box_constants=int(look['bprm'].shape[1]))
        self.backend_info['monte_carlo'] = dict(members=self.P, n_traj=B, chunks=self.backend_info['chunks'],
                                                launches=self.backend_info['chunks'] * (-(-n_steps // min(spl, 1 << 30))))
        return mc.FamilyMonteCarloResult(cost_sum, n_out, x_final, occ, n_steps, n_burn, seeds, int(traj_offset), t0, 'device')

    # ------------------------------------------------------------------ closed loops under lookahead controls over a horizon
    def _horizon_cost_to_go(self, J_next, n_steps, t0):
        """(the cost-to-go as [P][T_c][1][S] in the family's reals -- T_c = n_steps slices of a time-indexed one, the
        steps t0 .. t0 + n_steps - 1, or the one slice every step looks ahead into --, whether it is time-indexed): from
        dims, (P,) + dims or (P, T_J) + dims"""
        J_next = np.asarray(J_next)
        one = self.dims
        S = int(np.prod(self.dims))
        if J_next.shape in (one, (self.P,) + one):
            each = np.broadcast_to(J_next, (self.P,) + one)
            return np.ascontiguousarray(each, dtype=self.dtype).reshape(self.P, 1, 1, S), False
        if J_next.ndim != len(one) + 2 or J_next.shape[0] != self.P or J_next.shape[2:] != one:
            raise ValueError('J_next must have shape {} (one cost-to-go), {} (one per member) or ({}, T_J) + {} (a '
                             'time-indexed one per member), not {}'.format(one, (self.P,) + one, self.P, one, J_next.shape))
        if int(t0) != t0:
            raise ValueError('t0 = {} must be an integer to index a time-indexed cost-to-go'.format(t0))
        if t0 < 0 or t0 + n_steps > J_next.shape[1]:
            raise ValueError('t0 = {} and n_steps = {} need the cost-to-go steps {} .. {}: J_next has T_J = {}'.format(
                t0, n_steps, t0, t0 + n_steps - 1, J_next.shape[1]))
        part = J_next[:, int(t0):int(t0) + n_steps]
        return np.ascontiguousarray(part, dtype=self.dtype).reshape(self.P, n_steps, 1, S), True

    def _lookahead_horizon_tables(self, n_steps, t0):
        """(tabs, table, prm_timed, look) of a closed loop under lookahead controls over the steps t0 .. t0 + n_steps - 1,
        no GPU needed: what `_horizon_tables` returns -- so models that look data up as data[k] run, a row of constants
        per member and step -- and for `_run` the source of the unit, the members' box constants [P][n_box] and control
        steps [P][nu] in float64 and the bytes of these two rows (the caller adds what else a member takes).  The box is traced with a symbolic
        time index (`_lookahead_boxes`): its constants are per member, not per step."""
        boxes = self._lookahead_boxes(None if self.stationnary else t0)
        tabs, table, prm_timed = self._horizon_tables(n_steps, t0)
        bprm = np.ascontiguousarray([b.param_values() for b in boxes], dtype=np.float64).reshape(self.P, -1)
        steps = np.ascontiguousarray([s.control_steps for s in self.solvers], dtype=np.float64).reshape(self.P, self.nu)
        if np.isnan(steps).any():
            raise ValueError('member {}: a control step is NaN'.format(int(np.argwhere(np.isnan(steps))[0][0])))
        look = dict(source=codegen.family_lookahead_horizon_unit(tabs['model'], boxes[0], self.dtype, tabs['lanes']),
                    bprm=bprm, steps=steps, bytes=8 * (bprm.shape[1] + self.nu))
        return tabs, table, prm_timed, look

    def simulate_lookahead(self, J_next, x0, w=None, n_steps=None, t0=0):
        """`DPSolver.simulate_lookahead` of every member in one device call per cut of the steps (kernel
        sdp_family_simulate_lookahead, csrc/sdp_family_lookahead_horizon_kernel.h): (x (P, T+1, B, d), u (P, T, B, nu),
        g (P, T, B), q (P, T, B)), member p equal, bit for bit, to what `solvers[p].simulate_lookahead(J_next[p], x0[p],
        w[p], n_steps, t0)` returns, on its device path or -- models that look data up as data[k] -- its host path.

        J_next : dims (one cost-to-go for all members and steps), (P,) + dims (one per member), or (P, T_J) + dims, a
                 time-indexed one: step k of the call then looks ahead into J_next[p, t0 + k].  A time-indexed
                 cost-to-go always carries both leading axes.  From `bellman_recursion`'s (J, pol) with final cost J_fin
                 (P,) + dims that is `np.concatenate([J[:, 1:], J_fin[:, None]], axis=1)`: step k decides with the
                 cost-to-go of k + 1.
        x0, w, n_steps, t0 : as in `simulate` (the single-trajectory form included)
        q is the minimised expected value of every step.  A state without a valid lattice gives NaN controls and q, and
        the trajectory goes on as the model maps them.  Models that are symbolic in time and models that look data up as
        data[k] (traced per member and step) both run; every lattice is made on the device from the member's traced
        control_box, whose constants are per member, not per step; there is no host path."""
        d = len(self.dims)
        # ---- everything that is refused, before a device is touched
        x0, w, B, T, single = self._simulate_inputs(x0, w, n_steps)
        V_d, timed = self._horizon_cost_to_go(J_next, T, t0)
        dt = self.dtype
        rs = dt.itemsize
        tabs, table, prm_timed, look = self._lookahead_horizon_tables(T, t0)
        # (a member's cost-to-go slices and table rows, its start states, perturbations, states and the three outputs)
        look['bytes'] += self._horizon_bytes(V_d, table) + (d * B + (1 if self.W else 0) * T * B + (T + 1) * d * B
                                                            + T * self.nu * B + 2 * T * B) * rs
        # ---- member-major device arrays
        V_s = V_d.reshape(self.P, V_d.shape[1], -1)                                                       # [P][T or 1][S]
        x0_d = np.ascontiguousarray(np.moveaxis(x0, -1, 1), dtype=dt)                                     # [P][d][B]
        w_d = np.ascontiguousarray(w[:, :T], dtype=dt) if w is not None else None                        # [P][T][B]
        x = np.empty((self.P, T + 1, B, d), dtype=dt)
        u = np.empty((self.P, T, B, self.nu), dtype=dt)
        g = np.empty((self.P, T, B), dtype=dt)
        q = np.empty((self.P, T, B), dtype=dt)

        def work(prob, a, b):
            xs, us, g[a:b], q[a:b] = prob.simulate_lookahead_h(V_s[a:b], timed, table[a:b], prm_timed, self.horizon_chunk_bytes,
                                                               x0_d[a:b], None if w_d is None else w_d[a:b], T, t0)
            x[a:b], u[a:b] = np.moveaxis(xs, 2, 3), np.moveaxis(us, 2, 3)
        chunks = self._run(tabs, None, work, look_horizon=look)
        self.backend_info.update(lookahead_path='device', lookahead_box='device', box_constants=int(look['bprm'].shape[1]))
        self._horizon_info(chunks, B, T, V_d, timed, prm_timed, None)
        if single:
            return x[:, :, 0], u[:, :, 0], g[:, :, 0], q[:, :, 0]
        return x, u, g, q

    def monte_carlo_lookahead_horizon(self, J_next, x0, n_steps, seed=0, n_burn=0, n_traj=None, law=None, occupancy=False,
                                      traj_offset=0, t0=0):
        """`DPSolver.monte_carlo_lookahead` of every member under a cost-to-go of any of the three shapes
        `simulate_lookahead` takes, in one device call per cut of the steps (kernel sdp_family_montecarlo_lookahead_h,
        csrc/sdp_family_lookahead_horizon_kernel.h): a `montecarlo.FamilyMonteCarloResult` with path 'device', member p of
        every field equal, bit for bit, to what `solvers[p].monte_carlo_lookahead(J_next[p], ...)` returns.  The other
        arguments are `monte_carlo_lookahead`'s: `law` is the law the PLANT draws from, the expectation inside the backup
        runs over member p's own law.  Models that are symbolic in time and models that look data up as data[k] both
        run; a cost-to-go that is not time-indexed on a symbolic model gives the bits of `monte_carlo_lookahead`.
        Launches are cut at the cost-to-go's uploads (horizon_chunk_bytes) and at steps_per_launch.  Not built:
        deterministic members (use `simulate_lookahead`)."""
        d = len(self.dims)
        # ---- everything that is refused, before a device is touched
        for p, s in enumerate(self.solvers):
            if self._law_points(s) == 0:
                raise ValueError('member {}: a deterministic system has nothing to draw: use simulate_lookahead(J_next, x0, '
                                 'n_steps=...)'.format(p))
        laws = self._mc_laws(law)
        x0, B, n_steps, n_burn, seeds, spl = self._mc_inputs(x0, n_steps, n_burn, n_traj, seed, traj_offset)
        V_d, timed = self._horizon_cost_to_go(J_next, n_steps, t0)
        dt = self.dtype
        S, n_law, rs = int(np.prod(self.dims)), len(laws[0][1]), self.dtype.itemsize
        tabs, table, prm_timed, look = self._lookahead_horizon_tables(n_steps, t0)
        # (a member's cost-to-go slices and table rows, and what `monte_carlo_lookahead` counts)
        look['bytes'] += (self._horizon_bytes(V_d, table) + (d + 1) * B * rs + 8 * B + (8 * S if occupancy else 0)
                          + n_law * (8 + rs) + 8)
        # ---- member-major device arrays
        V_s = V_d.reshape(self.P, V_d.shape[1], -1)                                                       # [P][T or 1][S]
        x0_d = np.ascontiguousarray(np.moveaxis(x0, -1, 1), dtype=dt)                                     # [P][d][B]
        cum = np.ascontiguousarray([mc.cumulative(proba) for _, proba in laws])                           # [P][n_law]
        law_d = np.ascontiguousarray([grid for grid, _ in laws], dtype=dt)
        seeds_d = np.array(seeds, dtype=np.uint64)
        cost_sum = np.empty((self.P, B), dtype=dt)
        n_out = np.empty((self.P, B), dtype=np.int64)
        x_final = np.empty((self.P, B, d), dtype=dt)
        occ = np.empty((self.P,) + self.dims, dtype=np.int64) if occupancy else None

        def work(prob, a, b):
            c, n, xf, o = prob.montecarlo_lookahead_h(V_s[a:b], timed, table[a:b], prm_timed, self.horizon_chunk_bytes,
                                                      x0_d[a:b], n_steps, n_burn, seeds_d[a:b], traj_offset, cum[a:b],
                                                      law_d[a:b], t0, spl, occupancy)
            cost_sum[a:b], n_out[a:b], x_final[a:b] = c, n, np.moveaxis(xf, 1, 2)
            if occupancy:
                occ[a:b] = o.astype(np.int64).reshape((b - a,) + self.dims)
        chunks = self._run(tabs, None, work, look_horizon=look)
        self.backend_info.update(lookahead_path='device', lookahead_box='device', box_constants=int(look['bprm'].shape[1]))
        self._horizon_info(chunks, B, n_steps, V_d, timed, prm_timed, min(spl, 1 << 30))
        return mc.FamilyMonteCarloResult(cost_sum, n_out, x_final, occ, n_steps, n_burn, seeds, int(traj_offset), t0, 'device')

    # ------------------------------------------------------------------ state distributions under the members' policies
    def _transition_size(self):
        """(S, nnz, bytes) of ONE member's transition operator (DPSolver._transition_size: the members agree)"""
        S = int(np.prod(self.dims))
        nnz = S * max(self.W, 1) * (1 << len(self.dims))
        return S, nnz, forward.operator_bytes(nnz, S, self.dtype.itemsize)

    def _transition_bytes(self):
        """bytes of device arrays one member takes in transition_operator beside _member_bytes: its operator
        (forward.operator_bytes), its entries in emission order (targets and values), the temporaries of the sort (the
        sorted keys, the positions before and after, and as much again for the sort's own double buffers), the
        histogram, its policy, its mean costs and two vectors, its flag, its place in the list and its statistics"""
        S, nnz, nbytes = self._transition_size()
        rs = self.dtype.itemsize
        return nbytes + nnz * (4 + rs) + nnz * 24 + 8 * (S + 1) + S * rs * (self.nu + 3) + 32

    def _transition_most(self):
        """the most members a chunk of transition_operator may hold: entry positions are 32-bit words, rows 32-bit ids,
        and a reduction launch lists at most 65535 members"""
        S, nnz, _ = self._transition_size()
        return max(1, min((2 ** 32 - 1) // nnz, (2 ** 31 - 1) // S, 65535))

    def transition_operator(self, pol, t_k=None):
        """`DPSolver.transition_operator` of every member in one device call per chunk (kernel sdp_family_transitions,
        csrc/sdp_family_trans_kernel.h; one sort for all members): a `FamilyTransitionOperator`, member p of everything
        it returns equal, bit for bit, to what `solvers[p].transition_operator(pol[p], t_k)` returns on the device.

        pol : (P,) + dims + (nu,), or dims + (nu,): every member's policy
        t_k : time index of a non-stationary family (default 0).  Members symbolic in time get it as the kernel's `t`;
              members that look data up as data[k] are traced for that step, one row of constants per member.
        Deterministic members run as W = 1, P = [1].  A family has no host path."""
        one, each = self.dims + (self.nu,), (self.P,) + self.dims + (self.nu,)
        # ---- everything that is refused, before a device is touched
        if np.shape(pol) not in (one, each):
            raise ValueError('pol must have shape {} (one policy for all {} members) or {} (member p under pol[p]), '
                             'not {}'.format(one, self.P, each, np.shape(pol)))
        for p, s in enumerate(self.solvers):
            _, nnz, nbytes = s._transition_size()
            if nbytes > s.TRANSITION_MAX_BYTES:
                raise ValueError('member {}: the transition operator of this grid has nnz = {} entries and takes {} bytes: '
                                 'more than DPSolver.TRANSITION_MAX_BYTES = {} bytes'.format(p, nnz, nbytes, s.TRANSITION_MAX_BYTES))
            if nnz >= 1 << 32:
                raise ValueError('member {}: the transition operator of this grid has nnz = {} entries ({} bytes): entry '
                                 'positions are 32-bit words, at most 2**32 - 1 entries whatever the cap'.format(p, nnz, nbytes))
        pol = self._policy(pol)
        t_trace = None if self.stationnary else (0 if t_k is None else t_k)
        tabs = self._tables(t_trace)
        S, nnz, _ = self._transition_size()
        pol_d = pol.reshape(self.P, S, self.nu)
        parts = []

        def work(prob, a, b):
            parts.append((a, b, prob.transop_create(np.ascontiguousarray(pol_d[a:b]), 0 if t_trace is None else t_trace)))
        try:
            self._run(tabs, None, work, trans=dict(bytes=self._transition_bytes(), most=self._transition_most()))
        except Exception:
            for _, _, h in parts:
                nat.lib().sdp_transop_destroy(h)
            raise
        op = FamilyTransitionOperator(parts, self.dims, self.dtype, nnz)
        # (the operator's record: push times are added to it as the operator is used)
        self.backend_info = dict(self.backend_info, transition=op.info)
        return op

    def stationary_distribution(self, pol, t_k=None, **kw):
        """`transition_operator(pol, t_k).stationary(**kw)` in one call: the stationary state distribution of every
        member under its policy (a `forward.FamilyStationary` record).  The operator is closed when done."""
        unknown = sorted(set(kw) - {'mu0', 'tol', 'n_max', 'check_every'})
        if unknown:
            raise TypeError('stationary_distribution got unexpected keyword argument(s) {}'.format(', '.join(unknown)))
        # (what `stationary` refuses, before an operator is built)
        conv.validate(kw.get('tol', 1e-12), kw.get('check_every', 10))
        if int(kw.get('n_max', 10000)) < 1:
            raise ValueError('n_max must be at least 1')
        if kw.get('mu0') is not None and np.shape(kw['mu0']) not in (self.dims, (self.P,) + self.dims):
            raise ValueError('mu must have shape {} (the same for all {} members) or {} (member p from mu[p]), not {}'.format(
                self.dims, self.P, (self.P,) + self.dims, np.shape(kw['mu0'])))
        op = self.transition_operator(pol, t_k)
        try:
            return op.stationary(**kw)
        finally:
            op.close()

    def last_kernel_ms(self):
        """HIP-event time of the launches of the last sweep, evaluation or Monte Carlo call of a family that runs as one
        chunk (None otherwise)"""
        return self._handle[1].last_kernel_ms() if self._handle is not None else None

    def close(self):
        if self._handle is not None:
            self._handle[1].close()
            self._handle = None
