"""The families of tests/test_family_lookahead_horizon_plan.py (CPU) and tests/test_gpu_family_lookahead_horizon.py (GPU):
closed loops of a family under lookahead controls over a horizon (`SolverFamily.simulate_lookahead` and
`SolverFamily.monte_carlo_lookahead_horizon`, kernels sdp_family_simulate_lookahead and sdp_family_montecarlo_lookahead_h of
csrc/sdp_family_lookahead_horizon_kernel.h).  Built from tests/family_cases.py, tests/family_lookahead_cases.py and
tests/family_horizon_cases.py; no tests here.

parity     storage_ar1 in 8- and 4-byte reals (the members of family_lookahead_cases.AR1; a stationary model, run with one
           cost-to-go per member and with a time-indexed one, T = 8), three_d (81 lattice points on 64 lanes), finite_horizon
           (symbolic time in the model and the box; t0 = 1, n_steps = 5, T_J = 6), pv lookahead (deterministic, `data[k]`
           in the cost: a row of constants per member and step, T = 6) and family_horizon_cases.LOOKUP (stochastic,
           `data[k]` in the dynamics, a constant box).
           `pv lookahead` is NOT family_cases' pv_sized case: its member with E_rated = 1.0 coincides with P_rated = 1.0
           and its box traces with another structure (`PV_REFUSED`).
mapping    family_lookahead_cases.MAPPING[P], B = 5, 3 steps, a time-indexed cost-to-go.
cap        9 line members and family_lookahead_cases.cap_batch, 3 steps.
cuts       family_lookahead_cases.CUTS; no lattice, deterministic: those of family_lookahead_cases.

The time-indexed cost-to-go of member p is lookahead_cases.cost_to_go with another seed and another scale at every step
(`cost_to_go`), so that a wrong slice shows.  The yardsticks are the members' solo calls (on the device for models that are
symbolic in time, on the host for `data[k]`) and the pinned oracle chained step by step.
"""
import numpy as np

import family_cases as fc
import family_horizon_cases as fhc
import family_lookahead_cases as flc
import lookahead_cases as lc
import mc_lookahead_cases as mlc
from stodynprog_amd import SolverFamily

SEED, OFFSET, N_BURN = flc.SEED, flc.OFFSET, flc.N_BURN
THREADS = flc.THREADS


class Case(flc.Case):
    """a family with the horizon its closed loop is run over: n_steps steps from time index t0 under a cost-to-go of T_J
    steps; int_time: the members look data up as data[k] (their solo calls take the host path)"""

    def __init__(self, name, members, n_steps, t0=0, T_J=None, dtype=np.float64, int_time=False):
        flc.Case.__init__(self, name, members, t_k=t0, t0=t0, dtype=dtype)
        self.n_steps, self.T_J, self.int_time = n_steps, (n_steps + t0 if T_J is None else T_J), int_time

    def look(self, p):
        return lc.Case('{} member {}'.format(self.name, p), self.members[p], int_time=self.int_time,
                       path='host' if self.int_time else 'device')


def _of(case, n_steps, **kw):
    return Case(case.name, case.members, n_steps, dtype=case.dtype, **kw)


PV_MEMBERS = ((2.0, 1.0), (1.5, 0.8), (3.0, 1.2))
AR1_64, AR1_32, THREE_D = _of(flc.PARITY[0], 8), _of(flc.PARITY[1], 8), _of(flc.PARITY[2], 8)
FINITE = _of(flc.PARITY[3], 5, t0=1, T_J=6)
PV = Case('pv lookahead', [fc.pv_sized(E, scale) for E, scale in PV_MEMBERS], 6, int_time=True)
LOOKUP = Case('lookup', fhc.LOOKUP.case.members, 8, int_time=True)
PARITY = [AR1_64, AR1_32, THREE_D, FINITE, PV, LOOKUP]
STOCHASTIC = [c for c in PARITY if c is not PV]
PV_REFUSED = Case('pv_sized', fhc.PV_SIZED.case.members, 6, int_time=True)
MAPPING = {P: _of(flc.MAPPING[P], flc.STEPS_MAPPING) for P in flc.MAPPING_P}
B_MAPPING = flc.B_MAPPING
CAP = _of(flc.CAP, flc.STEPS_CAP)
CUTS = _of(flc.CUTS, 6)
NO_LATTICE = _of(flc.NO_LATTICE, 6)
NAN_ROW = flc.NAN_ROW
DETERMINISTIC = _of(flc.DETERMINISTIC, 6)
FAMILIES = PARITY + [MAPPING[P] for P in flc.MAPPING_P] + [CUTS, NO_LATTICE, DETERMINISTIC]


def family(case):
    return SolverFamily(case.solvers())


def lanes(case):
    fam = family(case)
    return fam._tables(None if fam.stationnary else case.t0)['lanes']


def tile(case):
    """trajectories of a workgroup: 4 waves of 64 / lanes"""
    return (64 // lanes(case)) * (THREADS // 64)


def cost_to_go(case, timed=True):
    """(P, T_J) + dims float64, member p at step k lookahead_cases.cost_to_go with the seed 10 p + k, scaled by
    1 + k / 4; or (P,) + dims, its slice of step t0"""
    J = np.stack([np.stack([lc.cost_to_go(s, seed=10 * p + k) * (1 + 0.25 * k) for k in range(case.T_J)])
                  for p, s in enumerate(case.solvers())])
    return J if timed else np.ascontiguousarray(J[:, case.t0])


def starts(case, B):
    return flc.starts(case, B)


def noise(case, B, seed=3):
    """(P, n_steps, B) values of every member's own perturbation grid (lookahead_cases.draws); None: deterministic"""
    solvers = case.solvers()
    if not solvers[0].perturb_grid:
        return None
    return np.stack([lc.draws(s, case.n_steps, B, seed=seed + p)[0] for p, s in enumerate(solvers)])


def oracle_closed_loop(case, p, J_p, x0_p, w_p):
    """(x, u, g, q) of member p by lookahead_cases.oracle_closed_loop: the pinned oracle chained step by step"""
    s = case.members[p]()
    return lc.oracle_closed_loop(s, lc.spec_of(case.look(p), s), J_p, x0_p, w_p, case.n_steps, case.t0)


def oracle_monte_carlo(case, p, J_p, x0_p, n_burn, seed=SEED, traj_offset=OFFSET, law=None, occupancy=True, nan_rows=()):
    """(cost_sum, n_outside, x_final, occupancy) of member p: mc_lookahead_cases.closed_loop and `reduce`"""
    s = case.members[p]()
    x, g = mlc.closed_loop(case.look(p), s, J_p, x0_p, case.n_steps, seed=seed, traj_offset=traj_offset, law=law,
                           t0=case.t0, nan_rows=nan_rows)
    return mlc.reduce(s, x, g, n_burn, occupancy=occupancy)


# ----------------------------------------------------------------------------------------------------------------------
# the cuts, restated (family_lookahead_horizon_checks and the two drivers in csrc/sdp_hip.hip)

def step_chunks(P, S, itemsize, n_steps, chunk_bytes, timed=True):
    """[(first, last), ...]: the steps of every upload of the cost-to-go of P members: whole steps of all members, at
    most chunk_bytes, a larger step a chunk of its own; a cost-to-go that is not time-indexed goes up once"""
    per = min(n_steps, max(1, int(chunk_bytes) // (P * S * itemsize))) if timed else n_steps
    return [(c, min(c + per, n_steps)) for c in range(0, n_steps, per)]


def launches(chunks, spl=None):
    """launches of a call with these step chunks: one per chunk (the closed loop) or one per steps_per_launch steps of it"""
    return sum(1 if spl is None else -(-(b - a) // spl) for a, b in chunks)


def sim_extra_bytes(fam, B, T, T_c, rows, n_box):
    """what `SolverFamily.simulate_lookahead` counts per member beside the handle's arrays: T_c cost-to-go slices, `rows`
    table rows, start states, perturbations, states, controls, costs and values, the box row and the control steps"""
    S, d, rs = int(np.prod(fam.dims)), len(fam.dims), fam.dtype.itemsize
    n_prm = fam._tables(None if fam.stationnary else 0)['prm'].shape[1]
    return ((T_c * S + rows * n_prm) * rs + (d * B + (1 if fam.W else 0) * T * B + (T + 1) * d * B + T * fam.nu * B + 2 * T * B) * rs
            + 8 * (n_box + fam.nu))


def mc_extra_bytes(fam, B, n_law, occupancy, T_c, rows, n_box):
    """what `SolverFamily.monte_carlo_lookahead_horizon` counts per member beside the handle's arrays"""
    S, rs = int(np.prod(fam.dims)), fam.dtype.itemsize
    n_prm = fam._tables(None if fam.stationnary else 0)['prm'].shape[1]
    return flc.mc_extra_bytes(fam, B, n_law, occupancy, n_box) + (T_c * S + rows * n_prm) * rs


def unit_sources():
    """the generated source of every unit the GPU tests run (for the build: they travel compiled): the unit and the sweep
    unit of every family at its first step, the lookahead unit of the parity families that `monte_carlo_lookahead` runs
    as well and the solo lookahead units of the members compared with solo calls"""
    out = []
    for case in FAMILIES:
        fam = family(case)
        tabs, _, _, look = fam._lookahead_horizon_tables(case.n_steps, case.t0)
        out += [tabs['source'], look['source']]
        if case in PARITY and not case.int_time:
            out.append(fam._lookahead_tables(None if fam.stationnary else case.t0, 0)[1]['source'])
        if case in PARITY or case in (CUTS, DETERMINISTIC):
            # (the solo host path of a `data[k]` model calls the lookahead of a unit per step)
            times = range(case.t0, case.t0 + case.n_steps) if case.int_time else [None if fam.stationnary else case.t0]
            for s in fam.solvers:
                out += [lc.unit_source(s, t) for t in times]
    return out
