"""The families of tests/test_family_lookahead_plan.py (CPU) and tests/test_gpu_family_lookahead.py (GPU): one-step
lookahead at arbitrary states and its Monte Carlo score for a family (`SolverFamily.lookahead`,
`SolverFamily.monte_carlo_lookahead`, kernels sdp_family_lookahead and sdp_family_montecarlo_lookahead of
csrc/sdp_family_lookahead_kernel.h).  The members come from tests/family_cases.py; no tests here.

parity     storage_ar1 in 8- and 4-byte reals with the members AR1 (a state-dependent box with per-member constants,
           lane counts 8, 8 and 16, other grid ends and laws per member, nu = 2 with a one-point control), three_d
           (a lattice of 81 points on 64 lanes: the stride of the control loop) and finite_horizon (symbolic time in
           the box; t_k = 2, t0 = 1).  Inventory is left out on purpose: with `cost_to_go` the oracle picks index 0
           at every state there.
mapping    line_members(P, 9) for P in MAPPING_P: every way the kernels map members to XCDs (`launch`); B = 5 is
           two tiles with 64 lanes, the second with one live group.
cap        9 line members and B with 9 * ceil(B / 4) tiles beyond the grid's bound: the stride loop's second trip.
cuts       five storage_ar1 members without coinciding box constants: steps_per_launch, traj_offset, member chunks.
laws       the parity storage family with per-member 9-point plant laws, and one shared law of 70 points.
seeds      two identical storage_ar1 members.
outside    storage_ar1 with E_rated = 10 and 2: shared start states inside member 0's grid and outside member 1's.
no lattice two parameterised copies of lookahead_cases.nan_box with different decays.
deterministic two parameterised copies of lookahead_cases.deterministic: the unit has `sdp_family_lookahead` alone.

`family_cases.AR1` itself is NOT a lookahead family: its member (10, 1, 0.5) has P_rated == dt == 1.0 in its box, one
node of the trace, so its box has four constants where the others have five (`REFUSED`).

The yardsticks are the solo device calls and the pinned oracle chained step by step (tests/lookahead_cases.py,
tests/mc_lookahead_cases.py), fed with `monte_carlo_draws`.
"""
import numpy as np

import family_cases as fc
import lookahead_cases as lc
import mc_lookahead_cases as mlc
from stodynprog_amd import SolverFamily, SysDescription, DPSolver, codegen
from stodynprog_amd.models import NormalLaw

SEED, OFFSET = mlc.SEED, mlc.OFFSET
T, N_BURN = lc.T_SIM, 2
THREADS = 256                    # SDP_FLOOK_THREADS of csrc/sdp_family_lookahead_kernel.h
PER_CU_MAX = 8

AR1 = [(2, 4, 0.8), (10, 1.5, 0.5), (5, 3, 0.8)]
AR1_FIVE = AR1 + [(3, 2, 0.6), (8, 3, 0.7)]


class Case(fc.Case):
    """a family with the time indices its lookahead (t_k) and its closed loop (t0) are checked at"""

    def __init__(self, name, members, t_k=None, t0=0, dtype=np.float64):
        fc.Case.__init__(self, name, members, dtype=dtype)
        self.t_k, self.t0 = t_k, t0

    def look(self, p):
        """member p as a case of tests/lookahead_cases.py (its states, its oracle spec)"""
        return lc.Case('{} member {}'.format(self.name, p), self.members[p])


_BY_NAME = {c.name: c for c in fc.CASES}
PARITY = [
    Case('storage_ar1 f64', [fc.storage_ar1(*a) for a in AR1]),
    Case('storage_ar1 f32', [fc.storage_ar1(*a, dtype=np.float32) for a in AR1], dtype=np.float32),
    Case('three_d', _BY_NAME['three_d'].members),
    Case('finite_horizon', _BY_NAME['finite_horizon'].members, t_k=2, t0=1),
]
REFUSED = Case('storage_ar1 coinciding', [fc.storage_ar1(*a) for a in fc.AR1])
MAPPING_P = (2, 4, 7, 8, 9, 17)
MAPPING = {P: Case('line P={}'.format(P), fc.line_members(P, fc.LINE_NX)) for P in MAPPING_P}
B_MAPPING, STEPS_MAPPING = 5, 3
CAP = MAPPING[9]
STEPS_CAP = 3
CUTS = Case('cuts', [fc.storage_ar1(*a) for a in AR1_FIVE])
LAWS = PARITY[0]
SEEDS = Case('seeds', [fc.storage_ar1(5, 3, 0.8), fc.storage_ar1(5, 3, 0.8)])
OUTSIDE = Case('outside', [fc.storage_ar1(10, 1.5, 0.5), fc.storage_ar1(2, 4, 0.8)])
B_OUTSIDE = 9


def nan_member(decay, dtype=np.float64):
    """lookahead_cases.nan_box with its decay as an argument: the upper end of the box is NaN at x == NAN_STATE"""
    def make():
        s = SysDescription((1, 1, 1), name='nan box')
        s.dyn = lambda x, u, w: (decay * x + 0.2 * u + w,)
        s.cost = lambda x, u, w: (x - 0.3) * (x - 0.3) + 0.1 * u * u
        s.control_box = lambda x: ((-1.0, 1.0 + 0.0 * (1.0 / (x - lc.NAN_STATE))),)
        s.perturb_laws = [NormalLaw(0, 0.1)]
        solver = DPSolver(s, dtype=dtype)
        solver.discretize_state(0, 1, 10)
        solver.discretize_perturb(-0.3, 0.3, 3)
        solver.control_steps = (0.25,)
        return solver
    return make


NO_LATTICE = Case('no lattice', [nan_member(0.9), nan_member(0.8)])
NAN_ROW = 3


def det_member(gain, slope):
    """lookahead_cases.deterministic with its gain and the slope of its box as arguments: no perturbation"""
    def make():
        s = SysDescription((1, 1, 0), name='deterministic')
        s.dyn = lambda x, u: (0.8 * x + gain * u,)
        s.cost = lambda x, u: (x - 0.4) * (x - 0.4) + 0.1 * u * u
        s.control_box = lambda x: ((-0.5 - slope * x, 0.5),)
        solver = DPSolver(s)
        solver.discretize_state(-1, 1, 11)
        solver.control_steps = (0.125,)
        return solver
    return make


DETERMINISTIC = Case('deterministic', [det_member(0.3, 0.25), det_member(0.35, 0.3)])      # `lookahead` alone: nothing to draw
FAMILIES = PARITY + [MAPPING[P] for P in MAPPING_P] + [CUTS, SEEDS, OUTSIDE, NO_LATTICE, DETERMINISTIC]
SOLO = PARITY + [CUTS, SEEDS, OUTSIDE, DETERMINISTIC]          # the families also compared with the members' solo device calls


def family(case):
    return SolverFamily(case.solvers())


def lanes(case):
    """SDP_LANES of the family's lookahead unit: the largest lane count of the members"""
    fam = family(case)
    return fam._tables(None if fam.stationnary else case.t_k)['lanes']


def tile(case):
    """states (trajectories) of a workgroup: 4 waves of 64 / lanes"""
    return (64 // lanes(case)) * (THREADS // 64)


def cost_to_go(case):
    """(P,) + dims float64: lookahead_cases.cost_to_go per member, seeded by the member's index"""
    return np.stack([lc.cost_to_go(s, seed=p) for p, s in enumerate(case.solvers())])


def states(case):
    """[P] arrays (B_p, d): lookahead_cases.states of every member (nodes, interiors, up to 20 % outside); the members
    of a case have grids of one shape, so B_p is the same for all and the arrays stack"""
    return np.stack([lc.states(case.look(p), s) for p, s in enumerate(case.solvers())])


def starts(case, B):
    """(P, B, d) start states inside every member's own grid (lookahead_cases.start_states, another seed per member)"""
    return np.stack([lc.start_states(case.look(p), s, B, seed=5 + p) for p, s in enumerate(case.solvers())])


def outside_starts():
    """(B, 2) shared start states: E in [3, 8] -- inside [0, 10], outside [0, 2] -- and a small mismatch"""
    rng = np.random.default_rng(7)
    return np.stack([rng.uniform(3., 8., size=B_OUTSIDE), rng.uniform(-0.5, 0.5, size=B_OUTSIDE)], axis=1)


def member_laws():
    """per member of LAWS a 9-point plant law that is not the solver's own (3 points)"""
    laws = []
    for p in range(len(LAWS.members)):
        grid = np.linspace(-0.6 - 0.1 * p, 0.5 + 0.2 * p, 9)
        proba = np.arange(1., 10.) ** (0.5 + 0.25 * p)
        laws.append((grid, proba / proba.sum()))
    return laws


def spread_laws(case):
    """per member a plant law on the solver's own perturbation grid with weights that make every point likely: the
    members' own laws put 0.9993 on their middle point at these grids, so under them nearly every draw is that point"""
    laws = []
    for p, s in enumerate(case.solvers()):
        proba = np.linspace(1., 2. + 0.5 * p, len(s.perturb_grid[0]))
        laws.append((np.asarray(s.perturb_grid[0], dtype=float), proba / proba.sum()))
    return laws


def long_law(n=70):
    """one law of 70 points: more than the 63 running sums sdp_mc_index counts through without a branch"""
    grid = np.linspace(-0.8, 0.8, n)
    proba = 1. + np.cos(np.linspace(0., 3., n)) ** 2
    return grid, proba / proba.sum()


# ----------------------------------------------------------------------------------------------------------------------
# yardstick (2): the pinned oracle

def oracle_lookahead(case, J_next, x, members=None):
    """(J (P, B), u (P, B, nu), idx (P, B)) by lookahead_cases.oracle_lookahead, member by member"""
    out = []
    for p, s in enumerate(case.solvers()):
        if members is not None and p not in members:
            continue
        look = case.look(p)
        out.append(lc.oracle_lookahead(s, lc.spec_of(look, s), J_next[p], x[p] if np.ndim(x) == 3 else x,
                                       None if s.sys.stationnary else case.t_k))
    return tuple(np.stack([o[k] for o in out]) for k in range(3))


def oracle_monte_carlo(case, p, J_p, x0_p, n_steps, n_burn, seed=SEED, traj_offset=OFFSET, law=None, occupancy=True,
                       nan_rows=()):
    """(cost_sum, n_outside, x_final, occupancy) of member p: mc_lookahead_cases.closed_loop (the oracle chained step
    by step on `monte_carlo_draws`) and `reduce`"""
    s = case.members[p]()
    x, g = mlc.closed_loop(case.look(p), s, J_p, x0_p, n_steps, seed=seed, traj_offset=traj_offset, law=law,
                           t0=case.t0, nan_rows=nan_rows)
    return mlc.reduce(s, x, g, n_burn, occupancy=occupancy)


# ----------------------------------------------------------------------------------------------------------------------
# the launch, restated

def cap_batch(cus, lanes=64):
    """the smallest ragged B (one live group in the last tile) whose 9 members make more tiles than the 8 * cus
    workgroups a launch has at most, whatever the occupancy query answers"""
    rows = (64 // lanes) * (THREADS // 64)
    tiles = (8 * cus) // 9 + 1
    return (tiles - 1) * rows + 1


def launch(B, lanes, n_active, cus, per_cu):
    """the host's grid of one family lookahead launch and the kernels' walk, restated (family_lookahead_grid in
    csrc/sdp_hip.hip, sdp_flook_walk in csrc/sdp_family_lookahead_kernel.h): tiles per member, XCDs per member,
    workgroups per XCD, and for every XCD the (member, tile) pairs its workgroups visit, in the order of its units,
    with the trip of the stride loop each is visited in"""
    rows = (64 // lanes) * (THREADS // 64)
    tiles = -(-B // rows)
    parts = 1 if n_active >= 8 else 8 // n_active
    per_part = -(-tiles // parts)
    wanted = -(-n_active // 8) * tiles if n_active >= 8 else per_part
    per_xcd = max(1, min(wanted, cus * min(per_cu, PER_CU_MAX) // 8))
    visits = []
    for xcd in range(8):
        first, part = xcd // parts, xcd % parts
        mine = (n_active - first + 7) // 8 if first < n_active else 0
        seen = []
        for unit in range(mine * per_part):
            t = part * per_part + unit % per_part
            if t < tiles:
                seen.append((first + 8 * (unit // per_part), t, unit // per_xcd))
        visits.append(seen)
    return dict(tiles=tiles, parts=parts, wanted=wanted, per_xcd=per_xcd, blocks=8 * per_xcd, visits=visits)


def chunk_bytes_for(fam, members, extra):
    """a chunk_bytes at which `members` members of a call that takes `extra` bytes a member beside the handle's fit in
    a chunk and one more does not"""
    per_member = fam._member_bytes(fam._tables()) + extra
    return per_member * members + per_member // 2


def mc_extra_bytes(fam, B, n_law, occupancy, n_box):
    """what `SolverFamily.monte_carlo_lookahead` counts per member beside the handle's arrays"""
    S, d, rs = int(np.prod(fam.dims)), len(fam.dims), fam.dtype.itemsize
    return (d + 1) * B * rs + 8 * B + (8 * S if occupancy else 0) + n_law * (8 + rs) + 8 + 8 * (n_box + fam.nu)


def unit_sources():
    """the generated source of every unit the GPU tests run (for the build: they travel compiled): the lookahead unit
    and the sweep unit of every family, and the solo lookahead units of the families compared with solo calls"""
    out = []
    for case in FAMILIES:
        fam = family(case)
        for t in sorted({case.t_k, case.t0}, key=str) if not fam.stationnary else [None]:
            tabs, look = fam._lookahead_tables(t, 0)
            out += [tabs['source'], look['source']]
        if case in SOLO or case is NO_LATTICE:
            for s in fam.solvers:
                for t in sorted({case.t_k, case.t0}, key=str) if not fam.stationnary else [None]:
                    out.append(lc.unit_source(s, t))
    return out
