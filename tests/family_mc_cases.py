"""The families of tests/test_family_mc_plan.py (CPU) and tests/test_gpu_family_montecarlo.py (GPU): Monte Carlo
evaluation of a family (`SolverFamily.monte_carlo`, kernel sdp_family_montecarlo of csrc/sdp_family_mc_kernel.h).  The
members come from tests/family_cases.py; no tests here.

parity     inventory P=3 (d = 1), storage_ar1 in 8- and 4-byte reals (d = 2), three_d (d = 3): B = 65 trajectories (a
           full wave and one lane), 24 steps of which 5 burn in, occupancy on, start states per member.  Every grid has
           fewer than 65 nodes, so at every step two trajectories share a node: the wave-combined atomic is used.
mapping    line_members(P, 9) for P in MAPPING_P: every way the kernel maps members to XCDs (`launch`); B = 257 is two
           tiles a member, the second with one live lane.
cap        9 line members and B with 9 * ceil(B / 256) tiles beyond the grid's bound: the stride loop's second trip.
cuts       storage_ar1 with five members: steps_per_launch, traj_offset splits and member chunks 2 + 2 + 1.
seeds      two identical storage_ar1 members.
laws       storage_ar1 f64 with per-member 9-point laws that are not the solvers' own, a law of 70 points (the binary
           search of sdp_mc_index starts at 64 entries of the running sum) and one shared law.
outside    storage_ar1 with E_rated = 10 and 2: shared start states inside member 0's grid and outside member 1's.

The policies are those of one value iteration of a zero cost-to-go: `fam.value_iteration` on the device, and
`policies` -- oracle/vi_numpy.py -- for the properties the CPU tests check.
"""
import numpy as np

import family_cases as fc
from stodynprog_amd import SolverFamily, codegen

B_PARITY, N_STEPS, N_BURN = 65, 24, 5
TILE = 256                       # trajectories per tile: SDP_FMC_TILE of csrc/sdp_family_mc_kernel.h
PER_CU_MAX = 8

BY_NAME = {c.name: c for c in fc.CASES}
PARITY = [BY_NAME[n] for n in ('inventory P=3', 'storage_ar1 f64', 'storage_ar1 f32', 'three_d')]
MAPPING_P = (2, 4, 7, 8, 9, 17)
MAPPING = {P: fc.Case('line P={}'.format(P), fc.line_members(P, fc.LINE_NX), oracle=True) for P in MAPPING_P}
B_MAPPING, STEPS_MAPPING = 257, 6
CAP = MAPPING[9]
STEPS_CAP = 3
CUTS = fc.CHUNKS
STEPS_CUTS = 20
SEEDS = fc.Case('seeds', [fc.storage_ar1(5, 4, 0.8), fc.storage_ar1(5, 4, 0.8)])
LAWS = BY_NAME['storage_ar1 f64']
OUTSIDE = fc.Case('outside', [fc.storage_ar1(10, 1, 0.5), fc.storage_ar1(2, 4, 0.8)])
B_OUTSIDE, STEPS_OUTSIDE = 65, 8
FAMILIES = PARITY + [MAPPING[P] for P in MAPPING_P] + [CUTS, SEEDS, OUTSIDE]


def cap_batch(cus):
    """the smallest B with B % 256 == 1 whose 9 members make more tiles than 8 * cus workgroups"""
    tiles = (8 * cus) // 9 + 1
    return (tiles - 1) * TILE + 1


def launch(B, n_active, cus, per_cu):
    """the host's grid of one family Monte Carlo launch and the kernel's walk, restated (sdp_family_montecarlo in
    csrc/sdp_hip.hip, the head of csrc/sdp_family_mc_kernel.h): tiles per member, XCDs per member, workgroups per XCD,
    and for every XCD the (member, tile) pairs its workgroups visit, in the order of its units, with the trip of the
    stride loop each is visited in"""
    tiles = -(-B // TILE)
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
            tile = part * per_part + unit % per_part
            if tile < tiles:
                seen.append((first + 8 * (unit // per_part), tile, unit // per_xcd))
        visits.append(seen)
    return dict(tiles=tiles, parts=parts, wanted=wanted, per_xcd=per_xcd, blocks=8 * per_xcd, visits=visits)


def starts(case, B, seed=0):
    """(P, B, d) start states in the case's reals' range, inside every member's own grid"""
    solvers = case.solvers()
    rng = np.random.default_rng(100 + seed + len(case.name))
    out = np.empty((len(solvers), B, len(solvers[0].state_grid)))
    for p, s in enumerate(solvers):
        for k, g in enumerate(s.state_grid):
            out[p, :, k] = rng.uniform(g[0] + 0.1 * (g[-1] - g[0]), g[-1] - 0.1 * (g[-1] - g[0]), size=B)
    return out


def outside_starts():
    """(B, 2) shared start states: E in [3, 8] -- inside [0, 10], outside [0, 2] -- and a small mismatch"""
    rng = np.random.default_rng(7)
    return np.stack([rng.uniform(3., 8., size=B_OUTSIDE), rng.uniform(-1., 1., size=B_OUTSIDE)], axis=1)


def policies(case):
    """(P,) + dims + (nu,): the policy of one value iteration of a zero cost-to-go, by oracle/vi_numpy.py"""
    out = []
    for make in case.members:
        dims = make()._shape()
        out.append(fc.oracle_sweeps(make, np.zeros(dims), 1)[0][0][2])
    return np.stack(out)


def host_run(s, pol, x0, n_steps, n_burn, seed, occupancy=False, law=None):
    """`DPSolver._monte_carlo_host` of one member with numpy alone: the policy looked up by oracle/vi_numpy.py's
    interpolator in the place of the device's.  (cost_sum, n_outside, x_final, occupancy)"""
    from oracle import vi_numpy

    def interp_on_state(A):
        it = vi_numpy.Interp(*s.state_grid)
        it.set_values(np.asarray(A, dtype=float))
        return it
    s.interp_on_state = interp_on_state
    grid, proba = s._mc_law(law)
    ids = s._mc_ids(x0.shape[0], 0)
    return s._monte_carlo_host(np.asarray(pol), np.asarray(x0, dtype=float), n_steps, n_burn, seed, ids, grid, proba,
                               occupancy, 0)


def member_laws():
    """per member of LAWS a 9-point law that is not the solver's own (3 points): another grid per member, uneven weights"""
    laws = []
    for p in range(len(LAWS.members)):
        grid = np.linspace(-1.5 - 0.25 * p, 1.2 + 0.5 * p, 9)
        proba = np.arange(1., 10.) ** (0.5 + 0.25 * p)
        laws.append((grid, proba / proba.sum()))
    return laws


def long_law(n=70):
    """one law of 70 points: more than the 63 running sums sdp_mc_index counts through without a branch"""
    grid = np.linspace(-2., 2., n)
    proba = 1. + np.cos(np.linspace(0., 3., n)) ** 2
    return grid, proba / proba.sum()


def shared_law():
    grid = np.array([-1., -0.25, 0.5, 2.])
    return grid, np.array([0.1, 0.4, 0.3, 0.2])


def chunk_bytes_for(fam, members, B, n_law, occupancy):
    """a chunk_bytes at which `members` members of a Monte Carlo run fit in a chunk and one more does not"""
    per_member = fam._member_bytes(fam._tables()) + fam._mc_member_bytes(B, n_law, occupancy)
    return per_member * members + per_member // 2


def solo(solvers):
    """the members as the GPU tests call them alone: the direct kernel's unit (every unit carries sdp_montecarlo)"""
    for s in solvers:
        s.kernel = 'generic'
    return solvers


def unit_sources():
    """the generated source of every unit the GPU tests run (for the build: they travel compiled): the Monte Carlo
    unit and the sweep unit of every family, and the solo 'generic' units they are compared with"""
    out = []
    for case in FAMILIES:
        fam = SolverFamily(case.solvers())
        tabs = fam._tables()
        out += [tabs['source'], codegen.family_mc_unit(tabs['model'], fam.dtype),
                codegen.family_policy_unit(tabs['model'], fam.dtype)]
        for s in solo(fam.solvers):
            out.append(s._kernel_plan(None, s._trace_now(None))['source'])
    return out
