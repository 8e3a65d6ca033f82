"""The families of tests/test_family_horizon_plan.py (CPU) and tests/test_gpu_family_horizon.py (GPU): closed loops of
a family over a horizon (`SolverFamily.simulate` and `SolverFamily.monte_carlo_horizon`, kernels sdp_family_simulate and
sdp_family_montecarlo_h of csrc/sdp_family_horizon_kernel.h).  The members come from tests/family_cases.py, the yardstick
of the `data[k]` families from tests/horizon_sim.py; no tests here.

pv_sized        3 members, 9 nodes, T = 6: deterministic, `data[k]` in the cost (a table of constants per step), a
                time-indexed policy.
finite_horizon  3 members, 9 nodes, 3 points: stochastic, a symbolic time index (one row of constants per member, step
                stride 0), a time-indexed policy of T_pol = 6 run from t0 = 1.
lookup          2 members built like `_data_member` of tests/test_family_mc_plan.py: stochastic with `data[k]`; run under a
                time-indexed and under a stationary policy.
storage_ar1     3 members, 7 x 5, 8- and 4-byte reals: a stationary model under a time-indexed policy (a receding schedule).
three_d         2 members, d = 3, nu = 2, the same.
line P=..       P in MAPPING_P: every way the kernels map members to XCDs; 9 members past both launch caps.
outside         storage_ar1 with E_rated = 10 and 2: shared starts inside member 0's grid and outside member 1's.

T = 8 steps unless stated.  The policies are random inside each member's box of step 0, a new draw at every step, so that
a wrong slice shows (`policies`); on the device also what `fam.bellman_recursion` returns where one exists.
"""
import numpy as np

import family_cases as fc
import family_mc_cases as mcc
import horizon_sim as hs                      # noqa: F401  (the chained oracle of the GPU tests)
import policies as pl
from stodynprog_amd import DPSolver, SolverFamily, SysDescription, codegen
from stodynprog_amd.models import NormalLaw

T = 8
SIM_TILE, MC_TILE = 64, 256                   # SDP_FH_SIM_TILE, SDP_FH_MC_TILE of csrc/sdp_family_horizon_kernel.h
BATCHES = (1, 63, 65, 257)
MAPPING_P = (2, 4, 7, 8, 9, 17)
B_MAPPING = 300
STEPS_CAP = 3
LOOKUP_DATA = np.linspace(0.1, 1., 16)


def lookup(decay, gain):
    """one state, one control, three points, with data[k] in the dynamics"""
    def make():
        data = LOOKUP_DATA * gain
        sysd = SysDescription((1, 1, 1), stationnary=False, name='lookup')
        sysd.dyn = lambda k, x, u, w: (decay * x + u + w + data[k],)
        sysd.cost = lambda k, x, u, w: x * x + 0.25 * u * u
        sysd.control_box = lambda k, x: ((-1., 1.),)
        sysd.perturb_laws = [NormalLaw(0, 0.1)]
        s = DPSolver(sysd)
        s.discretize_state(-2, 2, 9)
        s.discretize_perturb(-0.3, 0.3, 3)
        s.control_steps = (0.125,)
        return s
    return make


class Horizon(object):
    """a family with the horizon it is run over: n_steps steps from time index t0 under a policy of T_pol steps;
    int_time: the members look data up as data[k]"""

    def __init__(self, case, n_steps=T, t0=0, T_pol=None, int_time=False):
        self.case, self.name, self.n_steps, self.t0 = case, case.name, n_steps, t0
        self.T_pol = n_steps + t0 if T_pol is None else T_pol
        self.int_time = int_time
        self.dtype = case.dtype

    def solvers(self):
        return self.case.solvers()

    def __repr__(self):
        return self.name


BY_NAME = {c.name: c for c in fc.CASES}
PV_SIZED = Horizon(BY_NAME['pv_sized'], n_steps=6, int_time=True)
FINITE = Horizon(BY_NAME['finite_horizon'], n_steps=5, t0=1, T_pol=6)
LOOKUP = Horizon(fc.Case('lookup', [lookup(0.9, 1.0), lookup(0.8, 0.7)]), int_time=True)
AR1_64 = Horizon(BY_NAME['storage_ar1 f64'])
AR1_32 = Horizon(BY_NAME['storage_ar1 f32'])
THREE_D = Horizon(BY_NAME['three_d'])
PARITY = [PV_SIZED, FINITE, LOOKUP, AR1_64, AR1_32, THREE_D]
MAPPING = {P: Horizon(mcc.MAPPING[P]) for P in MAPPING_P}
CAP = Horizon(mcc.MAPPING[9], n_steps=STEPS_CAP)
OUTSIDE = Horizon(mcc.OUTSIDE)
CUTS = Horizon(mcc.CUTS)                      # storage_ar1 with five members: member chunks 3 + 2
FAMILIES = PARITY + [MAPPING[P] for P in MAPPING_P] + [OUTSIDE, CUTS]


def policies(hz, kind='random'):
    """(P, T_pol) + dims + (nu,): per member and step a policy of tests/policies.py inside the member's box of step 0, with
    another seed at every step"""
    return np.stack([np.stack([pl.policy(s, kind, seed=100 * p + k) for k in range(hz.T_pol)])
                     for p, s in enumerate(hz.solvers())])


def starts(hz, B, seed=0):
    """(P, B, d) start states inside every member's own grid"""
    return mcc.starts(hz.case, B, seed)


def noise(hz, B, seed=0):
    """(P, n_steps, B) perturbation sequences, every 7th trajectory with five times the spread; None for a deterministic family"""
    solvers = hz.solvers()
    if not solvers[0].sys.perturb:
        return None
    rng = np.random.default_rng(50 + seed + B)
    out = np.empty((len(solvers), hz.n_steps, B))
    for p, s in enumerate(solvers):
        w = s.perturb_grid[0]
        out[p] = rng.normal(0.0, (w[-1] - w[0]) / 6.0, (hz.n_steps, B))
    out[:, :, ::7] *= 5.0
    return out


def line_starts(B):
    return np.random.default_rng(B).uniform(-1.5, 1.5, size=(B, 1))


def sim_cap_batch(cus):
    """the smallest B with B % 64 == 1 at which XCD 0 of a family of 9 -- members 0 and 8 -- has more tiles of 64 than
    the cus * 32 / 8 workgroups an XCD gets"""
    tiles = (cus * 32 // 8) // 2 + 1
    return (tiles - 1) * SIM_TILE + 1


def launch(B, P, cap, tile):
    """the host's grid of one launch and the kernels' walk, restated (family_horizon_per_xcd in csrc/sdp_hip.hip,
    sdp_fh_walk in csrc/sdp_family_horizon_kernel.h) for a tile of `tile` trajectories and at most `cap` workgroups an XCD:
    per XCD the (member, tile, trip of the stride loop) it visits"""
    tiles = -(-B // tile)
    parts = 1 if P >= 8 else 8 // P
    per_part = -(-tiles // parts)
    wanted = -(-P // 8) * tiles if P >= 8 else per_part
    per_xcd = max(1, min(wanted, cap))
    visits = []
    for xcd in range(8):
        first, part = xcd // parts, xcd % parts
        mine = (P - first + 7) // 8 if first < P else 0
        seen = []
        for unit in range(mine * per_part):
            t = part * per_part + unit % per_part
            if t < tiles:
                seen.append((first + 8 * (unit // per_part), t, unit // per_xcd))
        visits.append(seen)
    return dict(tiles=tiles, parts=parts, wanted=wanted, per_xcd=per_xcd, blocks=8 * per_xcd, visits=visits)


def member_chunk_bytes(fam, extra, members):
    """a chunk_bytes at which `members` members of a run whose arrays take `extra` bytes a member fit in a chunk and one
    more does not"""
    per_member = fam._member_bytes(fam._tables(None if fam.stationnary else 0)) + extra
    return per_member * members + per_member // 2


def solo(solvers):
    return mcc.solo(solvers)


def unit_sources():
    """the generated source of every unit the GPU tests run (for the build: they travel compiled): the horizon unit and
    the sweep unit of every family at its first step, the evaluation and Monte Carlo units of the families whose other
    methods the tests call, and the solo 'generic' units the members are compared with"""
    out = []
    for hz in FAMILIES:
        fam = SolverFamily(hz.solvers())
        t_k = None if fam.stationnary else hz.t0
        tabs = fam._tables(t_k)
        out += [tabs['source'], codegen.family_horizon_unit(tabs['model'], fam.dtype)]
        if fam.stationnary:
            out += [codegen.family_mc_unit(tabs['model'], fam.dtype), codegen.family_policy_unit(tabs['model'], fam.dtype)]
        elif fam.W and not tabs['time_specialized']:
            out.append(codegen.family_mc_unit(tabs['model'], fam.dtype))
        if not fam.stationnary:
            out += [fam._tables(t)['source'] for t in range(hz.T_pol)]         # (bellman_recursion: a unit per step's lanes)
        for s in solo(fam.solvers):
            out.append(s._kernel_plan(t_k, s._trace_now(t_k))['source'])
    return out
