"""Transition operators of families: the cases of tests/test_family_forward_plan.py (CPU) and
tests/test_gpu_family_forward.py (GPU) as a table (not a test file), on the member constructors of tests/family_cases.py.
Every member's policy is `forward_cases.wave_policy` with the member's index as its seed: smooth, off every lattice and
different from member to member.  The definition every result is compared with is stodynprog_amd/forward.py on
`solvers[p]` and `pol[p]` (`definition`).  The shapes are the smallest at which kernel sdp_family_transitions
(csrc/sdp_family_trans_kernel.h), the block-diagonal CSR build and the member-aware pushes can still go wrong:

inventory       d = 1, 10 nodes: one ragged tile of 128 nodes; P = 1, and P = 3 with two identical members (under
                different policies).  By the definition its rows have 0 to 33 entries: empty rows (+0), lane rows and rows
                of k_push_group<16> all occur; member 2 converges at push 20 while the others run to n_max.
storage_ar1     7 x 5 = 35 nodes (one ragged tile of 64), members with other grid ends and laws; the AR(1) axis leaves
                the grid, so weights go negative; 8- and 4-byte reals.
three_d         (5, 4, 3) nodes, nu = 2: 32 nodes a tile, two tiles, the second ragged.
four_d          forward_cases._four_d's equations with their constants as arguments, 4 x 3 x 3 x 3 = 108 nodes: 16 nodes
                a tile, 7 tiles.
finite_horizon  symbolic in time, at t_k = 0 and 3.
pv_sized        deterministic (W = 1, P = [1]) and `data[k]`: another row of constants and another data array per member,
                at t_k = 1 and 3; the definition hands the callables the int.
nan             sqrt of the state: member 0's grid reaches below zero, so two of its nodes have NaN next states and NaN
                costs; member 1's does not.  The NaNs propagate in member 0 alone.
wide            300 nodes, W = 2.  Member 0's policy sends every node to one point: rows of 300 entries, k_push_group<64>,
                and the member is stationary after a few pushes.  Member 1 drifts slowly: every row under 8 entries (the
                lane path), not converged at n_max.  So the wide rows belong to a member that has left the run.
past the caps   line members on LONG_NX nodes, P = 2, sized for 256 compute units: more tiles than the entries kernel's
                grid has workgroups, more rows than k_push's grid has lanes, more nodes a member than the reduction's 64
                workgroups of 256 cover in one trip (`caps`; the GPU test asserts it on the device it runs on).
chunks          storage_ar1 with P = 5 and chunk_bytes such that it runs as 2 + 2 + 1.
shrink          family_cases.SHRINK's 16 inventory members under family_policy_cases.shrink_policies(), tol = 1e-10,
                check_every = 1: by forward.stationary the members stop after SHRINK_PUSHES pushes, so the list of
                running members goes 16 -> 10 -> 5 -> 0; capped at n_max = 19 with check_every = 3, the members that need
                20 or 21 end at the cap, not converged, with the delta of that last check.

Kernel sdp_family_transitions does not map members to XCDs (the head of its header says why), so there are no cases
per mapping.
"""
import functools

import numpy as np

import family_cases as fc
import family_policy_cases as fpc
import forward_cases as fwd
from stodynprog_amd import DPSolver, SysDescription, forward

# ---------------------------------------------------------------------------------------------------------------------
# the launch geometry, restated (csrc/sdp_family_trans_kernel.h; sdp_family_transop_create, transop_launch_push_as and
# sdp_transop_push_until_members in csrc/sdp_hip.hip)
THREADS = 256                      # SDP_FTRANS_THREADS
PUSH_LONG, PUSH_WIDE = 8, 256      # SDP_PUSH_LONG, SDP_PUSH_WIDE: rows of k_push_group<16> and <64> from these lengths on
REDUCTION_BLOCKS = 64              # workgroups of 256 nodes a member in the reduction of a check


def tile(d):
    """nodes of one member a workgroup holds: 2^d lanes a node (SDP_FTRANS_TILE)"""
    return THREADS >> d


def caps(P, S, d, cus):
    """name -> (workgroups wanted for one trip, the cap) of the launches a family's operators go through"""
    return {'sdp_family_transitions': (P * -(-S // tile(d)), cus * 8), 'k_push': (-(-P * S // 256), cus * 8),
            'sdp_family_diff_stats': (-(-S // 256), REDUCTION_BLOCKS)}


# ---------------------------------------------------------------------------------------------------------------------
# members beside those of family_cases
def four_d(a0, a1, a2, a3, target):
    """forward_cases._four_d's equations with their constants as arguments"""
    def make():
        s = SysDescription((4, 1, 1), name='four_d')
        s.dyn = lambda a, b, c, e, u, w: ((a0 * a + 0.5 * u) + w, a1 * b + 0.3 * a, (a2 * c + 0.45 * w) + 0.1 * e, a3 * e - 0.2 * u)
        s.cost = lambda a, b, c, e, u, w: ((a - target) * (a - target) + u * u) + (b * c + e * w)
        s.control_box = lambda a, b, c, e: ((0., 1.),)
        solver = DPSolver(s)
        solver.discretize_state(0, 1, 4, 0, 1, 3, -1, 1, 3, 0, 2, 3)
        solver.perturb_grid = [np.array([-0.2, 0.05, 0.3])]
        solver.perturb_proba = [np.array([0.25, 0.5, 0.25])]
        solver.control_steps = (0.5,)
        return solver
    return make


def rooted(gain, weight, x_min):
    """forward_cases._nan_state's equations with their constants as arguments, on [x_min, 2]: NaN where x < 0"""
    def make():
        s = SysDescription((1, 1, 1), name='rooted')
        s.dyn = lambda x, u, w: ((gain * np.sqrt(x) + u) + w,)
        s.cost = lambda x, u, w: weight * np.sqrt(x) + u * u
        s.control_box = lambda x: ((0., 1.),)
        solver = DPSolver(s)
        solver.discretize_state(x_min, 2, 7)
        solver.perturb_grid = [np.array([-0.25, 0.25])]
        solver.perturb_proba = [np.array([0.5, 0.5])]
        solver.control_steps = (0.5,)
        return solver
    return make


WIDE_NX = 300


def drift(decay, effort, spread):
    """x' = decay x + u + w on WIDE_NX nodes of [0, 1] with a two-point law of `spread` node spacings"""
    h = 1.0 / (WIDE_NX - 1)

    def make():
        s = SysDescription((1, 1, 1), name='drift')
        s.dyn = lambda x, u, w: ((decay * x + u) + w,)
        s.cost = lambda x, u, w: (x - 0.5) * (x - 0.5) + effort * u * u
        s.control_box = lambda x: ((-1., 1.),)
        solver = DPSolver(s)
        solver.discretize_state(0, 1, WIDE_NX)
        solver.perturb_grid = [np.array([-spread * h, 1.25 * spread * h])]
        solver.perturb_proba = [np.array([0.375, 0.625])]
        solver.control_steps = (0.5,)
        return solver
    return make


WIDE_MEMBERS = [drift(0.6, 1.1, 2.5), drift(1.02, 0.9, 2.0)]


def wide_policies():
    """member 0: u = 0.4 - 0.6 x, so every node goes to 0.4 (+ w); member 1: a drift of under a node spacing towards
    the middle, so the chain stays inside the grid and mixes slowly"""
    x = np.linspace(0., 1., WIDE_NX)
    h = 1.0 / (WIDE_NX - 1)
    return np.stack([0.4 - 0.6 * x, -0.02 * x + 0.35 * h * np.sin(9. * x)])[..., None]


LONG_NX = 8 * 256 * 128 + 129      # at 256 compute units: 2 x 2050 tiles against 2048 workgroups, 524546 rows against 524288 lanes


# ---------------------------------------------------------------------------------------------------------------------
class Case(object):
    """name; members (constructors); bounds of the wave policy per control, or `policies` (a function giving the stacked
    array); times: the t_k the operators are built at; time_index: how the definition hands t_k to the callables; stat:
    the arguments of `stationary`; solo: also compared with the solo device operator of every member"""

    def __init__(self, name, members, bounds=None, policies=None, times=(None,), time_index='real', dtype=np.float64,
                 stat=None, solo=False, nan=False):
        self.name, self.members, self.bounds, self.policies = name, list(members), bounds, policies
        self.times, self.time_index, self.dtype, self.solo, self.nan = times, time_index, np.dtype(dtype), solo, nan
        self.stat = dict(tol=1e-8, n_max=30, check_every=4) if stat is None else dict(stat)

    def __repr__(self):
        return self.name

    def solvers(self):
        return [make() for make in self.members]

    def policy(self, solvers=None):
        """(P,) + dims + (nu,) in the case's reals"""
        if self.policies is not None:
            return np.ascontiguousarray(self.policies(), dtype=self.dtype)
        solvers = self.solvers() if solvers is None else solvers
        return np.stack([fwd.wave_policy(s, self.bounds, seed=p) for p, s in enumerate(solvers)]).astype(self.dtype)


AR1_BOUNDS = [(-1., 1.), (0., 0.)]
CASES = [
    Case('inventory P=1', fc.INVENTORY[:1], [(2., 10.)], solo=True),
    Case('inventory P=3', fc.INVENTORY, [(2., 10.)], solo=True),
    Case('storage_ar1 f64', [fc.storage_ar1(*a) for a in fc.AR1], AR1_BOUNDS, solo=True),
    Case('storage_ar1 f32', [fc.storage_ar1(*a, dtype=np.float32) for a in fc.AR1], AR1_BOUNDS, dtype=np.float32,
         stat=dict(tol=1e-5, n_max=30, check_every=4), solo=True),
    Case('three_d', fc.STATIONARY[4].members, [(0., 1.), (0., 1.)]),
    Case('four_d', [four_d(0.8, 0.55, 0.6, 0.9, 0.35), four_d(0.7, 0.52, 0.65, 0.85, 0.4), four_d(0.75, 0.47, 0.72, 0.95, 0.62)],
         [(0., 1.)]),
    Case('finite_horizon', fc.HORIZON[0].members, [(-1., 1.)], times=(0, 3)),
    Case('pv_sized', fc.HORIZON[2].members, [(-0.5, 0.5)], times=(1, 3), time_index='int', solo=True),
    Case('nan', [rooted(1.1, 0.5, -1.), rooted(0.9, 0.6, 0.25)], [(0., 1.)], nan=True),
    Case('wide', WIDE_MEMBERS, policies=wide_policies, stat=dict(tol=1e-10, n_max=12, check_every=1)),
]
CHUNKS = Case('chunks', fc.CHUNKS.members, AR1_BOUNDS)
LONG = Case('past the caps', fc.line_members(2, LONG_NX), [(-0.5, 0.5)], stat=dict(tol=0., n_max=3, check_every=2))
BY_NAME = {c.name: c for c in CASES + [CHUNKS, LONG]}

# to a tolerance (by forward.stationary: tests/test_family_forward_plan.py)
SHRINK = dict(members=fc.SHRINK['members'], tol=1e-10, check_every=1, n_max=200)
SHRINK_PUSHES = [20, 21, 20, 18, 20, 18, 21, 18, 20, 20, 21, 18, 21, 18, 21, 18]
SHRINK_SIZES = [16, 10, 5, 0]
SHRINK_CAPPED = dict(tol=1e-10, check_every=3, n_max=19)
SHRINK_CASE = Case('shrink', SHRINK['members'], policies=fpc.shrink_policies, stat=SHRINK)


# ---------------------------------------------------------------------------------------------------------------------
def definition(case, solvers, pol, t_k):
    """per member (entries, (indptr, indices, data)) by stodynprog_amd/forward.py"""
    out = []
    for p, s in enumerate(solvers):
        e = forward.entries(s, pol[p], t_k, time_index=case.time_index)
        out.append((e, forward.csr(e.S, e.tgt, e.src, e.val)))
    return out


@functools.lru_cache(maxsize=None)
def reference(name, t_k):
    """the definition of a case at t_k, computed once and shared by the tests (leave it unchanged): (solvers, pol,
    [(entries, csr) per member])"""
    case = BY_NAME[name] if name != 'shrink' else SHRINK_CASE
    solvers = case.solvers()
    pol = case.policy(solvers)
    return solvers, pol, definition(case, solvers, pol, t_k)


def vectors(case, dims):
    """(P,) + dims: a signed random vector per member, in the case's reals"""
    P = len(case.members)
    return np.random.default_rng(11 + P).standard_normal((P,) + tuple(dims)).astype(case.dtype)


def chunk_bytes_for(fam, members):
    """a chunk_bytes at which `members` members' operators fit in a chunk and one more does not"""
    per_member = fam._member_bytes(fam._tables()) + fam._transition_bytes()
    return per_member * members + per_member // 2


def unit_sources():
    """the generated source of every unit the GPU tests run: the sweep unit (the handle's) and the transition unit of every
    case at every time, and the solo 'generic' units of the cases compared with the solo operator"""
    from stodynprog_amd import SolverFamily, codegen
    out = []
    for case in CASES + [CHUNKS, LONG, SHRINK_CASE]:
        fam = SolverFamily(case.solvers())
        for t_k in case.times:
            tabs = fam._tables(t_k)
            out += [tabs['source'], codegen.family_trans_unit(tabs['model'], fam.dtype)]
            for s in fam.solvers if case.solo else []:
                s.kernel = 'generic'
                out.append(s._kernel_plan(None if s.sys.stationnary else t_k, s._trace_now(t_k))['source'])
    return list(dict.fromkeys(out))
