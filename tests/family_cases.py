"""The families of tests/test_family_plan.py (CPU) and tests/test_gpu_family.py (GPU): for every case a list of
member constructors, each returning a fresh DPSolver set up exactly as for a solo call.  The shapes are the smallest at
which kernel sdp_family_sweep (csrc/sdp_family_kernel.h) can still go wrong:

inventory       D = 1, 10 nodes, W = 4, one box per member; P = 1 and P = 3 with two identical members.  A fourth
                member whose constants coincide (h == c) is the refusal the hash-consed trace forces.
storage_ar1     7 x 5 = 35 nodes (no multiple of the nodes per wavefront at any lane count), per-node boxes whose lattice
                sizes differ by node and by member (lane counts 8, 8 and 16), other grid ends and laws per member,
                nu = 2 with a one-point control; 8- and 4-byte reals.
three_d         D = 3, nu = 2: two_reservoirs' equations with their constants as arguments, (5, 4, 3) nodes, W = 3,
                a lattice of 81 points: more than the 64 lanes of a wavefront.
finite_horizon  models.finite_horizon with its coefficients as arguments: a symbolic time index, a box (and with it a
                lane count and a code object) that changes from step to step; bellman_recursion over 4 steps.
pv              models.pv_storage with another loss per member: deterministic, `data[k]` lifted per step.
pv_sized        the same with another capacity and another data array per member (the reference's det_storage_perf.py).
chunks          storage_ar1 with P = 5 and chunk_bytes such that it runs as 2 + 2 + 1.
tol             inventory, P = 3, rel_dp, tol = 1e-6, check_every = 3, n_iter = 200, with constants at which the
                members need different numbers of sweeps (18, 21, 18 by oracle/vi_numpy.py; those of `inventory` all
                need 18) and none reaches n_iter.

The cases above are compared with solo 'generic' calls on the device.  Those below (`Case(..., oracle=True)`) reach the
three ways the kernel maps listed members to XCDs and the second trip of its walk, and are compared with
oracle/vi_numpy.py alone (`oracle_sweeps`); no solo unit is built for them.  Their members are `line(...)`: 41 controls,
so 64 lanes and a tile of 4 nodes; member p of every line family is the same problem with the same start whatever P.

line P=..       P in MAPPING_P, 9 nodes (3 tiles, the last ragged): 1..3 members on an XCD (P >= 8), one XCD a member
                and idle XCDs (5..7), 8 / P XCDs a member, each a part of its tiles (P < 5).
line P=65       a second block of k_family_pick_ref (64 members a block).
line strided    P = 17, 515 nodes (129 tiles, the last ragged), 8- and 4-byte reals: 2 * 129 units on the XCDs with two
                members and 3 * 129 on XCD 0 exceed the cus workgroups an XCD gets (`launch`), so they walk again.
shrink          16 inventory members, rel_dp, tol = 1e-6, check_every = 1: by the oracle the list runs
                16 -> 13 -> 6 -> 4 -> 0 (`list_sizes`), through all three mappings, non-contiguous from the first drop.
chunks P>=8     line P=17 with chunk_bytes such that it runs as 9 + 8.
line long       P = 2 on 64 * 256 + 129 nodes: k_family_shift and sdp_family_diff_stats launch at most 64 workgroups of 256
                nodes a member, so the last 129 nodes are a second trip; and each of a member's 4 XCDs walks 1033 tiles.
"""
import numpy as np

from stodynprog_amd import DPSolver, SysDescription, models
from stodynprog_amd.models import NormalLaw


def as_dtype(solver, dtype):
    """the same problem in other reals"""
    s = DPSolver(solver.sys, dtype=dtype)
    s.state_grid, s.perturb_grid = solver.state_grid, solver.perturb_grid
    s.perturb_proba, s.control_steps = solver.perturb_proba, solver.control_steps
    s._state_grid_shape, s._state_ref_ind = solver._state_grid_shape, solver._state_ref_ind
    return s


def inventory(h, p, c):
    return lambda: models.inventory(None, h, p, c)[1]


def storage_ar1(E_rated, P_rated, p_corr, dtype=np.float64):
    return lambda: as_dtype(models.storage_ar1(None, n_E=7, n_P=5, n_w=3, steps=(0.5, 0.1), E_rated=E_rated,
                                               P_rated=P_rated, p_corr=p_corr)[1], dtype)


def three_d(inflow, gain, target, spill_cost):
    """models.two_reservoirs' equations with their constants as arguments, on (5, 4, 3) nodes"""
    def make():
        sysd = SysDescription((3, 2, 1), name='Two reservoirs')

        def dyn(a, b, y, u, v, w):
            return (a + (inflow + gain * y) - u, b + u - v, 0.3 + 0.7 * (y - 0.3) + w)

        def box(a, b, y):
            return ((0., 1.), (0., 1.))

        def cost(a, b, y, u, v, w):
            spill = np.where(a > 1.7, a - 1.7, 0.0 * a) + np.where(b > 1.7, b - 1.7, 0.0 * b)
            dry = np.where(a < 0.3, 0.3 - a, 0.0 * a) + np.where(b < 0.3, 0.3 - b, 0.0 * b)
            return (v - target) * (v - target) + 0.05 * (u - v) * (u - v) + spill_cost * spill + 8.0 * dry
        sysd.dyn, sysd.control_box, sysd.cost = dyn, box, cost
        sysd.perturb_laws = [NormalLaw(0, 0.1)]
        s = DPSolver(sysd)
        s.discretize_state(0., 2., 5, 0., 2., 4, -0.2, 0.8, 3)
        s.discretize_perturb(-0.3, 0.3, 3)
        s.control_steps = (0.125, 0.125)
        return s
    return make


def finite_horizon(decay, drift, track, effort, width):
    """models.finite_horizon(n_x=9, n_w=3) with its coefficients as arguments"""
    def make():
        fh = SysDescription((1, 1, 1), stationnary=False, name='finite horizon')

        def fh_dyn(k, x, u, w):
            return (decay * x + u + w + drift * k,)

        def fh_cost(k, x, u, w):
            return (x - track * k) ** 2 + effort * u * u

        def fh_box(k, x):
            return ((-1., 1. + width * k),)
        fh.dyn, fh.cost, fh.control_box = fh_dyn, fh_cost, fh_box
        fh.perturb_laws = [NormalLaw(0, 0.1)]
        s = DPSolver(fh)
        s.discretize_state(-2, 2, 9)
        s.discretize_perturb(-0.3, 0.3, 3)
        s.control_steps = (0.125,)
        return s
    return make


def pv(loss):
    return lambda: models.pv_storage(None, T=6, N_E=9, u_step=0.05, loss=loss)[1]


def pv_sized(E_rated, scale, T=6, dt=0.5, loss=0.05):
    """models.pv_storage with the capacity and the production data as arguments"""
    def make():
        P_rated = 1.0
        data = models.pv_profile(T + 24, dt)[24:] * scale           # (daylight hours: the data differ from step to step)
        sto = SysDescription((1, 1, 0), name='Deterministic Storage for PV', stationnary=False)

        def dyn_sto(k, E_sto, P_sto):
            return (E_sto + (P_sto - loss * abs(P_sto)) * dt,)

        def admissible_controls(k, E_sto):
            P_neg = np.max((-E_sto / (1 + loss) / dt, -P_rated))
            P_pos = np.min(((E_rated - E_sto) / (1 - loss) / dt, P_rated))
            return ((P_neg, P_pos),)

        def cost_model(k, E_sto, P_sto):
            P_grid = data[k] - P_sto
            over = np.where(P_grid > 0.4, P_grid - 0.4, 0)
            neg = np.where(P_grid < 0, P_grid, 0)
            return over ** 2 + neg ** 2 + 0 * P_sto ** 2
        sto.dyn, sto.control_box, sto.cost = dyn_sto, admissible_controls, cost_model
        s = DPSolver(sto)
        s.discretize_state(0, E_rated, 9)
        s.control_steps = (0.05,)
        return s
    return make


def line(decay, effort, target, n_x, dtype=np.float64):
    """one state, one control on 41 lattice points (64 lanes), three lifted constants"""
    def make():
        sysd = SysDescription((1, 1, 1), name='line')
        sysd.dyn = lambda x, u, w: (decay * x + u + w,)
        sysd.cost = lambda x, u, w: (x - target) * (x - target) + effort * u * u
        sysd.control_box = lambda x: ((-1., 1.),)
        sysd.perturb_laws = [NormalLaw(0, 0.1)]
        s = DPSolver(sysd, dtype=dtype)
        s.discretize_state(-2, 2, n_x)
        s.discretize_perturb(-0.3, 0.3, 3)
        s.control_steps = (0.05,)
        return s
    return make


def line_members(P, n_x, dtype=np.float64):
    """member p is the same problem in every line family (no two of its constants coincide up to p = 65)"""
    return [line(0.5 + 0.005 * p, 1.11 + 0.05 * p, -0.43 + 0.03 * p, n_x, dtype) for p in range(P)]


class Case(object):
    """oracle: compared with oracle/vi_numpy.py alone, so unit_sources() emits no solo unit for it"""

    def __init__(self, name, members, horizon=None, dtype=np.float64, oracle=False):
        self.name, self.members, self.horizon, self.dtype = name, list(members), horizon, np.dtype(dtype)
        self.oracle = oracle

    def solvers(self):
        return [make() for make in self.members]

    def __repr__(self):
        return self.name


INVENTORY = [inventory(0.5, 3, 1), inventory(0.7, 2, 1.5), inventory(0.5, 3, 1)]
COINCIDING = inventory(1.0, 3, 1.0)                # h == c: one node of the trace
AR1 = [(2, 4, 0.8), (10, 1, 0.5), (5, 4, 0.8)]
AR1_FIVE = AR1 + [(3, 2, 0.6), (8, 3, 0.7)]
TOL = dict(members=[inventory(0.5, 3, 1), inventory(2.0, 3, 1.5), inventory(0.5, 3, 1)],
           tol=1e-6, check_every=3, n_iter=200)

STATIONARY = [
    Case('inventory P=1', INVENTORY[:1]),
    Case('inventory P=3', INVENTORY),
    Case('storage_ar1 f64', [storage_ar1(*a) for a in AR1]),
    Case('storage_ar1 f32', [storage_ar1(*a, dtype=np.float32) for a in AR1], dtype=np.float32),
    Case('three_d', [three_d(0.65, 0.5, 0.8, 4.0), three_d(0.6, 0.4, 0.9, 3.0)]),
]
HORIZON = [
    Case('finite_horizon', [finite_horizon(0.9, 0.05, 0.1, 0.2, 0.5), finite_horizon(0.8, 0.04, 0.15, 0.3, 0.25),
                            finite_horizon(0.95, 0.06, 0.12, 0.25, 0.75)], horizon=4),
    Case('pv', [pv(0.05), pv(0.1), pv(0.0)], horizon=6),
    Case('pv_sized', [pv_sized(2.0, 1.0), pv_sized(1.0, 0.8), pv_sized(3.0, 1.2)], horizon=6),
]
CHUNKS = Case('chunks', [storage_ar1(*a) for a in AR1_FIVE])
CASES = STATIONARY + HORIZON + [CHUNKS]

# the cases compared with the oracle
MAPPING_P = (2, 4, 6, 7, 8, 9, 16, 17)
LINE_NX, STRIDED_NX = 9, 515
MAPPING = [Case('line P={}'.format(P), line_members(P, LINE_NX), oracle=True) for P in MAPPING_P]
MANY = Case('line P=65', line_members(65, LINE_NX), oracle=True)
STRIDED = [Case('line strided f64', line_members(17, STRIDED_NX), oracle=True),
           Case('line strided f32', line_members(17, STRIDED_NX, np.float32), dtype=np.float32, oracle=True)]
CHUNKS_17 = MAPPING[-1]
LONG_NX = 64 * 256 + 129
LONG = Case('line long', line_members(2, LONG_NX), oracle=True)
SHRINK = dict(members=[inventory(*a) for a in (
    (0.5, 3, 1), (2.0, 3, 1.5), (0.7, 2, 1.5), (0.3, 4, 1.25), (1.5, 2.5, 0.75), (0.25, 5, 2), (3.0, 4, 1.5), (0.6, 6, 1.75),
    (1.25, 3.5, 0.8), (0.9, 2.2, 1.1), (4.0, 5, 2.5), (0.1, 3, 1.2), (6.0, 8, 2.5), (0.05, 9, 4), (8.0, 9.5, 0.4),
    (0.02, 1.5, 0.9))], tol=1e-6, check_every=1, n_iter=200)
SHRINK_SWEEPS = [17, 19, 18, 16, 17, 17, 19, 17, 17, 18, 19, 16, 19, 17, 17, 16]      # by the oracle (test_family_plan.py)
SHRINK_SIZES = [16, 13, 6, 4, 0]
SHRINK_CASE = Case('shrink', SHRINK['members'], oracle=True)
ORACLE_CASES = MAPPING + [MANY] + STRIDED + [SHRINK_CASE, LONG]


def start(case, per_member=True):
    """a start array that differs from member to member (or one of shape dims), in the case's reals"""
    dims = case.solvers()[0]._shape()
    P = len(case.members)
    rng = np.random.default_rng(len(case.name) + P)
    shape = ((P,) + dims) if per_member else dims
    return rng.uniform(0., 2., size=shape).astype(case.dtype)


def line_start(case):
    """(P,) + dims in the case's reals: member p's start depends on p alone, so a line member has one oracle result
    whatever family it is in"""
    dims = case.members[0]()._shape()
    return np.stack([np.random.default_rng(1000 + p).uniform(0., 2., size=dims)
                     for p in range(len(case.members))]).astype(case.dtype)


def launch(S, lanes, n_active, cus):
    """the host's grid of one family backup, restated (family_backup in csrc/sdp_hip.hip, the head of
    csrc/sdp_family_kernel.h): tiles per member, XCDs per member, workgroups per XCD, and the units every XCD walks"""
    tile = (64 // lanes) * 4
    tiles = -(-S // tile)
    parts = 1 if n_active >= 8 else 8 // n_active
    per_part = -(-tiles // parts)
    per_xcd = max(1, min(-(-n_active // 8) * tiles if n_active >= 8 else per_part, cus))
    units = []
    for xcd in range(8):
        first = xcd // parts
        mine = (n_active - first + 7) // 8 if first < n_active else 0
        units.append(mine * per_part)
    return dict(tiles=tiles, parts=parts, per_xcd=per_xcd, units=units)


def list_sizes(sweeps, n_iter):
    """the distinct lengths of the list of members still running, from the sweeps each member needs"""
    sizes = [sum(1 for n in sweeps if n > k) for k in range(n_iter + 1)]
    return [n for i, n in enumerate(sizes) if i == 0 or n != sizes[i - 1]]


def oracle_sweeps(make, J0, n_iter, rel_dp=False, tol=None, check_every=1):
    """oracle/vi_numpy.py's value_iteration_real of one member, iterated: per sweep (J, J_ref or None, pol, idx), and
    with `tol` the checks [(k, dmin, dmax)] of stodynprog_amd/convergence.py's rule, stopping where it says so"""
    from oracle import vi_numpy
    from stodynprog_amd import convergence as conv
    s = make()
    spec = vi_numpy.Spec.from_solver(s)
    J = np.asarray(J0, dtype=s.dtype)
    out, checks = [], []
    for k in range(1, n_iter + 1):
        J_k, pol, idx, _ = vi_numpy.value_iteration_real(spec, (J, 0.) if rel_dp else J, s.dtype, rel_dp)
        J_k, ref = J_k if rel_dp else (J_k, None)
        out.append((J_k, ref, pol, idx))
        if tol is not None and conv.is_check(k, n_iter, check_every):
            dmin, dmax = conv.diff_stats(J_k, J, s.dtype)
            checks.append((k, dmin, dmax))
            if conv.converged(dmin, dmax, tol):
                break
        J = J_k
    return out, checks


def chunk_bytes_for(fam, members):
    """a chunk_bytes at which `members` members fit in a chunk and one more does not"""
    per_member = fam._member_bytes(fam._tables())
    return per_member * members + per_member // 2


def unit_sources():
    """the generated source of every family unit the GPU tests run (for the build: they travel compiled), and of
    the solo 'generic' units they are compared with (none for the cases compared with the oracle)"""
    from stodynprog_amd import SolverFamily
    out = []
    for case in CASES + [Case('tol', TOL['members'])] + ORACLE_CASES:
        fam = SolverFamily(case.solvers())
        steps = [None] if case.horizon is None else range(case.horizon)
        for t_k in steps:
            out.append(fam._tables(t_k)['source'])
            for s in [] if case.oracle else fam.solvers:
                s.kernel = 'generic'
                out.append(s._kernel_plan(None if s.sys.stationnary else t_k, s._trace_now(t_k))['source'])
    return out
