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


class Case(object):
    def __init__(self, name, members, horizon=None, dtype=np.float64):
        self.name, self.members, self.horizon, self.dtype = name, list(members), horizon, np.dtype(dtype)

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


def start(case, per_member=True):
    """a start array that differs from member to member (or one of shape dims), in the case's reals"""
    dims = case.solvers()[0]._shape()
    P = len(case.members)
    rng = np.random.default_rng(len(case.name) + P)
    shape = ((P,) + dims) if per_member else dims
    return rng.uniform(0., 2., size=shape).astype(case.dtype)


def chunk_bytes_for(fam, members):
    """a chunk_bytes at which `members` members fit in a chunk and one more does not"""
    per_member = fam._member_bytes(fam._tables())
    return per_member * members + per_member // 2


def unit_sources():
    """the generated source of every family unit the GPU tests run (for the build: they travel compiled), and of
    the solo 'generic' units they are compared with"""
    from stodynprog_amd import SolverFamily
    out = []
    for case in CASES + [Case('tol', TOL['members'])]:
        fam = SolverFamily(case.solvers())
        steps = [None] if case.horizon is None else range(case.horizon)
        for t_k in steps:
            out.append(fam._tables(t_k)['source'])
            for s in fam.solvers:
                s.kernel = 'generic'
                out.append(s._kernel_plan(None if s.sys.stationnary else t_k, s._trace_now(t_k))['source'])
    return out
