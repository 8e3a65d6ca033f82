"""Closed loops under a time-indexed policy: the yardstick and the cases (test infrastructure, like
tests/horizon_cases.py; not a test file).

The definition is the pinned oracle chained step by step: `simulate_indexed` calls oracle.vi_numpy.simulate for ONE
step with the policy slice pol[t0 + k] at time index t0 + k, and carries the state.

`spec_of` makes the oracle's spec of a solver.  Two adapters, neither of which changes a value:
- a model that looks its constants up as `data[k]` gets the time index as the int it stands for (the oracle hands
  it over as a scalar of the run's reals; an array cannot be indexed with one);
- the data arrays such a model closes over are handed to it as tuples of Python floats with the same bits, so that
  a 4-byte run stays in 4-byte arithmetic: numpy promotes `float32 array + float64 SCALAR` to float64, while a Python
  float is a weak scalar -- the constant rounded once to the run's reals, which is what the kernel parameter is.
Several perturbation variables go through tests/multi_perturb.flat_spec (the last argument is the index into the
flat law)."""
import types

import numpy as np

import horizon_cases as hc
import multi_perturb as mp
from oracle import vi_numpy
from stodynprog_amd import SysDescription, DPSolver
from stodynprog_amd.models import NormalLaw


def _weak(f):
    """`f` with every 1-D float64 array among its closure cells (and those of the functions it closes over) replaced by
    a tuple of Python floats of the same values"""
    if not isinstance(f, types.FunctionType) or not f.__closure__:
        return f
    cells = []
    for cell in f.__closure__:
        try:
            v = cell.cell_contents
        except ValueError:                               # an empty cell
            cells.append(cell)
            continue
        if isinstance(v, np.ndarray) and v.ndim == 1 and v.dtype == np.float64:
            v = tuple(float(e) for e in v)               # (float(): same bits, -0.0 included)
        elif isinstance(v, types.FunctionType):
            v = _weak(v)
        cells.append(types.CellType(v))
    g = types.FunctionType(f.__code__, f.__globals__, f.__name__, f.__defaults__, tuple(cells))
    g.__kwdefaults__ = f.__kwdefaults__
    return g


def spec_of(solver, int_time=False):
    """the oracle's spec of `solver`; int_time: the model indexes data with the time index (see the module text)"""
    if len(solver.sys.perturb) >= 2:
        return mp.flat_spec(solver)
    s = solver.sys
    if not int_time:
        return vi_numpy.Spec.from_solver(solver)

    def adapt(f):
        f = _weak(f)

        def g(k, *args, **kw):
            assert float(k) == int(k)
            return f(int(k), *args, **kw)
        return g

    return vi_numpy.Spec(adapt(s.dyn), adapt(s.cost), s.control_box, solver.state_grid, solver.perturb_grid,
                         solver.perturb_proba, solver.control_steps, s.params, s.stationnary)


def simulate_indexed(spec, pol, x0, w, T, t0, dtype):
    """(x, u, g) of T steps from time index t0 under the time-indexed policy `pol` ((T_pol,) + dims + (nu,)): per step one
    call of the oracle's closed loop with pol[t0 + k], the state carried.  w: (>= T, B), row k for step k of the run
    (several perturbation variables: indices into the flat law), or None."""
    x0 = np.atleast_2d(np.asarray(x0, dtype=float))
    xs, us, gs = [np.asarray(x0, dtype=dtype)], [], []
    with np.errstate(all='ignore'):
        for k in range(T):
            x, u, g = vi_numpy.simulate(spec, pol[t0 + k], xs[-1].astype(float), None if w is None else w[k:k + 1], 1,
                                        t0=t0 + k, dtype=dtype)
            xs.append(x[1])
            us.append(u[0])
            gs.append(g[0])
    nu = pol.shape[-1]
    B = x0.shape[0]
    return (np.stack(xs), np.stack(us) if us else np.zeros((0, B, nu), dtype=dtype),
            np.stack(gs) if gs else np.zeros((0, B), dtype=dtype))


def switching():
    """the time-dependent storage with data[k], but a Python `if data[k] > 0:` picks the expression of the stock's
    inflow: the steps do not share a structure (hc.TIME_DATA changes sign between steps 0 and 1), so no table of
    constants serves the horizon"""
    s = SysDescription((2, 1, 1), stationnary=False, name='storage whose structure changes with the step')
    d = np.array(hc.TIME_DATA)

    def lead(k, e):
        if d[k] > 0:
            return e + d[k]
        return (e - 0.5 * abs(e)) + d[k]
    s.dyn = lambda k, e, p, u, w: (lead(k, e) + (1.1 * u - 0.02 * abs(u)), (0.75 * p + 0.05 * k) + w)
    s.cost = lambda k, e, p, u, w: 0.01 * e + (((p - u) * (p - u) + 0.15 * u * u) + d[k] * u)
    s.control_box = lambda k, e, p: ((-1.0, 1.0),)
    s.perturb_laws = [NormalLaw(0, 0.3)]
    solver = DPSolver(s)
    solver.discretize_state(0, 4.0, 21, -2, 2, 13)
    solver.discretize_perturb(-0.9, 0.9, 5)
    solver.control_steps = (0.125,)
    return solver


def timing_problem(n_E=200, n_P=200):
    """the problem tools/horizon_sim_times.py measures: hc.storage on n_E x n_P nodes and 9 perturbation points.  The
    model's control box is a table of the 8 steps of its own horizon; the closed loops do not read the box, but every
    call plans its unit with the box of its first step, so one constant box serves a horizon of any length."""
    s = hc.storage(n_E=n_E, n_P=n_P, n_w=9)
    s.sys.control_box = lambda k, e, p: ((-1.0, 1.0),)
    return s


def policies(solver, kind, T):
    """a time-indexed policy (T,) + dims + (nu,): a different seed at every step, so that a wrong slice index shows"""
    import policies as P
    return np.stack([P.policy(solver, kind, seed=k) for k in range(T)])


# ----------------------------------------------------------------------------------------------------------------------
# the units the tests run: name -> (solver maker, the model indexes data with the time index, steps of its horizon)

def _generic(make):
    def f():
        s = make()
        s.kernel = 'generic'
        return s
    return f


def _finite_horizon():
    from stodynprog_amd import models
    return models.finite_horizon()[1]


def _pv_storage():
    from stodynprog_amd import models
    return models.pv_storage()[1]


T = hc.T                                 # 8 steps
SIMULATE = {
    'storage generic': (_generic(hc.storage), False, T),
    'storage': (hc.storage, False, T),
    'storage noise': (lambda: hc.storage(noise=0.25), False, T),
    'storage data[k]': (lambda: hc.storage(data=True), True, T),
    'storage fp32': (lambda: hc.storage(dtype=np.float32), False, T),
    'line': (hc.line, False, T),
    'reservoirs data[k]': (lambda: hc.reservoirs(data=True), True, T),
    # (the model's data has mp.HORIZON = 4 entries: its horizon is 4 steps, and the later start is step 1)
    'two variables data[k]': (lambda: mp.BY_NAME['horizon'].solver(np.float64), True, mp.HORIZON),
    'finite horizon': (_finite_horizon, False, T),
}
MONTE_CARLO = {
    'storage': SIMULATE['storage'],
    'storage data[k] fp32': (lambda: hc.storage(dtype=np.float32, data=True), True, T),
    'two variables data[k]': SIMULATE['two variables data[k]'],
}
# the units whose code objects tests/test_horizon_sim_plan.py reads, in both reals
PLANNED = {
    'storage': hc.storage,
    'storage data[k]': lambda: hc.storage(data=True),
    'line': hc.line,
    'reservoirs data[k]': lambda: hc.reservoirs(data=True),
    'two variables data[k]': lambda: mp.BY_NAME['horizon'].solver(np.float64),
    'pv_storage': _pv_storage,
}


def plan_source(solver, t=0):
    """the generated source of the unit that runs the horizon of `solver` from step t"""
    return solver._kernel_plan(t, solver._trace_now(t))['source']


def unit_sources():
    """every generated unit the tests of the time-indexed loops run (the build compiles them ahead)"""
    import policies as P
    out = []
    for make in PLANNED.values():
        for dt in (np.float64, np.float32):
            out.append(plan_source(P.as_dtype(make(), dt)))
    for make, _, _ in list(SIMULATE.values()) + list(MONTE_CARLO.values()):
        s = make()
        out += [plan_source(s, t) for t in (0, 1, 3)]
    out.append(plan_source(switching()))
    return out
