"""Parameter studies through ONE solver, family by family.  The callables read a mutable `coef` dict, as a user's
loop over a coefficient would: the first value runs literal constants, the second lifts them into kernel parameters,
the later ones reuse that code object and device problem (trace, box table, plan and problem are all kept from call to
call).  At every value the results must be what the reference computes at call time: oracle/vi_numpy bit for bit
(8-byte reals), or a fresh solver of the generic kernel (4-byte reals, and grids too large for the numpy oracle).

The values change, in turn, a stock coefficient (also more than doubling how far the controls reach along axis 0: the
row window, the staged box and the lead reach are predictions made from it), the exogenous coefficient (with a change
of sign), a cost coefficient and a control-box bound; the last call brings the first values back and must give the
first call's bits."""
import io
import contextlib

import numpy as np
import pytest

from oracle import vi_numpy
from stodynprog_amd import SysDescription, DPSolver, _native as nat
from stodynprog_amd.models import NormalLaw

pytestmark = pytest.mark.gpu

#        stock gain, exogenous coefficient, cost weight, control-box bound (no value equals another constant of the
#        models: two equal constants are one leaf of the DAG, and a new leaf structure starts over with literals)
VALUES = [(1.1, 0.75, 0.15, 1.0),
          (1.3, 0.75, 0.15, 1.0),      # the constants are lifted
          (1.3, -0.65, 0.15, 1.0),     # the lifted problem serves: sign change of the exogenous process
          (1.3, -0.65, 0.45, 1.0),     # .. a cost coefficient
          (3.3, -0.65, 0.45, 0.75),    # .. a box bound, and 2.25 x the reach along axis 0
          (1.1, 0.75, 0.15, 1.0)]      # the first values again


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def storage(coef, n_E=21, n_P=13, n_w=5, E_max=4.0, noise=0.0, dtype=np.float64):
    """a stock and an AR(1) exogenous process (storage-separable); `noise`: the perturbation also reaches the stock
    through a final sum (the shifted lattice)"""
    s = SysDescription((2, 1, 1), name='storage study')
    if noise:
        s.dyn = lambda e, p, u, w: ((e + coef['g'] * u - 0.02 * abs(u)) - noise * w, coef['rho'] * p + w)
    else:
        s.dyn = lambda e, p, u, w: (e + coef['g'] * u - 0.02 * abs(u), coef['rho'] * p + w)
    s.cost = lambda e, p, u, w: (p - u) * (p - u) + coef['k'] * u * u + 0.01 * e
    s.control_box = lambda e, p: ((-coef['cap'], coef['cap']),)
    s.perturb_laws = [NormalLaw(0, 0.3)]
    solver = DPSolver(s, dtype=dtype)
    solver.discretize_state(0, E_max, n_E, -2, 2, n_P)
    solver.discretize_perturb(-0.9, 0.9, n_w)
    solver.control_steps = (0.25,)
    return solver


def line(coef):
    """one state, x' = (x + g u) - rho w, a cost that does not see w"""
    s = SysDescription((1, 1, 1), name='line study')
    s.dyn = lambda x, u, w: (x + coef['g'] * u - coef['rho'] * w,)
    s.cost = lambda x, u, w: coef['k'] * u * u + 0.1 * x * x
    s.control_box = lambda x: ((-coef['cap'], coef['cap']),)
    s.perturb_laws = [NormalLaw(0, 0.3)]
    solver = DPSolver(s)
    solver.discretize_state(-4, 4, 65)
    solver.discretize_perturb(-0.9, 0.9, 9)
    solver.control_steps = (0.125,)
    solver.LINE_MIN_CELLS = 0                    # (the filtered line kernel at this size too)
    return solver


def reservoirs(coef):
    """two stocks driven by the controls next to an exogenous inflow (the reduced-array sweep)"""
    s = SysDescription((3, 2, 1), name='reservoirs study')
    s.dyn = lambda a, b, y, u, v, w: (a + 0.5 * (0.7 + 0.5 * y) - coef['g'] * u, b + coef['g'] * u - v,
                                      0.3 + coef['rho'] * (y - 0.3) + w)
    s.cost = lambda a, b, y, u, v, w: ((v - 0.8) * (v - 0.8) + coef['k'] * (u - v) * (u - v)
                                       + 4.0 * np.where(a > 1.7, a - 1.7, 0.0 * a) + 8.0 * np.where(b < 0.3, 0.3 - b, 0.0 * b))
    s.control_box = lambda a, b, y: ((0., coef['cap']), (0., 1.))
    s.perturb_laws = [NormalLaw(0, 0.1)]
    solver = DPSolver(s)
    solver.discretize_state(0., 2., 16, 0., 2., 12, -0.4, 0.8, 8)
    solver.discretize_perturb(-0.3, 0.3, 5)
    solver.control_steps = (0.125, 0.25)
    return solver


def coupled(coef):
    """the control also reaches the trailing state variables (a table per control)"""
    s = SysDescription((3, 1, 1), name='coupled study')
    s.dyn = lambda x0, x1, x2, u, w: (x0 + 0.1 * coef['g'] * u, 0.05 + coef['rho'] * x1 + 0.1 * x2 + w + 0.1 * u,
                                      0.05 + 0.1 * x1 + 0.8 * x2 + 0.5 * w)
    s.cost = lambda x0, x1, x2, u, w: (1.8 * x1 - 0.9 - u) * (1.8 * x1 - 0.9 - u) + coef['k'] * u * u + 0.25 * x0
    s.control_box = lambda x0, x1, x2: ((-coef['cap'], coef['cap']),)
    s.perturb_laws = [NormalLaw(0, 0.05)]
    solver = DPSolver(s)
    solver.discretize_state(0, 1, 12, 0, 1, 10, 0, 1, 9)
    solver.discretize_perturb(-0.15, 0.15, 7)
    solver.control_steps = (0.25,)
    return solver


# family: (solver maker, kernel, what backend_info must say at the first value, reference)
FAMILIES = {
    'column': (storage, 'column', dict(kernel='column', filter_form='reduced table', certified_filter=True), 'oracle'),
    'column fp32': (lambda c: storage(c, dtype=np.float32), 'column',
                    dict(kernel='column', filter_form='reduced table', certified_filter=True), 'generic'),
    'shifted lattice': (lambda c: storage(c, noise=0.05), 'column',
                        dict(kernel='column', filter_form='shifted lattice'), 'oracle'),
    'line': (line, 'auto', dict(kernel='line', filter_form='shifted lattice'), 'oracle'),
    'lead': (reservoirs, 'lead', dict(kernel='lead', filter_form='reduced array'), 'oracle'),
    'row window': (lambda c: storage(c, n_E=2048, n_P=5, n_w=11, E_max=20.0), 'column',
                   dict(kernel='column', table_per_control=False), 'generic'),
    'table per control': (coupled, 'column', dict(kernel='column', table_per_control=True), 'oracle'),
    'staged': (storage, 'staged', dict(kernel='staged'), 'oracle'),
    'generic': (storage, 'generic', dict(kernel='generic'), 'oracle'),
}


def _reference(make, coef, ref, V, pol_in, dtype):
    """value_iteration, three chained sweeps and a 3-step policy evaluation as the reference computes them now"""
    if ref == 'oracle':
        spec = vi_numpy.Spec.from_solver(make(coef))
        J, pol, idx, _ = vi_numpy.value_iteration(spec, V)
        K = V
        for _ in range(3):
            K = vi_numpy.value_iteration(spec, K)[0]
        E = vi_numpy.eval_policy(spec, pol_in, 3, J_zero=V)
        return J, pol, idx, K, E
    s = make(coef)
    s.kernel = 'generic'
    J, pol = s.value_iteration(V, report_time=False)
    idx = s.last_policy_index
    K, _ = quiet(s.value_iterations, V, 3)
    E = quiet(s.eval_policy, pol_in, 3, False, V)
    return J, pol, idx, K, E


@pytest.mark.timeout(900)
@pytest.mark.parametrize('family', sorted(FAMILIES))
def test_parameter_study_follows_the_values(gpu, monkeypatch, family):
    make, kernel, first_info, ref = FAMILIES[family]
    coef = dict(zip(('g', 'rho', 'k', 'cap'), VALUES[0]))
    solver = make(coef)
    solver.kernel = kernel
    dtype = solver.dtype
    compiled, recording = [], [False]
    real_compile = nat.compile_model
    monkeypatch.setattr(nat, 'compile_model',
                        lambda src, **k: (compiled.append(src) if recording[0] else None) or real_compile(src, **k))
    rng = np.random.default_rng(8)
    V = rng.standard_normal(solver._state_grid_shape).astype(dtype).astype(float)
    results, probs, n_compiled, infos = [], [], [], []
    for values in VALUES:
        coef.update(zip(('g', 'rho', 'k', 'cap'), values))
        recording[0] = True
        J, pol = solver.value_iteration(V, report_time=False)
        idx = solver.last_policy_index
        K, _ = quiet(solver.value_iterations, V, 3)
        # (the policy of the first value, on its lattice at every value: the controls are in any box the values give)
        pol_in = results[0][1] if results else pol
        E = quiet(solver.eval_policy, pol_in, 3, False, V)
        recording[0] = False
        infos.append(dict(solver.backend_info))
        Jr, polr, idxr, Kr, Er = _reference(make, coef, ref, V, pol_in, dtype)
        assert np.array_equal(J, Jr) and np.array_equal(pol, polr), (family, values)
        assert np.array_equal(idx, idxr), (family, values)
        assert np.array_equal(K, Kr), (family, values, 'value_iterations')
        assert np.array_equal(E, Er), (family, values, 'eval_policy')
        results.append((J, pol, K, E))
        probs.append([p for k, p in solver._cache.items() if k[0] == 'problem'][0])
        n_compiled.append(len(set(compiled)))
    for k, v in first_info.items():
        assert infos[0][k] == v, (family, k, infos[0])
    if family == 'line':
        # the filtered line kernel takes literal constants only: from the second value on the study runs the direct kernel
        assert all(i['kernel'] == 'generic' for i in infos[1:]), infos
    else:
        assert all(i['kernel'] == infos[0]['kernel'] for i in infos), infos
    if family == 'row window':
        assert all(i['row_window'] for i in infos), infos
    assert infos[0]['lifted_constants'] == 0 and all(i['lifted_constants'] > 0 for i in infos[1:]), infos
    # the lifted problem served the later values: no new code object, the same device problem
    assert probs[1] is probs[2] is probs[3], family
    assert n_compiled[3] == n_compiled[1], (family, n_compiled)
    # the first values again: the first call's bits
    for a, b in zip(results[0], results[-1]):
        assert np.array_equal(a, b), family
    assert not np.array_equal(results[0][0], results[2][0])


def test_bellman_recursion_with_time_indexed_data_on_the_column_kernel(gpu):
    """time-indexed data read by the dynamics (not only the cost, as in models.pv_storage): every step of the
    horizon is its own trace with lifted constants, one code object of the column kernel serves them all, and every
    step equals the oracle evaluated at that step"""
    inflow = np.array([0.3, -0.2, 0.5, 0.0, -0.4, 0.25])
    s = SysDescription((2, 1, 1), stationnary=False, name='time-indexed inflow')
    s.dyn = lambda k, e, p, u, w: (e + u - 0.02 * abs(u) + inflow[k], 0.8 * p + w)
    s.cost = lambda k, e, p, u, w: (p - u) * (p - u) + 0.1 * u * u
    s.control_box = lambda k, e, p: ((-1., 1.),)
    s.perturb_laws = [NormalLaw(0, 0.3)]
    solver = DPSolver(s)
    solver.discretize_state(0, 4, 21, -2, 2, 13)
    solver.discretize_perturb(-0.9, 0.9, 5)
    solver.control_steps = (0.25,)
    J_fin = np.random.default_rng(3).standard_normal((21, 13))
    T = len(inflow)
    J, pol = quiet(solver.bellman_recursion, T, J_fin)
    info = solver.backend_info
    assert info['kernel'] == 'column' and info['time_specialized'] and info['lifted_constants'] > 0, info
    spec = vi_numpy.Spec.from_solver(solver)
    nxt = J_fin
    for t in range(T - 1, -1, -1):
        Jo, po, _, _ = vi_numpy.value_iteration(spec, nxt, t_k=t)
        assert np.array_equal(J[t], Jo) and np.array_equal(pol[t], po), t
        nxt = Jo
