"""Systems with SEVERAL perturbation variables on the device (csrc/sdp_multiw_kernel.h) against the pinned oracle on the
flat law (tests/multi_perturb.py: `flat_spec`), bit for bit: every comparison of results is np.array_equal, no
tolerance appears in this file.  The cases are the table tests/multi_perturb.py; tests/test_multi_perturb_plan.py
checks on the CPU that each plans what it claims.

Backups: every case in both reals from four cost-to-go arrays (zeros, smooth, seeded random, one with NaN and +-inf),
sweeps 1 and 3 of three chained sweeps with and without the relative-DP shift, eval_policy with the fused shift and
its list of reference costs, the stopping sweep of `tol=` against the host rule of stodynprog_amd/convergence.py.  The
time-dependent case runs what a time-dependent system has: bellman_recursion over its horizon and eval_policy at
step 0.  `degenerate` (W = (5, 1)) also equals the ONE-variable system with the second variable's point a constant.
simulate equals the hand-written numpy loop, monte_carlo equals simulate fed with monte_carlo_draws, and a change of
the SECOND variable alone between two calls changes the result to the new oracle's."""
import functools

import numpy as np
import pytest

import multi_perturb as mp
import test_gpu_montecarlo as tm
from oracle import vi_numpy
from stodynprog_amd import SysDescription, DPSolver, convergence as conv, perturb
from stodynprog_amd.trace import TraceError

pytestmark = pytest.mark.gpu
_quiet, _close = tm._quiet, tm._close
INPUTS = ('zeros', 'smooth', 'random', 'non-finite')
STATIONARY = [c for c in mp.CASES if not c.horizon]


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.dtype.kind == 'f':
        assert got.dtype == want.dtype, (what, got.dtype, want.dtype)
    bad = ~((got == want) | ((got != got) & (want != want)))
    assert not bad.any(), '{}: differs from the oracle at {} of {} entries'.format(what, int(bad.sum()), got.size)


def _at_ref_zero(V, ref_ind):
    """the input as a differential cost: zero at the reference node (the non-finite entries are elsewhere)"""
    assert np.isfinite(V[ref_ind])
    return V - V[ref_ind]


@functools.lru_cache(maxsize=None)
def _oracle_sweeps(name, real, which, rel_dp):
    """three chained oracle sweeps of a stationary case on the flat law: [(J, refs so far, pol, idx), ...].  With the
    relative-DP shift the chain ends where the reference node's cost is not finite (the non-finite input): the next
    sweep's input is no differential cost, which the reference asserts (sdp.py:488)"""
    dt = mp.DTYPES[real]
    solver = mp.BY_NAME[name].solver(dt)
    spec = mp.flat_spec(solver)
    V = mp.inputs(solver._shape(), dt)[which]
    kw = {} if dt == np.float64 else dict(dtype=dt)        # (8-byte reals: the reference's own path of the oracle)
    out, refs = [], []
    with np.errstate(all='ignore'):
        J = (_at_ref_zero(V, spec.ref_ind), 0.) if rel_dp else V
        for _ in range(3):
            J, pol, idx, _ = vi_numpy.value_iteration(spec, J, rel_dp=rel_dp, **kw)
            if rel_dp:
                refs.append(float(J[1]))
            out.append(((J[0] if rel_dp else J).astype(dt), list(refs), pol.astype(dt), idx))
            if rel_dp and not J[0][spec.ref_ind] == 0.:
                break
    return out


@pytest.mark.parametrize('real', sorted(mp.DTYPES))
@pytest.mark.parametrize('case', STATIONARY, ids=repr)
def test_chained_sweeps_equal_the_oracle(gpu, case, real):
    dt = mp.DTYPES[real]
    solver = case.solver(dt)
    try:
        for which in INPUTS:
            V = mp.inputs(solver._shape(), dt)[which]
            for rel_dp in (False, True):
                want = _oracle_sweeps(case.name, real, which, rel_dp)
                J0 = (_at_ref_zero(V, solver._state_ref_ind), 0.) if rel_dp else V
                assert len(want) == 3 or which == 'non-finite'
                for n in (1, 3)[:1 if len(want) < 3 else 2]:
                    what = '{} {} {} rel_dp={} sweep {}'.format(case, real, which, rel_dp, n)
                    J, pol = _quiet(solver.value_iterations, J0, n, rel_dp=rel_dp, report_time=False, J_ref_full=True)
                    info = solver.backend_info
                    assert info['mode'] == 'traced' and info['kernel'] == 'generic' and info['perturb_vars'] == case.m
                    assert info['lanes_per_node'] == case.lanes
                    wJ, wrefs, wpol, widx = want[n - 1]
                    if rel_dp:
                        J, refs = J
                        _same(np.asarray(refs, dtype=float), np.asarray(wrefs), what + ' J_ref')
                    _same(J, wJ, what + ' J')
                    _same(pol, wpol, what + ' policy values')
                    _same(solver.last_policy_index, widx.astype(np.int32), what + ' policy index')
        # one sweep through value_iteration (host arrays in and out in one library call): the same bits
        V = mp.inputs(solver._shape(), dt)['random']
        J, pol = _quiet(solver.value_iteration, V, report_time=False)
        wJ, _, wpol, widx = _oracle_sweeps(case.name, real, 'random', False)[0]
        _same(J, wJ, 'value_iteration J')
        _same(pol, wpol, 'value_iteration policy')
        _same(solver.last_policy_index, widx.astype(np.int32), 'value_iteration index')
    finally:
        _close(solver)


def _policy(solver, spec):
    """a policy that is none of the lattice's: halfway between the box ends, tilted along the first axis"""
    shape = solver._shape()
    nu = len(solver.sys.control)
    pol = np.zeros(shape + (nu,))
    tilt = np.linspace(0.2, 0.8, shape[0]).reshape((-1,) + (1,) * (len(shape) - 1))
    for ind in np.ndindex(*shape):
        x = tuple(g[i] for g, i in zip(solver.state_grid, ind))
        box = solver.sys.control_box(*(((0,) + x) if not solver.sys.stationnary else x))
        for c, (lo, hi) in enumerate(box):
            pol[ind + (c,)] = lo + (hi - lo) * np.broadcast_to(tilt, shape)[ind]
    return pol


@pytest.mark.parametrize('real', sorted(mp.DTYPES))
@pytest.mark.parametrize('case', mp.CASES, ids=repr)
def test_eval_policy_with_the_fused_shift(gpu, case, real):
    dt = mp.DTYPES[real]
    solver = case.solver(dt)
    spec = mp.flat_spec(solver)
    pol = _policy(solver, spec)
    t_k = 0 if case.horizon else None
    try:
        for which in INPUTS:
            V = mp.inputs(solver._shape(), dt)[which]
            with np.errstate(all='ignore'):
                wJ, wrefs = vi_numpy.eval_policy(spec, pol, 3, rel_dp=True, J_zero=V, J_ref_full=True, dtype=dt, t_k=t_k)
            J, refs = _quiet(solver.eval_policy, pol, 3, rel_dp=True, J_zero=V, report_time=False, J_ref_full=True)
            assert solver.backend_info['mode'] == 'traced' and solver.backend_info['perturb_vars'] == case.m
            what = '{} {} {}'.format(case, real, which)
            _same(J, wJ, what + ' eval_policy J')
            _same(np.asarray(refs, dtype=float), np.asarray(wrefs, dtype=float), what + ' eval_policy J_ref')
        # .. and without the shift
        V = mp.inputs(solver._shape(), dt)['random']
        with np.errstate(all='ignore'):
            wJ = vi_numpy.eval_policy(spec, pol, 2, J_zero=V, dtype=dt, t_k=t_k)
        _same(_quiet(solver.eval_policy, pol, 2, J_zero=V, report_time=False), wJ, '{} {} no shift'.format(case, real))
    finally:
        _close(solver)


@pytest.mark.parametrize('real', sorted(mp.DTYPES))
def test_horizon_equals_the_oracle(gpu, real):
    """bellman_recursion of the time-dependent case, whose constants are DATA[k]: one code object, lifted parameters"""
    case = mp.BY_NAME['horizon']
    dt = mp.DTYPES[real]
    solver = case.solver(dt)
    spec = mp.flat_spec(solver)
    kw = {} if dt == np.float64 else dict(dtype=dt)
    try:
        for which in INPUTS:
            J_fin = mp.inputs(solver._shape(), dt)[which]
            J, pol = _quiet(solver.bellman_recursion, case.horizon, J_fin, report_time=False)
            assert solver.backend_info['time_specialized'] and solver.backend_info['lifted_constants'] > 0
            assert solver.backend_info['perturb_vars'] == 2
            nxt = J_fin
            for t in reversed(range(case.horizon)):
                with np.errstate(all='ignore'):
                    wJ, wpol, widx, _ = vi_numpy.value_iteration(spec, nxt, t_k=t, **kw)
                what = '{} {} step {}'.format(real, which, t)
                _same(J[t].astype(dt), wJ.astype(dt), what + ' J')
                _same(pol[t].astype(dt), wpol.astype(dt), what + ' policy')
                nxt = wJ.astype(dt)
            _same(solver.last_policy_index, widx.astype(np.int32), '{} {} index of step 0'.format(real, which))
    finally:
        _close(solver)


@pytest.mark.parametrize('real', sorted(mp.DTYPES))
@pytest.mark.parametrize('case', mp.CASES, ids=repr)
def test_tol_stops_at_the_sweep_of_the_host_rule(gpu, case, real):
    """the reduction of the convergence check is model-independent: the loop inside the library stops where the rule of
    stodynprog_amd/convergence.py, applied to the sweeps one by one, stops.  (The time-dependent case: eval_policy, the
    loop a time-dependent system has.)"""
    dt = mp.DTYPES[real]
    solver = case.solver(dt)
    n_max, tol = 8, 0.05
    V = mp.inputs(solver._shape(), dt)['smooth']
    try:
        if case.horizon:
            pol = _policy(solver, None)
            step = lambda J: _quiet(solver.eval_policy, pol, 1, J_zero=J, report_time=False)
            J_tol = _quiet(solver.eval_policy, pol, n_max, J_zero=V, report_time=False, tol=tol)
        else:
            step = lambda J: _quiet(solver.value_iteration, J, report_time=False)[0]
            J_tol, _ = _quiet(solver.value_iterations, V, n_max, report_time=False, tol=tol)
        record = solver.last_convergence
        J, met = V, False
        for k in range(1, n_max + 1):
            J_prev, J = J, step(J)
            dmin, dmax = conv.diff_stats(J, J_prev, dt)
            met = bool(conv.converged(dmin, dmax, tol))
            if met:
                break
        # (the oracle's sweeps on the CPU: one_lane meets this tolerance at sweep 4, full_wave at sweep 7, the undiscounted
        # models of the other cases never do and run all n_max sweeps -- both ends of the rule)
        if case.name in ('one_lane', 'full_wave'):
            assert met and k == {'one_lane': 4, 'full_wave': 7}[case.name], k
        assert record.n_iter == k and record.converged == met, (record, k, met)
        _same(J_tol, J, '{} {} J at the stopping sweep'.format(case, real))
    finally:
        _close(solver)


# ---------------------------------------------------------------------------------------------------------------------
# the degenerate variable: the bits of the pinned one-variable kernels

@pytest.mark.parametrize('real', sorted(mp.DTYPES))
def test_degenerate_variable_equals_the_one_variable_system(gpu, real):
    dt = mp.DTYPES[real]
    two, one = mp.BY_NAME['degenerate'].solver(dt), mp.degenerate_twin(dt)
    rng = np.random.default_rng(5)
    try:
        for which in INPUTS:
            V = mp.inputs(two._shape(), dt)[which]
            (J2, p2), (J1, p1) = (_quiet(s.value_iteration, V, report_time=False) for s in (two, one))
            assert two.backend_info['perturb_vars'] == 2 and one.backend_info['perturb_vars'] == 1
            _same(J2, J1, which + ' value_iteration J')
            _same(p2, p1, which + ' value_iteration policy')
            _same(two.last_policy_index, one.last_policy_index, which + ' index')
            pol = _policy(two, None)
            e2, e1 = (_quiet(s.eval_policy, pol, 3, rel_dp=True, J_zero=V, report_time=False, J_ref_full=True)
                      for s in (two, one))
            _same(e2[0], e1[0], which + ' eval_policy J')
            _same(e2[1], e1[1], which + ' eval_policy J_ref')
            b2, b1 = (_quiet(s.bellman_recursion, 3, V, report_time=False) for s in (two, one))
            _same(b2[0], b1[0], which + ' bellman_recursion J')
            _same(b2[1], b1[1], which + ' bellman_recursion policy')
        pol = _quiet(one.value_iteration, mp.inputs(two._shape(), dt)['smooth'], report_time=False)[1]
        x0 = tm._starts(two, 70, rng, margin=0.1)
        w1 = rng.uniform(-0.6, 0.6, (6, 70))
        w = np.stack([w1, np.full_like(w1, mp.DEGENERATE_POINT)], axis=1)           # (T, m, B)
        for a, b, name in zip(_quiet(two.simulate, pol, x0, w), _quiet(one.simulate, pol, x0, w1), 'xug'):
            _same(a, b, 'simulate ' + name)
    finally:
        _close(two)
        _close(one)


# ---------------------------------------------------------------------------------------------------------------------
# simulation and Monte Carlo

def _loop(solver, pol, x0, w):
    """the hand-written closed loop in the problem's reals, batched: the policy looked up by the reference's
    multilinear interpolation (oracle/vi_numpy.mlinterp_np), then the callables with w[k, i] for variable i"""
    dt = solver.dtype.type
    T, m, B = w.shape
    d, nu = len(solver.state_grid), len(solver.sys.control)
    smin = [g[0] for g in solver.state_grid]
    smax = [g[-1] for g in solver.state_grid]
    values = np.ascontiguousarray(np.moveaxis(pol, -1, 0).reshape(nu, -1), dtype=dt)
    x = np.zeros((T + 1, B, d), dtype=dt)
    u = np.zeros((T, B, nu), dtype=dt)
    g = np.zeros((T, B), dtype=dt)
    x[0] = x0.astype(dt)
    wd = w.astype(dt)
    with np.errstate(all='ignore'):
        for k in range(T):
            u[k] = vi_numpy.mlinterp_np(smin, smax, solver._shape(), values, x[k].T).T
            args = tuple(x[k, :, i] for i in range(d)) + tuple(u[k, :, c] for c in range(nu)) + tuple(wd[k])
            xn = solver.sys.dyn(*args)
            gk = solver.sys.cost(*args)
            assert all(np.asarray(v).dtype == dt for v in tuple(xn) + (gk,))
            for i in range(d):
                x[k + 1, :, i] = xn[i]
            g[k] = gk
    return x, u, g


@pytest.mark.parametrize('real', sorted(mp.DTYPES))
@pytest.mark.parametrize('name', ['ragged', 'wide'])
def test_simulate_equals_the_hand_written_loop(gpu, name, real):
    dt = mp.DTYPES[real]
    solver = mp.BY_NAME[name].solver(dt)
    m = len(solver.perturb_grid)
    rng = np.random.default_rng(11)
    try:
        pol = _oracle_sweeps(name, real, 'smooth', False)[0][2]
        x0 = tm._starts(solver, 70, rng, margin=0.1)
        w = rng.uniform(-1.0, 1.0, (6, m, 70))                  # (T, m, B): any values, not only the law's
        x, u, g = _quiet(solver.simulate, pol, x0, w)
        assert solver.backend_info['mode'] == 'traced'
        assert x.shape == (7, 70, len(solver.state_grid)) and u.shape == (6, 70, pol.shape[-1]) and g.shape == (6, 70)
        for got, want, what in zip((x, u, g), _loop(solver, pol, x0, w), 'xug'):
            _same(got, want, '{} {} simulate {}'.format(name, real, what))
        assert len({float(v) for v in x[-1, :, 0]}) > 60
        # one trajectory: w of shape (T, m); in 8-byte reals its controls are interp_on_state's
        x1, u1, g1 = _quiet(solver.simulate, pol, x0[3], w[:, :, 3])
        _same(x1, x[:, 3], 'one trajectory x')
        _same(g1, g[:, 3], 'one trajectory g')
        if dt == np.float64:
            laws = [solver.interp_on_state(np.ascontiguousarray(pol[..., c])) for c in range(pol.shape[-1])]
            for k in range(6):
                assert [float(law(*x1[k])) for law in laws] == [float(v) for v in u1[k]]
    finally:
        _close(solver)


@pytest.mark.parametrize('real', sorted(mp.DTYPES))
@pytest.mark.parametrize('name', ['ragged', 'wide'])
def test_monte_carlo_equals_the_replay(gpu, name, real):
    dt = mp.DTYPES[real]
    solver = mp.BY_NAME[name].solver(dt)
    m = len(solver.perturb_grid)
    rng = np.random.default_rng(13)
    B, T, n_burn = 300, 40, 5
    try:
        pol = _oracle_sweeps(name, real, 'smooth', False)[0][2]
        x0 = tm._starts(solver, B, rng, margin=0.05)
        idx, w = solver.monte_carlo_draws(9, B, T, traj_offset=17)
        wtab, P = perturb.product_law(solver.perturb_grid, solver.perturb_proba)
        assert idx.shape == (T, B) and w.shape == (T, m, B) and w.dtype == dt
        assert np.array_equal(w, np.moveaxis(wtab.astype(dt)[:, idx], 0, 1))
        assert len(np.unique(idx)) == P.size                    # every point of the flat law is drawn
        kw = dict(seed=9, n_burn=n_burn, occupancy=True, traj_offset=17)
        res = _quiet(solver.monte_carlo, pol, x0, T, **kw)
        assert res.path == 'device' and solver.backend_info['perturb_vars'] == m
        ref = tm._replay(solver, pol, x0, T, 9, n_burn, None, 17)
        tm._same(res, ref, '{} {}'.format(name, real), B * (T - n_burn))
        # the cut into launches and a split of the batch change no bit
        solver.steps_per_launch = 7
        tm._same(_quiet(solver.monte_carlo, pol, x0, T, **kw), ref, 'steps_per_launch = 7', B * (T - n_burn))
        solver.steps_per_launch = 1024
        lo = _quiet(solver.monte_carlo, pol, x0[:111], T, **kw)
        hi = _quiet(solver.monte_carlo, pol, x0[111:], T, **dict(kw, traj_offset=17 + 111))
        assert tm._eq(np.concatenate([lo.cost_sum, hi.cost_sum]), res.cost_sum)
        assert tm._eq(np.concatenate([lo.x_final, hi.x_final]), res.x_final)
        assert np.array_equal(lo.occupancy + hi.occupancy, res.occupancy)
        # a JOINT law that is no product: the points of a diagonal and one corner
        n = 4
        joint = (np.array([np.linspace(-0.5, 0.5, n) * (i + 1) for i in range(m)]), np.array([0.1, 0.2, 0.3, 0.4]))
        joint[0][:, -1] = 0.75
        res = _quiet(solver.monte_carlo, pol, x0, T, seed=3, n_burn=n_burn, law=joint, occupancy=True)
        tm._same(res, tm._replay(solver, pol, x0, T, 3, n_burn, joint, 0), 'joint law', B * (T - n_burn))
    finally:
        solver.steps_per_launch = 1024
        _close(solver)


# ---------------------------------------------------------------------------------------------------------------------
# call to call: only the second variable changes

@pytest.mark.parametrize('real', sorted(mp.DTYPES))
def test_second_variable_changes_between_calls(gpu, real):
    dt = mp.DTYPES[real]
    solver = mp.BY_NAME['ragged'].solver(dt)
    V = mp.inputs(solver._shape(), dt)['smooth']
    kw = {} if dt == np.float64 else dict(dtype=dt)

    def check(what):
        with np.errstate(all='ignore'):
            wJ, wpol, widx, _ = vi_numpy.value_iteration(mp.flat_spec(solver), V, **kw)
        J, pol = _quiet(solver.value_iteration, V, report_time=False)
        _same(J, wJ.astype(dt), what + ' J')
        _same(pol, wpol.astype(dt), what + ' policy')
        _same(solver.last_policy_index, widx.astype(np.int32), what + ' index')
        Je = _quiet(solver.eval_policy, pol, 2, J_zero=V, report_time=False)
        with np.errstate(all='ignore'):
            _same(Je, vi_numpy.eval_policy(mp.flat_spec(solver), pol, 2, J_zero=V, dtype=dt), what + ' eval_policy')
        return J

    try:
        J_a = check('first call')
        solver.perturb_grid[1] = np.array([-0.75, 0.5])                 # the second variable's grid alone
        J_b = check('second grid changed')
        solver.perturb_proba[1] = np.array([0.7, 0.3])                  # .. its law alone
        J_c = check('second law changed')
        solver.perturb_grid[1] = np.array([-0.75, 0.0, 0.5])            # .. a point more: another W, the same code object
        solver.perturb_proba[1] = np.array([0.5, 0.25, 0.25])
        J_d = check('second variable of three points')
        assert not np.array_equal(J_a, J_b) and not np.array_equal(J_b, J_c) and not np.array_equal(J_c, J_d)
    finally:
        _close(solver)


# ---------------------------------------------------------------------------------------------------------------------
# callables that cannot be traced: the same definition on the host paths

def _opaque(solver):
    """the same problem with callables the tracer refuses (they look at values): tabulated mode and the host loops"""
    s = solver.sys
    t = SysDescription((len(s.state), len(s.control), len(s.perturb)), name=s.name + ' (opaque)')
    dyn, cost = s.dyn, s.cost

    def look(v):
        np.asarray(v, dtype=float)               # (a symbol of the tracer is no number)
    if len(s.state) == 2 and len(s.perturb) == 2:
        def dyn2(a, y, u, w1, w2):
            look(a)
            return dyn(a, y, u, w1, w2)

        def cost2(a, y, u, w1, w2):
            look(a)
            return cost(a, y, u, w1, w2)
    else:
        raise NotImplementedError
    t.dyn, t.cost, t.control_box = dyn2, cost2, s.control_box
    out = DPSolver(t, dtype=solver.dtype)
    out.state_grid, out.perturb_grid, out.perturb_proba = solver.state_grid, solver.perturb_grid, solver.perturb_proba
    out._state_grid_shape, out._state_ref_ind = solver._state_grid_shape, solver._state_ref_ind
    out.control_steps = solver.control_steps
    return out


def test_untraceable_model_runs_the_same_definition(gpu):
    ref = mp.BY_NAME['ragged'].solver()
    solver = _opaque(ref)
    assert isinstance(solver._trace_now(None), TraceError)
    spec = mp.flat_spec(ref)
    rng = np.random.default_rng(17)
    for which in ('smooth', 'random'):
        V = mp.inputs(ref._shape(), np.float64)[which]
        wJ, _, wpol, widx = _oracle_sweeps('ragged', 'f64', which, False)[0]
        J, pol = _quiet(solver.value_iteration, V, report_time=False)
        assert solver.backend_info['mode'] == 'tabulated'
        _same(J, wJ, which + ' tabulated J')
        _same(pol, wpol, which + ' tabulated policy')
        _same(solver.last_policy_index, widx.astype(np.int32), which + ' tabulated index')
        with np.errstate(all='ignore'):
            wJe, wrefs = vi_numpy.eval_policy(spec, wpol, 3, rel_dp=True, J_zero=V, J_ref_full=True)
        Je, refs = _quiet(solver.eval_policy, wpol, 3, rel_dp=True, J_zero=V, report_time=False, J_ref_full=True)
        _same(Je, wJe, which + ' tabulated eval_policy')
        _same(refs, wrefs, which + ' tabulated J_ref')
    # one state point (the reference's _value_at_state_vect) on the flat law
    interp = solver.interp_on_state(V)
    x_k = (ref.state_grid[0][2], ref.state_grid[1][4])
    Jx, ux = solver._value_at_state_vect(x_k, interp)
    assert Jx == wJ[2, 4] and list(ux) == list(wpol[2, 4])
    # the host loops of simulate and monte_carlo: what the device computes for the traceable twin
    pol = wpol
    x0 = tm._starts(ref, 20, rng)
    w = rng.uniform(-1., 1., (5, 2, 20))
    try:
        for a, b, what in zip(_quiet(solver.simulate, pol, x0, w), _quiet(ref.simulate, pol, x0, w), 'xug'):
            _same(a, b, 'host simulate ' + what)
        kw = dict(seed=4, n_burn=2, occupancy=True, traj_offset=5)
        host, dev = _quiet(solver.monte_carlo, pol, x0, 12, **kw), _quiet(ref.monte_carlo, pol, x0, 12, **kw)
        assert host.path == 'host' and dev.path == 'device'
        assert tm._eq(host.cost_sum, dev.cost_sum) and tm._eq(host.x_final, dev.x_final)
        assert np.array_equal(host.n_outside, dev.n_outside) and np.array_equal(host.occupancy, dev.occupancy)
    finally:
        _close(ref)


def test_a_sweep_past_the_grid_cap(gpu):
    """`full_wave` (64 lanes, 4 nodes a workgroup) on cus * 8 * 4 + 129 nodes: sweep_blocks caps the grid at cus * 8
    workgroups, XCD x walks the x-th eighth of the tiles with a stride of cus, so seven XCDs walk twice.  The nodes of
    the later trips, the last 129 and a sample against the oracle on the flat law"""
    import lookahead_cases as lc                 # (the walk of sdp_lookahead is this kernel's: lookahead_later_trips)
    cus = gpu.device_info(0)['compute_units']
    n_x = cus * 8 * 4 + 129
    tiles, blocks = lc.lookahead_grid(n_x, 64, cus)
    later = lc.lookahead_later_trips(n_x, 64, cus)
    assert tiles > blocks == cus * 8 and len(later) >= 7 * 4, (tiles, blocks)
    solver = mp._full_wave(np.float64, n_x)
    V = np.random.default_rng(21).standard_normal(n_x)
    nodes = np.unique(np.concatenate([later, np.arange(n_x - 129, n_x), np.random.default_rng(22).choice(n_x, 300, replace=False)]))
    try:
        J, pol = _quiet(solver.value_iteration, V, report_time=False)
        info = solver.backend_info
        assert info['kernel'] == 'generic' and info['perturb_vars'] == 2 and info['lanes_per_node'] == 64
        with np.errstate(all='ignore'):
            Jo, polo, idxo, _ = vi_numpy.value_iteration(mp.flat_spec(solver), V, nodes=nodes)
        _same(J[nodes], Jo, 'J')
        _same(pol[nodes], polo, 'policy values')
        _same(solver.last_policy_index[nodes], idxo.astype(np.int32), 'policy index')
        assert len(np.unique(idxo)) > 8
    finally:
        _close(solver)
