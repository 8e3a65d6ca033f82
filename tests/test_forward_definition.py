"""stodynprog_amd/forward.py, the definition of the transition operator of a policy, against an independent
construction: the pinned oracle's eval_policy (oracle/vi_numpy.py), which knows nothing of entries or transposes.
No GPU.

Dense P, column by column: eval_policy is affine in the cost-to-go, J -> P J + gbar, so column t of P is
eval_policy(pol, 1, J_zero = e_t) - gbar with gbar = eval_policy(pol, 1) from zeros.  Grids of at most 100 nodes,
d = 1..4, in 8-byte reals (the reference's own path) and 4-byte reals (eval_policy_real).  The difference of two
evaluations carries the rounding of the costs it cancels, about u |g| per entry of P whatever the entry's size, which
is the reference's error and not the push's; the costs of these four models are therefore scaled by 2^-100 (a power of
two: the same roundings as unscaled, no subnormals), far below the smallest weight, so that the difference returns the
weights themselves.  The linear part does not depend on the cost; costs of order 1 are compared with the oracle in
the storage test below and, on the device, in tests/test_gpu_forward.py.

The stationary iteration is checked against the oracle's relative-DP evaluation of the same policy through the
identity, for ANY h,
    mu . g = mu . d - (P^T mu - mu) . h,        d = g + P h - h  in [lo, hi]  (the Odoni bounds of h),
so that for mu >= 0 of mass m and |P^T mu - mu| <= delta entrywise
    m lo - S delta max|h| - r <= mu . gbar <= m hi + S delta max|h| + r,        r = 8 S eps max|gbar|  (rounding)."""
import itertools
import math

import numpy as np
import pytest

from oracle import vi_numpy
from stodynprog_amd import SysDescription, DPSolver, forward, models

import forward_cases as fc


def _finish(s, state, law, steps):
    solver = DPSolver(s)
    solver.discretize_state(*state)
    solver.perturb_grid = [np.array(law[0], dtype=float)]
    solver.perturb_proba = [np.array(law[1], dtype=float)]
    solver.control_steps = tuple(steps)
    return solver


COST_SCALE = 2.0 ** -100
LAW_3 = ([-0.25, 0.0, 0.5], [0.25, 0.5, 0.25])
LAW_4 = ([-0.5, -0.125, 0.25, 0.5], [0.125, 0.375, 0.25, 0.25])


def _grid_1d():
    s = SysDescription((1, 1, 1), name='d1')
    s.dyn = lambda x, u, w: ((0.75 * x + u) + w,)                     # leaves [0, 3] at both ends
    s.cost = lambda x, u, w: ((x - 1.0) * (x - 1.0) + 0.5 * u * w) * COST_SCALE
    s.control_box = lambda x: ((-0.5, 0.5),)
    return _finish(s, (0, 3, 7), LAW_4, (0.25,)), [(-0.5, 0.5)]


def _grid_2d():
    s = SysDescription((2, 1, 1), name='d2')
    s.dyn = lambda x, y, u, w: ((0.5 * x + u) + 0.25 * w, 0.7 * y + w)
    s.cost = lambda x, y, u, w: ((x * y + u * u) + abs(w - x)) * COST_SCALE
    s.control_box = lambda x, y: ((0., 1.),)
    return _finish(s, (0, 2, 5, -1, 1, 4), LAW_3, (0.25,)), [(0., 1.)]


def _grid_3d():
    s = SysDescription((3, 2, 1), name='d3')
    s.dyn = lambda a, b, c, u, v, w: ((0.6 * a + u) + 0.5 * w, (0.5 * b + 0.25 * v) + 0.1 * a, 0.8 * c - 0.5 * w)
    s.cost = lambda a, b, c, u, v, w: (((a - u) * (a - u) + v * v) + (b * c) * w) * COST_SCALE
    s.control_box = lambda a, b, c: ((0., 1.), (-1., 1.))
    return _finish(s, (0, 2, 4, 0, 1, 3, -1, 1, 3), LAW_3, (0.5, 0.5)), [(0., 1.), (-1., 1.)]


def _grid_4d():
    s = SysDescription((4, 1, 1), name='d4')
    s.dyn = lambda a, b, c, e, u, w: ((0.5 * a + 0.5 * u) + 0.25 * w, 0.5 * b + 0.25 * a, (0.5 * c + 0.5 * w) + 0.125 * e,
                                     0.75 * e - 0.25 * u)
    s.cost = lambda a, b, c, e, u, w: (((a - 0.5) * (a - 0.5) + u * u) + (b * c + e * w)) * COST_SCALE
    s.control_box = lambda a, b, c, e: ((0., 1.),)
    return _finish(s, (0, 1, 3, 0, 1, 3, -1, 1, 2, 0, 2, 2), LAW_3, (0.5,)), [(0., 1.)]


GRIDS = {'1-D 7': _grid_1d, '2-D 5x4': _grid_2d, '3-D 4x3x3': _grid_3d, '4-D 3x3x2x2': _grid_4d}
_memo = {}


def built(name, dtkey):
    """solver, policy, entries, CSR, gbar and dense P of the oracle: once per (grid, reals), then read-only"""
    key = (name, dtkey)
    if key not in _memo:
        dt = fc.DTYPES[dtkey]
        s64, bounds = GRIDS[name]()
        s = fc.as_dtype(s64, dt)
        pol = fc.wave_policy(s, bounds).astype(dt)
        spec = vi_numpy.Spec.from_solver(s)
        kw = {} if dt == np.float64 else dict(dtype=dt)         # (8-byte reals: the reference's own path)
        gbar = vi_numpy.eval_policy(spec, pol, 1, **kw)
        S = gbar.size
        P = np.empty((S, S), dtype=dt)
        for t in range(S):
            e_t = np.zeros(S, dtype=dt)
            e_t[t] = 1
            P[:, t] = (vi_numpy.eval_policy(spec, pol, 1, J_zero=e_t.reshape(gbar.shape), **kw) - gbar).ravel()
        e = forward.entries(s, pol)
        csr = forward.csr(e.S, e.tgt, e.src, e.val)
        _memo[key] = (s, pol, e, csr, gbar, P)
        for a in (pol, gbar, P, e.tgt, e.src, e.val, e.mean_cost) + csr:
            a.setflags(write=False)
    return _memo[key]


CASES = list(itertools.product(sorted(GRIDS), sorted(fc.DTYPES)))


@pytest.mark.parametrize('name,dtkey', CASES)
def test_entry_count_order_and_types(name, dtkey):
    s, pol, e, csr, gbar, P = built(name, dtkey)
    dt = np.dtype(fc.DTYPES[dtkey])
    d = len(s.state_grid)
    S, W = gbar.size, len(s.perturb_grid[0])
    assert S <= 100 and e.S == S and e.W == W and e.V == 2 ** d
    assert e.tgt.size == e.src.size == e.val.size == S * W * 2 ** d
    assert e.tgt.dtype == np.int32 and e.src.dtype == np.int32 and e.val.dtype == dt and e.mean_cost.dtype == dt
    assert np.array_equal(e.src, np.repeat(np.arange(S), W * 2 ** d))             # emission order: s slowest
    assert e.tgt.min() >= 0 and e.tgt.max() < S
    indptr, indices, data = csr
    assert indptr.dtype == np.int64 and indices.dtype == np.int32 and data.dtype == dt
    assert indptr[0] == 0 and indptr[-1] == e.val.size and (np.diff(indptr) >= 0).all()
    for t in range(S):                                                            # stable: a row keeps the emission order
        pos = np.flatnonzero(e.tgt == t)
        assert np.array_equal(indices[indptr[t]:indptr[t + 1]], e.src[pos])
        assert np.array_equal(data[indptr[t]:indptr[t + 1]], e.val[pos])


@pytest.mark.parametrize('name,dtkey', CASES)
def test_weights_of_every_source_sum_to_one(name, dtkey):
    s, pol, e, csr, gbar, P = built(name, dtkey)
    ulp = np.finfo(fc.DTYPES[dtkey]).eps
    sums = np.array([math.fsum(row) for row in e.val.astype(float).reshape(e.S, -1)])
    print(name, dtkey, 'max |sum - 1| =', np.abs(sums - 1).max(), 'allowed', e.V * e.W * ulp)
    assert np.abs(sums - 1).max() <= e.V * e.W * ulp


@pytest.mark.parametrize('name,dtkey', CASES)
def test_mean_cost_is_the_oracles_one_step_evaluation(name, dtkey):
    s, pol, e, csr, gbar, P = built(name, dtkey)
    assert fc.same(e.mean_cost.reshape(gbar.shape), gbar)


@pytest.mark.parametrize('name,dtkey', CASES)
def test_push_is_the_transpose_of_the_oracles_operator(name, dtkey):
    """|push(mu) - P^T mu| <= gamma_n sum |val| |mu| per target, n the longest row, gamma_n = n u / (1 - n u)"""
    s, pol, e, csr, gbar, P = built(name, dtkey)
    dt = fc.DTYPES[dtkey]
    u = np.finfo(dt).eps / 2
    n = int(np.diff(csr[0]).max())
    gamma = n * u / (1 - n * u)
    absP = np.zeros((e.S, e.S))
    np.add.at(absP, (e.src, e.tgt), np.abs(e.val.astype(float)))
    for vec, mu in fc.vectors(e.S, dt).items():
        if vec == 'non-finite':
            continue
        got = forward.push(csr, mu).astype(float)
        want = P.astype(float).T @ mu.astype(float)
        bound = gamma * (absP.T @ np.abs(mu.astype(float)))
        worst = (np.abs(got - want) - bound).max()
        print(name, dtkey, vec, 'max |push - P^T mu| =', np.abs(got - want).max(), 'smallest slack', -worst)
        assert (np.abs(got - want) <= bound).all(), (name, dtkey, vec)


@pytest.mark.parametrize('name,dtkey', CASES)
def test_csr_sum_is_add_at_in_emission_order(name, dtkey):
    s, pol, e, csr, gbar, P = built(name, dtkey)
    dt = fc.DTYPES[dtkey]
    for vec, mu in fc.vectors(e.S, dt).items():
        want = np.zeros(e.S, dtype=dt)
        with np.errstate(all='ignore'):
            np.add.at(want, e.tgt, e.val * mu[e.src])
        assert fc.same(forward.push(csr, mu), want), vec
        assert fc.same(forward.push_row_by_row(csr, mu), want), vec
    mu = fc.vectors(e.S, dt)['random']
    assert fc.same(forward.push(csr, mu, 3), forward.push(csr, forward.push(csr, forward.push(csr, mu))))
    assert fc.same(forward.push(csr, mu.reshape(s._state_grid_shape)).ravel(), forward.push(csr, mu))


def test_nan_next_state_gives_cell_zero_and_nan_weights():
    q, lam, oml = forward.locate(np.linspace(0., 1., 5), np.array([np.nan, 7.0, -3.0, 0.5, 1e300, -np.inf]))
    assert q.tolist() == [0, 3, 0, 2, 0, 0]                       # (out of the int range: INT_MIN, clamped to 0)
    assert np.isnan(lam[0]) and np.isnan(oml[0])
    assert lam[1] == 28.0 - 3 and oml[1] == 1 - 25.0 and lam[2] == -12.0      # lam is not clamped
    case = fc.BY_NAME['nan_state']
    s = case.solver()
    e = forward.entries(s, case.policy(s))
    bad = np.isnan(e.val)
    assert bad.any() and (e.tgt[bad] <= 1).all() and np.isnan(e.mean_cost[:2]).all() and not np.isnan(e.mean_cost[2:]).any()
    out = forward.push(forward.csr(e.S, e.tgt, e.src, e.val), forward.uniform(e.S, np.float64))
    assert np.isnan(out[:2]).all()


def test_deterministic_system_is_one_point_of_weight_one():
    case = fc.BY_NAME['deterministic']
    s = case.solver()
    pol = case.policy(s)
    e = forward.entries(s, pol)
    assert (e.W, e.V) == (1, 4) and e.val.size == e.S * 4
    x, y = s.state_grid_full
    assert fc.same(e.mean_cost.reshape(x.shape), s.sys.cost(x, y, pol[..., 0]) * 1.0 + 0.0)


def test_stationary_arguments_and_stopping_rule():
    indptr, indices, data = forward.csr(2, [1, 0], [0, 1], np.array([1.0, 1.0]))        # a swap: period 2
    rec = forward.stationary((indptr, indices, data), None, mu0=np.array([1.0, 0.0]), tol=1e-12, n_max=9, check_every=2)
    assert (rec.n_done, rec.converged, rec.delta) == (9, False, 1.0) and rec.mu.tolist() == [0.0, 1.0]
    rec = forward.stationary((indptr, indices, data), np.array([2.0, 4.0]), tol=0.0, n_max=50, check_every=5)
    assert (rec.n_done, rec.converged, rec.delta, rec.average_cost, rec.mass) == (5, True, 0.0, 3.0, 1.0)
    nan = forward.stationary((indptr, indices, data), None, mu0=np.array([np.nan, 0.0]), tol=1.0, n_max=3, check_every=1)
    assert nan.n_done == 3 and not nan.converged and math.isnan(nan.delta)
    for bad in (dict(tol=-1.0), dict(tol=float('nan')), dict(check_every=0), dict(n_max=0)):
        with pytest.raises(ValueError):
            forward.stationary((indptr, indices, data), None, **bad)
    with pytest.raises(ValueError):
        forward.csr(2, [0, 2], [0, 1], np.ones(2))
    with pytest.raises(ValueError):
        forward.csr(2, [0, 1], [0, -1], np.ones(2))


@pytest.fixture(scope='module')
def storage():
    """storage + AR(1) on 13 x 9 nodes with 5 perturbation points, the AR(1) axis widened to [-9, 9] so that the
    chain stays on the grid (0.8 * 9 + 4 * 0.447 < 9); the policy of 60 relative-DP sweeps of the oracle"""
    _, solver = models.storage_ar1(n_E=13, n_P=9, n_w=5, steps=(0.25, 0.1))
    solver.discretize_state(0, 10., 13, -9., 9., 9)
    spec = vi_numpy.Spec.from_solver(solver)
    J = (np.zeros(spec.shape), 0.0)
    for _ in range(60):
        J, pol, _, _ = vi_numpy.value_iteration(spec, J, rel_dp=True)
    return solver, spec, pol


def test_stationary_average_cost_lies_in_the_odoni_bounds(storage):
    solver, spec, pol = storage
    e = forward.entries(solver, pol)
    csr = forward.csr(e.S, e.tgt, e.src, e.val)
    assert csr[2].min() >= 0
    assert fc.same(e.mean_cost.reshape(spec.shape), vi_numpy.eval_policy(spec, pol, 1))       # costs of order 1
    rec = forward.stationary(csr, e.mean_cost, tol=1e-13, n_max=5000, check_every=10)
    assert rec.converged and rec.mu.min() >= 0
    h, _ = vi_numpy.eval_policy(spec, pol, 300, rel_dp=True)
    d = vi_numpy.eval_policy(spec, pol, 1, J_zero=h) - h
    lo, hi = float(d.min()), float(d.max())
    S, eps = e.S, np.finfo(float).eps
    m, hmax = float(rec.mass), float(np.abs(h).max())
    r = 8 * S * eps * float(np.abs(e.mean_cost).max())
    slack = S * rec.delta * hmax + r
    print('pushes', rec.n_done, 'delta', rec.delta, 'mass - 1', m - 1, 'average cost', rec.average_cost, 'bounds', lo, hi,
          'slack', slack)
    assert m * lo - slack <= rec.average_cost <= m * hi + slack
    assert hi - lo < 1e-9                                     # (the evaluation has converged: the bounds bind)
