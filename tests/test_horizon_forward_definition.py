"""`forward.chain_entries` and `forward.propagate` (the definition of DPSolver.horizon_operator) in numpy alone: the
chain against a hand-written loop of `push_row_by_row`, bit for bit; the identity <mu_0, J_0> = sum_k <mu_k, gbar_k> +
<mu_T, J_fin> in exact rational arithmetic on a model that leaves the grid; the shapes of the record.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest

import forward_cases as fc
import horizon_forward_cases as hfc
from stodynprog_amd import SysDescription, DPSolver, forward


def _chain(row, dtype, T=None):
    s = row.solver(dtype)
    pol = row.policy(s)
    T = row.T if T is None else T
    es = forward.chain_entries(s, pol, T, 0, row.time_index)
    return s, pol, es, [forward.csr(e.S, e.tgt, e.src, e.val) for e in es], [e.mean_cost for e in es]


@pytest.mark.parametrize('dtkey', sorted(hfc.DTYPES))
@pytest.mark.parametrize('name', ['line', 'storage', 'two_variables', 'deterministic'])
def test_propagate_is_the_loop_of_row_by_row_pushes(name, dtkey):
    dt = hfc.DTYPES[dtkey]
    s, pol, es, ops, gbar = _chain(hfc.BY_NAME[name], dt, T=3)
    S = es[0].S
    dims = tuple(len(g) for g in s.state_grid)
    vec = fc.vectors(S, dt)
    batch = np.stack([vec['uniform'], vec['random'], vec['delta']]).reshape((3,) + dims)
    for mu0 in (vec['random'].reshape(dims), batch):
        res = forward.propagate(ops, gbar, mu0)
        assert res.mu.shape == (4,) + mu0.shape and res.mu.dtype == np.dtype(dt)
        assert res.step_cost.shape == (3,) + mu0.shape[:mu0.ndim - len(dims)] and res.step_cost.dtype == np.float64
        assert res.mass.shape == (4,) + mu0.shape[:mu0.ndim - len(dims)] and res.mass.dtype == np.dtype(dt)
        vectors = mu0.reshape(-1, S)
        for b, start in enumerate(vectors):
            cur = start
            for k in range(3):
                assert np.array_equal(res.mu.reshape(4, -1, S)[k, b], cur)
                cur = forward.push_row_by_row(ops[k], cur)
            assert np.array_equal(res.mu.reshape(4, -1, S)[3, b], cur)
        assert np.array_equal(res.total_cost, res.step_cost.sum(axis=0) + res.terminal_cost)
        assert np.array_equal(res.mass, res.mu.reshape(res.mass.shape + (-1,)).sum(axis=-1))
        assert np.all(res.terminal_cost == 0)
    J_fin = np.linspace(-1., 2., S).reshape(dims)
    with_fin = forward.propagate(ops, gbar, batch, J_fin)
    assert np.array_equal(with_fin.mu, forward.propagate(ops, gbar, batch).mu)
    assert np.allclose(with_fin.terminal_cost, with_fin.mu[3].reshape(3, S).astype(float) @ J_fin.ravel(), rtol=1e-12, atol=0)


def test_chain_entries_are_the_entries_of_every_step():
    """step k is `entries(solver, pol[t0 + k], t0 + k)`, a stationary policy the same array at every step: nothing about one
    step is defined again"""
    row = hfc.BY_NAME['storage']
    s = row.solver()
    pol = row.policy(s)
    for t0, n in ((0, row.T), (2, 3)):
        for k, e in enumerate(forward.chain_entries(s, pol, n, t0)):
            one = forward.entries(s, pol[t0 + k], t0 + k)
            assert all(fc.same(a, b) for a, b in zip(e[:4], one[:4])) and e[4:] == one[4:]
    for k, e in enumerate(forward.chain_entries(s, pol[1], 4, 3)):
        one = forward.entries(s, pol[1], 3 + k)
        assert all(fc.same(a, b) for a, b in zip(e[:4], one[:4]))
    with pytest.raises(ValueError) as err:
        forward.chain_entries(s, pol, 3, row.T - 2)
    assert str(pol.shape) in str(err.value)


def _seven_nodes():
    """7 nodes, W = 3, an expanding map that depends on the time index: next states outside the grid on both sides"""
    sysd = SysDescription((1, 1, 1), stationnary=False, name='seven nodes')
    sysd.dyn = lambda k, x, u, w: ((1.75 * x + u) + w * (1 + k),)
    sysd.cost = lambda k, x, u, w: (x - 0.25 * k) * (x - 0.25 * k) + u * w
    sysd.control_box = lambda k, x: ((-1., 1.),)
    s = DPSolver(sysd)
    s.discretize_state(-1, 1, 7)
    s.perturb_grid = [np.array([-0.5, 0.0, 0.75])]
    s.perturb_proba = [np.array([0.3, 0.5, 0.2])]
    s.control_steps = (0.5,)
    return s


def test_the_identity_holds_in_exact_rational_arithmetic():
    """<mu_0, J_0> = sum_k <mu_k, gbar_k> + <mu_T, J_fin> with the float entries taken as rationals: EQUAL, not close --
    the targets, sources and blocks of the chain are those of the backward pass"""
    s = _seven_nodes()
    T, S = 3, 7
    pol = np.stack([fc.wave_policy(s, [(-1., 1.)], seed=k) for k in range(T)])
    es = forward.chain_entries(s, pol, T)
    assert all(e.S == S and e.W == 3 and e.V == 2 and e.val.size == S * 6 for e in es)
    assert min(e.val.min() for e in es) < 0 and max(e.val.max() for e in es) > 1       # the model leaves the grid
    frac = lambda a: [Fraction(float(x)) for x in a]
    J_fin = frac(np.linspace(0.5, -1.25, S))
    mu0 = frac(np.random.default_rng(3).random(S))
    # backward: J_k = gbar_k + P_k J_{k+1}
    J = J_fin
    for e in reversed(es):
        new = frac(e.mean_cost)
        for t, src, v in zip(e.tgt.tolist(), e.src.tolist(), frac(e.val)):
            new[src] += v * J[t]
        J = new
    left = sum(m * j for m, j in zip(mu0, J))
    # forward: mu_{k+1} = P_k^T mu_k
    mu, right = mu0, Fraction(0)
    for e in es:
        right += sum(m * g for m, g in zip(mu, frac(e.mean_cost)))
        new = [Fraction(0)] * S
        for t, src, v in zip(e.tgt.tolist(), e.src.tolist(), frac(e.val)):
            new[t] += v * mu[src]
        mu = new
    right += sum(m * j for m, j in zip(mu, J_fin))
    assert left == right
    # .. and the float chain agrees with it to rounding
    ops = [forward.csr(e.S, e.tgt, e.src, e.val) for e in es]
    res = forward.propagate(ops, [e.mean_cost for e in es], np.array([float(m) for m in mu0]),
                            np.array([float(j) for j in J_fin]))
    assert abs(res.total_cost - float(left)) <= 1e-12 * max(1.0, abs(float(left)))


def test_propagate_refuses_what_is_no_chain():
    s, pol, es, ops, gbar = _chain(hfc.BY_NAME['line'], np.float64, T=2)
    with pytest.raises(ValueError):
        forward.propagate([], [], np.zeros(es[0].S))
    with pytest.raises(ValueError):
        forward.propagate(ops, gbar[:1], np.zeros(es[0].S))
    with pytest.raises(ValueError) as err:
        forward.propagate(ops, gbar, np.zeros(es[0].S + 1))
    assert str((es[0].S + 1,)) in str(err.value) and str(es[0].S) in str(err.value)
