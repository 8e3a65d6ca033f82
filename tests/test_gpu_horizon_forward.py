"""DPSolver.horizon_operator and DPSolver.propagate on the GPU against the definition (stodynprog_amd/forward.py:
chain_entries, csr, propagate), bit for bit, on the rows of tests/horizon_forward_cases.py: the CSR and the mean cost of
every step, every vector alone and all as one batch, the chain of the existing solo operators, windows of a policy,
forced parts, non-finite policies, grids past the launch caps, and the one-call form."""
import numpy as np
import pytest

import forward_cases as fc
import horizon_forward_cases as hfc
from stodynprog_amd import HorizonOperator, forward, _native as nat

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gpu():
    nat.require_gpu()


_cache = {}


def _inventory_policy(s):
    """4 steps of bellman_recursion on the stationary shop"""
    _, pol = s.bellman_recursion(4, np.zeros(tuple(len(g) for g in s.state_grid)), report_time=False)
    return np.asarray(pol)


def _setup(name, dtkey):
    """(row, solver, policy, definition: Entries and CSR of every step), made once per row and real"""
    key = (name, dtkey)
    if key not in _cache:
        row = hfc.BY_NAME[name]
        s = row.solver(hfc.DTYPES[dtkey])
        pol = _inventory_policy(s) if name == 'inventory' else row.policy(s)
        assert pol.shape[0] == row.T
        es = forward.chain_entries(s, pol, row.T, 0, row.time_index)
        _cache[key] = (row, s, pol, es, [forward.csr(e.S, e.tgt, e.src, e.val) for e in es])
    return _cache[key]


def _dims(s):
    return tuple(len(g) for g in s.state_grid)


def _batch(S, dt, dims):
    vec = fc.vectors(S, dt)
    return vec, np.stack([vec[k] for k in sorted(vec)]).reshape((len(vec),) + dims)


@pytest.mark.parametrize('dtkey', sorted(hfc.DTYPES))
@pytest.mark.parametrize('name', [r.name for r in hfc.ROWS])
def test_the_operator_is_the_definition(gpu, name, dtkey):
    row, s, pol, es, ops = _setup(name, dtkey)
    dims, dt = _dims(s), np.dtype(hfc.DTYPES[dtkey])
    op = s.horizon_operator(pol)
    try:
        assert op.path == ('host' if row.host else 'device') == s.backend_info['horizon_operator']['path']
        assert (op.n_steps, op.shape, op.nnz) == (row.T, dims, sum(e.val.size for e in es))
        info = s.backend_info['horizon_operator']
        assert info['n_steps'] == row.T and info['nnz'] == op.nnz and info['parts'] == (row.T if row.host else 1)
        assert info['bytes'] == row.T * forward.operator_bytes(es[0].val.size, es[0].S, dt.itemsize)
        assert info['entries_ms'] >= 0 and info['sort_ms'] > 0 and 'push_ms' not in info
        assert op.mean_cost.shape == (row.T,) + dims and op.mean_cost.dtype == dt
        for k in range(row.T):
            got = op.tocsr(k)
            assert all(fc.same(a, b) for a, b in zip(got, ops[k])), (name, k)
            assert fc.same(op.mean_cost[k].ravel(), es[k].mean_cost), (name, k)
        gbar = [e.mean_cost for e in es]
        vec, batch = _batch(es[0].S, dt, dims)
        J_fin = np.linspace(-1., 1., es[0].S).reshape(dims)
        want = forward.propagate(ops, gbar, batch, J_fin)
        got = op.propagate(batch, J_fin)
        assert s.backend_info['horizon_operator']['push_ms'] > 0
        assert fc.same(got.mu, want.mu) and got.mu.shape == (row.T + 1, len(vec)) + dims
        assert fc.same(got.mass, want.mass) and got.step_cost.shape == (row.T, len(vec))
        for a, b in ((got.step_cost, want.step_cost), (got.terminal_cost, want.terminal_cost), (got.total_cost, want.total_cost)):
            assert np.allclose(a, b, rtol=1e-12, atol=0, equal_nan=True)
        for i, key in enumerate(sorted(vec)):
            alone = op.propagate(vec[key].reshape(dims))
            assert alone.mu.shape == (row.T + 1,) + dims and fc.same(alone.mu, want.mu[:, i]), (name, key)
            assert alone.step_cost.shape == (row.T,) and np.all(alone.terminal_cost == 0)
    finally:
        op.close()
    with pytest.raises(ValueError):
        op.propagate(batch)


@pytest.mark.parametrize('dtkey', sorted(hfc.DTYPES))
@pytest.mark.parametrize('name', ['storage_ragged', 'storage_data', 'deterministic'])
def test_the_chain_of_solo_operators_gives_the_same(gpu, name, dtkey):
    row, s, pol, es, ops = _setup(name, dtkey)
    dims = _dims(s)
    mu0 = fc.vectors(es[0].S, s.dtype)['random'].reshape(dims)
    op = s.horizon_operator(pol)
    try:
        res = op.propagate(mu0)
        mu = mu0
        for k in range(row.T):
            solo = s.transition_operator(pol[k], t_k=k)
            try:
                assert all(np.array_equal(a, b) for a, b in zip(op.tocsr(k), solo.tocsr())), (name, k)
                assert np.array_equal(op.mean_cost[k], solo.mean_cost)
                assert np.array_equal(res.mu[k], mu)
                mu = solo.push(mu, 1)
            finally:
                solo.close()
        assert np.array_equal(res.mu[row.T], mu)
    finally:
        op.close()


@pytest.mark.parametrize('dtkey', sorted(hfc.DTYPES))
@pytest.mark.parametrize('name', ['line', 'storage'])
def test_a_window_of_the_policy(gpu, name, dtkey):
    row, s, pol, es, ops = _setup(name, dtkey)
    dims = _dims(s)
    assert row.T == 8
    mu0 = fc.vectors(es[0].S, s.dtype)['uniform'].reshape(dims)
    full = s.propagate(pol, mu0)
    win = s.horizon_operator(pol, n_steps=3, t0=2)
    try:
        assert win.n_steps == 3
        for k in range(3):
            assert all(np.array_equal(a, b) for a, b in zip(win.tocsr(k), ops[2 + k]))
        assert np.array_equal(win.propagate(full.mu[2]).mu, full.mu[2:6])
    finally:
        win.close()
    # a stationary policy over four steps of the model's own time: the definition
    es4 = forward.chain_entries(s, pol[5], 4, 1, row.time_index)
    ops4 = [forward.csr(e.S, e.tgt, e.src, e.val) for e in es4]
    got = s.propagate(pol[5], mu0, n_steps=4, t0=1)
    assert np.array_equal(got.mu, forward.propagate(ops4, [e.mean_cost for e in es4], mu0).mu)


@pytest.mark.parametrize('name, dtkey', [('storage', 'f64'), ('storage', 'f32'), ('storage_data', 'f64'), ('untraceable', 'f64')])
def test_no_cut_changes_a_bit(gpu, name, dtkey, monkeypatch):
    row, s, pol, es, ops = _setup(name, dtkey)
    dims = _dims(s)
    vec, batch = _batch(es[0].S, s.dtype, dims)
    whole = s.propagate(pol, batch)
    if row.T == 8:
        for n, runs in ((1, [1] * 8), (2, [2] * 4), (3, [3, 3, 2])):
            monkeypatch.setattr(HorizonOperator, 'part_steps', n)
            op = s.horizon_operator(pol)
            try:
                if not row.host:
                    assert [c for _, c in op.parts] == runs and s.backend_info['horizon_operator']['parts'] == len(runs)
                cut = op.propagate(batch)
                assert fc.same(cut.mu, whole.mu) and fc.same(op.mean_cost.ravel(), np.concatenate([e.mean_cost for e in es]))
                for k in (0, 3, 7):
                    assert all(fc.same(a, b) for a, b in zip(op.tocsr(k), ops[k]))
            finally:
                op.close()
        monkeypatch.setattr(HorizonOperator, 'part_steps', None)
    # the user's own cut: the first half, then the rest from its last distribution
    h = row.T // 2
    first = s.propagate(pol, batch, n_steps=h)
    second = s.propagate(pol, first.mu[-1], t0=h)
    assert fc.same(first.mu, whole.mu[:h + 1]) and fc.same(second.mu, whole.mu[h:])


@pytest.mark.parametrize('dtkey', sorted(hfc.DTYPES))
def test_a_policy_with_a_nan_and_an_infinite_entry(gpu, dtkey):
    row, s, pol, _, _ = _setup('storage', dtkey)
    dims = _dims(s)
    pol = pol.copy()
    pol[1][2, 3, 0], pol[4][5, 1, 0] = np.nan, np.inf
    es = forward.chain_entries(s, pol, row.T, 0, row.time_index)
    ops = [forward.csr(e.S, e.tgt, e.src, e.val) for e in es]
    node = 2 * dims[1] + 3
    assert np.isnan(es[1].val[es[1].src == node]).all() and (es[1].tgt[es[1].src == node] // dims[1] <= 1).all()   # cell 0 of axis 0
    mu0 = fc.vectors(es[0].S, s.dtype)['uniform'].reshape(dims)
    op = s.horizon_operator(pol)
    try:
        for k in range(row.T):
            assert all(fc.same(a, b) for a, b in zip(op.tocsr(k), ops[k])), k
            assert fc.same(op.mean_cost[k].ravel(), es[k].mean_cost)
        got = op.propagate(mu0)
    finally:
        op.close()
    assert np.isnan(got.mu[2]).any() and fc.same(got.mu, forward.propagate(ops, [e.mean_cost for e in es], mu0).mu)


def test_past_the_launch_caps(gpu):
    """two steps of the line model on a grid that takes the build's workgroups on a second trip through their (step, tile)
    units and, with two vectors, every push launch that meets all rows on a second trip through its rows"""
    cus = nat.device_info(0)['compute_units']
    B, T = 2, 2
    row = hfc.long_line(cus, B)
    s = row.solver()
    S = hfc.long_line_nodes(cus, B)
    assert hfc.units(T, S, 1) > hfc.build_blocks(T, S, 1, cus) == cus * hfc.BUILD_PER_CU
    pol = row.policy(s)
    es = forward.chain_entries(s, pol, T)
    ops = [forward.csr(e.S, e.tgt, e.src, e.val) for e in es]
    for indptr, _, _ in ops:
        lengths = np.diff(indptr)
        short, mid = int((lengths < hfc.PUSH_LONG).sum()), int(((lengths >= hfc.PUSH_LONG) & (lengths < hfc.PUSH_WIDE)).sum())
        one_trip = hfc.push_blocks(S, 256, cus * hfc.BUILD_PER_CU, B) * 256
        assert S > one_trip and (lengths[one_trip:] < hfc.PUSH_LONG).any() and short > 0     # the lane path's second trip
        assert -(-mid // 16) > hfc.push_blocks(mid, 16, cus * hfc.GROUP_PER_CU, B)
        assert (lengths >= hfc.PUSH_WIDE).any()
    rng = np.random.default_rng(11)
    mu0 = np.stack([np.full(S, 1.0 / S), rng.standard_normal(S)])
    op = s.horizon_operator(pol)
    try:
        for k in range(T):
            assert all(np.array_equal(a, b) for a, b in zip(op.tocsr(k), ops[k])), k
            assert np.array_equal(op.mean_cost[k], es[k].mean_cost)
        got = op.propagate(mu0)
    finally:
        op.close()
    assert np.array_equal(got.mu, forward.propagate(ops, [e.mean_cost for e in es], mu0).mu)


def test_propagate_in_one_call(gpu, monkeypatch):
    row, s, pol, es, ops = _setup('reservoirs', 'f64')
    dims = _dims(s)
    vec, batch = _batch(es[0].S, s.dtype, dims)
    J_fin = np.cos(np.arange(es[0].S, dtype=float)).reshape(dims)
    op = s.horizon_operator(pol)
    try:
        want = op.propagate(batch, J_fin)
    finally:
        op.close()
    opened, closed = [], []
    init, close = HorizonOperator.__init__, HorizonOperator.close
    monkeypatch.setattr(HorizonOperator, '__init__', lambda self, *a, **kw: (opened.append(self), init(self, *a, **kw))[1])
    monkeypatch.setattr(HorizonOperator, 'close', lambda self: (closed.append(self), close(self))[1])
    got = s.propagate(pol, batch, J_fin=J_fin)
    assert len(opened) == 1 and closed and closed[0] is opened[0] and not opened[0]._h
    for a, b in zip(got, want):
        assert fc.same(a, b)
    assert np.array_equal(got.total_cost, got.step_cost.sum(axis=0) + got.terminal_cost, equal_nan=True)
    finite = np.isfinite(got.total_cost)
    assert finite.any() and np.array_equal(got.total_cost[finite], (got.step_cost.sum(axis=0) + got.terminal_cost)[finite])
