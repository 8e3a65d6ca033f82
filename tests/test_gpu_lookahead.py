"""DPSolver.lookahead and simulate_lookahead on the device (kernels sdp_lookahead / sdp_simulate_lookahead,
csrc/sdp_lookahead_kernel.h) against the oracle, bit for bit, on every case of tests/lookahead_cases.py: the
device-made lattice, the host-made one, the host loop, value_iteration at the nodes, chunked time-indexed
cost-to-go arrays.  Each test builds its solver once; nothing loops over a failing step or tries it again."""
import functools

import numpy as np
import pytest

import lookahead_cases as lc

pytestmark = pytest.mark.gpu


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


@functools.lru_cache(maxsize=None)
def reference(name, n):
    """(solver's states, cost-to-go n, the oracle's answer at time index times[n]) of a case, computed once"""
    case = lc.BY_NAME[name]
    s = case.solver()
    X = lc.states(case, s)
    J_next = lc.cost_to_go(s, n)
    out = lc.oracle_lookahead(s, lc.spec_of(case, s), J_next, X, case.times[n])
    for a in (X, J_next) + out:
        a.setflags(write=False)
    return X, J_next, out


def check(got, want, what):
    J, u, idx = got
    Jo, uo, io = want
    assert idx.dtype == np.int32 and J.dtype == Jo.dtype and u.dtype == uo.dtype, what
    assert same(idx, io), (what, np.flatnonzero(idx != io)[:8])
    assert same(J, Jo), (what, np.flatnonzero(~(J == Jo))[:8])
    assert same(u, uo), what


@pytest.mark.parametrize('case', lc.CASES, ids=repr)
def test_lookahead_equals_the_oracle(case):
    s = case.solver()
    for n, t_k in enumerate(case.times):
        X, J_next, want = reference(case.name, n)
        got = s.lookahead(J_next, X, t_k)
        assert s.backend_info['lookahead_box'] == case.box, s.backend_info
        assert s.backend_info['lookahead_path'] == ('host' if case.name == 'untraceable' else 'device')
        check(got, want, (case, t_k, 'as planned'))
        # the lattice made by the host: the same bits
        got = s.lookahead(J_next, X, t_k, path='host')
        assert s.backend_info['lookahead_box'] == 'host'
        check(got, want, (case, t_k, 'host-made lattice'))


@pytest.mark.parametrize('case', lc.CASES, ids=repr)
def test_batch_sizes_around_a_wave(case):
    s = case.solver()
    X, J_next, want = reference(case.name, 0)
    t_k = case.times[0]
    for B in case.batches:
        rows = (np.arange(B) + len(X) - min(B, len(X))) % len(X)         # (the case's own states last: they are in)
        got = s.lookahead(J_next, X[rows], t_k)
        check(got, tuple(a[rows] for a in want), (case, B))
    one = s.lookahead(J_next, X[-1], t_k)                                 # a single state, shape (d,)
    check(one, tuple(a[-1:] for a in want), (case, 'one state'))


@pytest.mark.parametrize('name', lc.VI_CASES)
def test_at_the_nodes_it_is_value_iteration(name):
    case = lc.BY_NAME[name]
    s = case.solver()
    S = lc.n_nodes(s)
    X, J_next, _ = reference(name, 0)
    J, u, idx = s.lookahead(J_next, X[:S])
    shape = tuple(len(g) for g in s.state_grid)
    for kernel in ('generic', 'auto'):
        v = case.solver()
        v.kernel = kernel
        Jv, pol = v.value_iteration(J_next.astype(v.dtype), report_time=False)
        iv = v.last_policy_index
        assert same(J.reshape(shape), np.asarray(Jv, dtype=s.dtype)), (name, kernel)
        assert same(u.reshape(shape + (-1,)), np.asarray(pol, dtype=s.dtype)), (name, kernel)
        assert same(idx.reshape(shape), iv), (name, kernel)


def test_a_cost_flat_in_the_control_takes_the_first_point():
    case = lc.BY_NAME['flat']
    s = case.solver()
    X, J_next, _ = reference('flat', 0)
    J, u, idx = s.lookahead(J_next, X)
    assert np.all(idx == 0)


def test_the_first_nan_wins():
    case = lc.BY_NAME['lanes 8']
    s = case.solver()
    X = lc.states(case, s)
    J_next = lc.cost_to_go(s)
    J_next[4] = np.nan
    want = lc.oracle_lookahead(s, lc.spec_of(case, s), J_next, X)
    assert np.isnan(want[0]).any() and not np.isnan(want[0]).all()
    check(s.lookahead(J_next, X), want, 'device lattice')
    check(s.lookahead(J_next, X, path='host'), want, 'host lattice')


@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['f64', 'f32'])
def test_a_nan_box_end_gives_nan_and_minus_one(dtype):
    s = lc.nan_box(dtype)
    case = lc.Case('nan box', lc.nan_box)
    J_next = lc.cost_to_go(s)
    good = np.array([[0.1], [0.2], [0.7], [1.1]])
    X = np.concatenate([good[:2], [[lc.NAN_STATE]], good[2:]])
    want = lc.oracle_lookahead(s, lc.spec_of(case, s), J_next, good)
    keep = [0, 1, 3, 4]
    for path in (None, 'host'):
        J, u, idx = s.lookahead(J_next, X, path=path)
        assert s.backend_info['lookahead_box'] == ('host' if path else 'device')
        assert np.isnan(J[2]) and np.isnan(u[2]).all() and idx[2] == -1, path
        check((J[keep], u[keep], idx[keep]), want, path)                 # the other states of the batch are untouched


def _horizon(case):
    t0 = 0 if case.times[0] is None else case.times[0]
    return t0, lc.T_SIM


@pytest.mark.parametrize('case', lc.CASES, ids=repr)
def test_closed_loop_equals_the_chained_oracle(case):
    s = case.solver()
    spec = lc.spec_of(case, s)
    t0, T = _horizon(case)
    J_next = lc.cost_to_go(s)
    shape = tuple(len(g) for g in s.state_grid)
    for B in (1, 9, 65):
        x0 = lc.start_states(case, s, B)
        w, w_oracle = lc.draws(s, T, B)
        want = lc.oracle_closed_loop(s, spec, J_next, x0, w_oracle, T, t0)
        got = s.simulate_lookahead(J_next, x0, w, n_steps=T, t0=t0)
        assert s.backend_info['lookahead_path'] == case.path, (case, s.backend_info)
        for a, b, what in zip(got, want, 'xugq'):
            assert a.dtype == s.dtype and same(a, b), (case, B, what)
        host = s.simulate_lookahead(J_next, x0, w, n_steps=T, t0=t0, path='host')
        assert s.backend_info['lookahead_path'] == 'host'
        for a, b, what in zip(host, got, 'xugq'):
            assert same(a, b), (case, B, what, 'host against device')
    # step 0 from a node is the backup of that node (start_states: trajectory 0 starts at the middle node)
    node = tuple(n // 2 for n in shape)
    J, u, idx = s.lookahead(J_next, np.array([g[i] for g, i in zip(s.state_grid, node)]), None if s.sys.stationnary else t0)
    assert same(got[1][0, 0], u[0]) and same(got[3][0, 0], J[0])
    # the single-trajectory form
    x0 = lc.start_states(case, s, 1)
    w, _ = lc.draws(s, T, 1)
    w1 = None if w is None else w[..., 0]
    x, u, g, q = s.simulate_lookahead(J_next, x0[0], w1, n_steps=T, t0=t0)
    assert x.shape == (T + 1, len(shape)) and u.ndim == 2 and g.shape == (T,) and q.shape == (T,)


@pytest.mark.parametrize('name', ['searev', 'symbolic time', 'two_inflows'])
def test_step_zero_from_a_node_is_value_iterations_policy(name):
    case = lc.BY_NAME[name]
    s = case.solver()
    t0, T = _horizon(case)
    J_next = lc.cost_to_go(s)
    shape = tuple(len(g) for g in s.state_grid)
    S = lc.n_nodes(s)
    x0 = lc.states(case, s)[:S]
    w, _ = lc.draws(s, 1, S)
    x, u, g, q = s.simulate_lookahead(J_next, x0, w, n_steps=1, t0=t0)
    v = case.solver()
    v.kernel = 'generic'
    if s.sys.stationnary:
        Jv, pol = v.value_iteration(J_next, report_time=False)
    else:
        Jv, pol, _ = v._backup(J_next, t0, False)
    assert same(u[0].reshape(shape + (-1,)), pol) and same(q[0].reshape(shape), Jv)


@pytest.mark.parametrize('name', ['symbolic time', 'searev f32'])
def test_cutting_a_time_indexed_cost_to_go_changes_no_bit(name):
    case = lc.BY_NAME[name]
    s = case.solver()
    spec = lc.spec_of(case, s)
    T, t0 = lc.T_SIM, 1
    J_all = np.stack([lc.cost_to_go(s, k) for k in range(T + 2)])
    x0 = lc.start_states(case, s, 9)
    w, w_oracle = lc.draws(s, T, 9)
    want = lc.oracle_closed_loop(s, spec, J_all, x0, w_oracle, T, t0)
    whole = s.simulate_lookahead(J_all, x0, w, n_steps=T, t0=t0)
    assert s.backend_info['lookahead_path'] == 'device'
    for a, b, what in zip(whole, want, 'xugq'):
        assert same(a, b), (name, what)
    step_bytes = lc.n_nodes(s) * s.dtype.itemsize
    for steps in (1, 3):
        s.horizon_chunk_bytes = steps * step_bytes
        cut = s.simulate_lookahead(J_all, x0, w, n_steps=T, t0=t0)
        for a, b, what in zip(cut, whole, 'xugq'):
            assert same(a, b), (name, steps, what)
    with pytest.raises(ValueError):
        s.simulate_lookahead(J_all, x0, w, n_steps=T, t0=3)


# ----------------------------------------------------------------------------------------------------------------------
# batches past the launch caps: the rows a workgroup reaches after its first tile.  The whole batch against the numpy
# definition (stodynprog_amd/lookahead.py), the later trips also against the oracle; a chip on which the shape is not
# past the cap fails the assertion on the grid

DISTINCT = 2039


def _cus():
    from stodynprog_amd import _native as nat
    return nat.device_info(0)['compute_units']


def test_lookahead_past_the_grid_cap_with_64_lanes():
    from stodynprog_amd import lookahead as la
    case = lc.BY_NAME['lanes 64']
    s = case.solver()
    cus = _cus()
    B = cus * 8 * 4 + 33
    assert B == lc.cap_batch(64, cus)
    tiles, blocks = lc.lookahead_grid(B, 64, cus)
    later = lc.lookahead_later_trips(B, 64, cus)
    assert tiles > blocks == cus * 8 and len(later) >= 7 * 4, (tiles, blocks)       # every XCD but the last walks again
    J_next = lc.cost_to_go(s)
    X = lc.start_states(case, s, B)                                       # (every row another state)
    got = s.lookahead(J_next, X)
    assert s.backend_info['lookahead_path'] == 'device' and s.backend_info['lookahead_box'] == 'device'
    check(got, la.lookahead(s, J_next, X), 'the definition, every row')
    assert len(np.unique(got[2])) > 8
    rows = np.concatenate([later, np.arange(B - 40, B)])
    check(tuple(a[rows] for a in got), lc.oracle_lookahead(s, lc.spec_of(case, s), J_next, X[rows]), 'the oracle, later trips')


def test_lookahead_past_the_grid_cap_with_8_lanes():
    from stodynprog_amd import lookahead as la
    case = lc.BY_NAME['lanes 8']
    s = case.solver()
    cus = _cus()
    B = cus * 8 * 32 + 33
    assert B == lc.cap_batch(8, cus)
    tiles, blocks = lc.lookahead_grid(B, 8, cus)
    later = lc.lookahead_later_trips(B, 8, cus)
    assert tiles > blocks == cus * 8 and len(later) >= 32, (tiles, blocks)
    J_next = lc.cost_to_go(s)
    pick = lc.repeated_rows(B, DISTINCT)
    base = lc.start_states(case, s, DISTINCT)
    X = base[pick]
    got = s.lookahead(J_next, X)
    assert s.backend_info['lookahead_path'] == 'device' and s.backend_info['lookahead_box'] == 'device'
    check(got, tuple(a[pick] for a in la.lookahead(s, J_next, base)), 'the definition, every row')
    assert len(np.unique(got[2])) > 1
    rows = np.concatenate([later, np.arange(B - 40, B)])
    check(tuple(a[rows] for a in got), lc.oracle_lookahead(s, lc.spec_of(case, s), J_next, X[rows]), 'the oracle, later trips')


def test_closed_loop_past_the_grid_cap_with_8_lanes():
    from stodynprog_amd import lookahead as la
    case = lc.BY_NAME['lanes 8']
    s = case.solver()
    cus = _cus()
    T = 3
    B = cus * 8 * 32 + 33
    tiles, blocks = lc.simulate_grid(B, 8, cus)
    assert tiles > blocks == cus * 8, (tiles, blocks)                     # the tiles from `blocks` on: a second trip
    tail = blocks * 32 - 7
    J_next = lc.cost_to_go(s)
    pick = lc.repeated_rows(B, DISTINCT)
    base = lc.start_states(case, s, DISTINCT)
    w_base, _ = lc.draws(s, T, DISTINCT)
    x0, w = base[pick], np.ascontiguousarray(w_base[:, pick])
    got = s.simulate_lookahead(J_next, x0, w, n_steps=T)
    assert s.backend_info['lookahead_path'] == 'device'
    want = la.simulate_lookahead(s, J_next, base, w_base[:, None, :], T)
    for a, b, what in zip(got, want, 'xugq'):
        assert a.dtype == s.dtype and same(a, b[:, pick]), ('the definition', what)
    oracle = lc.oracle_closed_loop(s, lc.spec_of(case, s), J_next, x0[tail:], w[:, tail:], T)
    for a, b, what in zip(got, oracle, 'xugq'):
        assert same(a[:, tail:], b), ('the chained oracle, second trip', what)
    assert len(np.unique(got[0][-1])) > DISTINCT // 2                     # (the trajectories do differ)
