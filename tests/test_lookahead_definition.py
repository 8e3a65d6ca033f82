"""The numpy definition of the one-step lookahead at arbitrary states (stodynprog_amd/lookahead.py) against the
oracle (oracle/vi_numpy.py: backup_node, backup_node_real, value_iteration), bit for bit, at every state of every case
of tests/lookahead_cases.py; and the closed-loop definition against the oracle chained step by step.  No GPU."""
import numpy as np
import pytest

import lookahead_cases as lc
from oracle import vi_numpy
from stodynprog_amd import lookahead as la


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _index(case):
    return 'int' if case.int_time else 'real'


@pytest.mark.parametrize('case', lc.CASES, ids=repr)
def test_definition_equals_the_oracle_at_every_state(case):
    s = case.solver()
    spec = lc.spec_of(case, s)
    X = lc.states(case, s)
    for n, t_k in enumerate(case.times):
        J_next = lc.cost_to_go(s, n)
        J, u, idx = la.lookahead(s, J_next, X, t_k, _index(case))
        Jo, uo, io = lc.oracle_lookahead(s, spec, J_next, X, t_k)
        assert J.dtype == s.dtype and u.dtype == s.dtype and idx.dtype == np.int32
        assert J.shape == (len(X),) and u.shape == (len(X), len(s.sys.control))
        assert np.all(idx >= 0)
        assert same(idx, io) and same(J, Jo) and same(u, uo), (case, t_k)


@pytest.mark.parametrize('case', lc.CASES, ids=repr)
def test_at_the_nodes_it_is_value_iteration(case):
    s = case.solver()
    spec = lc.spec_of(case, s)
    S = lc.n_nodes(s)
    X = lc.states(case, s)[:S]
    t_k = case.times[0]
    J_next = lc.cost_to_go(s)
    dtype = None if s.dtype == np.float64 else s.dtype
    with np.errstate(all='ignore'):
        Jv, pol, iv, _ = vi_numpy.value_iteration(spec, J_next, t_k=t_k, dtype=dtype)
    J, u, idx = la.lookahead(s, J_next, X, t_k, _index(case))
    assert same(J, Jv.ravel()) and same(u, pol.reshape(S, -1)) and same(idx, iv.ravel())


@pytest.mark.parametrize('L', [1, 8, 64])
def test_lane_cases_reach_the_totals_around_the_lane_count(L):
    s = lc.lanes_model(L)
    assert s._box_plan()['lanes'] == L
    X = np.array(lc.LANE_STATES[L], dtype=float).reshape(-1, 1)
    lo, hi, n = la.lattice(s.sys.control_box, s.sys.params, s.control_steps, X, None, s.dtype)
    assert tuple(int(v) for v in n[0]) == lc.LANE_TOTALS[L]
    (a, b), = s.sys.control_box(float(X[-1, 0]))
    assert b < a                                          # hi < lo: one point at the centre
    assert lo[0, -1] == hi[0, -1] == (a + b) / 2


def test_a_cost_flat_in_the_control_takes_the_first_point():
    case = lc.BY_NAME['flat']
    s = case.solver()
    J, u, idx = la.lookahead(s, lc.cost_to_go(s), lc.states(case, s))
    assert np.all(idx == 0)


def test_the_first_nan_wins():
    case = lc.BY_NAME['lanes 8']
    s = case.solver()
    spec = lc.spec_of(case, s)
    J_next = lc.cost_to_go(s)
    J_next[4] = np.nan                                    # a node in the middle: some lattice points reach it
    X = lc.states(case, s)
    J, u, idx = la.lookahead(s, J_next, X)
    Jo, uo, io = lc.oracle_lookahead(s, spec, J_next, X)
    assert same(idx, io) and same(J, Jo) and same(u, uo)
    hit = np.isnan(J)
    assert hit.any() and not hit.all()
    # where a NaN is reached at all, the optimum is the FIRST lattice point that reaches one
    for b in np.flatnonzero(hit)[:8]:
        _, _, _, _, full = vi_numpy.backup_node(spec, tuple(X[b]), lc.oracle_interp(s, spec, J_next), full=True)
        assert idx[b] == int(np.flatnonzero(np.isnan(full.ravel()))[0])


@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['f64', 'f32'])
def test_a_nan_box_end_gives_nan_and_minus_one(dtype):
    s = lc.nan_box(dtype)
    case = lc.Case('nan box', lc.nan_box)
    spec = lc.spec_of(case, s)
    J_next = lc.cost_to_go(s)
    good = np.array([[0.1], [0.2], [0.7], [1.1]])
    X = np.concatenate([good[:2], [[lc.NAN_STATE]], good[2:]])
    J, u, idx = la.lookahead(s, J_next, X)
    assert np.isnan(J[2]) and np.isnan(u[2]).all() and idx[2] == -1
    keep = [0, 1, 3, 4]
    Jo, uo, io = lc.oracle_lookahead(s, spec, J_next, good)
    assert same(J[keep], Jo) and same(u[keep], uo) and same(idx[keep], io)


def test_a_lattice_of_two_to_the_31_points_is_none():
    lo, hi, n = la.lattice_of_ends(np.array([[0., 0.]]), np.array([[2. ** 31, 10.]]), (1.,), np.float64)
    assert tuple(n[0]) == (0, 11) and np.isnan(lo[0, 0]) and lo[0, 1] == 0.
    lo, hi, n = la.lattice_of_ends(np.array([[0.], [0.]]), np.array([[70000.], [70000.]]), (1., 1.), np.float64)
    assert tuple(n[:, 0]) == (0, 0)
    lo, hi, n = la.lattice_of_ends(np.array([[0.]]), np.array([[np.inf]]), (1.,), np.float64)
    assert n[0, 0] == 0


@pytest.mark.parametrize('case', lc.CASES, ids=repr)
@pytest.mark.parametrize('B', [1, 9])
def test_closed_loop_definition_equals_the_chained_oracle(case, B):
    s = case.solver()
    spec = lc.spec_of(case, s)
    t0 = 0 if case.times[0] is None else case.times[0]
    T = lc.T_SIM if t0 + lc.T_SIM <= 8 else 8 - t0
    J_next = lc.cost_to_go(s)
    x0 = lc.start_states(case, s, B)
    w, w_oracle = lc.draws(s, T, B)
    w3 = None if w is None else (w if w.ndim == 3 else w[:, None, :])
    x, u, g, q = la.simulate_lookahead(s, J_next, x0, w3, T, t0, _index(case))
    xo, uo, go, qo = lc.oracle_closed_loop(s, spec, J_next, x0, w_oracle, T, t0)
    assert x.shape == (T + 1, B, x0.shape[1]) and q.shape == (T, B)
    assert same(x, xo) and same(u, uo) and same(g, go) and same(q, qo)


def test_a_time_indexed_cost_to_go_is_read_at_t0_plus_k():
    case = lc.BY_NAME['symbolic time']
    s = case.solver()
    spec = lc.spec_of(case, s)
    J_all = np.stack([lc.cost_to_go(s, k) for k in range(8)])
    x0 = lc.start_states(case, s, 5)
    w, w_oracle = lc.draws(s, 4, 5)
    x, u, g, q = la.simulate_lookahead(s, J_all, x0, w[:, None, :], 4, 3)
    xo, uo, go, qo = lc.oracle_closed_loop(s, spec, J_all, x0, w_oracle, 4, 3)
    assert same(x, xo) and same(u, uo) and same(g, go) and same(q, qo)
    for bad in ((4, 5), (2, -1)):
        with pytest.raises(ValueError) as err:
            la.simulate_lookahead(s, J_all, x0, w[:, None, :], *bad)
        assert 'T_J = 8' in str(err.value)
