"""Every case of tests/tabulated_cases.py -- tabulated mode, the only path of a model the tracer refuses: the kernels
k_tab_cells<1 .. 4> and k_tab_reduce of sdp_tab_backup (csrc/sdp_hip.hip) under their four host drivers -- against
oracle/vi_numpy.py, the float64 definition with the sequential expectation.  Every comparison is numpy.array_equal on
ALL nodes (a NaN equals a NaN where the input has some): no sample, no tolerance.

- the sweep of every case on every input of the table (a finite horizon for the time-indexed case), the relative form
  once per case, and the cost variants with NaN, +inf and -inf at chosen controls;
- the chunked sweep: DPSolver._backup_tabulated with one node per sdp_tab_backup call and with batches of a few
  hundred to a few thousand cells, on lattices that grow along the sweep and on the mirrored problem, where they shrink;
- eval_policy with the oracle's policy and with one that lies off every lattice; the deterministic refusal;
- _value_at_state_vect / _value_at_state_loop on one interpolator's kept handle, small and large lattices in turn, and
  across set_values;
- lookahead on the host path, batches of 1, 7 and 65 states with grid nodes, states off the grid and states without a
  lattice, against the numpy definition (stodynprog_amd/lookahead.py);
- what a 4-byte solver does with such a model;
- the argument checks of the C entry.

tests/test_tabulated_cases_plan.py proves on the CPU that the cases have the lattices, ties and batches claimed."""
import contextlib
import ctypes as C
import functools
import io

import numpy as np
import pytest

import tabulated_cases as tc
from oracle import vi_numpy
from stodynprog_amd import lookahead as la

pytestmark = pytest.mark.gpu


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all='ignore'):
        return fn(*a, **k)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == 'f')


def differs(got, ref):
    """where (J, policy, index) differ from the oracle's: the first node and how many, or None"""
    J, Jo = np.ravel(got[0]), np.ravel(ref[0])
    assert J.shape == Jo.shape and J.dtype == Jo.dtype == np.float64
    n = J.size
    bad = ~((J == Jo) | (np.isnan(J) & np.isnan(Jo)))
    p, po = np.reshape(got[1], (n, -1)), np.reshape(ref[1], (n, -1))
    bad |= ~((p == po) | (np.isnan(p) & np.isnan(po))).all(axis=1)
    bad |= np.ravel(got[2]).astype(np.int64) != np.ravel(ref[2]).astype(np.int64)
    if not bad.any():
        return None
    k = int(np.flatnonzero(bad)[0])
    return 'first at node {} of {} that differ: J {!r} / {!r}, index {} / {}, control {} / {}'.format(
        k, int(bad.sum()), J[k], Jo[k], int(np.ravel(got[2])[k]), int(np.ravel(ref[2])[k]), p[k], po[k])


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    V = tc.inputs(shape)
    for v in V.values():
        v.setflags(write=False)
    return V


@functools.lru_cache(maxsize=None)
def _oracle(name, vname, mirrored=False, mark=None, dtype=np.float64):
    """the oracle's (J, policy, index) of a case on an input, computed once and shared; a finite-horizon case: per step,
    t ascending, from the final cost-to-go `vname`"""
    case = tc.BY_NAME[name]
    s = (case.mirrored if mirrored else case.make)()
    if mark:
        s = tc.with_cost_marks(s, mark)
    V = np.asarray(_inputs(s._shape())[vname], dtype=dtype).astype(float)
    if not case.t_fin:
        return tc.oracle_sweep(s, V)
    out, Jn = [None] * case.t_fin, V
    for t in reversed(range(case.t_fin)):
        out[t] = tc.oracle_sweep(s, Jn, t)
        Jn = out[t][0]
    return out


def _sweep(s, V):
    J, pol = quiet(s.value_iteration, V, report_time=False)
    assert s.backend_info['mode'] == 'tabulated', s.backend_info
    return J, pol, s.last_policy_index


# ---------------------------------------------------------------------------------------------------------------------
# the sweep
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case,vname', tc.RUNS, ids=['{}-{}'.format(c.name, v) for c, v in tc.RUNS])
def test_sweep_against_the_oracle_on_all_nodes(gpu, case, vname):
    s = case.solver()
    V = _inputs(s._shape())[vname]
    what = '{} on {}'.format(case, vname)
    if case.t_fin:
        J, pol = quiet(s.bellman_recursion, case.t_fin, V, report_time=False)
        assert s.backend_info['mode'] == 'tabulated'
        ref = _oracle(case.name, vname)
        for t in range(case.t_fin):
            idx = s.last_policy_index if t == 0 else ref[t][2]          # (the solver keeps the indices of its last sweep)
            d = differs((J[t], pol[t], idx), ref[t])
            assert d is None, '{}, step {}: {}'.format(what, t, d)
        assert not same(ref[0][0], ref[case.t_fin - 1][0])
        return
    d = differs(_sweep(s, V), _oracle(case.name, vname))
    assert d is None, '{}: {}'.format(what, d)
    if vname == 'random':           # the relative form, once per case
        spec = vi_numpy.Spec.from_solver(s)
        Vd = V - V[s._state_ref_ind]
        (Jr, r), polr = quiet(s.value_iteration, (Vd, 0.), rel_dp=True, report_time=False)
        with np.errstate(all='ignore'):
            (Jo, ro), po, io, _ = vi_numpy.value_iteration(spec, (Vd, 0.), rel_dp=True)
        assert Jr[s._state_ref_ind] == 0. and r == ro and np.isfinite(r)
        d = differs((Jr, polr, s.last_policy_index), (Jo, po, io))
        assert d is None, '{}, relative form: {}'.format(what, d)


@pytest.mark.parametrize('case,mark', tc.MARK_RUNS, ids=['{}-{}'.format(c.name, m) for c, m in tc.MARK_RUNS])
def test_nan_and_infinite_costs_follow_numpy_argmin(gpu, case, mark):
    s = tc.with_cost_marks(case.solver(), mark)
    ref = _oracle(case.name, 'random', mark=mark)
    d = differs(_sweep(s, _inputs(s._shape())['random']), ref)
    assert d is None, '{} with {}: {}'.format(case, mark, d)
    # (what the variant is there for, read off the oracle)
    J, idx = ref[0].ravel(), ref[2].ravel()
    if mark == 'inf nodes':
        assert ((J == np.inf) & (idx == 0)).sum() >= len(J) // 3
    elif mark == 'minus inf twice':
        assert ((J == -np.inf) & (idx == 5)).any()
    elif mark == 'finite at 70 alone':
        assert (np.isfinite(J) & (idx == 70)).any() and ((J == np.inf) & (idx == 0)).any()
    else:
        assert (np.isnan(J) & (idx == (37 if '37' in mark else 70))).any()


# ---------------------------------------------------------------------------------------------------------------------
# several sdp_tab_backup calls on one handle
# ---------------------------------------------------------------------------------------------------------------------
_CHUNKED = [(n, k, m) for n in sorted(tc.CHUNKS) for k in tc.CHUNKS[n] for m in (False, True)]


@pytest.mark.parametrize('name,chunk,mirrored', _CHUNKED,
                         ids=['{}-{}{}'.format(n, k, '-mirrored' if m else '') for n, k, m in _CHUNKED])
def test_chunked_sweep_is_the_single_call_and_the_oracle(gpu, name, chunk, mirrored):
    case = tc.BY_NAME[name]
    s = (case.mirrored if mirrored else case.make)()
    for vname in ('random', 'special'):
        V = _inputs(s._shape())[vname]
        with np.errstate(all='ignore'):
            J1, p1, _ = s._backup_tabulated(V, None, False)
            one = (J1, p1, s.last_policy_index)
            Jc, pc, r = s._backup_tabulated(V, None, False, chunk_cells=chunk)
        got = (Jc, pc, s.last_policy_index)
        assert r == 0.0
        what = '{}{} on {} in batches of {} cells'.format(name, ' mirrored' if mirrored else '', vname, chunk)
        d = differs(got, one)
        assert d is None, '{} / one call: {}'.format(what, d)
        d = differs(got, _oracle(name, vname, mirrored))
        assert d is None, '{} / oracle: {}'.format(what, d)


# ---------------------------------------------------------------------------------------------------------------------
# policy evaluation: one control per node
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['oracle', 'off lattice'])
@pytest.mark.parametrize('name', ['three states', 'two controls'])
def test_eval_policy_against_the_oracle(gpu, name, kind):
    s = tc.BY_NAME[name].solver()
    spec = vi_numpy.Spec.from_solver(s)
    V = _inputs(s._shape())
    pol = _oracle(name, 'random')[1] if kind == 'oracle' else tc.off_lattice_policy(s)
    if kind == 'off lattice':
        assert not same(pol, _oracle(name, 'random')[1])
    E, refs = quiet(s.eval_policy, pol, 3, rel_dp=True, J_zero=np.array(V['smooth']), report_time=False, J_ref_full=True)
    assert s.backend_info['mode'] == 'tabulated'
    with np.errstate(all='ignore'):
        Eo, refs_o = vi_numpy.eval_policy(spec, pol, 3, rel_dp=True, J_zero=np.array(V['smooth']), J_ref_full=True)
    assert E.dtype == np.float64 and same(E, Eo) and same(refs, refs_o) and len(refs) == 3
    assert np.isfinite(E).all() and E[s._state_ref_ind] == 0.
    # and a plain single step from zeros
    E1 = quiet(s.eval_policy, pol, 1, report_time=False)
    with np.errstate(all='ignore'):
        assert same(E1, vi_numpy.eval_policy(spec, pol, 1))


def test_eval_policy_of_a_deterministic_untraceable_model_is_refused(gpu):
    s = tc.BY_NAME['four states'].solver()
    pol = np.zeros(s._shape() + (2,))
    with pytest.raises(NotImplementedError) as e:
        quiet(s.eval_policy, pol, 1, report_time=False)
    assert str(e.value) == 'eval_policy of a deterministic system whose callables cannot be traced'


# ---------------------------------------------------------------------------------------------------------------------
# one node per call on the interpolator's handle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['line ragged', 'four states'])
def test_value_at_state_on_a_kept_handle_and_across_set_values(gpu, name):
    s = tc.BY_NAME[name].solver()
    V = _inputs(s._shape())
    nodes = tc.nodes_of(s)
    U = tc.lattice_sizes(s)
    order = tc.alternating(U)
    assert sorted(order) == list(range(len(nodes))) and U[order[0]] == U.min() and U[order[1]] == U.max()
    interp = s.interp_on_state(np.array(V['random']))
    handles = []
    for vname in ('random', 'smooth'):
        if vname != 'random':
            interp.set_values(np.array(V[vname]))
            assert '_tab' not in interp.__dict__                     # the handle of the old values is dropped
        Jo, po, _ = _oracle(name, vname)
        Jo, po = Jo.ravel(), po.reshape(len(nodes), -1)
        for n in order:
            with np.errstate(all='ignore'):
                J, u = s._value_at_state_vect(nodes[n], interp)
                Jl, ul = s._value_at_state_loop(nodes[n], interp)
            assert J == Jo[n] and list(u) == list(po[n]), '{} on {}: node {} ({} controls)'.format(name, vname, n, U[n])
            assert Jl == Jo[n] and tuple(ul) == tuple(po[n])
        handles.append(interp.__dict__['_tab'])
    assert handles[0] is not handles[1]
    assert not same(_oracle(name, 'random')[0], _oracle(name, 'smooth')[0])


# ---------------------------------------------------------------------------------------------------------------------
# lookahead on the host path
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', [1, 7, 65])
@pytest.mark.parametrize('name', ['two controls', 'three states', 'four states'])
def test_lookahead_of_a_mixed_batch_against_the_definition(gpu, name, B):
    s = tc.BY_NAME[name].solver()
    V = _inputs(s._shape())['random']
    x = tc.lookahead_states(s, B)
    with np.errstate(all='ignore'):
        J, u, idx = s.lookahead(V, x)
        Jd, ud, idxd = la.lookahead(s, V, x)
        Jr, ur, idxr = tc.lookahead_rule(s, V, x)
    assert s.backend_info['mode'] == 'tabulated' and s.backend_info['lookahead_path'] == 'host'
    assert J.dtype == u.dtype == np.float64 and idx.dtype == np.int32
    assert same(J, Jd) and same(u, ud) and same(idx, idxd), '{}, batch of {}: the definition'.format(name, B)
    assert same(J, Jr) and same(u, ur) and same(idx, idxr), '{}, batch of {}: the oracle interpolation'.format(name, B)
    dead = idx == -1
    assert dead.sum() == B // 7 and np.isnan(J[dead]).all() and np.isnan(u[dead]).all() and np.isfinite(J[~dead]).all()
    # at a grid node: the sweep's J, control and index
    Jo, po, io = _oracle(name, 'random')
    at = {tuple(n): k for k, n in enumerate(tc.nodes_of(s))}
    hit = [(b, at[tuple(r)]) for b, r in enumerate(x) if tuple(r) in at]
    assert hit
    for b, k in hit:
        assert J[b] == Jo.ravel()[k] and idx[b] == io.ravel()[k] and list(u[b]) == list(po.reshape(len(at), -1)[k])


# ---------------------------------------------------------------------------------------------------------------------
# a 4-byte solver with a model that does not trace
# ---------------------------------------------------------------------------------------------------------------------
def _four_byte(name):
    s = {'line ragged': tc.line, 'two controls': tc.two_controls}[name](dtype=np.float32)()
    assert s.dtype == np.float32 and all(np.asarray(g).dtype == np.float64 for g in s.state_grid)
    return s


@pytest.mark.parametrize('name', tc.FOUR_BYTE)
def test_a_four_byte_solver_sweeps_and_evaluates_in_float64(gpu, name):
    """the sweep and the evaluation of tabulated mode are float64 whatever DPSolver.dtype: the callables get float64
    arguments, a float32 cost-to-go is widened (exactly), J and the policy come back as float64 -- the bits of the
    8-byte solver and of the float64 oracle -- from value_iteration, value_iterations and eval_policy alike"""
    s = _four_byte(name)
    V = _inputs(s._shape())['random']
    got = _sweep(s, V)
    assert got[0].dtype == got[1].dtype == np.float64
    d = differs(got, _oracle(name, 'random'))
    assert d is None, d
    V32 = V.astype(np.float32)
    assert not same(V32.astype(float), V)
    d = differs(_sweep(s, V32), _oracle(name, 'random', dtype=np.float32))
    assert d is None, 'a float32 cost-to-go: {}'.format(d)
    # value_iterations: the chained calls
    J2, p2 = quiet(s.value_iterations, V, 2, report_time=False)
    idx2 = s.last_policy_index
    Jc, pc, ic = _sweep(s, _sweep(s, V)[0])
    assert J2.dtype == np.float64 and differs((J2, p2, idx2), (Jc, pc, ic)) is None
    assert differs((J2, p2, idx2), tc.oracle_sweep(s, _oracle(name, 'random')[0])) is None
    # eval_policy
    if name == 'two controls':
        pol = tc.off_lattice_policy(s)
        E, refs = quiet(s.eval_policy, pol, 2, rel_dp=True, J_zero=np.array(V), report_time=False, J_ref_full=True)
        with np.errstate(all='ignore'):
            Eo, refs_o = vi_numpy.eval_policy(vi_numpy.Spec.from_solver(s), pol, 2, rel_dp=True, J_zero=np.array(V), J_ref_full=True)
        assert E.dtype == np.float64 and same(E, Eo) and same(refs, refs_o)


@pytest.mark.parametrize('name', tc.FOUR_BYTE)
def test_a_four_byte_solver_looks_ahead_in_float64_from_rounded_states_and_boxes(gpu, name):
    """lookahead keeps the contract of the traced 4-byte path at its edges -- the state and the box ends are rounded to
    float32 ONCE, J and u come back as float32 -- and computes in float64 in between (tabulated_cases.lookahead_rule)"""
    s = _four_byte(name)
    V = _inputs(s._shape())['random']
    d = len(s._shape())
    rng = np.random.default_rng(12)
    x = np.concatenate([np.array(tc.nodes_of(s))[::5], rng.random((24, d)), [[tc.NAN_A] + [0.5] * (d - 1)]])
    with np.errstate(all='ignore'):
        J, u, idx = s.lookahead(V, x)
        Jr, ur, idxr = tc.lookahead_rule(s, V, x)
    assert s.backend_info['mode'] == 'tabulated' and J.dtype == u.dtype == np.float32 and idx.dtype == np.int32
    assert same(J, Jr) and same(u, ur) and same(idx, idxr)
    if name == 'two controls':
        assert idx[-1] == -1 and np.isnan(J[-1])
    # the float32 rounding of the states and of the box ends is part of the rule: the 8-byte rule differs
    s8 = tc.BY_NAME[name].solver()
    with np.errstate(all='ignore'):
        J8, u8, _ = tc.lookahead_rule(s8, V, x)
    assert not same(J8.astype(np.float32), J) and not same(u8.astype(np.float32), u)


# ---------------------------------------------------------------------------------------------------------------------
# the C entry
# ---------------------------------------------------------------------------------------------------------------------
def test_the_c_entry_checks_its_arguments(gpu):
    lib = gpu.lib()
    ptr = gpu.ptr
    V = np.arange(4.0)
    smin, smax, orders = np.zeros(1), np.ones(1), np.array([4], dtype=np.int64)
    h = C.c_void_p()
    gpu.check(lib.sdp_tab_create(1, ptr(smin), ptr(smax), ptr(orders), ptr(V), C.byref(h)))
    try:
        off = np.array([0, 2, 6], dtype=np.int64)                       # two nodes: one control and two, W = 2
        proba = np.array([0.25, 0.75])
        xn = np.array([[0., 1. / 3, 1., 1., 2. / 3, 2. / 3]])
        g = np.array([1., 1., 5., 5., 0.5, 0.5])
        J = np.full(2, -7.0)
        idx = np.full(2, -7, dtype=np.int64)

        def call(t=h, n=2, off=off, W=2, proba=proba, xn=xn, g=g, J=J, idx=idx):
            return lib.sdp_tab_backup(t, n, ptr(off), W, ptr(proba), ptr(xn), ptr(g), ptr(J), ptr(idx))
        # no node: nothing is written, nothing is read
        assert call(n=0) == 0 and call(n=0, proba=None, xn=None, g=None) == 0
        assert list(J) == [-7.0, -7.0] and list(idx) == [-7, -7]
        for bad, text in ((dict(t=None), b'NULL argument'), (dict(off=None), b'NULL argument'),
                          (dict(J=None), b'NULL argument'), (dict(idx=None), b'NULL argument'),
                          (dict(n=-1), b'negative size'), (dict(W=-1), b'negative size'),
                          (dict(off=np.array([0, 0, 0], dtype=np.int64)), b'empty lattice'),
                          (dict(off=np.array([0, 2, -6], dtype=np.int64)), b'empty lattice'),
                          (dict(xn=None), b'empty lattice'), (dict(g=None), b'empty lattice'),
                          (dict(proba=None), b'perturbation weights missing')):
            assert call(**bad) == -1, bad
            assert lib.sdp_last_error() == text, (bad, lib.sdp_last_error())
            assert list(J) == [-7.0, -7.0] and list(idx) == [-7, -7]
        # and the call the refusals were variations of: 0.25 * (1 + 0) + 0.75 * (1 + 1), then the second control
        assert call() == 0
        assert list(J) == [0.25 * 1.0 + 0.75 * 2.0, 0.25 * 2.5 + 0.75 * 2.5] and list(idx) == [0, 1]
        # W == 0 needs no weights: a cell per control
        J0, i0 = np.zeros(2), np.zeros(2, dtype=np.int64)
        assert call(W=0, proba=None, J=J0, idx=i0) == 0
        assert list(J0) == [1.0, 2.5] and list(i0) == [0, 2]
    finally:
        lib.sdp_tab_destroy(h)
