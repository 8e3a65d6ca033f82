"""The transition operator of a policy on the device (DPSolver.transition_operator: kernel sdp_transitions, the
library's stable sort into the CSR of P^T, k_push, sdp_transop_push_until) against its definition in numpy,
stodynprog_amd/forward.py, bit for bit -- entries, row pointers, mean cost, pushes and the stationary iteration -- on
the cases of tests/forward_cases.py in 8- and 4-byte reals; against the device's own eval_policy (the mean cost, and
the adjoint identity <mu, P J> = <P^T mu, J>); and `sdp_transop_from_coo` alone on adversarial row shapes."""
import ctypes as C

import numpy as np
import pytest

import forward_cases as fc
from stodynprog_amd import forward, TransitionOperator

pytestmark = pytest.mark.gpu

CASE_IDS = [c.name for c in fc.CASES]
_memo = {}
# eval_policy evaluates a non-stationary model at time index 0: the cases whose first t_k is that one
EVAL_CASES = [c for c in fc.DEVICE_CASES if c.times[0] in (None, 0)]


def definition(case, dtkey, t_k):
    """the case's entries and CSR from forward.py (computed once per process, never modified)"""
    key = (case.name, dtkey, t_k)
    if key not in _memo:
        s = case.solver(fc.DTYPES[dtkey])
        e = forward.entries(s, case.policy(s), t_k, time_index=case.time_index)
        csr = forward.csr(e.S, e.tgt, e.src, e.val)
        for a in csr + (e.mean_cost,):
            a.setflags(write=False)
        _memo[key] = (e, csr)
    return _memo[key]


def _assert_operator(op, e, csr, what):
    indptr, indices, data = op.tocsr()
    assert op.nnz == e.S * e.W * e.V == len(data), what
    assert indptr.dtype == np.int64 and indices.dtype == np.int32 and data.dtype == csr[2].dtype, what
    assert np.array_equal(indptr, csr[0]), what + ': indptr'
    assert np.array_equal(indices, csr[1]), what + ': indices'
    assert fc.same(data, csr[2]), what + ': data'


@pytest.mark.parametrize('dtkey', sorted(fc.DTYPES))
@pytest.mark.parametrize('case', fc.CASES, ids=CASE_IDS)
def test_operator_and_pushes_are_the_definition(gpu, case, dtkey):
    dt = fc.DTYPES[dtkey]
    for t_k in case.times:
        e, csr = definition(case, dtkey, t_k)
        s = case.solver(dt)
        op = s.transition_operator(case.policy(s), t_k)
        what = '{} {} t_k={}'.format(case.name, dtkey, t_k)
        try:
            assert op.path == ('host' if case.host else 'device'), what
            assert op.shape == tuple(len(g) for g in s.state_grid) and op.mean_cost.shape == op.shape
            info = s.backend_info['transition']
            assert info['nnz'] == op.nnz and info['bytes'] == op.nnz * (np.dtype(dt).itemsize + 4) + 8 * (e.S + 1)
            _assert_operator(op, e, csr, what)
            assert fc.same(op.mean_cost.ravel(), e.mean_cost), what + ': mean cost'
            for name, mu in fc.vectors(e.S, dt).items():
                for n in (1, 3):
                    got = op.push(mu.reshape(op.shape), n)
                    assert got.shape == op.shape and got.dtype == np.dtype(dt)
                    assert fc.same(got.ravel(), forward.push(csr, mu, n)), '{}: push({}, {})'.format(what, name, n)
            assert s.backend_info['transition']['push_ms'] >= 0
        finally:
            op.close()


@pytest.mark.parametrize('dtkey', sorted(fc.DTYPES))
@pytest.mark.parametrize('case', fc.DEVICE_CASES, ids=[c.name for c in fc.DEVICE_CASES])
def test_planned_unit_and_direct_kernel_give_one_csr(gpu, case, dtkey):
    """node ids and the policy are in the reference's C order whatever layout the plan stores its arrays in"""
    dt = fc.DTYPES[dtkey]
    t_k = case.times[-1]
    out = {}
    for kernel in (None, 'generic'):
        s = case.solver(dt, kernel)
        op = s.transition_operator(case.policy(s), t_k)
        out[kernel] = op.tocsr() + (op.mean_cost,)
        out[kernel, 'info'] = s.backend_info
        op.close()
    assert out['generic', 'info']['kernel'] == 'generic'
    if case.name in ('storage_ar1', 'searev'):
        assert out[None, 'info']['kernel'] != 'generic', out[None, 'info']['kernel']         # the column family
    for a, b in zip(out[None], out['generic']):
        assert fc.same(a, b), case.name


@pytest.mark.parametrize('dtkey', sorted(fc.DTYPES))
@pytest.mark.parametrize('case', EVAL_CASES, ids=[c.name for c in EVAL_CASES])
def test_mean_cost_and_adjoint_against_eval_policy(gpu, case, dtkey):
    """gbar is eval_policy(pol, 1) from zeros, bit for bit, and <mu, P J> = <P^T mu, J> with P J from the existing
    kernel sdp_evalpol: |mu . (eval_policy(pol, 1, J) - gbar) - push(mu) . J| <= (n_row + S + W 2^d) eps sum |val| |mu[src]|
    |J[tgt]|, n_row the longest row (the push's chain), S the two dot products, W 2^d the kernel's own sum per node"""
    dt = fc.DTYPES[dtkey]
    t_k = case.times[0]
    e, csr = definition(case, dtkey, t_k)
    s = case.solver(dt)
    pol = case.policy(s)
    op = s.transition_operator(pol, t_k)
    try:
        J0 = s.eval_policy(pol, 1, report_time=False)
        assert fc.same(J0, op.mean_cost), case.name
        if case.name == 'nan_state':
            return                            # (NaN weights: both sides of the identity are NaN)
        rng = np.random.default_rng(3)
        mu = rng.standard_normal(op.shape).astype(dt)
        J = rng.standard_normal(op.shape).astype(dt)
        PJ = s.eval_policy(pol, 1, J_zero=J.astype(float), report_time=False)
        lhs = np.dot(mu.ravel().astype(float), (PJ.astype(float) - op.mean_cost.astype(float)).ravel())
        rhs = np.dot(op.push(mu).ravel().astype(float), J.ravel().astype(float))
        n_row = int(np.diff(csr[0]).max())
        scale = float(np.sum(np.abs(e.val.astype(float)) * np.abs(mu.ravel()[e.src].astype(float))
                             * np.abs(J.ravel()[e.tgt].astype(float))))
        bound = (n_row + e.S + e.W * e.V) * np.finfo(dt).eps * scale
        print('{} {}: |lhs - rhs| = {:.3e}, bound {:.3e}'.format(case.name, dtkey, abs(lhs - rhs), bound))
        assert abs(lhs - rhs) <= bound
    finally:
        op.close()


STATIONARY_RUNS = (dict(tol=1e-6, n_max=200, check_every=7),       # to a tolerance
                   dict(tol=0.0, n_max=5, check_every=7),          # cut by n_max before the first regular check
                   dict(tol=0.0, n_max=14, check_every=7),         # cut by n_max at a regular check
                   dict(tol=1e-3, n_max=50, check_every=1),        # every push checked
                   dict(tol=1e-5, n_max=40, check_every=7, start=True))        # a given start


@pytest.mark.parametrize('dtkey', sorted(fc.DTYPES))
@pytest.mark.parametrize('case', fc.CASES, ids=CASE_IDS)
def test_stationary_iteration_is_the_numpy_one(gpu, case, dtkey):
    """mu bit for bit, and the same n_done, converged and delta as forward.stationary with the same arguments: every
    model (the host-built operator included), every t_k, both reals"""
    dt = fc.DTYPES[dtkey]
    for t_k in case.times:
        e, csr = definition(case, dtkey, t_k)
        s = case.solver(dt)
        op = s.transition_operator(case.policy(s), t_k)
        start = np.abs(np.random.default_rng(11).standard_normal(e.S)).astype(dt)
        try:
            for run in STATIONARY_RUNS:
                kw = {k: v for k, v in run.items() if k != 'start'}
                want = forward.stationary(csr, e.mean_cost, mu0=start if run.get('start') else None, **kw)
                got = op.stationary(mu0=start.reshape(op.shape) if run.get('start') else None, **kw)
                what = '{} {} t_k={} {}'.format(case.name, dtkey, t_k, run)
                assert got.n_done == want.n_done and got.converged == want.converged, (what, got.n_done, want.n_done)
                assert got.delta == want.delta or (got.delta != got.delta and want.delta != want.delta), what
                assert fc.same(got.mu.ravel(), want.mu), what
                assert got.mu.shape == op.shape
            assert s.backend_info['transition']['pushes'] == got.n_done
        finally:
            op.close()
        kw = dict(tol=1e-3, n_max=50, check_every=1)
        rec = s.stationary_distribution(case.policy(s), t_k, **kw)
        assert fc.same(rec.mu.ravel(), forward.stationary(csr, e.mean_cost, **kw).mu), (case.name, t_k)


def test_untraceable_model_gives_the_traced_operator(gpu):
    """the host path (entries from forward.py, uploaded through sdp_transop_from_coo) and the device path build the
    same operator of the same model"""
    host, dev = fc.BY_NAME['untraceable'], fc.BY_NAME['storage_ar1']
    sh, sd = host.solver(), dev.solver()
    a, b = sh.transition_operator(host.policy(sh)), sd.transition_operator(dev.policy(sd))
    try:
        assert (a.path, b.path) == ('host', 'device')
        assert sh.backend_info['mode'] == 'host entries'
        for x, y in zip(a.tocsr() + (a.mean_cost,), b.tocsr() + (b.mean_cost,)):
            assert fc.same(x, y)
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------------------------------------------------------
# sdp_transop_from_coo alone: the sort, the row build and the push on row shapes no model gives
# ---------------------------------------------------------------------------------------------------------------
def _adversarial(dtype):
    """S = 1000, nnz = 50 000, signed values: row 0 holds 20 000 entries, rows 1..6 exactly 63, 64, 65, 255, 256 and 257,
    rows 800..999 none, the rest at random over rows 7..799; the emission order is a seeded shuffle"""
    S, nnz = 1000, 50000
    rng = np.random.default_rng(42)
    fixed = [(0, 20000)] + list(zip(range(1, 7), (63, 64, 65, 255, 256, 257)))
    tgt = np.concatenate([np.full(n, t) for t, n in fixed])
    tgt = np.concatenate([tgt, rng.integers(7, 800, size=nnz - tgt.size)])
    tgt = rng.permutation(tgt).astype(np.int32)
    src = rng.integers(0, S, size=nnz).astype(np.int32)
    val = rng.standard_normal(nnz).astype(dtype)
    return S, tgt, src, val


@pytest.mark.parametrize('dtkey', sorted(fc.DTYPES))
def test_from_coo_on_adversarial_rows(gpu, dtkey):
    dt = fc.DTYPES[dtkey]
    S, tgt, src, val = _adversarial(dt)
    counts = np.bincount(tgt, minlength=S)
    assert counts[0] == 20000 and list(counts[1:7]) == [63, 64, 65, 255, 256, 257] and (counts[800:] == 0).all()
    order = np.argsort(tgt, kind='stable')
    op = TransitionOperator.from_coo((S,), tgt, src, val)
    try:
        indptr, indices, data = op.tocsr()
        assert np.array_equal(indptr, np.concatenate([[0], np.cumsum(counts)]))
        assert np.array_equal(indices, src[order]) and fc.same(data, val[order])
        assert op.mean_cost is None
        # a wave per row from 8 entries on (what the build sets), from 64, 65 and 256 (the listed rows on either side
        # of the line), for no row at all, and for every row that has an entry: the same bits
        for long_from in (None, 64, 65, 256, 0, 1):
            if long_from is not None:
                op.set_long_rows(long_from)
            for name, mu in fc.vectors(S, dt).items():
                want = np.zeros(S, dtype=dt)
                with np.errstate(all='ignore'):
                    np.add.at(want, tgt, val * mu[src])
                assert fc.same(op.push(mu), want), (name, long_from)
                assert fc.same(op.push(mu, 0), mu), name                    # no step: the vector itself
        op.set_long_rows(8)
        rec = op.stationary(mu0=fc.vectors(S, dt)['uniform'], tol=0.0, n_max=3, check_every=2)
        want = forward.stationary((indptr, indices, data), None, fc.vectors(S, dt)['uniform'], tol=0.0, n_max=3, check_every=2)
        assert rec.n_done == 3 and not rec.converged and rec.average_cost is None
        assert fc.same(rec.mu, want.mu) and (rec.delta == want.delta or rec.delta != rec.delta)
    finally:
        op.close()


def test_from_coo_smallest_operators(gpu):
    one = TransitionOperator.from_coo((1,), [0], [0], np.array([0.5]))
    assert [a.tolist() for a in one.tocsr()] == [[0, 1], [0], [0.5]]
    assert one.push(np.array([3.0]), 2).tolist() == [0.75]
    one.close()
    empty = TransitionOperator.from_coo((5,), [], [], np.zeros(0, dtype=np.float32))
    indptr, indices, data = empty.tocsr()
    assert indptr.tolist() == [0] * 6 and indices.size == 0 and data.size == 0 and data.dtype == np.float32
    out = empty.push(np.ones(5, dtype=np.float32))
    assert out.tolist() == [0.0] * 5 and not np.signbit(out).any()      # an empty row gives +0
    empty.close()


def test_from_coo_refuses_indices_outside_the_grid(gpu):
    lib = gpu.lib()
    val = np.ones(3)
    for tgt, src, word in (([0, 5, 1], [0, 1, 2], 'target'), ([0, 1, 2], [0, -1, 2], 'source'),
                           ([0, 1, 2], [0, 1, 5], 'source')):
        with pytest.raises(ValueError) as err:
            TransitionOperator.from_coo((5,), tgt, src, val)
        assert word in str(err.value) and 'outside [0, 5)' in str(err.value), str(err.value)
    h = C.c_void_p()
    t, s_ = np.array([0, 7], dtype=np.int32), np.array([0, 1], dtype=np.int32)
    assert lib.sdp_transop_from_coo(0, 5, 2, gpu.ptr(t), gpu.ptr(s_), gpu.ptr(val), C.byref(h)) == -1       # SDP_EINVAL
    assert b'entry 1: target 7' in lib.sdp_last_error() and not h.value
    assert lib.sdp_transop_push(None, None, 1) == -1


# ---------------------------------------------------------------------------------------------------------------
# past the launch caps: forward_cases.long_line, sized from the chip's compute units.  The whole grid is compared
# (the definition takes well under a second at this size): every entry, every row pointer, the mean cost; the pushes
# and the stationary iteration against forward.py's sequential sums over those verified entries
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtkey', sorted(fc.DTYPES))
def test_operator_and_pushes_past_the_launch_caps(gpu, dtkey):
    dt = np.dtype(fc.DTYPES[dtkey])
    cus = gpu.device_info(0)['compute_units']
    case = fc.long_line(cus)
    s = case.solver(dt.type)
    pol = case.policy(s)
    e = forward.entries(s, pol)
    csr = forward.csr(e.S, e.tgt, e.src, e.val)
    lengths = np.diff(csr[0])
    assert e.S == cus * 8 * 256 + 129 and e.W == 2 and e.V == 2
    caps = fc.long_line_caps(e.S, len(e.val), lengths, cus, dt.itemsize)
    print(caps)
    for name, (wanted, cap) in caps.items():
        # (k_diff_stats reads 16 bytes a lane: with 4-byte reals its cap is cus * 4096 nodes, and this grid is below it)
        if name != 'k_diff_stats' or dt.itemsize == 8:
            assert wanted > cap, (name, wanted, cap)
    assert lengths.max() < 256                               # (no row of k_push_group<64>)
    second = cus * 8 * 256                                   # the first row of k_push's second trip
    tail = np.zeros(e.S, dtype=dt)
    tail[e.S - 60] = 1.0                                     # what it becomes stays in the rows of the second trips
    vectors = {'random': np.random.default_rng(5).standard_normal(e.S).astype(dt), 'tail': tail}
    op = s.transition_operator(pol)
    try:
        assert op.path == 'device'
        _assert_operator(op, e, csr, 'long_line ' + dtkey)
        assert fc.same(op.mean_cost.ravel(), e.mean_cost)
        want = {(name, n): forward.push(csr, mu, n) for name, mu in vectors.items() for n in (1, 2)}
        assert np.flatnonzero(want['tail', 2]).min() >= second and np.count_nonzero(want['random', 2][second:]) > 100
        for long_from in (None, 1):                          # as built (rows of 8 entries on a group); every row on a group
            if long_from is not None:
                op.set_long_rows(long_from)
            for (name, n), w in want.items():
                assert fc.same(op.push(vectors[name], n), w), (name, n, long_from)
        op.set_long_rows(8)
        for kw in (dict(tol=0.0, n_max=2, check_every=1), dict(tol=0.3, n_max=3, check_every=1)):
            w = forward.stationary(csr, e.mean_cost, mu0=tail, **kw)
            got = op.stationary(mu0=tail, **kw)
            assert w.delta > 0 and got.delta == w.delta, (kw, got.delta, w.delta)      # the largest change is in the tail
            assert got.n_done == w.n_done and got.converged == w.converged and fc.same(got.mu.ravel(), w.mu), kw
    finally:
        op.close()


def test_from_coo_wide_rows_past_the_launch_cap(gpu):
    """k_push_group<64>, one wave a row of 256 entries or more, capped at cus * 64 workgroups of 4 waves: cus * 256 + 129
    rows of exactly 256 entries in a shuffled emission order.  4-byte reals: tgt, src and val take 12 bytes an entry,
    201 MB on 256 CUs; with 8-byte reals they would take 268 MB, over the 256 MiB a test here may use, so that
    instantiation is not reached."""
    dt = np.float32
    cus = gpu.device_info(0)['compute_units']
    S = cus * 256 + 129
    n = S * 256
    assert -(-S // 4) > cus * 64 and n * 12 < 256 << 20                 # past the cap of k_push_group<64>; the arrays' size
    rng = np.random.default_rng(64)
    tgt = rng.permutation(np.repeat(np.arange(S, dtype=np.int32), 256))
    src = rng.integers(0, S, size=n, dtype=np.int32)
    val = rng.standard_normal(n, dtype=dt)
    mu = rng.standard_normal(S, dtype=dt)
    want = np.zeros(S, dtype=dt)
    np.add.at(want, tgt, val * mu[src])                                  # per row in emission order: the stable sort's
    op = TransitionOperator.from_coo((S,), tgt, src, val)
    try:
        indptr, indices, data = op.tocsr()
        assert np.array_equal(indptr, np.arange(S + 1, dtype=np.int64) * 256)
        assert fc.same(op.push(mu), want)                               # (the order within a row decides the roundings)
        assert np.count_nonzero(want[cus * 256:]) == 129                # (the rows of the second trip)
    finally:
        op.close()
