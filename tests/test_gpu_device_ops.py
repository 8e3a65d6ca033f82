"""Every operator of trace._OPS on the device against numpy, value by value (the table of tests/device_ops.py), in
8-byte and 4-byte reals, through DPSolver.simulate with one step per row: exact rows bit for bit on every operand tuple
-- NaN, infinities, signed zeros, denormals, half-way values --, inexact rows by the class of the result and by their
distance from the correctly rounded value (mpmath); then the exact operators inside the sweep families, random models
against oracle/vi_numpy on the same callables."""
import contextlib
import io

import numpy as np
import pytest

import device_ops as D
from oracle import vi_numpy
from stodynprog_amd import codegen
from stodynprog_amd.trace import TraceError

pytestmark = pytest.mark.gpu

_RUNS = {}


def _unit_of(row, dtkey):
    for i, unit in enumerate(D.units(dtkey)):
        if row in unit:
            return i, unit
    raise KeyError(row.name)


def _run(dtkey, i):
    """(operands, device results, numpy results) of unit i: one launch, kept for every row of the unit"""
    key = (dtkey, i)
    if key not in _RUNS:
        ops = _RUNS.setdefault(('operands', dtkey), D.operands(D.DTYPES[dtkey]))
        unit = D.units(dtkey)[i]
        solver = D.unit_solver(unit, dtkey)

        def no_host_path(*a, **kw):
            raise AssertionError('simulate left the device path')
        solver._simulate_host = no_host_path
        B, T = len(ops[0]), len(unit)
        with contextlib.redirect_stdout(io.StringIO()):
            x, u, g = solver.simulate(np.zeros((3, 3, 1)), np.stack([ops[0], ops[1]], axis=1),
                                      np.broadcast_to(ops[2], (T, B)), t0=0)
        try:
            info = solver.backend_info
            assert info['mode'] == 'traced' and not info['time_specialized'], info
            assert g.shape == (T, B) and g.dtype == D.DTYPES[dtkey]
            # the identity dynamics: every operand reached every step as it was sent
            for k in range(T + 1):
                assert D.same_bits(x[k, :, 0], ops[0].astype(g.dtype), dtkey).all()
                assert D.same_bits(x[k, :, 1], ops[1].astype(g.dtype), dtkey).all()
        finally:
            for k in [k for k in solver._cache if k[0] == 'problem']:
                solver._cache.pop(k).close()
        _RUNS[key] = (ops, g, D.reference(unit, dtkey, ops))
    return _RUNS[key]


def _row_results(row, dtkey):
    i, unit = _unit_of(row, dtkey)
    ops, g, ref = _run(dtkey, i)
    k = unit.index(row)
    return ops, g[k], ref[k]


def _show(ops, arity, at):
    return ', '.join('({})'.format(', '.join(repr(float(v[j])) for v in ops[:max(arity, 1)])) for j in at[:6])


EXACT = [(r, dt) for r in D.ROWS if r.exact for dt in r.dtypes]
INEXACT = [(r, dt) for r in D.ROWS if not r.exact for dt in r.dtypes]


def _ids(pairs):
    return ['{}-{}'.format(r.name.replace(' ', '_'), dt) for r, dt in pairs]


@pytest.mark.parametrize('row,dtkey', EXACT, ids=_ids(EXACT))
def test_exact_row_has_numpys_bits_on_every_tuple(gpu, row, dtkey):
    ops, got, ref = _row_results(row, dtkey)
    keep = np.ones(len(got), dtype=bool)
    for tup in D.LEFT_OUT.get((row.name, dtkey), ()):
        hit = np.ones(len(got), dtype=bool)
        for v, t in zip(ops, tup):
            hit &= D.same_bits(v, np.full_like(v, t), 'f8')
        keep &= ~hit
    print('{} {}: {} tuples, {} left out'.format(row.name, dtkey, len(got), int((~keep).sum())))
    bad = np.flatnonzero(~D.same_bits(got, ref, dtkey) & keep)
    assert bad.size == 0, '{} {}: {} of {} tuples differ; operands {} give {} on the device, {} in numpy'.format(
        row.name, dtkey, bad.size, len(got), _show(ops if row.name not in D.OPERAND else (ops[2],), row.arity, bad),
        got[bad[:6]].tolist(), ref[bad[:6]].tolist())


def _class(v):
    """0 for a finite non-zero value; NaN, +-inf and +-0 each a class of their own"""
    c = np.zeros(v.shape, dtype=np.int8)
    c[np.isnan(v)] = 1
    c[np.isinf(v)] = 2
    c[v == 0] = 3
    c[(c > 1) & np.signbit(v)] *= -1
    return c


@pytest.mark.parametrize('row,dtkey', INEXACT, ids=_ids(INEXACT))
def test_inexact_row_has_numpys_result_class(gpu, row, dtkey):
    """wherever numpy's result is NaN, +-inf or +-0 the device's is the same, sign included"""
    ops, got, ref = _row_results(row, dtkey)
    special = _class(ref) != 0
    bad = np.flatnonzero(special & (_class(got) != _class(ref)))
    assert bad.size == 0, '{} {}: {} tuples; operands {} give {} on the device, {} in numpy'.format(
        row.name, dtkey, bad.size, _show(ops if row.name not in D.OPERAND else (ops[2],), row.arity, bad),
        got[bad[:6]].tolist(), ref[bad[:6]].tolist())


def _correctly_rounded(row, dtkey, ops, ref):
    """(indices of the distinct operand tuples inside the row's domain where numpy's result is finite and not zero, the
    correctly rounded results there)"""
    import mpmath
    mpmath.mp.prec = 300
    f = D._mp(row.mp)
    cols = [ops[D.OPERAND.get(row.name, 0)]] if row.arity == 1 else list(ops[:row.arity])
    _, first = np.unique(np.stack(cols).view(np.uint64), axis=1, return_index=True)
    inside, exact = [], []
    dom = row.domain[0]
    for j in np.sort(first):
        args = [float(c[j]) for c in cols]
        if not all(np.isfinite(a) for a in args) or (dom is not None and not dom(*args)):
            continue
        if not np.isfinite(ref[j]) or ref[j] == 0:          # (the class test's business; mpmath has no overflow)
            continue
        try:
            v = f(*[mpmath.mpf(a) for a in args])
        except (ValueError, ZeroDivisionError, OverflowError, mpmath.libmp.ComplexResult):
            continue
        if not isinstance(v, mpmath.mpf) or not mpmath.isfinite(v):
            continue
        if row.mp == 'atan2' and args[0] == 0 and np.signbit(args[0]):
            v = -v                                             # (mpmath has one zero: atan2(-0., x < 0) is -pi)
        r = D.round_to(v, dtkey)
        if r == 0.0 or np.isinf(r):
            continue
        inside.append(j)
        exact.append(r)
    return np.array(inside), np.array(exact, dtype=D.DTYPES[dtkey])


@pytest.mark.parametrize('row,dtkey', INEXACT, ids=_ids(INEXACT))
def test_inexact_row_is_within_its_recorded_distance_of_the_correctly_rounded_value(gpu, row, dtkey):
    ops, got, ref = _row_results(row, dtkey)
    at, exact = _correctly_rounded(row, dtkey, ops, ref)
    assert at.size > 20, (row.name, at.size)
    fin = np.isfinite(got[at]) & np.isfinite(ref[at])
    # (a finite value where the device or numpy overflows: the class test's business when numpy does, an error here
    # when the device alone does)
    assert not (np.isfinite(ref[at]) & ~np.isfinite(got[at])).any(), row.name
    d_dev = D.distance(got[at][fin], exact[fin], dtkey)
    d_np = D.distance(ref[at][fin], exact[fin], dtkey)
    worst = at[fin][int(np.argmax(d_dev))]
    recorded = D.MEASURED_ULPS.get((row.name, dtkey))
    print('ULPS {!r} {} device {} numpy {} over {} tuples ({}); worst at {}; recorded {}'.format(
        row.name, dtkey, int(d_dev.max()), int(d_np.max()), int(fin.sum()), row.domain[1],
        _show(ops if row.name not in D.OPERAND else (ops[2],), row.arity, [worst]), recorded))
    assert recorded is not None, 'no recorded distance for {} {}'.format(row.name, dtkey)
    assert int(d_dev.max()) <= D.ulp_bound(row.name, dtkey), (row.name, dtkey, int(d_dev.max()))


def test_numpy_on_this_host_agrees_with_itself_on_equal_operands(gpu):
    """minimum / maximum / fmin / fmax of zeros of opposite sign come from the CPU's min / max instruction: whatever
    this host's numpy answers, it must answer for a scalar and for arrays of every length and stride alike -- else the
    tuple has no definition and belongs in device_ops.LEFT_OUT.  (On x86-64 the answer is the second operand.)"""
    odd = []
    for dt in (np.float64, np.float32):
        for f in (np.minimum, np.maximum, np.fmin, np.fmax):
            for a, b in ((0.0, -0.0), (-0.0, 0.0), (0.0, 0.0), (-0.0, -0.0)):
                want = np.signbit(f(dt(a), dt(b)))
                for n in (1, 3, 8, 17, 64, 1000):
                    for stride in (1, 2):
                        A, B = np.full(n * stride, a, dt)[::stride], np.full(n * stride, b, dt)[::stride]
                        if not (np.signbit(f(A, B)) == want).all():
                            odd.append((f.__name__, dt.__name__, a, b, n, stride))
                if (a, b) in ((0.0, -0.0), (-0.0, 0.0)) and want != np.signbit(dt(b)):
                    odd.append((f.__name__, dt.__name__, a, b, 'not the second operand'))
    print('tuples on which numpy disagrees with itself:', odd)
    assert not odd, odd


@pytest.mark.parametrize('seed', D.WIDE_SEEDS)
def test_wide_random_models_match_numpy_bit_for_bit(gpu, seed):
    """the fuzz of test_gpu_sweep with the wider pool of exact forms: one sweep against the numpy oracle calling the very
    same callables -- the split emissions of the column and lead units see these operators too"""
    solver, exprs = D.wide_model(seed)
    model = solver._traced()
    assert not isinstance(model, TraceError)
    assert model.bit_exact, model.inexact_ops()
    V = np.random.default_rng(seed).standard_normal((13, 11))
    with np.errstate(all='ignore'):
        J, u = solver.value_iteration(V, report_time=False)
        Jo, uo, io, mo = vi_numpy.value_iteration(vi_numpy.Spec.from_solver(solver), V)
    lead_family = bool(codegen.lead_filter_applies(model, np.float64)) and not model.storage_separable
    permuted = (not lead_family and not model.storage_separable and codegen.lead_order(model, np.float64) is not None)
    lead_family = lead_family or permuted
    assert (solver.backend_info.get('controlled_order') is not None) == permuted
    assert solver.backend_info['kernel'] == ('lead' if lead_family else
                                             ('column' if model.storage_separable else 'generic'))
    assert not solver.backend_info.get('table_per_control')
    assert solver.backend_info['mode'] == 'traced'
    assert np.array_equal(J, Jo, equal_nan=True), exprs
    assert np.array_equal(solver.last_policy_index, io)
    assert np.array_equal(u, uo)
