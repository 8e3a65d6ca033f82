"""The table of tests/device_ops.py against the tracer, without a GPU: every operator of trace._OPS has a row, every
spelling the tracer accepts appears, each row traces to the operator it claims (an operator added later without a row
fails here), the rows' classes follow the model's own report, and the interpreted graph gives the callable's bits on the
table's operands."""
import os

import numpy as np
import pytest

import device_ops as D
from stodynprog_amd import trace, codegen, _native as nat
from stodynprog_amd.trace import trace_model, Sym

# what __array_ufunc__ / __array_function__ accept besides the two name tables of trace.py
SPECIAL_UFUNCS = {'power', 'float_power', 'heaviside', 'positive', 'reciprocal', 'logical_and', 'logical_or',
                  'logical_xor', 'bitwise_and', 'bitwise_or', 'bitwise_xor', 'logical_not', 'invert'}
FUNCTIONS = {'where', 'clip', 'interp', 'select'}
PYTHON = {'+', 'r+', '-', 'r-', '*', 'r*', '/', 'r/', '//', 'r//', '%', 'r%', '**', 'r**', 'neg', 'pos', 'abs',
          'lt', 'le', 'gt', 'ge', 'eq', 'ne', '&', '|', '^', '~', '.clip'}


def _trace(fn):
    return trace_model(lambda a, b, u, c: (a, b), lambda a, b, u, c: fn(a, b, c), 2, 1, 1)


def _ops(model):
    return {n.op for n in model.slice_nodes([model.cost])}


def test_every_operator_has_a_row_and_every_row_its_operator():
    reached = set()
    for row in D.ROWS:
        first = _trace(row.spellings[0])
        ops = _ops(first)
        assert row.op in ops, (row.name, row.op, sorted(ops))
        reached |= ops
        for fn in row.spellings[1:]:
            assert _trace(fn).structure_key() == first.structure_key(), row.name
        deps = {n.value for n in first.slice_nodes([first.cost]) if n.op == 'var'}
        assert len(deps) == row.arity and 'u0' not in deps, (row.name, deps)
    assert reached - {'var', 'const', 'bconst'} == set(trace._OPS)


def test_every_accepted_spelling_appears(monkeypatch):
    seen = set()
    ufunc, function = Sym.__array_ufunc__, Sym.__array_function__

    def spy_ufunc(self, uf, method, *inputs, **kw):
        seen.add(uf.__name__)
        return ufunc(self, uf, method, *inputs, **kw)

    def spy_function(self, func, types, args, kwargs):
        seen.add(func.__name__)
        return function(self, func, types, args, kwargs)
    monkeypatch.setattr(Sym, '__array_ufunc__', spy_ufunc)
    monkeypatch.setattr(Sym, '__array_function__', spy_function)
    for row in D.ROWS:
        for fn in row.spellings:
            _trace(fn)
    need = set(trace._UFUNC_BIN) | set(trace._UFUNC_UN) | SPECIAL_UFUNCS | FUNCTIONS
    # (np.mod and np.true_divide are numpy's other names of remainder and divide: the tracer sees the ufunc's own)
    arrives_as = {getattr(np, name).__name__ for name in need}
    assert arrives_as <= seen, sorted(arrives_as - seen)
    named = {n for row in D.ROWS for n in row.names}
    assert need | PYTHON <= named, sorted((need | PYTHON) - named)


def test_row_classes_follow_the_models_report():
    for row in D.ROWS:
        inexact = set(_trace(row.spellings[0]).inexact_ops())
        assert row.exact == (not inexact), (row.name, sorted(inexact))
        if not row.exact:
            assert row.mp is not None and row.domain is not None, row.name
            for dt in row.dtypes:
                assert (row.name, dt) in D.MEASURED_ULPS, (row.name, dt)
    assert not set(D.LEFT_OUT) - {(r.name, dt) for r in D.ROWS if r.exact for dt in r.dtypes}


@pytest.mark.parametrize('dtkey', ['f8', 'f4'])
def test_operands_hold_the_specials(dtkey):
    dt = D.DTYPES[dtkey]
    sp = D.specials(dt)
    fi = np.finfo(dt)
    for v in (0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 2.0 ** fi.nmant - 1, 2.0 ** fi.nmant + 1, float(fi.tiny), float(fi.max),
              float(fi.smallest_subnormal), np.inf, -np.inf, 3.0, -3.0, 5.0, -5.0):
        assert v in sp
    assert np.isnan(sp).sum() == 1 and (np.signbit(sp) & (sp == 0)).sum() == 1
    a, b, c = D.operands(dt)
    assert len(a) == len(sp) ** 3 + D.N_RANDOM
    for v in (a, b, c):
        assert np.array_equal(v.astype(dt).astype(np.float64), v, equal_nan=True)
    # the cross product is full: every pair and triple of specials, so every sign combination of +-3, +-5 with a zero
    # and an infinite divisor among them
    triples = set(zip(*(np.nan_to_num(v[:len(sp) ** 3], nan=123.0, posinf=np.inf, neginf=-np.inf).tolist() for v in (a, b, c))))
    assert len(triples) == (len(sp) - 1) ** 3           # (the two zeros are one key; the signs: test above)


@pytest.mark.parametrize('dtkey', ['f8', 'f4'])
def test_spellings_agree_in_numpy_and_the_graph_gives_the_callables_bits(dtkey):
    """all the spellings of a row are one numpy computation, and (8-byte, exact rows) the interpreted DAG repeats it bit for bit:
    what is left to the GPU test is the C++ spelling alone"""
    ops = D.operands(D.DTYPES[dtkey])
    for unit in D.units(dtkey):
        ref = D.reference(unit, dtkey, ops)
        for k, row in enumerate(unit):
            for fn in row.spellings[1:]:
                other = D.reference([row._replace(spellings=[fn])], dtkey, ops)[0]
                assert D.same_bits(ref[k], other, dtkey).all(), row.name
            if dtkey == 'f8' and row.exact:
                m = _trace(row.spellings[0])
                _, g = trace.evaluate(m, [ops[0], ops[1]], [np.zeros_like(ops[0])], [ops[2]])
                g = np.broadcast_to(np.asarray(g, dtype=np.float64), ref[k].shape)
                assert D.same_bits(ref[k], g, dtkey).all(), row.name


def test_round_to_is_one_correct_rounding():
    import mpmath
    mpmath.mp.prec = 300
    rng = np.random.default_rng(5)
    for dtkey, dt in D.DTYPES.items():
        fi = np.finfo(dt)
        xs = np.concatenate([rng.uniform(-4, 4, 200), [float(fi.max), float(fi.tiny), float(fi.smallest_subnormal) * 3]])
        xs = xs.astype(dt)
        for x in xs:
            up = np.nextafter(x, dt(np.inf))
            lo, hi = mpmath.mpf(float(x)), mpmath.mpf(float(up)) if np.isfinite(up) else mpmath.mpf(2) ** (fi.maxexp)
            mid = (lo + hi) / 2
            assert D.round_to(lo, dtkey) == float(x)
            assert D.round_to(lo + (hi - lo) / 3, dtkey) == float(x)
            assert D.round_to(lo + 2 * (hi - lo) / 3, dtkey) == float(up)
            even = float(x) if (np.asarray(x).view(D.UINT[dtkey]) & 1) == 0 else float(up)
            assert D.round_to(mid, dtkey) == even, (x, dtkey)
        assert D.round_to(mpmath.mpf(float(fi.smallest_subnormal)) / 4, dtkey) == 0.0
        assert D.distance(np.array([1.0], dt), np.nextafter(np.array([1.0], dt), dt(2)), dtkey)[0] == 1
        assert D.distance(np.array([-0.0], dt), np.array([fi.smallest_subnormal], dt), dtkey)[0] == 1


@pytest.mark.skipif(not os.path.exists(nat.HIPCC), reason='hipcc not installed')
@pytest.mark.parametrize('dtkey', ['f8', 'f4'])
def test_units_generate_and_the_first_compiles_for_gfx950(dtkey, tmp_path, monkeypatch):
    sources = []
    for unit in D.units(dtkey):
        solver = D.unit_solver(unit, dtkey)
        model = solver._trace_now(0)
        assert not isinstance(model, trace.TraceError) and model.t_value is None and model.time_dep
        sources.append(D.unit_source(solver))
    assert len(set(sources)) == len(sources)
    monkeypatch.setattr(nat, 'KCACHE', str(tmp_path))
    assert os.path.getsize(nat.compile_model(sources[0])) > 1000


def test_wide_models_are_bit_exact_and_use_the_wider_pool():
    used = set()
    for seed in D.WIDE_SEEDS:
        solver, _ = D.wide_model(seed)
        model = solver._traced()
        assert not isinstance(model, trace.TraceError)
        assert model.bit_exact, (seed, model.inexact_ops())
        used |= {n.op for n in model.live_nodes()}
    assert {'floor', 'ceil', 'rint', 'trunc', 'sign', 'fmin', 'fmax', 'min', 'max', 'b2r', 'and', 'or', 'not',
            'select', 'sqrt', 'square', 'div'} <= used, sorted(used)
