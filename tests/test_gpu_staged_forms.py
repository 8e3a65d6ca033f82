"""Every chunk form of the LDS-staged tile kernel that the planner gives (csrc/sdp_staged_kernel.h; the table
tests/staged_forms.py: cu = 4, 2, 1; cw = W, a divisor of W, ragged; one to four state variables; both real types; no
perturbation; two controls; a per-node box; folded dynamics; boxes that fit, are cut on the leading axes, are cut down
to the last axis, or are not staged at all) on the device against the direct kernel (kernel = 'generic', which stages
nothing) on every node and against the numpy oracle (oracle/vi_numpy.py through Spec.from_solver; in float32 for the
4-byte runs) on the case's sample, bit for bit: every comparison of results is np.array_equal, with NaN equal to NaN
where NaN is put in; no tolerance appears in this file.  tests/test_staged_forms_plan.py checks on the CPU that each
case plans what it claims and that its chunks and staging paths are what the table says.

Per case and real type: one sweep from a smooth and from a random input; three chained sweeps with the value array
resident, with and without the relative-DP shift; +inf, -inf and NaN written where `Reach` places staged boxes and just
past their cuts.  Once: the host-array path and a two-step finite-horizon recursion on a case with cw < W (the staged
rows of tests/horizon_cases.py plan cw = W = 5: checked in tests/test_staged_forms_plan.py).

That the file can fail was seen with two arithmetic-only edits of the kernel on a scratch copy.  With acc[] zeroed at the
start of every w chunk, every run with cw < W fails (16 runs, in all three per-run tests, and the two single tests)
except the two of `budget_32`, where every control of every node misses a box and is summed again from global memory.
With outside[] cleared at the start of every w chunk, every run that claims early misses fails (9 runs).  Of the older
tests/test_gpu_staged.py only test_box_larger_than_the_lds_budget_is_cut_not_wrong notices either edit (its 2048-byte
budget plans cw < W); nothing at the natural budget did."""
import contextlib
import io

import numpy as np
import pytest

import staged_forms as sf
from stodynprog_amd import codegen

pytestmark = pytest.mark.gpu


def _quiet(f, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all='ignore'):
        return f(*a, **kw)


def _close(*solvers):
    for s in solvers:
        for k in [k for k in s._cache if k[0] == 'problem']:
            s._cache.pop(k).close()


def _same(got, want, what, nan=False):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.dtype.kind == 'f':
        assert got.dtype == want.dtype, (what, got.dtype, want.dtype)
    if not np.array_equal(got, want, equal_nan=nan):
        bad = ~((got == want) | ((got != got) & (want != want)))
        where = np.flatnonzero(bad.reshape(-1))
        raise AssertionError('{}: differs at {} of {} entries, first at flat index {}: {!r} / {!r}'.format(
            what, int(bad.sum()), got.size, int(where[0]), got.reshape(-1)[where[0]], want.reshape(-1)[where[0]]))


def _pair(case, rs, monkeypatch):
    """the staged and the direct solver of a run, under the case's budget"""
    if case.budget is not None:
        monkeypatch.setattr(codegen, 'STAGED_LDS_BYTES', case.budget)
    return case.solver(rs), case.solver(rs, 'generic')


def _is_claimed(s, case, rs):
    """the unit that ran is the one the table claims"""
    info = s.backend_info
    assert info['mode'] == 'traced' and info['kernel'] == 'staged', info
    assert info['staged'] == case.plan(rs, len(s._shape())), (case, rs, info['staged'])
    assert info['bit_exact_model'] and not info['inexact_ops'], info


def _input(case, rs, which, s):
    return sf.inputs(s._shape())[which].astype(sf.REALS[rs])


def _result(s, out, rel_dp=False):
    J, pol = out
    ref = None
    if rel_dp:
        J, ref = J
    return np.asarray(J), np.asarray(pol), np.asarray(s.last_policy_index), ref


def _compare(a, b, what, nan=False):
    _same(a[0], b[0], what + ': J', nan)
    _same(a[1], b[1], what + ': policy values', nan)
    _same(a[2], b[2], what + ': policy index')
    assert (a[3] is None and b[3] is None) or np.array_equal(np.asarray(a[3], dtype=float), np.asarray(b[3], dtype=float),
                                                              equal_nan=nan), (what, a[3], b[3])


@pytest.mark.parametrize('case,rs', sf.RUNS, ids=sf.RUN_IDS)
def test_one_sweep_equals_the_direct_kernel_and_the_oracle(gpu, monkeypatch, case, rs):
    stg, gen = _pair(case, rs, monkeypatch)
    S = int(np.prod(stg._shape()))
    try:
        for which in sf.INPUTS:
            what = '{} f{} {}'.format(case, rs, which)
            V = _input(case, rs, which, stg)
            a = _result(stg, _quiet(stg.value_iterations, V, 1, report_time=False))
            _is_claimed(stg, case, rs)
            b = _result(gen, _quiet(gen.value_iterations, V, 1, report_time=False))
            assert gen.backend_info['kernel'] == 'generic' and gen.backend_info['staged'] is None
            _compare(a, b, what + ', staged / direct kernel')
            nodes, Jo, polo, idxo = sf.oracle(case.name, rs, which)
            for name, r in (('staged', a), ('direct kernel', b)):
                _same(r[0].ravel()[nodes], Jo, '{}, {} / oracle: J'.format(what, name))
                _same(r[2].ravel()[nodes], idxo, '{}, {} / oracle: policy index'.format(what, name))
                _same(r[1].reshape(S, -1)[nodes], polo, '{}, {} / oracle: policy values'.format(what, name))
    finally:
        _close(stg, gen)


@pytest.mark.parametrize('case,rs', sf.RUNS, ids=sf.RUN_IDS)
def test_chained_sweeps_equal_the_direct_kernel(gpu, monkeypatch, case, rs):
    """three sweeps with the value array resident, with and without the relative-DP shift"""
    stg, gen = _pair(case, rs, monkeypatch)
    try:
        V = _input(case, rs, 'random', stg)
        ref = stg._state_ref_ind
        for rel_dp in (False, True):
            J0 = ((V - V[ref]).astype(V.dtype), 0.) if rel_dp else V
            kw = dict(rel_dp=rel_dp, report_time=False, J_ref_full=True)
            a = _result(stg, _quiet(stg.value_iterations, J0, 3, **kw), rel_dp)
            _is_claimed(stg, case, rs)
            b = _result(gen, _quiet(gen.value_iterations, J0, 3, **kw), rel_dp)
            assert gen.backend_info['kernel'] == 'generic'
            _compare(a, b, '{} f{} rel_dp={}, sweep 3'.format(case, rs, rel_dp))
            assert np.isfinite(a[0]).all() and (not rel_dp or (a[0][ref] == 0 and len(a[3]) == 3))
    finally:
        _close(stg, gen)


@pytest.mark.parametrize('case,rs', sf.RUNS, ids=sf.RUN_IDS)
def test_special_values(gpu, monkeypatch, case, rs):
    """+inf, -inf and NaN, each on its own, in the input at vertices that `Reach` sees read from staged boxes of every
    path the case claims, and at vertices that cells which missed their box read from global memory (the nodes of cut
    tiles): the staged copy carries them like the direct kernel's loads (cf. tests/test_gpu_lead.py::test_special_values)"""
    stg, gen = _pair(case, rs, monkeypatch)
    r = sf.reach(case.name, rs)
    spots = []
    for path in case.paths[rs]:
        spots += r.read_vertices[path] + r.missed_vertices[path]
    spots = sorted(set(spots))
    assert spots
    try:
        base = _input(case, rs, 'random', stg)
        for value in (np.inf, -np.inf, np.nan):
            V = base.copy()
            V.reshape(-1)[spots] = value
            assert not np.isfinite(V).all()
            a = _result(stg, _quiet(stg.value_iterations, V, 1, report_time=False))
            _is_claimed(stg, case, rs)
            b = _result(gen, _quiet(gen.value_iterations, V, 1, report_time=False))
            _compare(a, b, '{} f{} with {} at {} nodes'.format(case, rs, value, len(spots)), nan=True)
            assert not np.isfinite(b[0]).all(), (case, rs, value, 'the special value reaches no node')
    finally:
        _close(stg, gen)


def _smallest_with_several_boxes():
    runs = [(int(np.prod(c.solver()._shape())), c) for c in sf.CASES if 'boxes' in c.claimed(8) and c.budget is None]
    return min(runs, key=lambda sc: sc[0])[1]


def test_the_host_array_path_with_several_boxes(gpu, monkeypatch):
    """value_iteration on numpy arrays (one library call, arrays through page-locked memory) on a case with cw < W,
    with and without the relative-DP shift, against the resident path and the direct kernel.  (The phased branch of
    that call needs 8 MiB of values: tests/test_gpu_staged.py runs it at 112^3 nodes, which plan (4, W).)"""
    case = _smallest_with_several_boxes()
    assert case.plans[8][1] < sf.reach(case.name, 8).W
    stg, gen = _pair(case, 8, monkeypatch)
    try:
        V = _input(case, 8, 'random', stg)
        ref = stg._state_ref_ind
        for rel_dp in (False, True):
            J0 = (V - V[ref], 0.) if rel_dp else V
            a = _result(stg, _quiet(stg.value_iteration, J0, rel_dp=rel_dp, report_time=False), rel_dp)
            _is_claimed(stg, case, 8)
            b = _result(gen, _quiet(gen.value_iteration, J0, rel_dp=rel_dp, report_time=False), rel_dp)
            c = _result(stg, _quiet(stg.value_iterations, J0, 1, rel_dp=rel_dp, report_time=False), rel_dp)
            _compare(a, b, '{}: value_iteration, rel_dp={}, staged / direct kernel'.format(case, rel_dp))
            _compare(a, c, '{}: value_iteration / value_iterations, rel_dp={}'.format(case, rel_dp))
    finally:
        _close(stg, gen)


def test_a_finite_horizon_with_several_boxes(gpu, monkeypatch):
    """two steps of bellman_recursion on the smallest case with cw < W against the direct kernel"""
    case = _smallest_with_several_boxes()
    stg, gen = _pair(case, 8, monkeypatch)
    try:
        J_fin = _input(case, 8, 'smooth', stg)
        Ja, pa = _quiet(stg.bellman_recursion, 2, J_fin, report_time=False)
        _is_claimed(stg, case, 8)
        Jb, pb = _quiet(gen.bellman_recursion, 2, J_fin, report_time=False)
        assert gen.backend_info['kernel'] == 'generic' and Ja.shape == (2,) + J_fin.shape
        _same(Ja, Jb, '{}: bellman_recursion J'.format(case))
        _same(pa, pb, '{}: bellman_recursion policy'.format(case))
        assert not np.array_equal(Ja[0], Ja[1])
    finally:
        _close(stg, gen)
