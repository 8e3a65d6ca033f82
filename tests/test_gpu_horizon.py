"""Finite-horizon recursion (bellman_recursion of a time-dependent system) in every kernel family and at the shapes of
the column forms: tests/horizon_cases.py.  Over one horizon the control box, and with it the lattice, changes from
step to step -- 1 control, fewer than 8, 8 m + 1, 2^p, 2^p - 1 and 2^p + 1 --, so the kernels run with fewer
controls than their control table holds; the stock drifts, the exogenous process and a cost coefficient of a control
term move with the time index.  At every step k, from the kernel's own J[k + 1]:

- J, policy values and indices are bit for bit those of the same family without the filter (the long way) and of the
  direct kernel (kernel='generic');
- 8-byte reals equal the numpy oracle evaluated at step k bit for bit (indices exact or proved ties), on every node of
  the small grids and on column_forms.sample_nodes of the large ones; 4-byte reals are within 1e-5 of it from a smooth
  J_fin, with indices exact where the fp64 margin exceeds fp32 resolution;
- backend_info names the claimed family, the unit that ran carries the claimed capacity, the horizon compiles the
  claimed number of code objects, and the problem of each step evicts the previous one.

The held-tail cases also run from a J_fin with NaN blocks and inf rows, bit for bit against the other two kernels."""
import contextlib
import io

import numpy as np
import pytest

import column_forms as cf
import horizon_cases as hc
from conftest import assert_sweep_parity
from oracle import vi_numpy
from policies import smooth_value
from stodynprog_amd import codegen, _native as nat

pytestmark = pytest.mark.gpu


def _quiet(f, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all='ignore'):
        return f(*a, **kw)


def _problems(s):
    return [k for k in s._cache if k[0] == 'problem']


def _close(*solvers):
    for s in solvers:
        for k in _problems(s):
            s._cache.pop(k).close()


def _horizon(s, T, J_fin, compiled):
    """bellman_recursion of `s`; per step k: backend_info, the policy index and the source key of the unit that ran.
    `compiled`: the list nat.compile_model appends to (only this solver's compilations are kept)"""
    steps = {}
    real = s._backup

    def backup(J_next, t_k, rel_dp):
        out = real(J_next, t_k, rel_dp)
        keys = _problems(s)
        steps[t_k] = dict(info=dict(s.backend_info), idx=np.array(s.last_policy_index),
                          skeys=[k[3] for k in keys])
        return out
    s._backup = backup
    compiled.clear()
    compiled.append(True)
    try:
        J, pol = _quiet(s.bellman_recursion, T, J_fin)
    finally:
        del s._backup
        compiled.remove(True)
    return J, pol, steps, list(compiled)


def _one_step(s, J_next, k):
    J, pol, _ = _quiet(s._backup, np.asarray(J_next), k, False)
    return J, pol, np.array(s.last_policy_index)


def _same(a, b, what):
    assert np.array_equal(a[0], b[0], equal_nan=True), what + ': J differs'
    assert np.array_equal(a[2], b[2]), what + ': policy index differs'
    assert np.array_equal(a[1], b[1], equal_nan=True), what + ': policy differs'


@pytest.fixture
def compiled(monkeypatch):
    """sources nat.compile_model is asked for while the list holds a True (the solver under test)"""
    out = []
    real = nat.compile_model
    monkeypatch.setattr(nat, 'compile_model',
                        lambda src, **k: (out.append(src) if True in out else None) or real(src, **k))
    return out


def _check_oracle(s, J_next, k, got, nodes, what, dtype, finite=True):
    """step k of `s` from J_next (`got` = (J, pol, idx)) against the numpy oracle at step k"""
    spec = vi_numpy.Spec.from_solver(s)
    V64 = np.asarray(J_next, dtype=np.float64)
    J, pol, idx = (np.asarray(a) for a in got)
    if nodes is None:
        Jo, po, io_, mo = vi_numpy.value_iteration(spec, V64, t_k=k)
        J, idx, pol = J.ravel(), idx.ravel(), pol.reshape(-1, pol.shape[-1])
        Jo, io_, mo, po = Jo.ravel(), io_.ravel(), mo.ravel(), po.reshape(-1, po.shape[-1])
    else:
        Jo, po, io_, mo = vi_numpy.value_iteration(spec, V64, t_k=k, nodes=nodes)
        J, idx = J.ravel()[nodes], idx.ravel()[nodes]
        pol = pol.reshape(-1, pol.shape[-1])[nodes]
    if np.dtype(dtype).itemsize == 8:
        assert np.array_equal(J, Jo, equal_nan=True), '{}: J differs from the oracle at {} of {} nodes'.format(
            what, int((~((J == Jo) | (np.isnan(J) & np.isnan(Jo)))).sum()), J.size)
        if finite:
            assert_sweep_parity(J, idx, Jo, io_, mo, what, prove=(s, V64, k), nodes=nodes)
            same = idx == io_
            assert np.array_equal(pol[same], po[same]), what + ': policy values differ from the oracle'
        else:
            assert np.array_equal(idx, io_), what + ': policy index differs from the oracle'
        return
    # 4-byte reals: bit for bit the float32 oracle at step k, next to the bar against the 8-byte one
    with np.errstate(all='ignore'):
        J32, p32, i32, _ = vi_numpy.value_iteration(spec, np.asarray(J_next, dtype=np.float32), t_k=k, nodes=nodes,
                                                    dtype=np.float32)
    assert np.array_equal(J, J32.ravel(), equal_nan=True), what + ': J differs from the float32 oracle'
    assert np.array_equal(idx, i32.ravel()), what + ': policy index differs from the float32 oracle'
    assert np.array_equal(pol, p32.reshape(-1, p32.shape[-1]), equal_nan=True), what + ': policy differs from the float32 oracle'
    rel = np.abs(J - Jo).max() / np.abs(Jo).max()
    assert rel < 1e-5, (what, rel)
    clear = mo > 1e-5 * np.maximum(1.0, np.abs(Jo))
    assert (idx[clear] == io_[clear]).all(), what + ': index differs where the fp64 margin exceeds fp32 resolution'


def _per_step_plan_checks(fam_or_case, steps, sources, T, claim_info, claim_utab, what):
    """backend_info at every step, the unit that ran and its capacity, the code objects of the horizon"""
    by_key = {codegen.source_key(src): src for src in sources}
    for k in range(T):
        st = steps[k]
        for key, v in claim_info.items():
            assert st['info'].get(key) == v, (what, k, key, st['info'])
        assert len(st['skeys']) == 1, (what, k, 'problems held', len(st['skeys']))
        src = by_key.get(st['skeys'][0])
        assert src is not None, (what, k, 'the unit that ran was not compiled for this horizon')
        if claim_utab is not None:
            assert cf.macro(src, 'SDP_COL_UTAB_N') == claim_utab(k), (what, k, cf.macro(src, 'SDP_COL_UTAB_N'))
    assert len(set(sources)) == fam_or_case.units, (what, 'code objects', len(set(sources)))


@pytest.mark.timeout(600)
@pytest.mark.parametrize('fam', hc.FAMILIES, ids=[f.name for f in hc.FAMILIES])
def test_family_horizon_against_the_other_kernels_and_the_oracle(gpu, compiled, fam):
    s = fam.solver()
    others = {label: fam.solver(**kw) for label, kw in fam.compared().items()}
    try:
        shape = s._state_grid_shape
        if fam.ref == 'oracle32':
            J_fin = smooth_value(s)
        else:
            J_fin = np.random.default_rng(11).standard_normal(shape)
        J_fin = J_fin.astype(s.dtype).astype(float)
        J, pol, steps, sources = _horizon(s, hc.T, J_fin, compiled)
        assert sorted(steps) == list(range(hc.T))
        if fam.form == 'tabulated':
            assert all(st['info']['mode'] == 'tabulated' for st in steps.values())
        else:
            utab = (lambda k: str(hc.capacity(fam.sizes[k]))) if fam.table else None
            _per_step_plan_checks(fam, steps, sources, hc.T, fam.info, utab, fam.name)
            assert len(_problems(s)) <= 1
        # (flat ids of (n0, n1, 1) are those of (n0, n1))
        nodes = cf.sample_nodes(shape + (1,) * (3 - len(shape)), n=300) if fam.ref == 'oracle sampled' else None
        for k in range(hc.T - 1, -1, -1):
            J_next = J_fin if k == hc.T - 1 else J[k + 1]
            mine = (J[k], pol[k], steps[k]['idx'])
            what = '{} step {} ({} controls)'.format(fam, k, fam.sizes[k])
            for label, o in others.items():
                _same(mine, _one_step(o, J_next, k), '{}: vs {}'.format(what, label))
                if fam.info.get('kernel') and label == 'long way':
                    assert not o.backend_info['certified_filter'], o.backend_info
                if label == 'direct kernel':
                    assert o.backend_info['kernel'] == 'generic'
            _check_oracle(s, J_next, k, mine, nodes, what, s.dtype)
    finally:
        _close(s, *others.values())


def _special_values(V):
    """(tests/test_gpu_column_forms.py) a NaN block inside some columns, whole columns of +inf from some row on"""
    n0, n1, n2 = V.shape
    V = V.copy()
    V[n0 // 3:n0 // 3 + 9, 1:3, n2 // 2:n2 // 2 + 2] = np.nan
    V[n0 - 1, n1 // 2, 0] = np.nan
    V[(3 * n0) // 4:, n1 - 2, 1:4] = np.inf
    V[:5, n1 // 2 + 1, n2 - 1] = np.inf
    return V


@pytest.mark.timeout(600)
@pytest.mark.parametrize('case,geometry', hc.PAIRS, ids=['{}-{}'.format(c.name, g) for c, g in hc.PAIRS])
def test_column_form_horizon_against_the_other_kernels_and_the_oracle(gpu, compiled, debug_defines, case, geometry):
    if case.debug:
        debug_defines.set(**case.debug)
    T = len(case.sizes)
    s = case.solver(geometry)
    long_ = case.solver(geometry, certified_filter=False)
    gen = case.solver(geometry, kernel='generic')
    try:
        shape = s._state_grid_shape
        nodes = cf.sample_nodes(shape, n=300, seed=len(case.name))
        f32 = case.dtype.itemsize == 4
        J_fin = smooth_value(s) if f32 else np.random.default_rng(2000 + case.form.n0).standard_normal(shape)
        J_fin = J_fin.astype(case.dtype).astype(float)
        inputs = [('seeded', J_fin)]
        if case.hold:
            inputs.append(('NaN / inf', _special_values(J_fin)))
        for label, Jf in inputs:
            J, pol, steps, sources = _horizon(s, T, Jf, compiled)
            info = dict(kernel='column', certified_filter=True, time_specialized=False)
            _per_step_plan_checks(case, steps, sources, T, info, lambda k: case.claims(geometry)['SDP_COL_UTAB_N'],
                                  '{} {} {}'.format(case, geometry, label))
            src = sources[0]
            assert not [m for m, v in case.claims(geometry).items() if cf.macro(src, m) != v]
            assert cf.hold_geometry(src) == case.hold
            for k in range(T - 1, -1, -1):
                J_next = Jf if k == T - 1 else J[k + 1]
                mine = (J[k], pol[k], steps[k]['idx'])
                what = '{} {} {} step {} ({} controls)'.format(case, geometry, label, k, case.sizes[k])
                _same(mine, _one_step(long_, J_next, k), what + ': vs the long way')
                assert long_.backend_info['kernel'] == 'column' and not long_.backend_info['certified_filter']
                _same(mine, _one_step(gen, J_next, k), what + ': vs the direct kernel')
                assert gen.backend_info['kernel'] == 'generic'
                if label == 'seeded':
                    _check_oracle(s, J_next, k, mine, nodes, what, case.dtype)
            assert len(_problems(s)) <= 1
    finally:
        _close(s, long_, gen)
