"""The 4-byte kernels bit for bit against the float32 oracle (oracle/vi_numpy.py, dtype=np.float32: the direct
kernel's definition restated in numpy float32, one correctly rounded operation per operator on both sides).

The cases are the table tests/fp32_cases.py.  Per case, for every kernel it runs in -- always the direct kernel
(kernel='generic': the yardstick of the other 4-byte tests, itself never checked before), and the family 'auto' or a
named kernel plans, with and without its filter -- J, the policy index and the policy values of one sweep equal the
oracle's with np.array_equal, from three cost-to-go arrays: standard normal, smooth, and one with NaN and +-inf.  On
every node up to 20 000 nodes, above that on column_forms.sample_nodes plus 2 000 random nodes.  No tolerance
appears in this file.

Beyond one sweep: three sweeps chained on the device against three oracle sweeps; eval_policy for 5 steps with and
without the relative-DP shift for the policy kinds of tests/policies.py; bellman_recursion of the time-dependent model."""
import contextlib
import io

import numpy as np
import pytest

import fp32_cases as fc
import policies
from oracle import vi_numpy
from stodynprog_amd import models

pytestmark = pytest.mark.gpu
F32 = np.float32


def _quiet(f, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all='ignore'):
        return f(*a, **kw)


def _close(*solvers):
    for s in solvers:
        for k in [k for k in s._cache if k[0] == 'problem']:
            s._cache.pop(k).close()


def _differ(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return int((~((a == b) | ((a != a) & (b != b)))).sum())


def _equal(got, want, what):
    """J, policy values and policy index: the oracle's bits (NaN where the oracle has NaN)"""
    for g, w, name in zip(got, want, ('J', 'policy values', 'policy index')):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        if name != 'policy index':
            assert g.dtype == F32 and w.dtype == F32, (what, name, g.dtype, w.dtype)
        assert np.array_equal(g, w, equal_nan=(name != 'policy index')), \
            '{}: {} differs from the float32 oracle at {} of {} entries'.format(what, name, _differ(g, w), g.size)


def _at(out, nodes):
    J, pol, idx = (np.asarray(a) for a in out)
    if nodes is None:
        return J, pol, idx
    return J.ravel()[nodes], pol.reshape(-1, pol.shape[-1])[nodes], idx.ravel()[nodes]


def _oracle(spec, V, nodes, t_k=None):
    with np.errstate(all='ignore'):
        J, pol, idx, _ = vi_numpy.value_iteration(spec, V, nodes=nodes, t_k=t_k, dtype=F32)
    return J, pol, idx


def _sweep(s, V):
    J, pol = _quiet(s.value_iteration, V, report_time=False)
    return J, pol, np.asarray(s.last_policy_index)


def _inputs(ref, seed):
    """standard normal, smooth (the closed form of the benchmark on its model, policies.smooth_value elsewhere), and
    the normal one with NaN and +-inf: float32 arrays, rounded once here for both sides"""
    shape = ref._state_grid_shape
    normal = np.random.default_rng(seed).standard_normal(shape).astype(F32)
    if ref.sys.name == models.synthetic3d(N=8)[0].name:
        smooth = models.synthetic3d_V0(ref.state_grid, F32)
    else:
        smooth = policies.smooth_value(ref).astype(F32)
    return [('normal V', normal, True), ('smooth V', smooth, True), ('NaN / inf V', fc.special_values(normal), False)]


def _with_special_nodes(nodes, special):
    """a sample of nodes, and up to 300 of the nodes where `special` is NaN or +-inf with it (their neighbours' next
    states read them): every input of a case is compared on the same nodes"""
    if nodes is None:
        return None
    bad = np.flatnonzero(~np.isfinite(special.ravel()))
    return np.unique(np.concatenate([nodes, bad[::max(1, len(bad) // 300)]]))


def _run_checks(case, run, s):
    info = s.backend_info
    want = {'generic': 'generic', 'staged': 'staged'}.get(run.family, 'column')
    assert info['kernel'] == want, (case, run, info['kernel'])
    if run.family == 'table per control':
        assert info['table_per_control'], (case, run)
    if run.filtered is not None:
        assert bool(info['certified_filter']) == run.filtered, (case, run, info['certified_filter'])
    assert s.dtype == F32 and info['bit_exact_model'] and not info['inexact_ops'], (case, run, info['inexact_ops'])
    assert not fc.unmet(case, run, fc.plan_of(s)), fc.unmet(case, run, fc.plan_of(s))


def _case_sweeps(case, seed):
    ref = case.reference()
    spec = vi_numpy.Spec.from_solver(ref)
    inputs = _inputs(ref, seed)
    nodes = _with_special_nodes(fc.nodes_of(ref._state_grid_shape, seed), inputs[2][1])
    want = [_oracle(spec, V, nodes) for _, V, _ in inputs]
    for (label, V, finite), w in zip(inputs, want):
        if not finite and nodes is None:        # (on a sample the special entries may lie between the sampled nodes' reads)
            assert np.isnan(w[0]).any() or np.isinf(w[0]).any(), (case, 'the special values reach no node')
    chain = None
    if case.chain:
        assert nodes is None
        J = inputs[1][1]
        for _ in range(3):
            chain = _oracle(spec, J, None)
            J = chain[0]
    for run in case.runs:
        s = case.solver(run)
        try:
            for (label, V, _), w in zip(inputs, want):
                _equal(_at(_sweep(s, V), nodes), w, '{} in {}, {}'.format(case, run, label))
                _run_checks(case, run, s)
            if chain is not None:
                J3, pol3 = _quiet(s.value_iterations, inputs[1][1], 3, report_time=False)
                _equal((J3, pol3, np.asarray(s.last_policy_index)), chain, '{} in {}, 3 chained sweeps'.format(case, run))
        finally:
            _close(s)
    return ref, spec, inputs


def _case_policies(case, ref, spec, inputs):
    """eval_policy for 5 steps, plain and with the relative-DP shift (every step's reference cost), per policy kind"""
    J0 = (inputs[1][1] * F32(0.1)).astype(F32)
    for kind in case.policies:
        gen = case.solver(fc.GENERIC if fc.GENERIC in case.runs else case.runs[0])
        pol = _quiet(policies.policy, gen, kind, seed=3).astype(F32)
        _close(gen)
        with np.errstate(all='ignore'):
            plain = vi_numpy.eval_policy(spec, pol, 5, False, J0, dtype=F32)
            rel, refs = vi_numpy.eval_policy(spec, pol, 5, True, J0, J_ref_full=True, dtype=F32)
        for run in case.runs:
            s = case.solver(run)
            try:
                what = '{} in {}, eval_policy of a {} policy'.format(case, run, kind)
                E = _quiet(s.eval_policy, pol, 5, False, J0, report_time=False)
                assert E.dtype == F32 and np.array_equal(E, plain, equal_nan=True), \
                    '{}: J differs at {} of {} nodes'.format(what, _differ(E, plain), E.size)
                Er, r = _quiet(s.eval_policy, pol, 5, True, J0, report_time=False, J_ref_full=True)
                assert Er.dtype == F32 and np.array_equal(Er, rel, equal_nan=True), \
                    '{} with rel_dp: J differs at {} of {} nodes'.format(what, _differ(Er, rel), Er.size)
                assert np.array_equal(np.asarray(r, dtype=float), refs, equal_nan=True), (what, r, refs)
            finally:
                _close(s)


@pytest.mark.timeout(600)
@pytest.mark.parametrize('case', fc.CASES, ids=[c.name for c in fc.CASES])
def test_float32_kernels_equal_the_float32_oracle_bit_for_bit(gpu, case):
    ref, spec, inputs = _case_sweeps(case, seed=fc.CASES.index(case))
    _case_policies(case, ref, spec, inputs)


# 512^3: three uploads and sweeps per kernel and 3 x 20 000 oracle nodes; the limit ends a hang, it is no performance bar
@pytest.mark.timeout(1500)
def test_config5_512cubed_equals_the_float32_oracle_on_the_sampled_nodes(gpu):
    """BASELINE config 5 at full size on the 20 000 nodes of test_fp32_512cubed_against_fp64_oracle
    (tests/test_gpu_sweep.py), the column kernel and the direct kernel"""
    case = fc.CONFIG5
    ref = case.reference()
    spec = vi_numpy.Spec.from_solver(ref)
    shape = ref._state_grid_shape
    inputs = _inputs(ref, 5)
    nodes = _with_special_nodes(np.unique(np.random.default_rng(9).integers(0, int(np.prod(shape)), 20000)), inputs[2][1])
    want = [_oracle(spec, V, nodes) for _, V, _ in inputs]
    for run in case.runs:
        s = case.solver(run)
        try:
            for (label, V, _), w in zip(inputs, want):
                _equal(_at(_sweep(s, V), nodes), w, '{} in {}, {}'.format(case, run, label))
                _run_checks(case, run, s)
        finally:
            _close(s)


@pytest.mark.parametrize('T', [3, 11])
def test_bellman_recursion_in_float32_equals_the_oracle_step_by_step(gpu, T):
    """the time-dependent model (models.finite_horizon): the time index reaches dyn and cost as float32(t_k), the box
    of step t_k is the host's in float64, rounded once"""
    _, fh = models.finite_horizon()
    s = policies.as_dtype(fh, F32)
    spec = vi_numpy.Spec.from_solver(fh)
    J_fin = policies.smooth_value(fh).astype(F32)
    try:
        J, pol = _quiet(s.bellman_recursion, T, J_fin)
    finally:
        _close(s)
    nxt = J_fin
    for t in range(T)[::-1]:
        Jo, po, _ = _oracle(spec, nxt, None, t_k=t)
        assert np.array_equal(J[t].astype(F32), Jo, equal_nan=True) and np.array_equal(J[t].astype(F32).astype(float), J[t]), t
        assert np.array_equal(pol[t].astype(F32), po), t
        nxt = Jo
