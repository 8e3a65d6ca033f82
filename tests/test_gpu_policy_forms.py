"""eval_policy and policy_iteration with the policies a user may hand them (tests/policies.py: on the lattice, smooth
off the lattice, reaching beyond the box, uniform at random per node, with NaN and infinities), in every form of the
column family (tests/column_forms.py) and every family of the parameter study (tests/policies.FAMILIES).

For every run, eval_policy(pol, 3, rel_dp, J_zero=V, J_ref_full) from a standard-normal V and eval_policy(pol, 2):

- J and every J_ref are bit for bit those of the direct kernel (kernel='generic', csrc/sdp_sweep_kernel.h
  sdp_evalpol) on the same problem, on all nodes;
- 8-byte reals: bit for bit the numpy oracle (oracle/vi_numpy.eval_policy) on all nodes.  Where the grid is too big
  for the vectorised oracle (the 'many' geometry: 2^22 nodes x 32 perturbation points), a single step from V is
  compared with it on sampled nodes instead (rows 0 and n0 - 1, the last column, the split boundaries);
- 4-byte reals: from a smooth cost-to-go (policies.smooth_value), within the bar of
  test_fp32_512cubed_against_fp64_oracle (1e-5 of the largest |J|) of the fp64 oracle on finite entries, with NaN and
  infinities in the same places.  (From the standard-normal V the 4-byte rounding of the next state, about 6e-8 of
  the axis, moves J by the slope of V, up to 2.5e-5 of the largest |J| at 512 to 1024 rows: bit parity with the
  direct kernel is checked there, the oracle is not);
- backend_info names the family or form the case claims."""
import contextlib
import io

import numpy as np
import pytest

import column_forms as cf
import policies as P
from oracle import vi_numpy

pytestmark = pytest.mark.gpu

ORACLE_POINTS = 1 << 21          # nodes x perturbation points the whole-grid oracle is run on


def _quiet(f, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all='ignore'):
        return f(*a, **kw)


def _evals(s, pol, V):
    J3, ref3 = _quiet(s.eval_policy, pol, 3, True, V, report_time=False, J_ref_full=True)
    J2 = _quiet(s.eval_policy, pol, 2, report_time=False)
    return J3, np.atleast_1d(ref3), J2


def _oracle_evals(s, pol, V):
    spec = vi_numpy.Spec.from_solver(s)
    with np.errstate(all='ignore'):
        J3, ref3 = vi_numpy.eval_policy(spec, pol, 3, True, np.array(V, dtype=float), True)
        J2 = vi_numpy.eval_policy(spec, pol, 2)
    return J3, ref3, J2


def _bits(a, b, what):
    for x, y, name in zip(a, b, ('J (3 steps, relative)', 'J_ref', 'J (2 steps)')):
        x, y = np.asarray(x), np.asarray(y)
        bad = ~((x == y) | (np.isnan(x) & np.isnan(y)))
        assert not bad.any(), '{}: {} differs at {} of {} entries'.format(what, name, int(bad.sum()), bad.size)


def _near(a, b, what, bar=1e-5):
    """4-byte results `a` against the fp64 oracle `b`"""
    for x, y, name in zip(a, b, ('J (3 steps, relative)', 'J_ref', 'J (2 steps)')):
        x, y = np.asarray(x, dtype=float), np.asarray(y, dtype=float)
        assert np.array_equal(np.isnan(x), np.isnan(y)), '{}: {}: NaN elsewhere'.format(what, name)
        assert np.array_equal(np.isposinf(x), np.isposinf(y)) and np.array_equal(np.isneginf(x), np.isneginf(y)), \
            '{}: {}: infinities elsewhere'.format(what, name)
        fin = np.isfinite(y)
        if fin.any():
            rel = np.abs(x[fin] - y[fin]).max() / max(1.0, np.abs(y[fin]).max())
            assert rel < bar, (what, name, rel)


def _check(s, gen, pol, V, what, nodes=None):
    """the runs of `s` against the direct kernel `gen` and the oracle (4-byte reals: against the direct kernel from
    V, against the oracle from a smooth cost-to-go)"""
    out = _evals(s, pol, V)
    _bits(out, _evals(gen, pol, V), what + ' vs direct kernel')
    assert gen.backend_info['kernel'] == 'generic'
    if s.dtype == np.float32:
        V = P.smooth_value(s)
        what += ' (smooth V)'
        out = _evals(s, pol, V)
        _bits(out, _evals(gen, pol, V), what + ' vs direct kernel')
    # (the oracle sees the policy as the device does: in the solver's reals)
    pol_d = np.asarray(pol, dtype=s.dtype).astype(float)
    V_d = np.asarray(V, dtype=s.dtype).astype(float)
    n_points = int(np.prod(s._state_grid_shape)) * len(s.perturb_grid[0])
    # Policies beyond the box send the next state up to 3.5 box reaches off the grid: the 4-byte lerp weight there is
    # hundreds of cells, and its rounding (6e-8 of it) reaches the extrapolated value times the slope of V -- up to
    # 2.2e-5 of the largest |J| at 512 rows.  The bar is 1e-4 for them (the direct kernel: bit for bit as above).
    bar = 1e-4 if ' outside' in what else 1e-5
    if n_points <= ORACLE_POINTS:
        ref = _oracle_evals(s, pol_d, V_d)
        if s.dtype == np.float64:
            _bits(out, ref, what + ' vs oracle')
        else:
            _near(out, ref, what + ' vs oracle', bar)
    else:
        assert nodes is not None
        J1 = _quiet(s.eval_policy, pol, 1, False, V, report_time=False).ravel()[nodes]
        with np.errstate(all='ignore'):
            Jo = vi_numpy.eval_policy(vi_numpy.Spec.from_solver(s), pol_d, 1, J_zero=V_d, nodes=nodes)
        if s.dtype == np.float64:
            _bits((J1, [0.], J1), (Jo, [0.], Jo), what + ' one step vs oracle')
        else:
            _near((J1, [0.], J1), (Jo, [0.], Jo), what + ' one step vs oracle', bar)
    return out


def _close(*solvers):
    for s in solvers:
        for k in [k for k in s._cache if k[0] == 'problem']:
            s._cache.pop(k).close()


@pytest.mark.timeout(600)
@pytest.mark.parametrize('case,geometry', cf.PAIRS, ids=['{}-{}'.format(c.name, g) for c, g in cf.PAIRS])
def test_column_form_evaluates_any_policy(gpu, debug_defines, case, geometry):
    if case.debug:
        debug_defines.set(**case.debug)
    auto = case.solver(geometry)
    gen = case.solver(geometry, kernel='generic')
    try:
        shape = auto._state_grid_shape
        nodes = cf.sample_nodes(shape, seed=len(case.name))
        V = np.random.default_rng(2000 + case.n0 + case.n_u).standard_normal(shape)
        for kind in P.KINDS:
            pol = P.policy(auto, kind, seed=case.n_u, V=V)
            _check(auto, gen, pol, V, '{} {} {}'.format(case, geometry, kind), nodes)
            info = auto.backend_info
            assert info['kernel'] == 'column' and info['certified_filter'], info
            src = auto._kernel_plan()['source']
            assert not cf.missing_claims(case, geometry, src), cf.missing_claims(case, geometry, src)
    finally:
        _close(auto, gen)


@pytest.mark.timeout(600)
@pytest.mark.parametrize('family', P.FAMILIES, ids=[f.name for f in P.FAMILIES])
def test_family_evaluates_any_policy(gpu, family):
    s = family.solver()
    gen = family.solver(kernel='generic')
    try:
        V = np.random.default_rng(31).standard_normal(s._state_grid_shape)
        for kind in P.KINDS:
            pol = P.policy(s, kind, seed=7, V=V)
            _check(s, gen, pol, V, '{} {}'.format(family, kind))
            for k, v in family.info.items():
                assert s.backend_info[k] == v, (family, kind, k, s.backend_info)
            if family.plans == 'row window':
                assert s.backend_info['row_window'], (family, kind, s.backend_info)
    finally:
        _close(s, gen)


@pytest.mark.timeout(600)
@pytest.mark.parametrize('family', [f for f in P.FAMILIES if f.plans in ('line', 'lead', 'staged', 'table per control')],
                         ids=lambda f: f.name)
def test_policy_iteration_matches_the_direct_kernel(gpu, family):
    s = family.solver()
    gen = family.solver(kernel='generic')
    try:
        pol = P.policy(s, 'smooth', seed=5)
        for rel_dp in (False, True):
            a = _quiet(s.policy_iteration, pol, 3, 2, rel_dp)
            info = dict(s.backend_info)
            b = _quiet(gen.policy_iteration, pol, 3, 2, rel_dp)
            assert info['kernel'] == family.info['kernel'], (family, info)
            (Ja, pa), (Jb, pb) = a, b
            assert np.array_equal(pa, pb), (family, rel_dp, 'policy')
            for x, y in zip(Ja if rel_dp else (Ja,), Jb if rel_dp else (Jb,)):
                assert np.array_equal(x, y), (family, rel_dp, 'J')
    finally:
        _close(s, gen)


# ----------------------------------------------------------------------------------------------------------------------
# the direct kernel's eval_policy, k_shift and k_diff_stats past their launch caps

def past_the_caps_start(S, dtype):
    """a standard-normal start, zero at the reference node, with two spikes among the last 129 nodes: the extremes of
    J_2 - J_1 then lie where only the last trip of k_diff_stats' loop reads"""
    V = np.random.default_rng(3).standard_normal(S)
    V[S // 2] = 0.
    V[S - 50], V[S - 90] = 1e3, -1e3
    return V.astype(dtype)


@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['f64', 'f32'])
def test_direct_kernel_evaluates_a_policy_past_its_launch_caps(gpu, dtype):
    """one state on cus * 16 * 256 + 129 nodes (forward_cases.long_line), kernel = 'generic', rel_dp, two sweeps with a
    tolerance nobody meets: both sweeps and their reference costs against the oracle on every node, the statistics
    against convergence.diff_stats of the downloaded arrays"""
    import forward_cases as fwd
    from stodynprog_amd import convergence as conv
    dt = np.dtype(dtype)
    cus = gpu.device_info(0)['compute_units']
    case = fwd.long_line(cus, 16)
    s = case.solver(dtype, 'generic')
    S = s._shape()[0]
    last = S - 129                                                        # the first node of every kernel's last trip
    vec = 16 // dt.itemsize
    assert S == cus * 16 * 256 + 129 and s._state_ref_ind == (S // 2,)
    assert -(-S // 256) > cus * 16 and last == cus * 16 * 256                              # sdp_evalpol and k_shift: 256 nodes a workgroup
    assert -(-(S // vec) // 256) > cus * 4 and last % (cus * 4 * 256 * vec) == 0           # k_diff_stats: 16 bytes a lane
    pol = case.policy(s)
    V = past_the_caps_start(S, dtype)
    spec = vi_numpy.Spec.from_solver(s)
    with np.errstate(all='ignore'):
        J1o, ref1o = vi_numpy.eval_policy(spec, pol, 1, True, V, True, dtype=dtype)
        J2o, ref2o = vi_numpy.eval_policy(spec, pol, 2, True, V, True, dtype=dtype)
    d = J2o.astype(float) - J1o.astype(float)
    assert min(d.argmax(), d.argmin()) >= last
    try:
        J1, ref1 = _quiet(s.eval_policy, pol, 1, True, V, report_time=False, J_ref_full=True)
        assert s.backend_info['kernel'] == 'generic'
        J2, ref2 = _quiet(s.eval_policy, pol, 2, True, V, report_time=False, J_ref_full=True, tol=0.0, check_every=1)
        rec = s.last_convergence
        assert J1.dtype == dt and np.array_equal(J1, J1o) and np.array_equal(np.atleast_1d(ref1), ref1o)
        assert J2.dtype == dt and np.array_equal(J2, J2o) and np.array_equal(np.atleast_1d(ref2), ref2o)
        assert rec.n_iter == 2 and rec.checked == [1, 2] and not rec.converged
        assert (rec.dmin[0], rec.dmax[0]) == conv.diff_stats(J1, V, dt)
        assert (rec.dmin[1], rec.dmax[1]) == conv.diff_stats(J2, J1, dt)
    finally:
        _close(s)
