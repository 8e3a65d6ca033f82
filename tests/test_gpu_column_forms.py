"""Every form of the column family in tests/column_forms.py, at a grid big enough for the persistent loop to carry
its state from unit to unit ('many': 128 x 128 columns) and, for the held tail and some 1024-thread forms, at one
where column_grid splits every column into row ranges ('split': 8 x 8 columns).  Per case and geometry:

- the unit that ran is the column kernel with the certified filter and carries the macros the case claims;
- on three inputs -- sweep 3 of the benchmark's chain from synthetic3d_V0, a seeded standard-normal cost-to-go
  (several survivors per node: the second pass's walk over them), and for the held tail NaN blocks and inf rows --
  J, policy index and policy values are bit for bit those of the same family without the filter (every control the
  long way) and of the direct kernel (kernel='generic', which shares none of the table code), on ALL nodes;
- against the numpy oracle on >= 500 sampled nodes that include rows 0 and n0 - 1, the last column and the rows
  around every split boundary: 8-byte reals bit for bit (indices exact or proved ties), 4-byte reals within 1e-5
  with indices exact where the fp64 margin exceeds fp32 resolution;
- three sweeps chained in device memory equal three single sweeps of the direct kernel, and for resident chunks
  the policy evaluation (sdp_evalpol_col) equals the direct kernel's."""
import contextlib
import io

import numpy as np
import pytest

import column_forms as cf
from conftest import assert_sweep_parity
from stodynprog_amd import codegen, models

pytestmark = pytest.mark.gpu


def _quiet(f, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all='ignore'):
        return f(*a, **kw)


def _ran_source(s):
    """the generated source of the device problem the solver holds -- the unit that ran"""
    src = s._kernel_plan()['source']
    keys = [k for k in s._cache if k[0] == 'problem']
    assert [k[3] for k in keys] == [codegen.source_key(src)], 'the problem that ran is not the planned unit'
    return src


def _sweep(s, V):
    J, pol = _quiet(s.value_iteration, V, report_time=False)
    return J, pol, s.last_policy_index


def _same(a, b, what):
    assert np.array_equal(a[0], b[0], equal_nan=True), what + ': J differs'
    assert np.array_equal(a[2], b[2]), what + ': policy index differs'
    assert np.array_equal(a[1], b[1], equal_nan=True), what + ': policy differs'


def _special_values(V):
    """a NaN block inside some columns, whole columns of +inf from some row on in others"""
    n0, n1, n2 = V.shape
    V = V.copy()
    V[n0 // 3:n0 // 3 + 9, 1:3, n2 // 2:n2 // 2 + 2] = np.nan
    V[n0 - 1, n1 // 2, 0] = np.nan
    V[(3 * n0) // 4:, n1 - 2, 1:4] = np.inf
    V[:5, n1 // 2 + 1, n2 - 1] = np.inf
    return V


def _against_oracle(case, geometry, V, out, nodes, what, finite, smooth=False):
    """the sweep `out` from V on `nodes`, against the numpy oracle in fp64 (`finite`: no NaN / inf in V; `smooth`:
    V is the benchmark's chain)"""
    from oracle import vi_numpy
    ref = case.solver(geometry, dtype=np.float64)      # (the oracle's spec only reads the discretisation)
    V64 = np.asarray(V, dtype=np.float64)
    with np.errstate(all='ignore'):
        Jo, _, io_, mo = vi_numpy.value_iteration(vi_numpy.Spec.from_solver(ref), V64, nodes=nodes)
    J, idx = out[0].ravel()[nodes], out[2].ravel()[nodes]
    if case.dtype.itemsize == 8:
        assert np.array_equal(J, Jo, equal_nan=True), '{}: J differs from the oracle at {} of {} nodes'.format(
            what, int((~((J == Jo) | (np.isnan(J) & np.isnan(Jo)))).sum()), len(nodes))
        if finite:
            assert_sweep_parity(J, idx, Jo, io_, mo, what, prove=(ref, V64), nodes=nodes)
        else:
            assert np.array_equal(idx, io_), what + ': policy index differs from the oracle'
        return
    # 4-byte reals: bit for bit the float32 oracle (the direct kernel's definition restated in numpy float32) ...
    V32 = np.asarray(V, dtype=np.float32)
    with np.errstate(all='ignore'):
        J32, p32, i32_, _ = vi_numpy.value_iteration(vi_numpy.Spec.from_solver(ref), V32, nodes=nodes, dtype=np.float32)
    assert np.array_equal(J, J32, equal_nan=True), what + ': J differs from the float32 oracle'
    assert np.array_equal(idx, i32_), what + ': policy index differs from the float32 oracle'
    assert np.array_equal(out[1].reshape(-1, p32.shape[-1])[nodes], p32, equal_nan=True), \
        what + ': policy differs from the float32 oracle'
    # ... and the bar of test_fp32_512cubed_against_fp64_oracle against the 8-byte one
    scale = np.abs(Jo).max()
    rel = np.abs(J - Jo).max() / scale
    assert rel < 1e-5, (what, rel)
    if smooth:
        clear = mo > 1e-5 * np.maximum(1.0, np.abs(Jo))
        assert (idx[clear] == io_[clear]).all(), what + ': index differs where the fp64 margin exceeds fp32 resolution'
        return
    # A standard-normal V changes by O(1) from row to row: the fp32 rounding of x0' (~6e-8, 3e-5 of a row at 512 rows)
    # moves a cost by about 1e-5 there, and a pick may differ at larger margins.  Where it does, the control it picked
    # must be optimal within twice the bar of J (once for the fp32 error of its own cost, once for J's): its fp64 cost,
    # from the complete per-control vector, within 2e-5 of the scale of J of the minimum.
    spec = vi_numpy.Spec.from_solver(ref)
    interp = vi_numpy.Interp(*spec.state_grid)
    interp.set_values(V64)
    for flat, i32 in zip(nodes[idx != io_], idx[idx != io_]):
        x_k = tuple(g[i] for g, i in zip(spec.state_grid, np.unravel_index(int(flat), spec.shape)))
        with np.errstate(all='ignore'):
            costs = np.asarray(vi_numpy.backup_node(spec, x_k, interp, None, full=True)[4], dtype=float).ravel()
        assert costs[int(i32)] - costs.min() <= 2e-5 * scale, (what, int(flat), int(i32), costs[int(i32)] - costs.min())


@pytest.mark.timeout(300)
@pytest.mark.parametrize('case,geometry', cf.PAIRS, ids=['{}-{}'.format(c.name, g) for c, g in cf.PAIRS])
def test_column_form_against_the_long_way_the_direct_kernel_and_the_oracle(gpu, debug_defines, case, geometry):
    if case.debug:
        debug_defines.set(**case.debug)
    auto = case.solver(geometry)
    long_ = case.solver(geometry, certified_filter=False)
    gen = case.solver(geometry, kernel='generic')
    try:
        shape = auto._state_grid_shape
        nodes = cf.sample_nodes(shape, seed=len(case.name))
        resident = cf.claims(case, geometry).get('SDP_COL_WRES') is not None
        # (a) the benchmark's chain: three single sweeps of the direct kernel from the closed-form V0 ...
        V0 = models.synthetic3d_V0(auto.state_grid, case.dtype)
        g1 = _sweep(gen, V0)
        g2 = _sweep(gen, g1[0])
        g3 = _sweep(gen, g2[0])
        assert gen.backend_info['kernel'] == 'generic'
        # ... equal three sweeps chained in device memory by the form under test (its state across launches)
        J3, pol3 = _quiet(auto.value_iterations, V0, 3, report_time=False)
        _same((J3, pol3, auto.last_policy_index), g3, '{} chained x 3'.format(case))
        # the plan: the column kernel with the filter, and the unit that ran is the form the case claims
        info = auto.backend_info
        assert info['kernel'] == 'column' and info['certified_filter'], info
        src = _ran_source(auto)
        assert not cf.missing_claims(case, geometry, src), cf.missing_claims(case, geometry, src)
        assert cf.hold_geometry(src) == case.hold
        # sweep 3 of the chain, one sweep from J_2, by all three kernels
        a = _sweep(auto, g2[0])
        lw = _sweep(long_, g2[0])
        assert long_.backend_info['kernel'] == 'column' and not long_.backend_info['certified_filter']
        _same(a, lw, '{} sweep 3: filter vs long way'.format(case))
        _same(a, g3, '{} sweep 3: column vs direct kernel'.format(case))
        _against_oracle(case, geometry, g2[0], a, nodes, '{} {} sweep 3'.format(case, geometry), True, True)
        # (b) a seeded standard-normal cost-to-go: several survivors per node
        Vb = np.random.default_rng(1000 + case.n0 + case.n_u).standard_normal(shape).astype(case.dtype)
        b = _sweep(auto, Vb)
        _same(b, _sweep(long_, Vb), '{} normal V: filter vs long way'.format(case))
        _same(b, _sweep(gen, Vb), '{} normal V: column vs direct kernel'.format(case))
        _against_oracle(case, geometry, Vb, b, nodes, '{} {} normal V'.format(case, geometry), True)
        # (c) held tail: NaN blocks inside some columns, inf rows in others (those nodes take the long way)
        if case.hold:
            Vc = _special_values(Vb)
            c = _sweep(auto, Vc)
            assert np.isnan(c[0]).any()
            _same(c, _sweep(long_, Vc), '{} NaN / inf: filter vs long way'.format(case))
            _same(c, _sweep(gen, Vc), '{} NaN / inf: column vs direct kernel'.format(case))
            _against_oracle(case, geometry, Vc, c, nodes, '{} {} NaN / inf'.format(case, geometry), False)
        # the unit is still the one the case claims (no other problem was made on the way)
        assert _ran_source(auto) == src
        # policy evaluation of resident chunks (sdp_evalpol_col) against the direct kernel's
        if resident:
            E1 = _quiet(auto.eval_policy, g3[1], 4, True, report_time=False, J_ref_full=True)
            E2 = _quiet(gen.eval_policy, g3[1], 4, True, report_time=False, J_ref_full=True)
            assert np.array_equal(E1[0], E2[0]) and np.array_equal(E1[1], E2[1]), '{}: eval_policy'.format(case)
    finally:
        for s in (auto, long_, gen):
            for k_ in [k_ for k_ in s._cache if k_[0] == 'problem']:
                s._cache.pop(k_).close()
