"""The uniform bound stage of the branch and bound (SDP_BNB_UNIFORM of csrc/sdp_colfilter_kernel.h) on the device, at the
smallest grids that plan it: a stock axis of 12 rows, 16 x 16 columns, 8 perturbation points.  No grid this small
selects the resident-chunk form by itself (the planner takes it where it lets a CU hold more workgroups, from about
128 rows x 32 points on): it is FORCED here by its planning switch SDP_COL_WRES, as the wres cases of
tests/column_forms.py do; the forms at the sizes that select them run in tests/test_gpu_column_forms.py.  The model is the
benchmark's shape with a gain that carries the controls +-8 rows along the stock: most block ends of most nodes lie
beyond the axis, in the padding of the reduced table.

Per case J, policy index and policy of three sweeps chained in device memory are bit for bit those of the direct kernel
(kernel='generic', which shares none of the table code) and of the SAME unit with the stage switched off by its debug
define (the bound stage that locates every block end per node).  Both of those are exact whatever the first pass does:
that the uniform stage RAN, and pruned, is shown by the diagnostic build that stores the number of blocks each node
asked for (SDP_DIAG_BNB_COUNT; -1 where a wave took the full first pass instead)."""
import contextlib
import io

import numpy as np
import pytest

from stodynprog_amd import DPSolver, SysDescription
from stodynprog_amd.models import NormalLaw

N0, N1, N2, N_W, WRES = 12, 16, 16, 8, 4
FORCED = {'SDP_COL_WRES': str(WRES)}
COUNT = dict(FORCED, SDP_EXTRA_DEFINES='SDP_DIAG_BNB_COUNT=1')     # diagnostic build: J := blocks asked for + 100 x the guess's block


def system(reach_rows=8.0, horizon=False):
    """x0' = x0 + b u with b = reach_rows rows of the stock axis per unit of control, exogenous x1, x2; a cost that the
    perturbation does not reach (with a time index: in the cost and the box only -- X of x0' = X + a stays the stock)"""
    b = reach_rows / (N0 - 1)
    s = SysDescription((3, 1, 1), stationnary=not horizon, name='uniform bound stage')
    if horizon:
        s.dyn = lambda k, x0, x1, x2, u, w: (x0 + b * u, 0.1 + 0.6 * x1 + 0.2 * x2 + w, 0.2 + 0.1 * x1 + 0.5 * x2 + 0.5 * w)
        s.cost = lambda k, x0, x1, x2, u, w: 0.3 * x0 + (((0.8 * x1 - 0.3) - u) * ((0.8 * x1 - 0.3) - u) + (0.05 * k - 0.1) * u)
        s.control_box = lambda k, x0, x1, x2: ((-1.0, 1.0 - 0.125 * k),)
    else:
        s.dyn = lambda x0, x1, x2, u, w: (x0 + b * u, 0.1 + 0.6 * x1 + 0.2 * x2 + w, 0.2 + 0.1 * x1 + 0.5 * x2 + 0.5 * w)
        s.cost = lambda x0, x1, x2, u, w: 0.3 * x0 + (((0.8 * x1 - 0.3) - u) * ((0.8 * x1 - 0.3) - u) + 0.01 * (u * u))
        s.control_box = lambda x0, x1, x2: ((-1.0, 1.0),)
    s.perturb_laws = [NormalLaw(0, 0.05)]
    return s


def solver(n_u=64, kernel='auto', reach_rows=8.0, horizon=False):
    s = DPSolver(system(reach_rows, horizon))
    s.discretize_state(0, 1, N0, 0, 1, N1, 0, 1, N2)
    s.discretize_perturb(-0.15, 0.15, N_W)
    s.control_steps = (2. / (n_u - 1.5),)                      # n_u points on [-1, 1] (the step kept off an integer quotient)
    s.kernel = kernel
    return s


# (n_u, reach in rows): the stock axis shorter than the reach; a last block of one control; a lattice inside the axis' cells
CASES = {'reach_8_rows': (64, 8.0), 'u57_short_last_block': (57, 8.0), 'u9_reach_1_row': (9, 1.0)}


def units():
    """the generated sources of this file's problems (__graft_entry__.build compiles them ahead of the run)"""
    out = []
    saved = DPSolver.debug_defines
    try:
        for n_u, reach in CASES.values():
            for dbg, kernel in ((FORCED, 'auto'), (dict(FORCED, SDP_BNB_UNIFORM='0'), 'auto'), (None, 'generic')):
                DPSolver.debug_defines = dbg
                out.append(solver(n_u, kernel, reach)._kernel_plan()['source'])
        for dbg in (COUNT, dict(COUNT, SDP_BNB_UNIFORM='0')):
            DPSolver.debug_defines = dbg
            out.append(solver(64, 'auto', 8.0)._kernel_plan()['source'])
        for dbg, kernel in ((FORCED, 'auto'), (dict(FORCED, SDP_BNB_UNIFORM='0'), 'auto'), (None, 'generic')):
            DPSolver.debug_defines = dbg
            fh = solver(64, kernel, 8.0, horizon=True)
            out += [fh._kernel_plan(t, fh._trace_now(t))['source'] for t in range(3)]
    finally:
        DPSolver.debug_defines = saved
    return out


def _quiet(f, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all='ignore'):
        return f(*a, **kw)


def _close(*solvers):
    for s in solvers:
        for k in [k for k in s._cache if k[0] == 'problem']:
            s._cache.pop(k).close()


def _V0(seed=5):
    return np.random.default_rng(seed).standard_normal((N0, N1, N2))


def _three(debug_defines, n_u, reach, V0, sweeps=3):
    """`sweeps` chained sweeps by the unit with the stage, the same unit without it, the direct kernel"""
    out = []
    for dbg, kernel in ((FORCED, 'auto'), (dict(FORCED, SDP_BNB_UNIFORM='0'), 'auto'), (None, 'generic')):
        debug_defines.unset('SDP_COL_WRES', 'SDP_BNB_UNIFORM')
        if dbg:
            debug_defines.set(**dbg)
        s = solver(n_u, kernel, reach)
        try:
            src = s._kernel_plan()['source']
            assert ('#define SDP_BNB_UNIFORM 1' in src) == (dbg == FORCED), (dbg, kernel)
            if kernel == 'auto':
                assert '#define SDP_COL_WRES {}'.format(WRES) in src and '#define SDP_COL_BNB 1' in src
            J, pol = _quiet(s.value_iterations, V0, sweeps, report_time=False)
            assert s.backend_info['kernel'] == ('column' if kernel == 'auto' else 'generic')
            out.append((J, pol, s.last_policy_index.copy()))
        finally:
            _close(s)
    return out


def _same(a, b, what):
    assert np.array_equal(a[0], b[0], equal_nan=True), what + ': J differs'
    assert np.array_equal(a[2], b[2]), what + ': policy index differs'
    assert np.array_equal(a[1], b[1], equal_nan=True), what + ': policy differs'


pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', sorted(CASES))
def test_three_chained_sweeps_keep_their_bits(gpu, debug_defines, name):
    n_u, reach = CASES[name]
    uni, off, gen = _three(debug_defines, n_u, reach, _V0())
    assert np.isfinite(uni[0]).all()
    _same(uni, gen, name + ': uniform stage vs direct kernel')
    _same(uni, off, name + ': uniform stage vs the stage switched off')
    if reach > 4:
        assert len(np.unique(uni[2])) > 8                      # (the policy uses the lattice: blocks are pruned and kept)


def test_the_uniform_stage_runs_and_prunes(gpu, debug_defines):
    """every node went through the branch and bound (no wave fell back to the full first pass), most of its 8 blocks were
    ruled out, and the stage keeps no more blocks than the bound that locates every end per node, up to what 8 u S_node
    more slack can cost"""
    V1 = None
    need = {}
    for key, dbg in (('warm', FORCED), ('uniform', COUNT), ('off', dict(COUNT, SDP_BNB_UNIFORM='0'))):
        debug_defines.unset('SDP_COL_WRES', 'SDP_BNB_UNIFORM', 'SDP_EXTRA_DEFINES')
        debug_defines.set(**dbg)
        s = solver(64, 'auto', 8.0)
        try:
            src = s._kernel_plan()['source']
            assert ('#define SDP_BNB_UNIFORM 1' in src) == (key != 'off')
            if key == 'warm':                                  # (two sweeps of the product: a cost-to-go with structure)
                V1, _ = _quiet(s.value_iterations, _V0(), 2, report_time=False)
                continue
            J, _ = _quiet(s.value_iterations, V1, 1, report_time=False)
            cnt = np.round(J).astype(int)
            assert (cnt >= 0).all(), key + ': a wave took the full first pass'
            need[key] = cnt % 100
        finally:
            _close(s)
    n_blocks = 8
    assert need['uniform'].min() >= 1 and need['uniform'].max() <= n_blocks
    assert need['uniform'].mean() < 0.75 * n_blocks, need['uniform'].mean()        # blocks were ruled out
    assert (need['uniform'] < n_blocks).mean() > 0.9
    assert need['uniform'].mean() <= need['off'].mean() * 1.02 + 0.02, (need['uniform'].mean(), need['off'].mean())


def test_a_nan_and_infinities_in_one_column(gpu, debug_defines):
    V0 = _V0(6)
    V0[5, 7, 9] = np.nan
    V0[2, 7, 9] = np.inf
    V0[9, 7, 9] = -np.inf
    V0[0, 3, 3] = np.inf                                       # (row 0: the padding below the axis is continued from it)
    V0[N0 - 1, 12, 1] = -np.inf
    for sweeps in (1, 3):                                      # (one sweep: the planted values themselves are what a node sees)
        uni, off, gen = _three(debug_defines, 64, 8.0, V0, sweeps)
        assert np.isnan(uni[0]).any() and np.isfinite(uni[0]).any()
        _same(uni, gen, 'NaN / inf, {} sweeps: uniform stage vs direct kernel'.format(sweeps))
        _same(uni, off, 'NaN / inf, {} sweeps: uniform stage vs the stage switched off'.format(sweeps))


def test_a_finite_horizon_whose_steps_plan_the_stage(gpu, debug_defines):
    VT = _V0(7)
    out = []
    for dbg, kernel in ((FORCED, 'auto'), (dict(FORCED, SDP_BNB_UNIFORM='0'), 'auto'), (None, 'generic')):
        debug_defines.unset('SDP_COL_WRES', 'SDP_BNB_UNIFORM')
        if dbg:
            debug_defines.set(**dbg)
        s = solver(64, kernel, 8.0, horizon=True)
        try:
            for t in range(3):
                assert ('#define SDP_BNB_UNIFORM 1' in s._kernel_plan(t, s._trace_now(t))['source']) == (dbg == FORCED)
            J, pol = _quiet(s.bellman_recursion, 3, VT, report_time=False)
            out.append((np.asarray(J), np.asarray(pol)))
        finally:
            _close(s)
    for other, what in ((out[2], 'direct kernel'), (out[1], 'stage switched off')):
        assert np.array_equal(out[0][0], other[0], equal_nan=True), 'horizon: J differs from the ' + what
        assert np.array_equal(out[0][1], other[1], equal_nan=True), 'horizon: policy differs from the ' + what
