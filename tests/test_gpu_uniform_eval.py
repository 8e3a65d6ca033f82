"""The uniform EVALUATION stage of the branch and bound (SDP_BNB_UNIFORM_EVAL of csrc/sdp_colfilter_kernel.h) on the device,
at the shapes of tests/test_gpu_uniform_bound.py, whose model this is: a stock axis of 12 rows, 16 x 16 columns, 8
perturbation points, the resident-chunk form forced by its planning switch SDP_COL_WRES.  A unit that plans the uniform
bound stage plans this stage with it: every control of lane r is evaluated at row r + k_c + phi_c of the padded reduced
table, from one record per control, instead of at the reference's own cell -- and the radius pays for the distance.

Per case J, policy index and policy of three sweeps chained in device memory are bit for bit those of the direct kernel
(kernel='generic') and of the SAME unit with the stage switched off by its debug define (SDP_BNB_UNIFORM_EVAL = 0: the
evaluation that locates every control per node, with the radius of before).  One case runs on the axis [0.5, 3.5], whose
positions the reference forms by a true division.  That the stage RAN, and keeps no more blocks than before up to what a
little more slack can cost, is shown by the diagnostic build that stores the number of blocks each node asked for."""
import numpy as np
import pytest

from stodynprog_amd import DPSolver

import test_gpu_uniform_bound as ub
from test_gpu_uniform_bound import COUNT, FORCED, N0, N1, N2, _close, _quiet, _same, _V0

OFF = dict(FORCED, SDP_BNB_UNIFORM_EVAL='0')
SWITCHES = ('SDP_COL_WRES', 'SDP_BNB_UNIFORM', 'SDP_BNB_UNIFORM_EVAL', 'SDP_EXTRA_DEFINES')


def solver(n_u=64, kernel='auto', reach_rows=8.0, horizon=False, lo=0.0, hi=1.0, n0=N0):
    """the bound-stage test's problem, on a stock axis [lo, hi] of n0 rows (the gain still carries the controls
    +-reach_rows rows along it)"""
    s = ub.solver(n_u, kernel, reach_rows * (hi - lo) * (N0 - 1.0) / (n0 - 1.0), horizon)
    if (lo, hi, n0) != (0.0, 1.0, N0):
        s.discretize_state(lo, hi, n0, 0, 1, N1, 0, 1, N2)
    return s


# (n_u, reach in rows, the stock axis): most cells in the padding; a partial last block; a lattice inside the axis' cells;
# an axis whose form is not the unit axis
CASES = {'reach_8_rows': (64, 8.0, 0.0, 1.0), 'u57_short_last_block': (57, 8.0, 0.0, 1.0),
         'u9_reach_1_row': (9, 1.0, 0.0, 1.0), 'axis_0.5_3.5': (64, 8.0, 0.5, 3.5)}
_TRIPLE = ((FORCED, 'auto'), (OFF, 'auto'), (None, 'generic'))
COUNTED = ('reach_8_rows', 'axis_0.5_3.5')                   # the cases whose block counts are read: one per axis form


def units():
    """the generated sources of this file's problems (__graft_entry__.build compiles them ahead of the run)"""
    out = []
    saved = DPSolver.debug_defines
    try:
        for n_u, reach, lo, hi in CASES.values():
            for dbg, kernel in _TRIPLE:
                DPSolver.debug_defines = dbg
                out.append(solver(n_u, kernel, reach, lo=lo, hi=hi)._kernel_plan()['source'])
        for name in COUNTED:
            n_u, reach, lo, hi = CASES[name]
            for dbg in (COUNT, dict(COUNT, SDP_BNB_UNIFORM_EVAL='0')):
                DPSolver.debug_defines = dbg
                out.append(solver(n_u, 'auto', reach, lo=lo, hi=hi)._kernel_plan()['source'])
        for dbg, kernel in _TRIPLE:
            DPSolver.debug_defines = dbg
            fh = solver(64, kernel, 8.0, horizon=True)
            out += [fh._kernel_plan(t, fh._trace_now(t))['source'] for t in range(3)]
    finally:
        DPSolver.debug_defines = saved
    return out


def _plans_it(src):
    return '#define SDP_BNB_UNIFORM_EVAL 1' in src


def _three(debug_defines, case, V0, sweeps=3):
    """`sweeps` chained sweeps by the unit with the stage, the same unit without it, the direct kernel"""
    n_u, reach, lo, hi = CASES[case]
    out = []
    for dbg, kernel in _TRIPLE:
        debug_defines.unset(*SWITCHES)
        if dbg:
            debug_defines.set(**dbg)
        s = solver(n_u, kernel, reach, lo=lo, hi=hi)
        try:
            src = s._kernel_plan()['source']
            assert _plans_it(src) == (dbg == FORCED), (dbg, kernel)
            if kernel == 'auto':
                assert '#define SDP_BNB_UNIFORM 1' in src and '#define SDP_COL_WRES {}'.format(ub.WRES) in src
            J, pol = _quiet(s.value_iterations, V0, sweeps, report_time=False)
            assert s.backend_info['kernel'] == ('column' if kernel == 'auto' else 'generic')
            assert (s.backend_info['uniform_eval'] is not None) == (dbg == FORCED)
            out.append((J, pol, s.last_policy_index.copy()))
        finally:
            _close(s)
    return out


pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', sorted(CASES))
def test_three_chained_sweeps_keep_their_bits(gpu, debug_defines, name):
    uni, off, gen = _three(debug_defines, name, _V0())
    assert np.isfinite(uni[0]).all()
    _same(uni, gen, name + ': uniform evaluation vs direct kernel')
    _same(uni, off, name + ': uniform evaluation vs the stage switched off')
    if CASES[name][1] > 4:
        assert len(np.unique(uni[2])) > 8                      # (the policy uses the lattice: blocks are pruned and kept)


@pytest.mark.parametrize('name', COUNTED)
def test_the_stage_runs_and_asks_for_no_more_blocks(gpu, debug_defines, name):
    """every node went through the branch and bound (no wave failed the kernel's own checks and took every control the
    long way -- which would give the right bits without the stage ever running), on the unit axis and on the axis whose
    positions the reference forms by a division; and with the position term in the radius -- hence in the bound stage's
    slack -- a node asks for no more blocks than before, up to the allowance tests/test_gpu_uniform_bound.py grants for 8 u
    more slack"""
    n_u, reach, lo, hi = CASES[name]
    V1 = None
    need = {}
    for key, dbg in (('warm', FORCED), ('eval', COUNT), ('off', dict(COUNT, SDP_BNB_UNIFORM_EVAL='0'))):
        debug_defines.unset(*SWITCHES)
        debug_defines.set(**dbg)
        s = solver(n_u, 'auto', reach, lo=lo, hi=hi)
        try:
            assert _plans_it(s._kernel_plan()['source']) == (key != 'off')
            if key == 'warm':                                  # (two sweeps of the product: a cost-to-go with structure)
                V1, _ = _quiet(s.value_iterations, _V0(), 2, report_time=False)
                continue
            J, _ = _quiet(s.value_iterations, V1, 1, report_time=False)
            cnt = np.round(J).astype(int)
            assert (cnt >= 0).all(), key + ': a wave did not run the branch and bound'
            need[key] = cnt % 100
        finally:
            _close(s)
    print(name, 'blocks asked for per node: stage on {:.4f}, off {:.4f}'.format(need['eval'].mean(), need['off'].mean()))
    assert need['eval'].min() >= 1 and need['eval'].max() <= 8
    assert need['eval'].mean() <= need['off'].mean() * 1.02 + 0.02, (need['eval'].mean(), need['off'].mean())


def test_a_nan_and_infinities_in_one_column(gpu, debug_defines):
    V0 = _V0(6)
    V0[5, 7, 9] = np.nan
    V0[2, 7, 9] = np.inf
    V0[9, 7, 9] = -np.inf
    V0[0, 3, 3] = np.inf                                       # (row 0: the padding below the axis is continued from it)
    V0[N0 - 1, 12, 1] = -np.inf
    for sweeps in (1, 3):                                      # (one sweep: the planted values themselves are what a node sees)
        uni, off, gen = _three(debug_defines, 'reach_8_rows', V0, sweeps)
        assert np.isnan(uni[0]).any() and np.isfinite(uni[0]).any()
        _same(uni, gen, 'NaN / inf, {} sweeps: uniform evaluation vs direct kernel'.format(sweeps))
        _same(uni, off, 'NaN / inf, {} sweeps: uniform evaluation vs the stage switched off'.format(sweeps))


def test_a_finite_horizon_whose_steps_plan_the_stage(gpu, debug_defines):
    VT = _V0(7)
    out = []
    for dbg, kernel in _TRIPLE:
        debug_defines.unset(*SWITCHES)
        if dbg:
            debug_defines.set(**dbg)
        s = solver(64, kernel, 8.0, horizon=True)
        try:
            for t in range(3):
                assert _plans_it(s._kernel_plan(t, s._trace_now(t))['source']) == (dbg == FORCED)
            J, pol = _quiet(s.bellman_recursion, 3, VT, report_time=False)
            out.append((np.asarray(J), np.asarray(pol)))
        finally:
            _close(s)
    for other, what in ((out[2], 'direct kernel'), (out[1], 'stage switched off')):
        assert np.array_equal(out[0][0], other[0], equal_nan=True), 'horizon: J differs from the ' + what
        assert np.array_equal(out[0][1], other[1], equal_nan=True), 'horizon: policy differs from the ' + what
