"""Every case of tests/line_forms.py -- every lane count the planner gives the line kernel (csrc/sdp_line_kernel.h), both
branches of the lane formula, W from 1 to 1024, every form the header branches on at lanes 1, 32 and 64 -- on every
input value array of the table.  Per case and input:

- three chained sweeps give J, policy and policy index of the direct kernel (kernel='generic', which shares none of
  the filter's code) bit for bit, on all nodes;
- the first and the third of them are the numpy oracle's bit for bit: on every node up to 2e6 cells per sweep, beyond
  that on the nodes around the tile boundaries (line_forms.Case.sample_nodes).  No tolerance anywhere;
- one more sweep from the input by the SDP_LINE_DIAG build gives the same bits, and its nine counters add up: every
  node is decided at the first level, left to the second, or bad; every node left to the second level is decided
  there or left to the long way; where the lattice is unusable or the input holds a NaN, every node is bad and the
  long way evaluates every control of every node exactly once, whatever the lane count cuts the lattice into;
- the counters the table claims for the case and input (line_forms.PATHS) are non-zero: a case written to reach
  "two survivors at the second level" did;
- at lanes 32 and 64, with every half-width multiplied by 1e18: the same bits, nothing decided at the first level,
  the candidates the long way."""
import ctypes as C

import numpy as np
import pytest

import line_forms as lf
from oracle import vi_numpy

pytestmark = pytest.mark.gpu

_PAIRS = [(c, v) for c in lf.CASES for v in c.input_names]


def _close(*solvers):
    for s in solvers:
        for k in [k for k in s._cache if k[0] == 'problem']:
            s._cache.pop(k).close()


def _sweep(s, V):
    with np.errstate(all='ignore'):
        J, pol = s.value_iteration(V, report_time=False)
    return J.copy(), pol.copy(), s.last_policy_index.copy()


def _chain(s, V0, sweeps=3):
    out, V = [], V0
    for _ in range(sweeps):
        out.append(_sweep(s, V))
        V = out[-1][0]
    return out


def _counted_sweep(gpu, s, V):
    """one sweep of a SDP_LINE_DIAG solver with the counters on (tools/line_diag.py): (J, policy, index), {counter: n}"""
    prob = s._problem()
    gpu.check(gpu.lib().sdp_problem_debug_stamps(prob.h, 1, None, 0))          # (a fresh, zeroed buffer)
    out = _sweep(s, V)
    assert s._problem() is prob, 'the sweep ran on another problem than the one that counts'
    st = np.zeros(16, dtype=np.uint64)
    gpu.check(gpu.lib().sdp_problem_debug_stamps(prob.h, 1, st.ctypes.data_as(C.c_void_p), st.size))
    assert not st[9:].any()
    return out, dict(zip(lf.COUNTERS, (int(v) for v in st[:9])))


def _differs(a, b):
    """where two sweeps (J, policy, index) differ: the first node and how many, or None"""
    bad = ~((a[0] == b[0]) | (np.isnan(a[0]) & np.isnan(b[0])))
    pa, pb = a[1].reshape(a[0].size, -1), b[1].reshape(b[0].size, -1)
    bad |= ~((pa == pb) | (np.isnan(pa) & np.isnan(pb))).all(axis=1)
    bad |= np.asarray(a[2]).ravel() != np.asarray(b[2]).ravel()
    if not bad.any():
        return None
    k = int(np.flatnonzero(bad)[0])
    return 'first at node {} of {} that differ: J {!r} / {!r}, index {} / {}'.format(
        k, int(bad.sum()), a[0][k], b[0][k], int(np.ravel(a[2])[k]), int(np.ravel(b[2])[k]))


@pytest.mark.timeout(120)
@pytest.mark.parametrize('case,vname', _PAIRS, ids=['{}-{}'.format(c.name, v) for c, v in _PAIRS])
def test_line_form_against_the_direct_kernel_the_oracle_and_its_counters(gpu, case, vname):
    V0 = case.inputs()[vname]
    line, gen, diag = case.solver(), case.solver('generic'), case.solver(debug=lf.DIAG)
    wide = case.solver(debug=lf.DIAG_WIDE) if lf.runs_wide(case) else None
    what = '{} ({} lanes) on {}'.format(case, case.lanes, vname)
    try:
        # ---- bits against the direct kernel, three chained sweeps
        ref = _chain(gen, V0)
        got = _chain(line, V0)
        info = line.backend_info
        assert info['kernel'] == 'line' and info['lanes_per_node'] == case.lanes and gen.backend_info['kernel'] == 'generic', info
        for k, (a, b) in enumerate(zip(got, ref)):
            d = _differs(a, b)
            assert d is None, '{}, sweep {}: line / direct kernel: {}'.format(what, k + 1, d)
        # ---- bits against the oracle, sweeps 1 and 3
        nodes = case.sample_nodes()
        spec = vi_numpy.Spec.from_solver(line)
        for k in (0, 2):
            V = V0 if k == 0 else ref[k - 1][0]
            with np.errstate(all='ignore'):
                Jo, po, io, _ = vi_numpy.value_iteration(spec, V, nodes=nodes)
            J, pol, idx = got[k]
            d = _differs((J[nodes], pol.reshape(case.n_x, -1)[nodes], idx[nodes]), (Jo, po, io))
            assert d is None, '{}, sweep {}: line kernel / oracle on {} nodes: {}'.format(what, k + 1, len(nodes), d)
        # ---- the diagnostic build: the same bits, and counters that add up
        out, n = _counted_sweep(gpu, diag, V0)
        print('COUNTERS', repr(case.name), repr(vname), n)
        assert diag.backend_info['debug_defines'] == lf.DIAG
        d = _differs(out, got[0])
        assert d is None, '{}: diagnostic build / product: {}'.format(what, d)
        assert n['single1'] + n['pair1'] + n['undecided1'] + n['bad'] == case.n_x, (what, n)
        assert n['single2'] + n['pair2'] + n['left2'] == n['undecided1'], (what, n)
        # (a node left to the second level evaluates at least the control with the smallest upper end there)
        assert n['evals2'] >= n['undecided1'] and n['long way'] >= n['left2'], (what, n)
        counts = lf.control_counts(diag)
        if not case.usable or vname == 'special':
            assert n['bad'] == case.n_x, (what, n)
            assert n['long way'] == int(counts.sum()), (what, n, int(counts.sum()))
        missing = [k for k in lf.claimed(case, vname) if not n[k]]
        assert not missing, '{}: claimed and not reached: {} ({})'.format(what, missing, n)
        # ---- every half-width x 1e18, at the lane counts with 32 and 64 slices a wave
        if wide is not None:
            out, n = _counted_sweep(gpu, wide, V0)
            print('COUNTERS WIDE', repr(case.name), repr(vname), n)
            assert wide.backend_info['debug_defines'] == lf.DIAG_WIDE
            d = _differs(out, got[0])
            assert d is None, '{}: half-widths x 1e18 / product: {}'.format(what, d)
            # (a node whose box collapses to one control point has one survivor whatever the half-widths are)
            lone = 0 if n['bad'] == case.n_x else case.collapsed
            assert n['single1'] == lone and n['pair1'] == 0 and n['long way'] > 0, (what, n)
            assert n['single1'] + n['pair1'] + n['undecided1'] + n['bad'] == case.n_x, (what, n)
    finally:
        _close(*[s for s in (line, gen, diag, wide) if s is not None])
