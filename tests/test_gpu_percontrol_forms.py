"""Every case of tests/percontrol_forms.py -- the table per control (csrc/sdp_colu_kernel.h) with wide and narrow
table builds in both real types, one to seven chunks of perturbation points, units of 63 to 501 rows, every
(SDP_LEAD_HAS_W, SDP_COST_HAS_W) pair, two to four state variables and the three walks of sdp_col_of_unit -- at every
geometry of the case, on every input of the table.  The trailing axes are sized from the compute units of the chip the
test runs on, and the units the launch code then cuts are asserted from the restated split rule: where the claimed unit
shape is not reached the test fails, nothing skips.  Per case, geometry and input:

- three chained sweeps give J, policy and policy index of the direct kernel (kernel='generic') bit for bit, on all nodes;
- the first and the third of them are the numpy oracle's bit for bit (the float32 oracle for 4-byte reals) on a few
  hundred random nodes, rows 0 and n0 - 1, the rows on either side of every unit boundary, and the whole last column;
- on the random input: two steps of eval_policy and one value iteration in relative form, against the direct kernel.

No tolerance anywhere.  (tests/test_gpu_window_forms.py runs the row window's table through the same functions.)"""
import functools

import numpy as np
import pytest

import percontrol_forms as pf
from oracle import vi_numpy

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def cus(gpu):
    return int(gpu.device_info(0)['compute_units'])


def _ids(runs):
    return ['{}-{}-{}'.format(c.name, g, v) for c, g, v in runs]


def _close(*solvers):
    for s in solvers:
        for k in [k for k in s._cache if k[0] == 'problem']:
            s._cache.pop(k).close()


@functools.lru_cache(maxsize=2)
def _inputs(shape, rs):
    return pf.inputs(shape, rs)


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


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == 'f')


def _differs(a, b):
    """where two sweeps (J, policy, index) differ: the first node and how many, or None (a NaN equals a NaN)"""
    n = a[0].size
    Ja, Jb = np.ravel(a[0]), np.ravel(b[0])
    assert Ja.dtype == Jb.dtype and Ja.shape == Jb.shape
    bad = ~((Ja == Jb) | (np.isnan(Ja) & np.isnan(Jb)))
    pa, pb = np.reshape(a[1], (n, -1)), np.reshape(b[1], (n, -1))
    bad |= ~((pa == pb) | (np.isnan(pa) & np.isnan(pb))).all(axis=1)
    bad |= np.ravel(a[2]) != np.ravel(b[2])
    if not bad.any():
        return None
    k = int(np.flatnonzero(bad)[0])
    return 'first at entry {} of {} that differ: J {!r} / {!r}, index {} / {}'.format(
        k, int(bad.sum()), Ja[k], Jb[k], int(np.ravel(a[2])[k]), int(np.ravel(b[2])[k]))


def run_case(case, geometry, vname, cus, bounds_of, info_key):
    """the checks of the module's docstring for one (case, geometry, input); `bounds_of(solver, plan, cus)`: the units
    [(i_lo, i_hi)] of a column after asserting that they are what the case claims; `info_key`: the entry of
    backend_info that names the form"""
    col, gen = case.solver(geometry, 'column', cus), case.solver(geometry, 'generic', cus)
    what = '{} at {} on {}'.format(case, geometry, vname)
    try:
        shape = col._shape()
        bounds = bounds_of(col, col._kernel_plan(), cus)
        V0 = _inputs(shape, case.rs)[vname]
        # ---- bits against the direct kernel, three chained sweeps
        ref = _chain(gen, V0)
        got = _chain(col, V0)
        info = col.backend_info
        assert info['kernel'] == 'column' and info[info_key] and gen.backend_info['kernel'] == 'generic', info
        assert got[0][0].dtype == case.dtype
        for k, (a, b) in enumerate(zip(got, ref)):
            d = _differs(a, b)
            assert d is None, '{}, sweep {}: column / direct kernel: {}'.format(what, k + 1, d)
        # ---- bits against the oracle, sweeps 1 and 3
        nodes = pf.sample_nodes(shape, bounds)
        spec = vi_numpy.Spec.from_solver(col)
        for k in (0, 2):
            V = V0 if k == 0 else ref[k - 1][0]
            with np.errstate(all='ignore'):
                if case.rs == 8:
                    Jo, po, io, _ = vi_numpy.value_iteration(spec, V, nodes=nodes)
                else:
                    Jo, po, io, _ = vi_numpy.value_iteration(spec, np.asarray(V, dtype=np.float32), nodes=nodes, dtype=np.float32)
            J, pol, idx = got[k]
            d = _differs((J.ravel()[nodes], pol.reshape(J.size, -1)[nodes], idx.ravel()[nodes]),
                         (Jo, po, io.astype(idx.dtype)))
            assert d is None, '{}, sweep {}: column kernel / oracle on {} nodes: {}'.format(what, k + 1, len(nodes), d)
        # ---- policy evaluation and the relative form, once per case and geometry
        if vname == 'random':
            Ea, fa = gen.eval_policy(ref[0][1], 2, rel_dp=True, report_time=False, J_ref_full=True)
            Eb, fb = col.eval_policy(got[0][1], 2, rel_dp=True, report_time=False, J_ref_full=True)
            assert col.backend_info[info_key]
            assert _same(Ea, Eb) and _same(fa, fb), '{}: eval_policy in relative form'.format(what)
            Vd = V0 - V0[gen._state_ref_ind]
            (Ka, ra), pa = gen.value_iteration((Vd, 0.), rel_dp=True, report_time=False)
            (Kb, rb), pb = col.value_iteration((Vd, 0.), rel_dp=True, report_time=False)
            assert _same(Ka, Kb) and ra == rb and _same(pa, pb), '{}: value iteration in relative form'.format(what)
    finally:
        _close(col, gen)


def _bounds(col, plan, cus, case, geometry):
    shape = col._shape()
    assert plan['unit'].form == 'table per control', plan['unit']
    bounds = pf.sweep_bounds(col, cus, plan['col_seg_nodes'])
    rows = {hi - lo for lo, hi in bounds}
    assert rows == case.units[geometry], '{} at {} on {} compute units: units of {} rows, claimed {}'.format(
        case, geometry, cus, sorted(rows), sorted(case.units[geometry]))
    if geometry == 'many':
        launches = len(pf.launch_columns(shape, case.rs, col.host_overlap))
        assert pf.walk_branch(shape, len(bounds), launches) == case.walk, (case, shape, len(bounds), launches)
    return bounds


@pytest.mark.timeout(120)
@pytest.mark.parametrize('case,geometry,vname', pf.RUNS, ids=_ids(pf.RUNS))
def test_percontrol_form_against_the_direct_kernel_and_the_oracle(gpu, cus, case, geometry, vname):
    run_case(case, geometry, vname, cus, lambda col, plan, cus: _bounds(col, plan, cus, case, geometry), 'table_per_control')
