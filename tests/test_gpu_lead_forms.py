"""Every form of the reduced-array sweep that the planner gives (csrc/sdp_lead_kernel.h; the table tests/lead_forms.py:
m = 1, 2, 3 stocks, with and without an exogenous axis, listed first, last, in the middle and interleaved, a cost that
sees the perturbation, three controls on a per-node box) on the device against the numpy oracle (oracle/vi_numpy.py
through Spec.from_solver, on all nodes) and against the direct kernel (kernel = 'generic', which shares none of the
re-indexing), bit for bit: every comparison of results is np.array_equal with NaN equal to NaN, no tolerance appears in
this file.  tests/test_lead_forms_plan.py checks on the CPU that each case plans what it claims and that the oracle's
policies use the control lattice.

Per small case: sweeps 1 and 3 of a chain kept on the device from four cost-to-go arrays (zeros, smooth, seeded random,
one with NaN and +-inf), with and without the relative-DP shift; one sweep through value_iteration (host arrays in and
out); eval_policy of a policy that is none of the lattice's, with the fused shift and without.  With every radius
multiplied by 1e12 every node takes the long way -- the second pass alone on the plane-major copy -- and the bits stay;
on the flat objective a permuted form keeps the bits at the proven radius and at half of it, and a radius cut by 1e6
is noticed.  The large case runs value_iteration in four phases of the node range, each of which walks every
plane-major position of the permuted view and drops the nodes outside its range: the same bits as the unphased sweep,
as the direct kernel on all nodes, and as the oracle on 2000 sampled nodes."""
import contextlib
import functools
import io

import numpy as np
import pytest

import lead_forms as lf
from oracle import vi_numpy

pytestmark = pytest.mark.gpu
_SMALL_IDS = [c.name for c in lf.SMALL]


def _quiet(f, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all='ignore'):
        return f(*a, **kw)


def _close(*solvers):
    for s in solvers:
        for k in [k for k in s._cache if k[0] == 'problem']:
            s._cache.pop(k).close()


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.dtype.kind == 'f':
        assert got.dtype == want.dtype, (what, got.dtype, want.dtype)
    bad = ~((got == want) | ((got != got) & (want != want)))
    where = np.flatnonzero(bad.reshape(-1) if bad.ndim else bad.reshape(1))
    assert not bad.any(), '{}: differs at {} of {} entries, first at flat index {}'.format(
        what, int(bad.sum()), got.size, int(where[0]) if where.size else -1)


def _is_lead(s, case):
    """the unit that ran is the one the table claims"""
    info = s.backend_info
    assert info['mode'] == 'traced' and info['kernel'] == 'lead' and info['filter_form'] == 'reduced array', info
    assert info['controlled_axes'] == case.lead_axes, info
    assert info['controlled_order'] == (list(case.lead_perm) if case.permuted else None), info


def _at_ref_zero(V, ref_ind):
    """the input as a differential cost: zero at the reference node (the non-finite entries are elsewhere)"""
    assert np.isfinite(V[ref_ind])
    return V - V[ref_ind]


@functools.lru_cache(maxsize=None)
def _oracle_sweeps(name, which, rel_dp):
    """three chained oracle sweeps of a small case: [(J, refs so far, pol, idx), ...].  With the relative-DP shift the
    chain ends where the reference node's cost is not finite (the non-finite input): the next sweep's input is no
    differential cost, which the reference asserts (sdp.py:488).  (`which`: an input of the table, or 'flat')"""
    s = lf.BY_NAME[name].solver()
    spec = vi_numpy.Spec.from_solver(s)
    V = lf.flat_input(s) if which == 'flat' else lf.inputs(s._shape())[which]
    out, refs = [], []
    with np.errstate(all='ignore'):
        J = (_at_ref_zero(V, spec.ref_ind), 0.) if rel_dp else V
        for _ in range(3):
            J, pol, idx, _ = vi_numpy.value_iteration(spec, J, rel_dp=rel_dp)
            if rel_dp:
                refs.append(float(J[1]))
            out.append(((J[0] if rel_dp else J).copy(), list(refs), pol, idx.astype(np.int32)))
            if rel_dp and not J[0][spec.ref_ind] == 0.:
                break
    return out


def _check_sweep(s, got, want, rel_dp, what):
    J, pol = got
    wJ, wrefs, wpol, widx = want
    if rel_dp:
        J, refs = J
        _same(np.asarray(refs, dtype=float), np.asarray(wrefs), what + ' J_ref')
    _same(J, wJ, what + ' J')
    _same(s.last_policy_index, widx, what + ' policy index')
    _same(pol, wpol, what + ' policy values')


@pytest.mark.parametrize('case', lf.SMALL, ids=_SMALL_IDS)
def test_chained_sweeps_equal_the_oracle_and_the_direct_kernel(gpu, case):
    lead, gen = case.solver(), case.solver('generic')
    shape = lead._shape()
    try:
        for which in lf.INPUTS:
            V = lf.inputs(shape)[which]
            for rel_dp in (False, True):
                want = _oracle_sweeps(case.name, which, rel_dp)
                J0 = (_at_ref_zero(V, lead._state_ref_ind), 0.) if rel_dp else V
                assert len(want) == 3 or (which == 'non-finite' and rel_dp)
                for n in (1, 3)[:1 if len(want) < 3 else 2]:
                    what = '{} {} rel_dp={} sweep {}'.format(case, which, rel_dp, n)
                    kw = dict(rel_dp=rel_dp, report_time=False, J_ref_full=True)
                    got = _quiet(lead.value_iterations, J0, n, **kw)
                    _is_lead(lead, case)
                    _check_sweep(lead, got, want[n - 1], rel_dp, what + ': lead / oracle')
                    twin = _quiet(gen.value_iterations, J0, n, **kw)
                    assert gen.backend_info['kernel'] == 'generic'
                    _check_sweep(gen, twin, want[n - 1], rel_dp, what + ': direct kernel / oracle')
        # one sweep through value_iteration (host arrays in and out in one library call): the same bits
        V = lf.inputs(shape)['random']
        got = _quiet(lead.value_iteration, V, report_time=False)
        _is_lead(lead, case)
        _check_sweep(lead, got, _oracle_sweeps(case.name, 'random', False)[0], False, '{}: value_iteration'.format(case))
        J0 = (_at_ref_zero(V, lead._state_ref_ind), 0.)
        (J, ref), pol = _quiet(lead.value_iteration, J0, rel_dp=True, report_time=False)
        _check_sweep(lead, ((J, [ref]), pol), _oracle_sweeps(case.name, 'random', True)[0], True,
                     '{}: value_iteration, rel_dp'.format(case))
    finally:
        _close(lead, gen)


def _policy(solver):
    """a policy that is none of the lattice's: halfway between the box ends, tilted along the first axis"""
    shape = solver._shape()
    nu = len(solver.sys.control)
    pol = np.zeros(shape + (nu,))
    tilt = np.broadcast_to(np.linspace(0.2, 0.8, shape[0]).reshape((-1,) + (1,) * (len(shape) - 1)), shape)
    for ind in np.ndindex(*shape):
        x = tuple(g[i] for g, i in zip(solver.state_grid, ind))
        for c, (lo, hi) in enumerate(solver.sys.control_box(*x)):
            pol[ind + (c,)] = lo + (hi - lo) * tilt[ind]
    return pol


@pytest.mark.parametrize('case', lf.SMALL, ids=_SMALL_IDS)
def test_eval_policy_with_the_fused_shift_and_without(gpu, case):
    lead, gen = case.solver(), case.solver('generic')
    spec = vi_numpy.Spec.from_solver(lead)
    pol = _policy(lead)
    try:
        for which in lf.INPUTS:
            V = lf.inputs(lead._shape())[which]
            what = '{} {}'.format(case, which)
            with np.errstate(all='ignore'):
                wJ, wrefs = vi_numpy.eval_policy(spec, pol, 3, rel_dp=True, J_zero=V.copy(), J_ref_full=True)
            for s in (lead, gen):
                J, refs = _quiet(s.eval_policy, pol, 3, rel_dp=True, J_zero=V, report_time=False, J_ref_full=True)
                name = s.backend_info['kernel']
                _same(J, wJ, '{} eval_policy J ({})'.format(what, name))
                _same(np.asarray(refs, dtype=float), np.asarray(wrefs, dtype=float), '{} eval_policy J_ref ({})'.format(what, name))
            _is_lead(lead, case)
            assert gen.backend_info['kernel'] == 'generic'
            # .. and without the shift
            with np.errstate(all='ignore'):
                wJ = vi_numpy.eval_policy(spec, pol, 3, J_zero=V.copy())
            _same(_quiet(lead.eval_policy, pol, 3, J_zero=V, report_time=False), wJ, what + ' eval_policy, no shift')
            _is_lead(lead, case)
    finally:
        _close(lead, gen)


@pytest.mark.parametrize('name', sorted(n for n, runs in lf.RADIUS_RUNS.items() if 'wide' in runs))
def test_every_node_the_long_way_gives_the_same_bits(gpu, debug_defines, name):
    """every radius x 1e12: no node is decided by the first pass, all of them evaluate every control by the second
    pass on the plane-major copy -- its strides alone are under test"""
    case = lf.BY_NAME[name]
    debug_defines.set(**lf.RADIUS_RUNS[name]['wide'])
    s = case.solver()
    try:
        assert lf.macro(s._kernel_plan()['source'], 'SDP_LEAD_FILTER_SCALE') is not None
        for which in lf.INPUTS:
            V = lf.inputs(s._shape())[which]
            want = _oracle_sweeps(name, which, False)
            for n in (1, 3):
                got = _quiet(s.value_iterations, V, n, report_time=False)
                _is_lead(s, case)
                assert s.backend_info['debug_defines'] == lf.RADIUS_RUNS[name]['wide']
                _check_sweep(s, got, want[n - 1], False, '{} {} radius x 1e12, sweep {}'.format(name, which, n))
    finally:
        _close(s)


def test_a_permuted_form_notices_a_radius_far_too_small(gpu, debug_defines):
    """`flat_permuted` on the cost-to-go whose slopes its cost cancels: the reference's argmin hangs on the last bits
    of its roundings.  Same bits at the proven radius and at half of it; with the radius cut by 1e6 the first pass
    picks its own minimum and the policy index differs somewhere -- so a wrong first pass on a permuted view would
    be noticed by the tests above."""
    case = lf.BY_NAME['flat_permuted']
    want = _oracle_sweeps(case.name, 'flat', False)
    assert len(np.unique(want[0][3])) > 5
    solvers = []
    try:
        def run(kernel='auto'):
            s = case.solver(kernel)
            solvers.append(s)
            V = lf.flat_input(s)
            got = _quiet(s.value_iterations, V, 1, report_time=False)
            return s, got
        gen, got = run('generic')
        assert gen.backend_info['kernel'] == 'generic'
        _check_sweep(gen, got, want[0], False, 'flat: direct kernel / oracle')
        s, got = run()
        _is_lead(s, case)
        _check_sweep(s, got, want[0], False, 'flat: the proven radius')
        s3, got3 = s, _quiet(s.value_iterations, lf.flat_input(s), 3, report_time=False)
        _check_sweep(s3, got3, want[2], False, 'flat: the proven radius, sweep 3')
        debug_defines.set(**lf.RADIUS_RUNS[case.name]['half'])
        s, got = run()
        _is_lead(s, case)
        assert lf.macro(s._kernel_plan()['source'], 'SDP_LEAD_FILTER_SCALE') == '0.5'
        _check_sweep(s, got, want[0], False, 'flat: half the proven radius')
        debug_defines.set(**lf.RADIUS_RUNS[case.name]['far too small'])
        s, got = run()
        _is_lead(s, case)
        assert float(lf.macro(s._kernel_plan()['source'], 'SDP_LEAD_FILTER_SCALE')) == 1e-6
        assert (s.last_policy_index != want[0][3]).sum() > 0
    finally:
        _close(*solvers)


@pytest.mark.timeout(300)
@pytest.mark.parametrize('case', [c for c in lf.CASES if c.sampled], ids=repr)
def test_the_phased_host_path_on_a_permuted_form(gpu, case):
    """`phased_permuted`, 8 MiB of values: value_iteration runs the backup in four phases of the node range
    (sdp_problem_backup_host), value_iterations in one launch"""
    assert case.permuted
    lead, gen = case.solver(), case.solver('generic')
    shape = lead._shape()
    S = int(np.prod(shape))
    nodes = case.sample_nodes(shape)
    V = np.random.default_rng(31).standard_normal(shape)
    spec = vi_numpy.Spec.from_solver(lead)
    try:
        assert lead.host_overlap and V.nbytes >= 8 << 20
        J1, pol1 = _quiet(lead.value_iteration, V, report_time=False)             # phased
        idx1 = lead.last_policy_index.copy()
        _is_lead(lead, case)
        J2, pol2 = _quiet(lead.value_iterations, V, 1, report_time=False)         # one launch
        idx2 = lead.last_policy_index.copy()
        _is_lead(lead, case)
        Jg, polg = _quiet(gen.value_iterations, V, 1, report_time=False)
        idxg = gen.last_policy_index.copy()
        assert gen.backend_info['kernel'] == 'generic'
        for what, (J, pol, idx) in (('phased', (J1, pol1, idx1)), ('one launch', (J2, pol2, idx2))):
            _same(J, Jg, what + ' / direct kernel: J')
            _same(idx, idxg, what + ' / direct kernel: policy index')
            _same(pol, polg, what + ' / direct kernel: policy values')
        _same(J1, J2, 'phased / one launch: J')
        _same(idx1, idx2, 'phased / one launch: policy index')
        _same(pol1, pol2, 'phased / one launch: policy values')
        with np.errstate(all='ignore'):
            Jo, polo, idxo, _ = vi_numpy.value_iteration(spec, V, nodes=nodes)
        assert len(np.unique(idxo)) >= 5
        for what, (J, pol, idx) in (('phased', (J1, pol1, idx1)), ('one launch', (J2, pol2, idx2))):
            _same(J.ravel()[nodes], Jo, what + ' / oracle: J')
            _same(idx.ravel()[nodes], idxo.astype(np.int32), what + ' / oracle: policy index')
            _same(pol.reshape(S, -1)[nodes], polo, what + ' / oracle: policy values')
        # the phased call with the relative-DP shift: J waits for the shift, the policy does not
        ref_flat = int(np.ravel_multi_index(lead._state_ref_ind, shape))
        V0 = _at_ref_zero(V, lead._state_ref_ind)
        (Jr, ref), polr = _quiet(lead.value_iteration, (V0, 0.), rel_dp=True, report_time=False)
        idxr = lead.last_policy_index.copy()
        _is_lead(lead, case)
        (Jrg, refg), polrg = _quiet(gen.value_iteration, (V0, 0.), rel_dp=True, report_time=False)
        _same(Jr, Jrg, 'phased, rel_dp / direct kernel: J')
        _same(idxr, gen.last_policy_index, 'phased, rel_dp / direct kernel: policy index')
        _same(polr, polrg, 'phased, rel_dp / direct kernel: policy values')
        assert float(ref) == float(refg)
        with np.errstate(all='ignore'):
            Jo, polo, idxo, _ = vi_numpy.value_iteration(spec, V0, nodes=np.append(nodes, ref_flat))
        assert float(ref) == float(Jo[-1]) and Jr[lead._state_ref_ind] == 0.
        _same(Jr.ravel()[nodes], Jo[:-1] - Jo[-1], 'phased, rel_dp / oracle: J')
        _same(idxr.ravel()[nodes], idxo[:-1].astype(np.int32), 'phased, rel_dp / oracle: policy index')
        _same(polr.reshape(S, -1)[nodes], polo[:-1], 'phased, rel_dp / oracle: policy values')
    finally:
        _close(lead, gen)
