"""Families of same-shaped problems on the device (tests/family_cases.py): member p of every result of a SolverFamily
equals, with np.array_equal, what a fresh `solvers[p]` with kernel = 'generic' returns from the same method -- value,
policy values, lattice indices, reference costs and convergence records; the solo side is never the code under test.  The cases made
with oracle=True -- every mapping of listed members to XCDs, more than 64 members, a walk past the launch cap, a list
that shrinks through the mappings -- are compared with oracle/vi_numpy.py instead, so no device kernel is their
reference."""
import functools

import numpy as np
import pytest

import family_cases as fc
from stodynprog_amd import SolverFamily, _native as nat

pytestmark = pytest.mark.gpu

BY_NAME = {c.name: c for c in fc.CASES}


def _solo(case):
    out = case.solvers()
    for s in out:
        s.kernel = 'generic'
    return out


def _rel_start(case, J0):
    """the start with the reference node of every member at zero"""
    J0 = np.array(J0)
    ref = case.solvers()[0]._state_ref_ind
    J0[(slice(None),) + ref] = 0.
    return J0


@functools.lru_cache(maxsize=None)
def solo_results(name, method, rel_dp=False):
    """the solo calls of a case, once per session: per member (J, J_ref or None, pol, idx)"""
    case = BY_NAME[name]
    J0 = fc.start(case)
    if rel_dp:
        J0 = _rel_start(case, J0)
    out = []
    for p, s in enumerate(_solo(case)):
        start = (J0[p], 0.) if rel_dp else J0[p]
        if method == 'value_iteration':
            J, pol = s.value_iteration(start, rel_dp, report_time=False)
        else:
            J, pol = s.value_iterations(start, 5, rel_dp, report_time=False)
        J, ref = J if rel_dp else (J, None)
        out.append((J, ref, pol, np.array(s.last_policy_index)))
    return out


def _same(fam, got, want, rel_dp):
    J, pol = got
    J, refs = J if rel_dp else (J, None)
    idx = fam.last_policy_index
    assert J.shape == (fam.P,) + fam.dims and pol.shape == (fam.P,) + fam.dims + (fam.nu,)
    assert idx.shape == (fam.P,) + fam.dims and idx.dtype == np.int32
    for p, (Jp, ref, polp, idxp) in enumerate(want):
        assert J[p].dtype == Jp.dtype
        assert np.array_equal(J[p], Jp, equal_nan=True), ('J', p)
        assert np.array_equal(pol[p], polp, equal_nan=True), ('policy', p)
        assert np.array_equal(idx[p], idxp), ('index', p)
        if rel_dp:
            assert refs.shape == (fam.P,) and refs[p] == ref, ('J_ref', p)


@pytest.mark.parametrize('rel_dp', [False, True], ids=['plain', 'rel_dp'])
@pytest.mark.parametrize('case', fc.STATIONARY, ids=repr)
def test_value_iteration_is_the_solo_call(case, rel_dp):
    fam = SolverFamily(case.solvers())
    J0 = fc.start(case)
    if rel_dp:
        J0 = _rel_start(case, J0)
    got = fam.value_iteration((J0, np.zeros(fam.P)) if rel_dp else J0, rel_dp)
    _same(fam, got, solo_results(case.name, 'value_iteration', rel_dp), rel_dp)
    info = fam.backend_info
    assert info['kernel'] == 'family' and info['members'] == fam.P and info['chunks'] == 1
    assert info['lanes'] == max(s._box_plan()['lanes'] for s in fam.solvers)
    assert info['lifted_constants'] == len(fam.solvers[0]._trace_now(None).param_values()) and info['module'].endswith('.hsaco')
    assert fam.last_convergence is None


@pytest.mark.parametrize('rel_dp', [False, True], ids=['plain', 'rel_dp'])
@pytest.mark.parametrize('case', fc.STATIONARY, ids=repr)
def test_five_value_iterations_are_the_solo_call(case, rel_dp):
    fam = SolverFamily(case.solvers())
    J0 = fc.start(case)
    if rel_dp:
        J0 = _rel_start(case, J0)
    got = fam.value_iterations((J0, np.zeros(fam.P)) if rel_dp else J0, 5, rel_dp)
    _same(fam, got, solo_results(case.name, 'value_iterations', rel_dp), rel_dp)
    if rel_dp:
        (_, full), _ = fam.value_iterations((J0, 0.), 5, True, J_ref_full=True)
        assert isinstance(full, list) and len(full) == fam.P and all(r.shape == (5,) for r in full)
        for p, s in enumerate(_solo(case)):
            (_, want), _ = s.value_iterations((J0[p], 0.), 5, True, report_time=False, J_ref_full=True)
            assert np.array_equal(full[p], want)


def test_a_start_of_shape_dims_is_every_members_start():
    case = BY_NAME['storage_ar1 f64']
    fam = SolverFamily(case.solvers())
    J0 = fc.start(case, per_member=False)
    assert J0.shape == fam.dims
    J, pol = fam.value_iterations(J0, 2)
    J_all, pol_all = fam.value_iterations(np.stack([J0] * fam.P), 2)
    assert np.array_equal(J, J_all) and np.array_equal(pol, pol_all)
    for p, s in enumerate(_solo(case)):
        Jp, polp = s.value_iterations(J0, 2, report_time=False)
        assert np.array_equal(J[p], Jp) and np.array_equal(pol[p], polp)


@pytest.mark.parametrize('case', fc.HORIZON, ids=repr)
def test_bellman_recursion_is_the_solo_call(case, capsys):
    fam = SolverFamily(case.solvers())
    T = case.horizon
    J_fin = fc.start(case)
    J, pol = fam.bellman_recursion(T, J_fin)
    assert J.shape == (fam.P, T) + fam.dims and pol.shape == (fam.P, T) + fam.dims + (fam.nu,)
    assert fam.backend_info['kernel'] == 'family'
    assert fam.backend_info['time_specialized'] == case.name.startswith('pv')
    for p, s in enumerate(_solo(case)):
        Jp, polp = s.bellman_recursion(T, J_fin[p], report_time=False)
        assert J[p].dtype == Jp.dtype and np.array_equal(J[p], Jp), ('J', p)
        assert np.array_equal(pol[p], polp), ('policy', p)
        assert np.array_equal(fam.last_policy_index[p], s.last_policy_index), ('index', p)
    capsys.readouterr()
    # a start of shape dims
    J1, pol1 = fam.bellman_recursion(T, J_fin[0])
    assert np.array_equal(J1[0], J[0]) and np.array_equal(pol1[0], pol[0])


def test_chunks_change_no_bit():
    case = fc.CHUNKS
    whole = SolverFamily(case.solvers())
    cut = SolverFamily(case.solvers())
    cut.chunk_bytes = fc.chunk_bytes_for(cut, 2)
    J0 = _rel_start(case, fc.start(case))
    for rel_dp in (False, True):
        start = (J0, 0.) if rel_dp else J0
        a = whole.value_iterations(start, 3, rel_dp)
        b = cut.value_iterations(start, 3, rel_dp)
        assert whole.backend_info['chunks'] == 1 and cut.backend_info['chunks'] == 3
        Ja, Jb = (a[0][0], b[0][0]) if rel_dp else (a[0], b[0])
        assert np.array_equal(Ja, Jb) and np.array_equal(a[1], b[1])
        assert np.array_equal(whole.last_policy_index, cut.last_policy_index)
        if rel_dp:
            assert np.array_equal(a[0][1], b[0][1])
    # .. and with members leaving the list at different sweeps
    a = whole.value_iterations((J0, 0.), 60, True, tol=1e-3, check_every=2)
    b = cut.value_iterations((J0, 0.), 60, True, tol=1e-3, check_every=2)
    assert [r.n_iter for r in whole.last_convergence] == [r.n_iter for r in cut.last_convergence]
    assert np.array_equal(a[0][0], b[0][0]) and np.array_equal(a[0][1], b[0][1]) and np.array_equal(a[1], b[1])
    # the first members are those of the storage_ar1 case
    want = solo_results('storage_ar1 f64', 'value_iterations', False)
    J5, _ = whole.value_iterations(np.concatenate([fc.start(BY_NAME['storage_ar1 f64']), J0[3:]]), 5)
    for p in range(3):
        assert np.array_equal(J5[p], want[p][0])


def test_run_to_a_tolerance_is_the_solo_call_member_by_member():
    t = fc.TOL
    case = fc.Case('tol', t['members'])
    fam = SolverFamily(case.solvers())
    J0 = np.zeros(fam.dims)
    (J, refs), pol = fam.value_iterations((J0, 0.), t['n_iter'], True, tol=t['tol'], check_every=t['check_every'],
                                          J_ref_full=True)
    records = fam.last_convergence
    assert len(records) == fam.P and isinstance(refs, list)
    counts = []
    for p, s in enumerate(_solo(case)):
        (Jp, refp), polp = s.value_iterations((J0, 0.), t['n_iter'], True, report_time=False, J_ref_full=True,
                                              tol=t['tol'], check_every=t['check_every'])
        want, got = s.last_convergence, records[p]
        counts.append(want.n_iter)
        assert got.n_iter == want.n_iter and got.converged == want.converged and got.checked == want.checked
        assert got.tol == want.tol and got.check_every == want.check_every
        for field in ('dmin', 'dmax', 'span', 'lower', 'upper'):
            assert np.array_equal(getattr(got, field), getattr(want, field)), (field, p)
        assert np.array_equal(J[p], Jp) and np.array_equal(pol[p], polp) and np.array_equal(refs[p], refp)
        assert np.array_equal(fam.last_policy_index[p], s.last_policy_index)
        # .. which is the call with n_iter = the sweeps the member ran
        twin = _solo(case)[p]
        (Jk, refk), polk = twin.value_iterations((J0, 0.), want.n_iter, True, report_time=False)
        assert np.array_equal(J[p], Jk) and np.array_equal(pol[p], polk) and refs[p][-1] == refk
    print('sweeps per member:', counts)
    assert len(set(counts)) > 1 and max(counts) < t['n_iter'] and all(r.converged for r in records)
    # J_ref without J_ref_full: the last reference cost of every member
    (_, last), _ = fam.value_iterations((J0, 0.), t['n_iter'], True, tol=t['tol'], check_every=t['check_every'])
    assert last.shape == (fam.P,) and np.array_equal(last, [r[-1] for r in refs])
    # n_iter reached by nobody's tolerance: every member runs all sweeps, and the record says so
    fam.value_iterations((J0, 0.), 4, True, tol=0., check_every=3)
    assert [r.n_iter for r in fam.last_convergence] == [4] * fam.P and [r.checked for r in fam.last_convergence] == [[3, 4]] * fam.P
    for p, s in enumerate(_solo(case)):
        s.value_iterations((J0, 0.), 4, True, report_time=False, tol=0., check_every=3)
        assert np.array_equal(fam.last_convergence[p].dmax, s.last_convergence.dmax)
        assert fam.last_convergence[p].converged == s.last_convergence.converged


# ----------------------------------------------------------------------------------------------------------------------
# every way the kernel maps listed members to XCDs, and the second trip of its walk (the cases of family_cases.py
# made with oracle=True): the reference is oracle/vi_numpy.py per member, never a device kernel

@functools.lru_cache(maxsize=None)
def line_oracle(n_x, dtype, p, n_iter, rel_dp):
    """member p of every line family on n_x nodes: per sweep (J, J_ref or None, pol, idx), once per session"""
    case = fc.Case('line', fc.line_members(p + 1, n_x, dtype), dtype=dtype, oracle=True)
    J0 = fc.line_start(case)
    if rel_dp:
        J0 = _rel_start(case, J0)
    out, _ = fc.oracle_sweeps(case.members[p], J0[p], n_iter, rel_dp)
    return out


def _line_want(case, n_iter, rel_dp):
    n_x = case.members[0]()._shape()[0]
    return [line_oracle(n_x, case.dtype.type, p, n_iter, rel_dp) for p in range(len(case.members))]


def _same_as_oracle(fam, got, want, rel_dp, n_iter, full=False):
    """`got` of value_iteration (n_iter = 1) or value_iterations against the oracle's sweep n_iter, every node of
    every member; J_ref is the last reference cost, or with `full` the history"""
    J, pol = got
    J, refs = J if rel_dp else (J, None)
    idx = fam.last_policy_index
    assert J.shape == (fam.P,) + fam.dims and J.dtype == fam.dtype
    assert pol.shape == (fam.P,) + fam.dims + (fam.nu,) and pol.dtype == fam.dtype
    assert idx.shape == (fam.P,) + fam.dims and idx.dtype == np.int32
    for p, sweeps in enumerate(want):
        Jp, _, polp, idxp = sweeps[n_iter - 1]
        assert np.array_equal(J[p], Jp, equal_nan=True), ('J', p)
        assert np.array_equal(pol[p], polp, equal_nan=True), ('policy', p)
        assert np.array_equal(idx[p], idxp), ('index', p)
        if rel_dp and full:
            assert np.array_equal(refs[p], [s[1] for s in sweeps[:n_iter]]), ('J_ref history', p)
        elif rel_dp:
            assert refs[p] == sweeps[n_iter - 1][1], ('J_ref', p)


def _cus():
    return nat.device_info(0)['compute_units']


@pytest.mark.parametrize('case', fc.MAPPING, ids=repr)
def test_every_mapping_of_members_to_xcds_against_the_oracle(case):
    fam = SolverFamily(case.solvers())
    P, S = fam.P, int(np.prod(fam.dims))
    grid = fc.launch(S, fam._tables()['lanes'], P, _cus())
    # the form this P is for: several members on an XCD, one XCD a member with idle XCDs, several XCDs a member
    assert grid['tiles'] == 3 and S % 4
    if P >= 8:
        assert grid['parts'] == 1 and max(grid['units']) == -(-P // 8) * 3 and (P % 8 == 0 or min(grid['units']) < max(grid['units']))
    elif P >= 5:
        assert grid['parts'] == 1 and grid['units'].count(0) == 8 - P
    else:
        assert grid['parts'] == 8 // P > 1 and grid['parts'] * max(grid['units']) >= 3
    assert grid['per_xcd'] == max(grid['units'])                        # (no second trip here: that is `strided`)
    J0 = fc.line_start(case)
    got = fam.value_iteration(J0)
    assert fam.backend_info['kernel'] == 'family' and fam.backend_info['lanes'] == 64 and fam.backend_info['chunks'] == 1
    _same_as_oracle(fam, got, _line_want(case, 1, False), False, 1)
    J0 = _rel_start(case, J0)
    want = _line_want(case, 3, True)
    _same_as_oracle(fam, fam.value_iteration((J0, np.zeros(P)), True), want, True, 1)
    got = fam.value_iterations((J0, 0.), 3, True, J_ref_full=True)
    assert isinstance(got[0][1], list) and all(r.shape == (3,) for r in got[0][1])
    _same_as_oracle(fam, got, want, True, 3, full=True)


def test_more_members_than_a_block_of_the_reference_pick():
    case = fc.MANY
    fam = SolverFamily(case.solvers())
    assert fam.P > 64                                                   # k_family_pick_ref: blocks of 64 members
    J0 = _rel_start(case, fc.line_start(case))
    got = fam.value_iteration((J0, np.zeros(fam.P)), True)
    assert fam.backend_info['chunks'] == 1
    _same_as_oracle(fam, got, _line_want(case, 3, True), True, 1)
    assert got[0][1].shape == (fam.P,) and len(set(got[0][1].tolist())) == fam.P      # (every member its own J_ref)


@pytest.mark.parametrize('case', fc.STRIDED, ids=repr)
def test_the_strided_walk_against_the_oracle(case):
    fam = SolverFamily(case.solvers())
    P, S = fam.P, int(np.prod(fam.dims))
    cus = _cus()
    grid = fc.launch(S, fam._tables()['lanes'], P, cus)
    # past the cap: every XCD walks its units with a stride of per_xcd = cus workgroups, the XCDs with two members
    # have 2 * tiles units and XCD 0, with three, 3 * tiles
    assert S % 4 and grid['tiles'] == 129 and 2 * grid['tiles'] > cus, (grid, cus)
    assert grid['per_xcd'] == cus and min(grid['units']) == 2 * grid['tiles'] > grid['per_xcd']
    assert grid['units'][0] == 3 * grid['tiles'] >= grid['per_xcd'] * 3 // 2
    J0 = fc.line_start(case)
    got = fam.value_iteration(J0)
    assert fam.backend_info['lanes'] == 64 and fam.backend_info['chunks'] == 1
    want = _line_want(case, 1, False)
    assert min(len(np.unique(w[0][3])) for w in want) > 8               # (the argmin moves along the grid)
    _same_as_oracle(fam, got, want, False, 1)


def test_a_list_that_shrinks_through_every_mapping():
    t = fc.SHRINK
    case = fc.SHRINK_CASE
    fam = SolverFamily(case.solvers())
    J0 = np.zeros(fam.dims)
    (J, refs), pol = fam.value_iterations((J0, 0.), t['n_iter'], True, tol=t['tol'], check_every=t['check_every'],
                                          J_ref_full=True)
    records = fam.last_convergence
    assert len(records) == fam.P and isinstance(refs, list) and fam.backend_info['chunks'] == 1
    counts = []
    for p, make in enumerate(t['members']):
        sweeps, checks = fc.oracle_sweeps(make, J0, t['n_iter'], True, t['tol'], t['check_every'])
        n = len(sweeps)
        counts.append(n)
        Jp, _, polp, idxp = sweeps[-1]
        got = records[p]
        assert got.n_iter == n and got.converged and got.checked == [c[0] for c in checks] == list(range(1, n + 1)), p
        assert got.tol == t['tol'] and got.check_every == t['check_every']
        assert np.array_equal(got.dmin, [c[1] for c in checks]) and np.array_equal(got.dmax, [c[2] for c in checks]), p
        ref_hist = np.array([s[1] for s in sweeps])
        assert np.array_equal(refs[p], ref_hist), ('J_ref history', p)
        assert np.array_equal(got.span, got.dmax - got.dmin)
        assert np.array_equal(got.lower, got.dmin + ref_hist) and np.array_equal(got.upper, got.dmax + ref_hist)
        assert got.span[-1] <= t['tol'] and (got.span[:-1] > t['tol']).all(), p       # convergence.py's rule
        assert np.array_equal(J[p], Jp) and np.array_equal(pol[p], polp), p
        assert np.array_equal(fam.last_policy_index[p], idxp), p
    print('sweeps per member:', counts)
    assert counts == fc.SHRINK_SWEEPS and fc.list_sizes(counts, t['n_iter']) == fc.SHRINK_SIZES


def test_chunks_of_eight_members_and_more_change_no_bit():
    case = fc.CHUNKS_17
    whole = SolverFamily(case.solvers())
    cut = SolverFamily(case.solvers())
    cut.chunk_bytes = fc.chunk_bytes_for(cut, 9)
    assert cut._chunks(cut._tables()) == [(0, 9), (9, 17)]
    J0 = _rel_start(case, fc.line_start(case))
    want = _line_want(case, 3, True)
    a = whole.value_iterations((J0, 0.), 3, True, J_ref_full=True)
    b = cut.value_iterations((J0, 0.), 3, True, J_ref_full=True)
    assert whole.backend_info['chunks'] == 1 and cut.backend_info['chunks'] == 2
    assert np.array_equal(a[0][0], b[0][0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(whole.last_policy_index, cut.last_policy_index)
    assert all(np.array_equal(x, y) for x, y in zip(a[0][1], b[0][1]))
    _same_as_oracle(cut, b, want, True, 3, full=True)
    _same_as_oracle(whole, a, want, True, 3, full=True)


def test_shift_and_statistics_past_their_64_workgroups():
    """k_family_shift and sdp_family_diff_stats run at most 64 workgroups of 256 nodes a member: on 64 * 256 + 129 nodes
    the last 129 are a second trip.  The backup against the oracle on those nodes, on the first and last node of every
    XCD's part and on a sample; the shift against J - J[ref] of the plain call's own array; the statistics against
    convergence.diff_stats of the downloaded arrays, with the extremes of the first check among the last 129 nodes"""
    from oracle import vi_numpy
    from stodynprog_amd import convergence as conv
    case = fc.LONG
    fam = SolverFamily(case.solvers())
    S = fam.dims[0]
    second = 64 * 256
    assert S == second + 129 and -(-S // 256) > 64                       # bx of family_backup and sdp_family_vi_until
    grid = fc.launch(S, 64, fam.P, _cus())
    assert grid['parts'] == 4 and min(grid['units']) > 2 * grid['per_xcd']          # and the backup walks three times
    J0 = _rel_start(case, fc.line_start(case))
    J0[:, S - 50], J0[:, S - 90] = 1e3, -1e3
    J, pol = fam.value_iteration(J0)
    idx = fam.last_policy_index
    per_part = -(-grid['tiles'] // 4) * 4                                # nodes of a part
    nodes = np.unique(np.concatenate([np.arange(second, S), np.arange(0, S, per_part), np.arange(per_part - 1, S, per_part),
                                      np.random.default_rng(2).choice(S, 300, replace=False)]))
    for p, s in enumerate(fam.solvers):
        Jo, polo, idxo, _ = vi_numpy.value_iteration_real(vi_numpy.Spec.from_solver(s), J0[p], fam.dtype, nodes=nodes)
        assert np.array_equal(J[p][nodes], Jo) and np.array_equal(pol[p][nodes], polo) and np.array_equal(idx[p][nodes], idxo), p
    ref = fam.solvers[0]._state_ref_ind
    (J1, refs), pol1 = fam.value_iteration((J0, np.zeros(fam.P)), True)
    for p in range(fam.P):
        assert refs[p] == J[p][ref] and np.array_equal(J1[p], J[p] - J[p][ref]), p
    assert np.array_equal(pol1, pol)
    (J2, _), _ = fam.value_iterations((J0, 0.), 2, True, tol=0., check_every=1)
    for p, rec in enumerate(fam.last_convergence):
        assert rec.n_iter == 2 and rec.checked == [1, 2]
        d = J1[p] - J0[p]
        assert min(d.argmin(), d.argmax()) >= second
        assert (rec.dmin[0], rec.dmax[0]) == conv.diff_stats(J1[p], J0[p], fam.dtype), p
        assert (rec.dmin[1], rec.dmax[1]) == conv.diff_stats(J2[p], J1[p], fam.dtype), p
