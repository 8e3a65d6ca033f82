"""Families of same-shaped problems on the device (tests/family_cases.py): member p of every result of a SolverFamily
equals, with np.array_equal, what a fresh `solvers[p]` with kernel = 'generic' returns from the same method -- value,
policy values, lattice indices, reference costs and convergence records; the solo side is never the code under test."""
import functools

import numpy as np
import pytest

import family_cases as fc
from stodynprog_amd import SolverFamily

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
