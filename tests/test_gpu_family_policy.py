"""Policy evaluation and iteration of families on the device (tests/family_policy_cases.py): member p of every result
of SolverFamily.eval_policy / policy_iteration equals, with np.array_equal, what a fresh `solvers[p]` with
kernel = 'generic' returns from the same method -- in both forms of the evaluation, a launch per step ('steps') and all
steps of a member in one workgroup with its values in LDS ('resident').  The cases to a tolerance, the shapes of the
resident walk and the cases past the launch caps are compared with oracle/vi_numpy.py, so no device kernel is their
reference."""
import functools

import numpy as np
import pytest

import family_cases as fc
import family_policy_cases as pc
from oracle import vi_numpy
from stodynprog_amd import SolverFamily, _native as nat

pytestmark = pytest.mark.gpu

FORMS = ['steps', 'resident']
BY_NAME = {c.name: c for c in fc.STATIONARY}


def _solo(case):
    out = case.solvers()
    for s in out:
        s.kernel = 'generic'
    return out


def _family(case, form):
    fam = SolverFamily(case.solvers())
    fam.evaluation = form
    return fam


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(J_zero [P] + dims, pol [P] + dims + (nu,)) of a STATIONARY case: a start that differs per member, and the
    policy of fam.value_iteration on it plus a small offset per node -- off the control lattice"""
    case = BY_NAME[name]
    J0 = fc.start(case)
    _, pol = SolverFamily(case.solvers()).value_iteration(J0)
    pol = pc.off_lattice(pol, case)
    J0.setflags(write=False)
    pol.setflags(write=False)
    return J0, pol


@functools.lru_cache(maxsize=None)
def solo_eval(name, n_iter, rel_dp):
    """the solo eval_policy of every member, once per session: (J, reference costs of every step or None)"""
    J0, pol = inputs(name)
    out = []
    for p, s in enumerate(_solo(BY_NAME[name])):
        got = s.eval_policy(pol[p], n_iter, rel_dp, J_zero=J0[p], report_time=False, J_ref_full=True)
        out.append(got if rel_dp else (got, None))
    return out


@functools.lru_cache(maxsize=None)
def solo_iteration(name, rel_dp):
    J0, pol = inputs(name)
    out = []
    for p, s in enumerate(_solo(BY_NAME[name])):
        J, polp = s.policy_iteration(pol[p], 7, 2, rel_dp)
        out.append((J if rel_dp else (J, None)) + (polp, np.array(s.last_policy_index)))
    return out


def _same_record(got, want):
    assert got.n_iter == want.n_iter and got.converged == want.converged and got.checked == want.checked
    assert got.tol == want.tol and got.check_every == want.check_every
    for field in ('dmin', 'dmax', 'span', 'lower', 'upper'):
        assert np.array_equal(getattr(got, field), getattr(want, field), equal_nan=True), field


# ----------------------------------------------------------------------------------------------------------------------
# against the solo calls

@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('rel_dp', [False, True], ids=['plain', 'rel_dp'])
@pytest.mark.parametrize('n_iter', [1, 5])
@pytest.mark.parametrize('case', fc.STATIONARY, ids=repr)
def test_eval_policy_is_the_solo_call(case, n_iter, rel_dp, form, capsys):
    J0, pol = inputs(case.name)
    want = solo_eval(case.name, n_iter, rel_dp)
    capsys.readouterr()
    fam = _family(case, form)
    got = fam.eval_policy(pol, n_iter, rel_dp, J_zero=J0, J_ref_full=True)
    assert capsys.readouterr().out == ''                                # the solo progress lines are not printed
    J, refs = got if rel_dp else (got, None)
    assert J.shape == (fam.P,) + fam.dims and fam.last_convergence is None
    for p, (Jp, refp) in enumerate(want):
        assert J[p].dtype == Jp.dtype and np.array_equal(J[p], Jp), ('J', p)
        if rel_dp:
            assert refs[p].shape == (n_iter,) and np.array_equal(refs[p], refp), ('J_ref', p)
    info = fam.backend_info
    assert info['kernel'] == 'family' and info['evaluation'] == form and info['chunks'] == 1
    S, rs = int(np.prod(fam.dims)), fam.dtype.itemsize
    assert info['evaluation_lds_bytes'] == (2 * S * rs + pc.RESIDENT_REDUCTION_BYTES if form == 'resident' else 0)
    if rel_dp:
        # without J_ref_full: the last reference cost of every member
        _, last = fam.eval_policy(pol, n_iter, True, J_zero=J0)
        assert last.shape == (fam.P,) and np.array_equal(last, [r[-1] for r in refs])
    if case.dtype == np.float32:
        for p, s in enumerate(case.solvers()):
            o = vi_numpy.eval_policy_real(vi_numpy.Spec.from_solver(s), pol[p], n_iter, np.float32, rel_dp, J_zero=J0[p],
                                          J_ref_full=True)
            Jo, refo = o if rel_dp else (o, None)
            assert np.array_equal(J[p], Jo) and (not rel_dp or np.array_equal(refs[p], refo)), p


def test_auto_takes_the_resident_form_from_two_steps_on():
    case = BY_NAME['storage_ar1 f64']
    J0, pol = inputs(case.name)
    fam = SolverFamily(case.solvers())
    assert fam.evaluation == 'auto'
    for n_iter, form in ((1, 'steps'), (2, 'resident'), (5, 'resident')):
        J = fam.eval_policy(pol, n_iter, J_zero=J0)
        assert fam.backend_info['evaluation'] == form == pc.form(35, np.float64, n_iter)
        if n_iter == 5:
            assert all(np.array_equal(J[p], Jp) for p, (Jp, _) in enumerate(solo_eval(case.name, 5, False)))
    # no steps: the start itself
    assert np.array_equal(fam.eval_policy(pol, 0, J_zero=J0), J0)


@pytest.mark.parametrize('form', FORMS)
def test_a_policy_of_shape_dims_nu_is_every_members_policy(form):
    case = BY_NAME['storage_ar1 f64']
    J0, pol = inputs(case.name)
    fam = _family(case, form)
    J, refs = fam.eval_policy(pol[1], 3, True, J_zero=J0[2])
    J_all, refs_all = fam.eval_policy(np.stack([pol[1]] * fam.P), 3, True, J_zero=np.stack([J0[2]] * fam.P))
    assert np.array_equal(J, J_all) and np.array_equal(refs, refs_all)
    for p, s in enumerate(_solo(case)):
        Jp, refp = s.eval_policy(pol[1], 3, True, J_zero=J0[2], report_time=False)
        assert np.array_equal(J[p], Jp) and refs[p] == refp, p


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('rel_dp', [False, True], ids=['plain', 'rel_dp'])
@pytest.mark.parametrize('case', fc.STATIONARY, ids=repr)
def test_policy_iteration_is_the_solo_call(case, rel_dp, form, capsys):
    _, pol0 = inputs(case.name)
    want = solo_iteration(case.name, rel_dp)
    capsys.readouterr()
    fam = _family(case, form)
    got, pol = fam.policy_iteration(pol0, 7, 2, rel_dp)
    assert capsys.readouterr().out == ''
    J, refs = got if rel_dp else (got, None)
    assert fam.last_convergence is None and fam.backend_info['evaluation'] == form
    for p, (Jp, refp, polp, idxp) in enumerate(want):
        assert J[p].dtype == Jp.dtype and np.array_equal(J[p], Jp), ('J', p)
        assert np.array_equal(pol[p], polp), ('policy', p)
        assert np.array_equal(fam.last_policy_index[p], idxp), ('index', p)
        if rel_dp:
            assert refs.shape == (fam.P,) and refs[p] == refp, ('J_ref', p)


# ----------------------------------------------------------------------------------------------------------------------
# to a tolerance

@pytest.mark.parametrize('form', FORMS)
def test_evaluation_to_a_tolerance_stops_every_member_at_its_own_step(form):
    t = pc.SHRINK
    case = fc.Case('shrink', t['members'])
    pol = pc.shrink_policies()
    fam = _family(case, form)
    J, refs = fam.eval_policy(pol, t['n_iter'], True, tol=t['tol'], check_every=t['check_every'], J_ref_full=True)
    records = fam.last_convergence
    assert [r.n_iter for r in records] == pc.SHRINK_STEPS and all(r.converged for r in records)
    assert [len(r) for r in refs] == pc.SHRINK_STEPS
    for p, s in enumerate(_solo(case)):
        Jp, refp = s.eval_policy(pol[p], t['n_iter'], True, report_time=False, J_ref_full=True, tol=t['tol'],
                                 check_every=t['check_every'])
        _same_record(records[p], s.last_convergence)
        assert np.array_equal(J[p], Jp) and np.array_equal(refs[p], refp), p
        # .. which is the call with n_iter = the steps the member ran
        Jk, refk = s.eval_policy(pol[p], pc.SHRINK_STEPS[p], True, report_time=False, J_ref_full=True)
        assert np.array_equal(J[p], Jk) and np.array_equal(refs[p], refk), p
    # every third step checked and a cap of 17: the members that need 18 steps stop at the cap with a last check there
    c = pc.SHRINK_CAPPED
    J, refs = fam.eval_policy(pol, c['n_iter'], True, tol=t['tol'], check_every=c['check_every'], J_ref_full=True)
    records = fam.last_convergence
    for p, s in enumerate(_solo(case)):
        Jp, refp = s.eval_policy(pol[p], c['n_iter'], True, report_time=False, J_ref_full=True, tol=t['tol'],
                                 check_every=c['check_every'])
        _same_record(records[p], s.last_convergence)
        assert np.array_equal(J[p], Jp) and np.array_equal(refs[p], refp), p
        need = pc.SHRINK_STEPS[p]
        if need == 18:
            assert records[p].n_iter == 17 and records[p].checked[-1] == 17 and not records[p].converged
        else:
            assert records[p].n_iter == (15 if need <= 15 else 17) and records[p].converged


@pytest.mark.parametrize('form', FORMS)
def test_policy_iteration_to_a_tolerance_is_the_solo_call(form, capsys):
    t = pc.LINE
    case = fc.Case('line tol', t['members'])
    pol0 = pc.line_policies()
    fam = _family(case, form)
    (J, refs), pol = fam.policy_iteration(pol0, t['n_val'], t['n_pol'], True, tol=t['tol'], check_every=t['check_every'])
    assert capsys.readouterr().out == ''
    records = fam.last_convergence
    assert [r.n_improvements for r in records] == pc.LINE_IMPROVEMENTS and all(r.stable for r in records)
    assert [r.evaluations[0].n_iter for r in records] == pc.LINE_STEPS
    for p, s in enumerate(_solo(case)):
        (Jp, refp), polp = s.policy_iteration(pol0[p], t['n_val'], t['n_pol'], True, tol=t['tol'], check_every=t['check_every'])
        want = s.last_convergence
        assert records[p].n_improvements == want.n_improvements and records[p].stable == want.stable
        assert len(records[p].evaluations) == len(want.evaluations)
        for a, b in zip(records[p].evaluations, want.evaluations):
            _same_record(a, b)
        assert np.array_equal(J[p], Jp) and refs[p] == refp and np.array_equal(pol[p], polp), p
        assert np.array_equal(fam.last_policy_index[p], s.last_policy_index), p
    capsys.readouterr()


# ----------------------------------------------------------------------------------------------------------------------
# shapes of the resident walk

@pytest.mark.parametrize('n_x', pc.walk_sizes())
def test_resident_walk(n_x):
    case = pc.walk_case(n_x)
    pol = pc.line_policy(case)
    J0 = fc.line_start(case)
    Jo, refo, _ = pc.oracle_eval(case.members[0], pol[0], 3, True, J_zero=J0[0])
    fits = n_x <= pc.resident_nodes(np.float64)
    fam = SolverFamily(case.solvers())
    got = {}
    for form in ['steps', 'auto'] + (['resident'] if fits else []):
        fam.evaluation = form
        got[form] = fam.eval_policy(pol, 3, True, J_zero=J0, J_ref_full=True)
        assert fam.backend_info['evaluation'] == (form if form != 'auto' else pc.form(n_x, np.float64, 3))
        J, refs = got[form]
        assert np.array_equal(J[0], Jo) and np.array_equal(refs[0], refo), form
    if not fits:
        fam.evaluation = 'resident'
        with pytest.raises(ValueError) as err:
            fam.eval_policy(pol, 3, True, J_zero=J0)
        assert str(2 * n_x * 8) in str(err.value)


# ----------------------------------------------------------------------------------------------------------------------
# past every new launch cap

@pytest.mark.parametrize('case', [pc.LONG, pc.STRIDED], ids=repr)
def test_the_steps_kernel_walks_past_its_cap(case):
    cus = nat.device_info(0)['compute_units']
    S, P = case.members[0]()._shape()[0], len(case.members)
    grid = pc.launch_steps(S, P, cus)
    assert grid['wanted'] > cus and max(grid['units']) > grid['per_xcd'] == cus, grid      # a second trip
    pol = pc.line_policy(case)
    J0 = fc.line_start(case)
    fam = _family(case, 'auto')
    J, refs = fam.eval_policy(pol, 2, True, J_zero=J0, J_ref_full=True)
    assert fam.backend_info['evaluation'] == 'steps'
    for p, make in enumerate(case.members):
        Jo, refo, _ = pc.oracle_eval(make, pol[p], 2, True, J_zero=J0[p])
        assert np.array_equal(J[p], Jo) and np.array_equal(refs[p], refo), p
    # the statistics launch (64 workgroups of 256 nodes a member at most) and the shift of the members that stop
    fam.eval_policy(pol, 2, True, J_zero=J0, tol=0., check_every=1)
    for p, make in enumerate(case.members[:2]):
        _, _, checks = pc.oracle_eval(make, pol[p], 2, True, J_zero=J0[p], tol=0.)
        rec = fam.last_convergence[p]
        assert rec.checked == [1, 2] and np.array_equal(rec.dmin, [c[1] for c in checks]) \
            and np.array_equal(rec.dmax, [c[2] for c in checks]), p


def test_the_resident_kernel_strides_over_more_members_than_workgroups():
    cus = nat.device_info(0)['compute_units']
    case = pc.many(cus + 3)
    grid = pc.launch_resident(len(case.members), cus)
    assert grid['wanted'] > grid['blocks'] == cus
    rng = np.random.default_rng(11)
    pol = rng.uniform(0., 4., size=(len(case.members), 10, 1))
    fam = _family(case, 'resident')
    J, refs = fam.eval_policy(pol, 3, True, J_ref_full=True)
    for p, make in enumerate(case.members):
        Jo, refo, _ = pc.oracle_eval(make, pol[p], 3, True)
        assert np.array_equal(J[p], Jo) and np.array_equal(refs[p], refo), p
    # the policy compare (one block row a member) on as many members: the improvement of a stable policy
    fam.evaluation = 'steps'
    (J1, r1), pol1 = fam.policy_iteration(pol, 3, 1, True)
    (J2, r2), pol2 = fam.policy_iteration(pol1, 3, 5, True, tol=0.)
    rec = fam.last_convergence
    for p in (0, cus, cus + 2):
        spec = vi_numpy.Spec.from_solver(case.members[p]())
        _, polo, _, _ = vi_numpy.value_iteration_real(spec, (J1[p], 0.), np.float64, True)
        want_stable = np.array_equal(polo, pol1[p])
        assert (rec[p].n_improvements == 1 and rec[p].stable) == want_stable, p


def test_the_policy_compare_past_its_64_workgroups():
    """k_family_policy_differs launches at most 64 workgroups of 256 values a member: the last 129 values of
    family_cases.LONG are a second trip.  The sweep's policy, known on the host, is compared on the device with copies
    of itself that differ in one value"""
    case = fc.LONG
    fam = SolverFamily(case.solvers())
    S = fc.LONG_NX
    assert S * fam.nu > 64 * 256
    _, pol = fam.value_iteration(fc.line_start(case))
    prob = fam._handle[1]
    prob.set_policy(pol)
    assert prob.compare_policy().tolist() == [True, True]
    for p, node, value in ((0, S - 1, 0.5), (1, 64 * 256, 0.5), (1, 0, 0.5), (0, S - 2, np.nan)):
        other = pol.copy()
        other[p, node, 0] = value if np.isnan(value) else other[p, node, 0] + value
        prob.set_policy(other)
        assert prob.compare_policy().tolist() == [q != p for q in range(2)], (p, node)


# ----------------------------------------------------------------------------------------------------------------------
# chunks

@pytest.mark.parametrize('form', FORMS)
def test_chunks_change_no_bit(form):
    case = fc.CHUNKS
    whole, cut = _family(case, form), _family(case, form)
    tabs = cut._tables()
    cut.chunk_bytes = (cut._member_bytes(tabs) + cut._policy_bytes()) * 2 + cut._member_bytes(tabs) // 2
    assert cut._chunks(tabs, cut._policy_bytes()) == [(0, 2), (2, 4), (4, 5)]
    J0 = fc.start(case)
    _, pol = whole.value_iteration(J0)
    pol = pc.off_lattice(pol, case)
    a = whole.eval_policy(pol, 6, True, J_zero=J0, J_ref_full=True)
    b = cut.eval_policy(pol, 6, True, J_zero=J0, J_ref_full=True)
    assert whole.backend_info['chunks'] == 1 and cut.backend_info['chunks'] == 3
    assert np.array_equal(a[0], b[0]) and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))
    a = whole.policy_iteration(pol, 6, 3, True, tol=1e-3)
    b = cut.policy_iteration(pol, 6, 3, True, tol=1e-3)
    assert cut.backend_info['chunks'] == 3
    assert np.array_equal(a[0][0], b[0][0]) and np.array_equal(a[0][1], b[0][1]) and np.array_equal(a[1], b[1])
    assert [(r.n_improvements, r.stable, [e.n_iter for e in r.evaluations]) for r in whole.last_convergence] \
        == [(r.n_improvements, r.stable, [e.n_iter for e in r.evaluations]) for r in cut.last_convergence]
