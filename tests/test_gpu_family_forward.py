"""Transition operators of a family on the device (SolverFamily.transition_operator: kernel sdp_family_transitions, one
stable sort for all members into a block-diagonal CSR, the member-aware k_push / k_push_group and
sdp_transop_push_until_members) against the definition in numpy, stodynprog_amd/forward.py on `solvers[p]` and
`pol[p]`, bit for bit: tocsr(p), mean_cost, push with 1 and 3 steps, and stationary (mu, n_done, converged, delta),
on the cases of tests/family_forward_cases.py; and against the solo device operator of every member where the case
says so."""
import numpy as np
import pytest

import family_forward_cases as ffc
from forward_cases import same
from stodynprog_amd import SolverFamily, FamilyTransitionOperator, forward

pytestmark = pytest.mark.gpu

RUNS = [(case, t_k) for case in ffc.CASES for t_k in case.times]
RUN_IDS = ['{} t_k={}'.format(case.name, t_k) if t_k is not None else case.name for case, t_k in RUNS]


def _same_scalar(a, b):
    return (a != a and b != b) or a == b


def _assert_members(op, ref, what):
    """tocsr(p) and mean_cost of every member are the definition's"""
    assert isinstance(op, FamilyTransitionOperator) and len(op) == len(ref)
    assert op.nnz == sum(e.S * e.W * e.V for e, _ in ref), what
    for p, (e, csr) in enumerate(ref):
        indptr, indices, data = op.tocsr(p)
        assert indptr.dtype == np.int64 and indices.dtype == np.int32 and data.dtype == csr[2].dtype, what
        assert np.array_equal(indptr, csr[0]), '{}: indptr of member {}'.format(what, p)
        assert np.array_equal(indices, csr[1]), '{}: indices of member {}'.format(what, p)
        assert same(data, csr[2]), '{}: data of member {}'.format(what, p)
        assert same(op.mean_cost[p].ravel(), e.mean_cost), '{}: mean cost of member {}'.format(what, p)


def _assert_pushes(op, ref, mu, what):
    for n in (1, 3):
        got = op.push(mu, n)
        assert got.shape == mu.shape and got.dtype == mu.dtype, what
        for p, (e, csr) in enumerate(ref):
            assert same(got[p].ravel(), forward.push(csr, mu[p].ravel(), n)), '{}: push(.., {}) of member {}'.format(what, n, p)
    assert op.info['push_ms'] >= 0 and op.info['pushes'] == 3


def _assert_stationary(res, ref, stat, what, mu0=None):
    """every member's record is forward.stationary's; returns the definition's records"""
    assert isinstance(res, forward.FamilyStationary) and len(res) == len(ref)
    records = []
    for p, (e, csr) in enumerate(ref):
        d = forward.stationary(csr, e.mean_cost, mu0=None if mu0 is None else mu0[p].ravel(), **stat)
        records.append(d)
        where = '{}: stationary of member {} ({} pushes by the definition)'.format(what, p, d.n_done)
        print(where, 'n_done', res.n_done[p], 'converged', res.converged[p], 'delta', res.delta[p], d.delta)
        assert res.n_done[p] == d.n_done == res[p].n_done, where
        assert bool(res.converged[p]) == d.converged == res[p].converged, where
        assert _same_scalar(float(res.delta[p]), d.delta) and _same_scalar(res[p].delta, d.delta), where
        assert same(res.mu[p].ravel(), d.mu), where
        assert same(res[p].mu.ravel(), d.mu), where
        assert _same_scalar(float(res.average_cost[p]), d.average_cost), where
        assert _same_scalar(float(res.mass[p]), float(d.mass)), where
    return records


@pytest.mark.parametrize('case,t_k', RUNS, ids=RUN_IDS)
def test_every_member_is_the_definition(gpu, case, t_k):
    solvers, pol, ref = ffc.reference(case.name, t_k)
    fam = SolverFamily(case.solvers())
    what = '{} t_k={}'.format(case.name, t_k)
    op = fam.transition_operator(pol, t_k)
    try:
        assert op.shape == fam.dims and op.mean_cost.shape == (fam.P,) + fam.dims and op.P == fam.P
        info = fam.backend_info['transition']
        assert info is op.info and info['entries'] == op.nnz and info['chunks'] == 1 and info['members'] == fam.P
        assert info['bytes'] == op.nnz * (case.dtype.itemsize + 4) + 8 * (fam.P * ref[0][0].S + 1)
        assert info['build_ms'] >= 0
        _assert_members(op, ref, what)
        if case.nan:
            assert np.isnan(op.tocsr(0)[2]).any() and not np.isnan(op.tocsr(1)[2]).any()
        mu = ffc.vectors(case, fam.dims)
        _assert_pushes(op, ref, mu, what)
        # one vector for all members
        got = op.push(mu[0], 1)
        for p, (e, csr) in enumerate(ref):
            assert same(got[p].ravel(), forward.push(csr, mu[0].ravel(), 1)), what
        records = _assert_stationary(op.stationary(**case.stat), ref, case.stat, what)
        if case.nan:
            assert np.isnan(records[0].mu).any() and not records[0].converged and not np.isnan(records[1].mu).any()
        if case.name == 'wide':
            assert records[0].converged and records[0].n_done < records[1].n_done == case.stat['n_max']
        # .. and from a start of the caller's, after which a plain push runs every member again
        _assert_stationary(op.stationary(mu0=np.abs(mu), **case.stat), ref, case.stat, what + ' from mu0', np.abs(mu))
        _assert_pushes(op, ref, mu, what + ' after stationary')
    finally:
        op.close()
    with pytest.raises(ValueError, match='closed'):
        op.push(mu)


SOLO = [(case, t_k) for case, t_k in RUNS if case.solo]


@pytest.mark.parametrize('case,t_k', SOLO, ids=[i for i, (c, _) in zip(RUN_IDS, RUNS) if c.solo])
def test_every_member_is_its_solo_device_operator(gpu, case, t_k):
    solvers, pol, ref = ffc.reference(case.name, t_k)
    fam = SolverFamily(case.solvers())
    mu = ffc.vectors(case, fam.dims)
    op = fam.transition_operator(pol, t_k)
    try:
        pushed = op.push(mu, 3)
        res = op.stationary(**case.stat)
        for p, s in enumerate(case.solvers()):
            s.kernel = 'generic'
            solo = s.transition_operator(pol[p], t_k)
            try:
                assert solo.path == 'device'
                for a, b in zip(op.tocsr(p), solo.tocsr()):
                    assert same(a, b), (case.name, p)
                assert same(op.mean_cost[p], solo.mean_cost), (case.name, p)
                assert same(pushed[p], solo.push(mu[p], 3)), (case.name, p)
                one = solo.stationary(**case.stat)
                assert same(res.mu[p], one.mu) and res.n_done[p] == one.n_done and bool(res.converged[p]) == one.converged
                assert _same_scalar(float(res.delta[p]), one.delta) and _same_scalar(res[p].average_cost, one.average_cost)
            finally:
                solo.close()
    finally:
        op.close()


def test_chunks_change_no_bit(gpu):
    case = ffc.CHUNKS
    solvers, pol, ref = ffc.reference(case.name, None)
    mu = ffc.vectors(case, solvers[0]._shape())
    out = {}
    for chunked in (False, True):
        fam = SolverFamily(case.solvers())
        if chunked:
            fam.chunk_bytes = ffc.chunk_bytes_for(fam, 2)
        op = fam.transition_operator(pol)
        try:
            assert op.info['chunks'] == (3 if chunked else 1) and [(a, b) for a, b, _ in op.parts] == (
                [(0, 2), (2, 4), (4, 5)] if chunked else [(0, 5)])
            _assert_members(op, ref, 'chunks')
            res = op.stationary(**case.stat)
            out[chunked] = [op.tocsr(p) for p in range(5)] + [op.mean_cost, op.push(mu, 3), res.mu, res.n_done, res.delta]
            _assert_stationary(res, ref, case.stat, 'chunks')
        finally:
            op.close()
    for a, b in zip(out[False][:5], out[True][:5]):
        assert all(same(x, y) for x, y in zip(a, b))
    for a, b in zip(out[False][5:], out[True][5:]):
        assert same(a, b)
    # the one-call form, chunked as well
    fam = SolverFamily(case.solvers())
    fam.chunk_bytes = ffc.chunk_bytes_for(fam, 2)
    res = fam.stationary_distribution(pol, **case.stat)
    assert same(res.mu, out[False][7]) and fam.backend_info['transition']['chunks'] == 3


def test_members_stop_at_their_own_push(gpu):
    """16 inventory members to a tolerance: the list of running members goes 16 -> 10 -> 5 -> 0; and capped, with checks
    every third push, the slow members end at n_max with the delta of that last check"""
    case = ffc.SHRINK_CASE
    solvers, pol, ref = ffc.reference('shrink', None)
    fam = SolverFamily(case.solvers())
    op = fam.transition_operator(pol)
    try:
        _assert_members(op, ref, 'shrink')
        stat = dict(tol=ffc.SHRINK['tol'], check_every=ffc.SHRINK['check_every'], n_max=ffc.SHRINK['n_max'])
        res = op.stationary(**stat)
        _assert_stationary(res, ref, stat, 'shrink')
        assert res.n_done.tolist() == ffc.SHRINK_PUSHES and res.converged.all()
        assert op.info['pushes'] == max(ffc.SHRINK_PUSHES)
        capped = op.stationary(**ffc.SHRINK_CAPPED)
        records = _assert_stationary(capped, ref, ffc.SHRINK_CAPPED, 'shrink capped')
        n_max = ffc.SHRINK_CAPPED['n_max']
        assert capped.n_done.tolist() == [min(n, n_max) for n in ffc.SHRINK_PUSHES]
        assert capped.converged.tolist() == [n < n_max for n in ffc.SHRINK_PUSHES] and not capped.converged.all()
        assert all(r.delta > ffc.SHRINK_CAPPED['tol'] for r, n in zip(records, ffc.SHRINK_PUSHES) if n > n_max)
        # every row to a wave, and every row to a lane: no result depends on it
        for min_entries in (1, 0):
            op.set_long_rows(min_entries)
            _assert_stationary(op.stationary(**stat), ref, stat, 'shrink, long rows from {}'.format(min_entries))
    finally:
        op.close()


def test_past_the_launch_caps(gpu):
    """more tiles than the entries kernel's grid has workgroups, more rows than k_push's grid has lanes, more nodes a
    member than the reduction covers in one trip: every workgroup walks again"""
    case = ffc.LONG
    cus = gpu.device_info(0)['compute_units']
    S = ffc.LONG_NX
    for name, (wanted, cap) in ffc.caps(len(case.members), S, 1, cus).items():
        assert wanted > cap, (name, wanted, cap)
    solvers, pol, ref = ffc.reference(case.name, None)
    lengths = np.concatenate([np.diff(csr[0]) for _, csr in ref])
    assert (lengths < ffc.PUSH_LONG).any() and (lengths >= ffc.PUSH_LONG).any()        # both push paths run
    fam = SolverFamily(solvers)
    op = fam.transition_operator(pol)
    try:
        _assert_members(op, ref, case.name)
        mu = ffc.vectors(case, fam.dims)
        got = op.push(mu, 2)
        for p, (e, csr) in enumerate(ref):
            assert same(got[p], forward.push(csr, mu[p], 2)), p
        _assert_stationary(op.stationary(**case.stat), ref, case.stat, case.name)
        # every row to a lane: all of k_push's lanes have a row
        op.set_long_rows(0)
        got = op.push(mu, 1)
        for p, (e, csr) in enumerate(ref):
            assert same(got[p], forward.push(csr, mu[p], 1)), p
    finally:
        op.close()
