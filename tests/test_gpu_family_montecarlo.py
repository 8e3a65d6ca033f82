"""Monte Carlo evaluation of families on the device (tests/family_mc_cases.py): member p of every field of
`SolverFamily.monte_carlo` equals, with np.array_equal, what `solvers[p].monte_carlo` returns on its device path
(kernel sdp_montecarlo of the member's own unit) -- for every way the kernel maps members to XCDs, past the bound of
its grid, however the run is cut into launches, batches and member chunks, with one seed or one per member, with the
members' own laws or the caller's, and with grid ends that differ from member to member."""
import functools

import numpy as np
import pytest

import family_cases as fc
import family_mc_cases as mcc
from stodynprog_amd import SolverFamily, montecarlo as mc, _native as nat

pytestmark = pytest.mark.gpu

FIELDS = ('cost_sum', 'cost_mean', 'n_outside', 'x_final', 'occupancy')


def _family(case):
    return SolverFamily(case.solvers())


def _solo(case):
    return mcc.solo(case.solvers())


@functools.lru_cache(maxsize=None)
def policy(name):
    """(P,) + dims + (nu,): one value iteration of a zero cost-to-go, on the device"""
    case = {c.name: c for c in mcc.FAMILIES}[name]
    fam = _family(case)
    _, pol = fam.value_iteration(np.zeros(fam.dims))
    fam.close()
    pol.setflags(write=False)
    return pol


def _same_member(one, ref, what):
    assert one.path == ref.path == 'device', what
    for name in FIELDS:
        a, b = getattr(one, name), getattr(ref, name)
        if b is None:
            assert a is None, (what, name)
            continue
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.dtype, b.dtype, a.shape, b.shape)
        assert np.array_equal(a, b), (what, name, int((a != b).sum()))
    # (a NaN mean -- a member that left its grid for good -- is the same NaN)
    assert np.array_equal([one.mean, one.stderr], [ref.mean, ref.stderr], equal_nan=True), what
    assert (one.n_steps, one.n_burn, one.seed, one.traj_offset, one.n_traj) == \
        (ref.n_steps, ref.n_burn, ref.seed, ref.traj_offset, ref.n_traj), what


def _compare(res, solvers, pol, x0, n_steps, seeds, what, laws=None, **kw):
    """every member of a family result against the solo call"""
    assert len(res) == len(solvers)
    for p, s in enumerate(solvers):
        ref = s.monte_carlo(pol[p], x0[p] if x0.ndim == 3 else x0, n_steps, seed=seeds[p] if np.ndim(seeds) else seeds,
                            law=None if laws is None else laws[p], **kw)
        _same_member(res[p], ref, '{} member {}'.format(what, p))
        for name in FIELDS[:4]:
            assert np.array_equal(getattr(res, name)[p], getattr(ref, name)), (what, p, name)
        assert np.array_equal([res.mean[p], res.stderr[p]], [ref.mean, ref.stderr], equal_nan=True), (what, p)


@pytest.mark.parametrize('case', mcc.PARITY, ids=repr)
def test_parity_with_the_solo_call(case):
    fam, pol = _family(case), policy(case.name)
    x0 = mcc.starts(case, mcc.B_PARITY)
    kw = dict(n_burn=mcc.N_BURN, occupancy=True, traj_offset=1000)
    res = fam.monte_carlo(pol, x0, mcc.N_STEPS, seed=3, **kw)
    assert res.cost_sum.dtype == res.x_final.dtype == fam.dtype and res.n_outside.dtype == np.int64
    assert res.cost_sum.shape == (fam.P, mcc.B_PARITY) and res.x_final.shape == x0.shape
    assert res.occupancy.shape == (fam.P,) + fam.dims and res.occupancy.dtype == np.int64
    assert np.all(res.occupancy.reshape(fam.P, -1).sum(axis=1) == mcc.B_PARITY * (mcc.N_STEPS - mcc.N_BURN))
    info = fam.backend_info['monte_carlo']
    assert info == dict(members=fam.P, n_traj=mcc.B_PARITY, chunks=1, launches=1) and fam.last_kernel_ms() > 0
    solvers = _solo(case)
    _compare(res, solvers, pol, x0, mcc.N_STEPS, 3, repr(case), **kw)
    # without the occupancy: the same reductions
    bare = fam.monte_carlo(pol, x0, mcc.N_STEPS, seed=3, n_burn=mcc.N_BURN, traj_offset=1000)
    assert bare.occupancy is None and bare[0].occupancy is None
    for name in FIELDS[:4]:
        assert np.array_equal(getattr(bare, name), getattr(res, name)), name
    if case.name == 'storage_ar1 f64':
        # one member once more from the definition: its draws in numpy, replayed through simulate, summed on the host
        p = 1
        s = solvers[p]
        _, w = fam.monte_carlo_draws(3, mcc.B_PARITY, mcc.N_STEPS, traj_offset=1000)
        x, _, g = s.simulate(pol[p], x0[p], w[p])
        acc = np.zeros(mcc.B_PARITY, dtype=s.dtype)
        for k in range(mcc.N_BURN, mcc.N_STEPS):
            acc = acc + g[k].astype(s.dtype)
        assert np.array_equal(res.cost_sum[p], acc) and np.array_equal(res.x_final[p], x[-1])
        smin, smax = [g_[0] for g_ in s.state_grid], [g_[-1] for g_ in s.state_grid]
        outside = ~np.all((x[mcc.N_BURN:mcc.N_STEPS] >= smin) & (x[mcc.N_BURN:mcc.N_STEPS] <= smax), axis=2)
        assert np.array_equal(res.n_outside[p], outside.sum(axis=0))
        occ = np.zeros(fam.dims, dtype=np.int64)
        np.add.at(occ, tuple(mc.nearest_nodes(x[mcc.N_BURN:mcc.N_STEPS], s.state_grid, s.dtype).reshape(-1, 2).T), 1)
        assert np.array_equal(res.occupancy[p], occ)
    fam.close()


@functools.lru_cache(maxsize=None)
def line_policies():
    """member p of a line family is the same problem whatever P: the policies of the largest family serve them all"""
    return policy(mcc.MAPPING[max(mcc.MAPPING_P)].name)


@functools.lru_cache(maxsize=None)
def line_solo(p, B, n_steps):
    """line member p alone: its policy and its solo result"""
    pol = line_policies()[p]
    s = mcc.solo([fc.line_members(p + 1, fc.LINE_NX)[p]()])[0]
    return pol, s.monte_carlo(pol, line_starts(B), n_steps, seed=5, occupancy=True)


def line_starts(B):
    return np.random.default_rng(B).uniform(-1.5, 1.5, size=(B, 1))


def _line_family(P, B, n_steps):
    fam = _family(mcc.MAPPING[P])
    pol = np.stack([line_solo(p, B, n_steps)[0] for p in range(P)])
    res = fam.monte_carlo(pol, line_starts(B), n_steps, seed=5, occupancy=True)
    for p in range(P):
        _same_member(res[p], line_solo(p, B, n_steps)[1], 'line P={} member {}'.format(P, p))
    fam.close()
    return res


@pytest.mark.parametrize('P', mcc.MAPPING_P)
def test_every_mapping_of_members_to_xcds(P):
    plan = mcc.launch(mcc.B_MAPPING, P, 256, 8)
    assert plan['tiles'] == 2 and mcc.B_MAPPING % 256 == 1             # the second tile has one live lane
    _line_family(P, mcc.B_MAPPING, mcc.STEPS_MAPPING)


def test_past_the_launch_cap():
    cus = nat.device_info(0)['compute_units']
    B = mcc.cap_batch(cus)
    assert B % 256 == 1 and 9 * (-(-B // 256)) > 8 * cus
    for per_cu in range(1, 9):
        plan = mcc.launch(B, 9, cus, per_cu)
        assert max(trip for xcd in plan['visits'] for _, _, trip in xcd) >= 1      # a second trip of the stride loop
    _line_family(9, B, mcc.STEPS_CAP)


def test_cuts_change_no_bit():
    case = mcc.CUTS
    fam, pol = _family(case), policy(case.name)
    B, T = 70, mcc.STEPS_CUTS
    x0 = mcc.starts(case, B)
    kw = dict(seed=9, n_burn=3, occupancy=True, traj_offset=12)
    whole = fam.monte_carlo(pol, x0, T, **kw)
    assert fam.backend_info['monte_carlo']['launches'] == 1
    _compare(whole, _solo(case), pol, x0, T, 9, 'cuts', n_burn=3, occupancy=True, traj_offset=12)

    def same(res, what):
        for name in FIELDS:
            assert np.array_equal(getattr(res, name), getattr(whole, name)), (what, name)
        assert np.array_equal(res.mean, whole.mean) and np.array_equal(res.stderr, whole.stderr)
    # launches of 1, 7 and 1024 steps
    for spl in (1, 7, 1024):
        fam.steps_per_launch = spl
        same(fam.monte_carlo(pol, x0, T, **kw), 'steps_per_launch = {}'.format(spl))
        assert fam.backend_info['monte_carlo']['launches'] == -(-T // spl)
    del fam.steps_per_launch
    # the batch in two calls
    cut = 37
    a = fam.monte_carlo(pol, x0[:, :cut], T, **kw)
    b = fam.monte_carlo(pol, x0[:, cut:], T, **dict(kw, traj_offset=12 + cut))
    for name in FIELDS[:4]:
        assert np.array_equal(np.concatenate([getattr(a, name), getattr(b, name)], axis=1), getattr(whole, name)), name
    assert np.array_equal(a.occupancy + b.occupancy, whole.occupancy)
    # the members in chunks of 2 + 2 + 1
    fam.chunk_bytes = mcc.chunk_bytes_for(fam, 2, B, 3, True)
    same(fam.monte_carlo(pol, x0, T, **kw), 'chunks')
    assert fam.backend_info['monte_carlo'] == dict(members=5, n_traj=B, chunks=3, launches=3)
    assert fam.last_kernel_ms() is None
    fam.close()


def test_seeds():
    case = mcc.SEEDS
    fam, pol = _family(case), policy(case.name)
    x0 = mcc.starts(case, 65)[0]                                        # (B, d): shared
    # (the members' own law has three points, the outer two of weight 3e-4: a law whose draws tell two seeds apart)
    law = mcc.shared_law()
    one = fam.monte_carlo(pol, x0, 20, seed=4, law=law)
    assert one.seeds == (4, 4)
    for name in FIELDS[:4]:
        assert np.array_equal(getattr(one, name)[0], getattr(one, name)[1]), name
    assert one.paired(0, 1) == (0., 0.)
    two = fam.monte_carlo(pol, x0, 20, seed=(4, 5), law=law)
    assert two.seeds == (4, 5) and not np.array_equal(two.cost_sum[0], two.cost_sum[1])
    assert np.array_equal(two.cost_sum[0], one.cost_sum[0])
    _compare(two, _solo(case), pol, x0, 20, (4, 5), 'seeds', laws=[law] * 2)
    with pytest.raises(ValueError):
        two.paired(0, 1)
    fam.close()
    # members that differ, one seed: the paired difference by its definition
    case = mcc.LAWS
    fam, pol = _family(case), policy(case.name)
    x0 = np.broadcast_to(mcc.starts(case, 65)[0], (3, 65, 2)) * np.array([0.2, 1.])     # inside every member's grid
    res = fam.monte_carlo(pol, x0, 20, seed=6, law=law)
    diff = res.cost_mean[0] - res.cost_mean[1]
    assert res.paired(0, 1) == (float(diff.mean()), float(diff.std(ddof=1) / np.sqrt(65)))
    assert res.paired(0, 1)[1] > 0
    fam.close()


def test_laws():
    case = mcc.LAWS
    fam, pol = _family(case), policy(case.name)
    x0 = mcc.starts(case, mcc.B_PARITY)
    solvers = _solo(case)
    kw = dict(n_burn=2, occupancy=True)
    # a law per member, none of them the solver's own
    laws = mcc.member_laws()
    res = fam.monte_carlo(pol, x0, mcc.N_STEPS, seed=11, law=laws, **kw)
    _compare(res, solvers, pol, x0, mcc.N_STEPS, 11, 'law per member', laws=laws, **kw)
    own = fam.monte_carlo(pol, x0, mcc.N_STEPS, seed=11, **kw)
    assert not np.array_equal(own.cost_sum, res.cost_sum)
    # 70 points: the binary search of the index
    long_ = mcc.long_law()
    res = fam.monte_carlo(pol, x0, mcc.N_STEPS, seed=11, law=long_, **kw)
    _compare(res, solvers, pol, x0, mcc.N_STEPS, 11, 'long law', laws=[long_] * 3, **kw)
    # one law for all members
    shared = mcc.shared_law()
    res = fam.monte_carlo(pol, x0, mcc.N_STEPS, seed=11, law=shared, **kw)
    _compare(res, solvers, pol, x0, mcc.N_STEPS, 11, 'shared law', laws=[shared] * 3, **kw)
    fam.close()


def test_outside_counts_per_member():
    case = mcc.OUTSIDE
    fam, pol = _family(case), policy(case.name)
    x0 = mcc.outside_starts()
    res = fam.monte_carlo(pol, x0, mcc.STEPS_OUTSIDE, seed=3)
    assert res.n_outside[0].sum() == 0 and res.n_outside[1].sum() > 0
    assert np.all(res.n_outside[1] >= 1)                                # (every start lies outside member 1's grid)
    _compare(res, _solo(case), pol, x0, mcc.STEPS_OUTSIDE, 3, 'outside')
    fam.close()


def test_the_other_methods_return_what_they_returned_before():
    case = mcc.LAWS
    fam, pol = _family(case), policy(case.name)
    J0 = fc.start(case)
    before = fam.value_iteration(J0), fam.eval_policy(pol, 6, rel_dp=True)
    handle = fam._handle[1]
    res = fam.monte_carlo(pol, mcc.starts(case, mcc.B_PARITY), mcc.N_STEPS, seed=2, occupancy=True)
    assert fam._handle[1] is handle                                     # the handle is reused
    after = fam.value_iteration(J0), fam.eval_policy(pol, 6, rel_dp=True)
    again = fam.monte_carlo(pol, mcc.starts(case, mcc.B_PARITY), mcc.N_STEPS, seed=2, occupancy=True)
    for a, b in zip(before[0] + before[1], after[0] + after[1]):
        assert np.array_equal(a, b)
    for name in FIELDS:
        assert np.array_equal(getattr(res, name), getattr(again, name)), name
    fam.close()
