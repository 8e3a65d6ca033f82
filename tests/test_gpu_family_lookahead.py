"""One-step lookahead and its Monte Carlo score for families on the device (tests/family_lookahead_cases.py): member p
of every result of `SolverFamily.lookahead` / `SolverFamily.monte_carlo_lookahead` equals, with np.array_equal, (1) what
`solvers[p].lookahead` / `.monte_carlo_lookahead` returns on its device path and (2) the pinned oracle chained step by
step on `monte_carlo_draws` -- for every way the kernels map members to XCDs, past the bound of their grid, however
the run is cut into launches, batches and member chunks, with one seed or one per member, with the members' own laws or
the caller's, with grid ends that differ from member to member, and at a state without a valid lattice."""
import functools

import numpy as np
import pytest

import family_lookahead_cases as flc
import lookahead_cases as lc
import mc_lookahead_cases as mlc
from stodynprog_amd import _native as nat

pytestmark = pytest.mark.gpu

FIELDS = ('cost_sum', 'cost_mean', 'n_outside', 'x_final', 'occupancy')
SEED, OFFSET, T, N_BURN = flc.SEED, flc.OFFSET, flc.T, flc.N_BURN


@functools.lru_cache(maxsize=None)
def cost_to_go(name):
    case = {c.name: c for c in flc.FAMILIES}[name]
    J = flc.cost_to_go(case)
    J.setflags(write=False)
    return J


def _same_member(one, ref, what):
    assert one.path == ref.path == 'device', what
    for name in FIELDS:
        a, b = getattr(one, name), getattr(ref, name)
        if b is None:
            assert a is None, (what, name)
            continue
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.dtype, b.dtype, a.shape, b.shape)
        assert np.array_equal(a, b), (what, name, int((a != b).sum()))
    assert np.array_equal([one.mean, one.stderr], [ref.mean, ref.stderr], equal_nan=True), what
    assert (one.n_steps, one.n_burn, one.seed, one.traj_offset, one.n_traj) == \
        (ref.n_steps, ref.n_burn, ref.seed, ref.traj_offset, ref.n_traj), what


def _against_solo(res, case, J, x0, n_steps, seeds, what, laws=None, **kw):
    for p, s in enumerate(case.solvers()):
        ref = s.monte_carlo_lookahead(J[p], x0[p] if x0.ndim == 3 else x0, n_steps, seed=seeds[p] if np.ndim(seeds) else seeds,
                                      law=None if laws is None else laws[p], **kw)
        assert s.backend_info['lookahead_path'] == 'device' and s.backend_info['lookahead_box'] == 'device', what
        _same_member(res[p], ref, '{} member {}'.format(what, p))


def _against_oracle(res, case, J, x0, n_steps, n_burn, what, occupancy=True, rows=None, traj_offset=OFFSET):
    """every member of a family result against the oracle's closed loop; rows: a slice of the trajectories only"""
    for p in range(len(case.members)):
        x0_p = x0[p] if x0.ndim == 3 else x0
        if rows is None:
            want = flc.oracle_monte_carlo(case, p, J[p], x0_p, n_steps, n_burn, traj_offset=traj_offset, occupancy=occupancy)
            mlc.check(res[p], want, '{} member {}'.format(what, p), occupancy=occupancy)
        else:
            want = flc.oracle_monte_carlo(case, p, J[p], x0_p[rows], n_steps, n_burn, traj_offset=traj_offset + rows.start,
                                          occupancy=False)
            one = res[p]
            assert mlc.same(one.cost_sum[rows], want[0]) and mlc.same(one.n_outside[rows], want[1]), (what, p)
            assert mlc.same(one.x_final[rows], want[2]), (what, p)


# ----------------------------------------------------------------------------------------------------------------------
# parity

@pytest.mark.parametrize('case', flc.PARITY, ids=repr)
def test_lookahead_equals_the_solo_calls_and_the_oracle(case):
    fam = flc.family(case)
    J = cost_to_go(case.name)
    x = flc.states(case)
    tile = flc.tile(case)
    for xs in (x, x[:, :tile + 1], x[0]):
        J_opt, u_opt, idx = fam.lookahead(J, xs, case.t_k)
        P, B = len(fam), xs.shape[-2]
        assert J_opt.shape == (P, B) and u_opt.shape == (P, B, fam.nu) and idx.shape == (P, B) and idx.dtype == np.int32
        assert J_opt.dtype == u_opt.dtype == fam.dtype
        info = fam.backend_info
        assert (info['kernel'], info['lookahead_path'], info['lookahead_box']) == ('family', 'device', 'device'), info
        for p, s in enumerate(case.solvers()):
            ref = s.lookahead(J[p], xs[p] if xs.ndim == 3 else xs, case.t_k)
            assert s.backend_info['lookahead_box'] == 'device'
            for a, b, name in zip((J_opt[p], u_opt[p], idx[p]), ref, ('J', 'u', 'idx')):
                assert a.dtype == b.dtype and mlc.same(a, b), (case, p, name, B)
        want = flc.oracle_lookahead(case, J, xs)
        for a, b, name in zip((J_opt, u_opt, idx), want, ('J', 'u', 'idx')):
            assert mlc.same(a, b.astype(a.dtype)), (case, name, B)
    fam.close()


@pytest.mark.parametrize('occupancy', (True, False), ids=('occupancy', 'plain'))
@pytest.mark.parametrize('case', flc.PARITY, ids=repr)
def test_monte_carlo_equals_the_solo_calls_and_the_oracle(case, occupancy):
    fam = flc.family(case)
    J = cost_to_go(case.name)
    B = (64 // fam._tables(None if fam.stationnary else case.t0)['lanes']) * 4 + 1      # a workgroup's tile and one more group
    x0 = flc.starts(case, B)
    kw = dict(n_burn=N_BURN, occupancy=occupancy, traj_offset=OFFSET, t0=case.t0)
    res = fam.monte_carlo_lookahead(J, x0, T, seed=SEED, **kw)
    assert res.path == 'device' and res.seeds == (SEED,) * len(fam) and fam.backend_info['lookahead_box'] == 'device'
    assert res.cost_sum.shape == (len(fam), B) and res.cost_sum.dtype == fam.dtype
    _against_solo(res, case, J, x0, T, SEED, repr(case), **kw)
    _against_oracle(res, case, J, x0, T, N_BURN, repr(case), occupancy=occupancy)
    # common random numbers: the paired difference is that of the members' own results
    diff = res[0].cost_mean - res[1].cost_mean
    assert res.paired(0, 1) == (float(diff.mean()), float(diff.std(ddof=1) / np.sqrt(B)))
    if occupancy:
        # once more under plant laws that make every point of the members' grids likely (their own hardly leave the middle)
        laws = flc.spread_laws(case)
        spread = fam.monte_carlo_lookahead(J, x0, T, seed=SEED, law=laws, **kw)
        assert not mlc.same(spread.x_final, res.x_final)
        _against_solo(spread, case, J, x0, T, SEED, repr(case) + ' spread', laws=laws, **kw)
        for p in range(len(fam)):
            want = flc.oracle_monte_carlo(case, p, J[p], x0[p], T, N_BURN, law=laws[p])
            mlc.check(spread[p], want, '{} spread member {}'.format(case, p))
    fam.close()


# ----------------------------------------------------------------------------------------------------------------------
# mapping and cap: the oracle alone

@pytest.mark.parametrize('P', flc.MAPPING_P)
def test_every_mapping_of_members_to_xcds(P):
    case = flc.MAPPING[P]
    fam = flc.family(case)
    J = cost_to_go(case.name)
    x0 = flc.starts(case, flc.B_MAPPING)
    J_opt, u_opt, idx = fam.lookahead(J, x0)
    for a, b, name in zip((J_opt, u_opt, idx), flc.oracle_lookahead(case, J, x0), ('J', 'u', 'idx')):
        assert mlc.same(a, b), (P, name)
    res = fam.monte_carlo_lookahead(J, x0, flc.STEPS_MAPPING, seed=SEED, n_burn=1, occupancy=True, traj_offset=OFFSET)
    _against_oracle(res, case, J, x0, flc.STEPS_MAPPING, 1, repr(case))
    fam.close()


def test_a_batch_past_the_grid_bound():
    case = flc.CAP
    fam = flc.family(case)
    P = len(fam)
    cus = nat.device_info(0)['compute_units']
    B = flc.cap_batch(cus)
    assert P * -(-B // 4) > 8 * cus and B % 4 == 1
    J = cost_to_go(case.name)
    # every row carries one of a few distinct states: the lookahead is a function of a row's own inputs
    distinct = flc.starts(case, 7)
    pick = lc.repeated_rows(B, 7)
    x = distinct[:, pick]
    J_opt, u_opt, idx = fam.lookahead(J, x)
    for a, b, name in zip((J_opt, u_opt, idx), flc.oracle_lookahead(case, J, distinct), ('J', 'u', 'idx')):
        assert mlc.same(a, b[:, pick]), name
    # the closed loop: the whole batch equals its parts below the bound, and the rows of the first and of the last
    # tiles -- member 8's are reached in the second trip of XCD 0's workgroups -- the oracle's
    run = lambda lo, hi: fam.monte_carlo_lookahead(J, x[:, lo:hi], flc.STEPS_CAP, seed=SEED, n_burn=1, occupancy=True,
                                                   traj_offset=OFFSET + lo)
    big = run(0, B)
    assert int(big.occupancy.sum()) == P * B * (flc.STEPS_CAP - 1)
    cuts = (0, B // 3, B // 3 + 131, B)
    parts = [run(lo, hi) for lo, hi in zip(cuts[:-1], cuts[1:])]
    for name in ('cost_sum', 'n_outside', 'x_final'):
        assert mlc.same(np.concatenate([getattr(q, name) for q in parts], axis=1), getattr(big, name)), name
    assert mlc.same(sum(q.occupancy for q in parts), big.occupancy)
    for rows in (slice(0, 6), slice(B - 9, B)):
        _against_oracle(big, case, J, x, flc.STEPS_CAP, 1, 'cap', rows=rows)
    fam.close()


# ----------------------------------------------------------------------------------------------------------------------
# cuts, laws, seeds, outside, no lattice

def test_no_cut_changes_a_bit():
    case = flc.CUTS
    fam = flc.family(case)
    J = cost_to_go(case.name)
    B = 21
    x0 = flc.starts(case, B)
    kw = dict(seed=SEED, n_burn=N_BURN, occupancy=True)
    whole = fam.monte_carlo_lookahead(J, x0, T, traj_offset=OFFSET, **kw)
    assert fam.backend_info['chunks'] == 1
    _against_solo(whole, case, J, x0, T, SEED, 'cuts', n_burn=N_BURN, occupancy=True, traj_offset=OFFSET)
    look = fam.lookahead(J, x0)

    def same(res, what):
        for name in FIELDS:
            assert mlc.same(getattr(res, name), getattr(whole, name)), (what, name)
    for spl in (1, 3, T):
        fam.steps_per_launch = spl
        same(fam.monte_carlo_lookahead(J, x0, T, traj_offset=OFFSET, **kw), spl)
        assert fam.backend_info['monte_carlo']['launches'] == -(-T // spl)
    del fam.steps_per_launch
    # a batch split over two calls by traj_offset
    lo = fam.monte_carlo_lookahead(J, x0[:, :8], T, traj_offset=OFFSET, **kw)
    hi = fam.monte_carlo_lookahead(J, x0[:, 8:], T, traj_offset=OFFSET + 8, **kw)
    for name in ('cost_sum', 'n_outside', 'x_final'):
        assert mlc.same(np.concatenate([getattr(lo, name), getattr(hi, name)], axis=1), getattr(whole, name)), name
    assert mlc.same(lo.occupancy + hi.occupancy, whole.occupancy)
    # member chunks 2 + 2 + 1, in both calls
    n_box = fam.backend_info['box_constants']
    fam.chunk_bytes = flc.chunk_bytes_for(fam, 2, flc.mc_extra_bytes(fam, B, 3, True, n_box))
    same(fam.monte_carlo_lookahead(J, x0, T, traj_offset=OFFSET, **kw), 'chunks')
    assert fam.backend_info['chunks'] == 3
    rs, d = fam.dtype.itemsize, len(fam.dims)
    fam.chunk_bytes = flc.chunk_bytes_for(fam, 2, (d + 1 + fam.nu) * B * rs + 4 * B + 8 * (n_box + fam.nu))
    for a, b in zip(fam.lookahead(J, x0), look):
        assert mlc.same(a, b)
    assert fam.backend_info['chunks'] == 3
    fam.close()


def test_the_plant_draws_from_the_callers_law_and_the_backup_keeps_the_members_own():
    case = flc.LAWS
    fam = flc.family(case)
    J = cost_to_go(case.name)
    B = 9
    x0 = flc.starts(case, B)
    kw = dict(n_burn=N_BURN, occupancy=True, traj_offset=OFFSET)
    for laws, law in ((flc.member_laws(), flc.member_laws()), ([flc.long_law()] * len(fam), flc.long_law())):
        res = fam.monte_carlo_lookahead(J, x0, T, seed=SEED, law=law, **kw)
        # (the solo call sums its backup over the solver's own law whatever `law` is: equal bits say the family did too)
        _against_solo(res, case, J, x0, T, SEED, 'laws', laws=laws, **kw)
        for p in range(len(fam)):
            want = flc.oracle_monte_carlo(case, p, J[p], x0[p], T, N_BURN, law=laws[p])
            mlc.check(res[p], want, 'laws member {}'.format(p))
    own = fam.monte_carlo_lookahead(J, x0, T, seed=SEED, **kw)
    assert not mlc.same(own.cost_sum, res.cost_sum)
    fam.close()


def test_one_seed_gives_identical_members_identical_results():
    case = flc.SEEDS
    fam = flc.family(case)
    J = np.broadcast_to(cost_to_go(case.name)[0], (2,) + fam.dims)
    x0 = flc.starts(case, 9)[0]
    law = flc.spread_laws(case)[0]             # (a plant law under which the draws differ from step to step)
    one = fam.monte_carlo_lookahead(J, x0, T, seed=SEED, n_burn=N_BURN, law=law)
    assert mlc.same(one.cost_sum[0], one.cost_sum[1]) and mlc.same(one.x_final[0], one.x_final[1])
    assert one.paired(0, 1) == (0.0, 0.0)
    two = fam.monte_carlo_lookahead(J, x0, T, seed=(SEED, SEED + 1), n_burn=N_BURN, law=law)
    assert mlc.same(two.cost_sum[0], one.cost_sum[0]) and not mlc.same(two.x_final[1], one.x_final[1])
    _against_solo(two, case, J, x0, T, (SEED, SEED + 1), 'seeds', laws=[law, law], n_burn=N_BURN)
    fam.close()


def test_a_member_counts_what_lies_outside_its_own_grid():
    case = flc.OUTSIDE
    fam = flc.family(case)
    J = cost_to_go(case.name)
    x0 = flc.outside_starts()
    res = fam.monte_carlo_lookahead(J, x0, T, seed=SEED, occupancy=True, traj_offset=OFFSET)
    assert res.n_outside[0].sum() == 0 and res.n_outside[1].sum() > 0 and np.all(res.n_outside[1] >= 1)
    _against_solo(res, case, J, x0, T, SEED, 'outside', occupancy=True, traj_offset=OFFSET)
    _against_oracle(res, case, J, x0, T, 0, 'outside')
    fam.close()


def test_a_state_without_a_lattice():
    case = flc.NO_LATTICE
    fam = flc.family(case)
    J = cost_to_go(case.name)
    B, row = 9, flc.NAN_ROW
    x0 = flc.starts(case, B)
    x0[:, row] = lc.NAN_STATE
    J_opt, u_opt, idx = fam.lookahead(J, x0)
    keep = np.arange(B) != row
    assert np.isnan(J_opt[:, row]).all() and np.isnan(u_opt[:, row]).all() and (idx[:, row] == -1).all()
    want = flc.oracle_lookahead(case, J, x0[:, keep])
    for a, b, name in zip((J_opt, u_opt, idx), want, ('J', 'u', 'idx')):
        assert mlc.same(a[:, keep], b), name
    for p, s in enumerate(case.solvers()):
        for a, b in zip((J_opt[p], u_opt[p], idx[p]), s.lookahead(J[p], x0[p])):
            assert mlc.same(a, b), p
    res = fam.monte_carlo_lookahead(J, x0, T, seed=SEED, n_burn=N_BURN, occupancy=True, traj_offset=OFFSET)
    assert np.isnan(res.cost_sum[:, row]).all() and (res.n_outside[:, row] == T - N_BURN).all()
    for p in range(len(fam)):
        want = flc.oracle_monte_carlo(case, p, J[p], x0[p], T, N_BURN, nan_rows=(row,))
        mlc.check(res[p], want, 'no lattice member {}'.format(p))
        assert not np.isnan(res.cost_sum[p, keep]).any()
    fam.close()


def test_a_deterministic_family_looks_ahead_and_has_nothing_to_draw():
    case = flc.DETERMINISTIC
    fam = flc.family(case)
    J = cost_to_go(case.name)
    x = flc.states(case)
    got = fam.lookahead(J, x)
    assert fam.backend_info['lookahead_box'] == 'device' and fam.W == 0
    for p, s in enumerate(case.solvers()):
        for a, b, name in zip((got[0][p], got[1][p], got[2][p]), s.lookahead(J[p], x[p]), ('J', 'u', 'idx')):
            assert a.dtype == b.dtype and mlc.same(a, b), (p, name)
        assert s.backend_info['lookahead_box'] == 'device'
    for a, b, name in zip(got, flc.oracle_lookahead(case, J, x), ('J', 'u', 'idx')):
        assert mlc.same(a, b), name
    assert min(len(np.unique(i)) for i in got[2]) >= 3
    with pytest.raises(ValueError) as err:
        fam.monte_carlo_lookahead(J, x[:, :4], 3)
    assert 'member 0' in str(err.value) and 'nothing to draw' in str(err.value)
    fam.close()
