"""Closed loops of families under lookahead controls over a horizon, on the device
(tests/family_lookahead_horizon_cases.py): member p of every result of `SolverFamily.simulate_lookahead` /
`SolverFamily.monte_carlo_lookahead_horizon` equals, on bits, (1) what `solvers[p].simulate_lookahead` /
`.monte_carlo_lookahead` returns -- on its device path for models that are symbolic in time, on its host path for models
that look data up as `data[k]` -- and (2) the pinned oracle chained step by step; for every way the kernels map members
to XCDs, past the bound of their grid, however the run is cut into cost-to-go chunks, launches, batches and member
chunks, with the members' own laws or the caller's, and at a state without a valid lattice.

Not covered: 4-byte reals with `data[k]` models (the solo host path has no 4-byte twin to compare with)."""
import functools

import numpy as np
import pytest

import family_lookahead_cases as flc
import family_lookahead_horizon_cases as fhl
import lookahead_cases as lc
import mc_lookahead_cases as mlc
from stodynprog_amd import _native as nat

pytestmark = pytest.mark.gpu

FIELDS = ('cost_sum', 'cost_mean', 'n_outside', 'x_final', 'occupancy')
NAMES = ('x', 'u', 'g', 'q')
SEED, OFFSET, N_BURN = fhl.SEED, fhl.OFFSET, fhl.N_BURN
same = mlc.same


@functools.lru_cache(maxsize=None)
def cost_to_go(name, timed=True):
    case = {c.name: c for c in fhl.FAMILIES}[name]
    J = fhl.cost_to_go(case, timed)
    J.setflags(write=False)
    return J


def _path(case):
    return 'host' if case.int_time else 'device'


def _same_result(one, ref, what):
    for name in FIELDS:
        a, b = getattr(one, name), getattr(ref, name)
        if b is None:
            assert a is None, (what, name)
            continue
        assert same(a, b), (what, name, int((mlc.bits(a) != mlc.bits(b)).sum()))
    assert np.array_equal([one.mean, one.stderr], [ref.mean, ref.stderr], equal_nan=True), what


def _sim_against_solo(got, case, J, x0, w, what):
    for p, s in enumerate(case.solvers()):
        ref = s.simulate_lookahead(J[p], x0[p] if x0.ndim == 3 else x0, None if w is None else (w[p] if w.ndim == 3 else w),
                                   n_steps=case.n_steps, t0=case.t0)
        assert s.backend_info['lookahead_path'] == _path(case), (what, p)
        for a, b, name in zip(got, ref, NAMES):
            assert same(a[p], b), (what, p, name, int((mlc.bits(a[p]) != mlc.bits(b)).sum()))


def _sim_against_oracle(got, case, J, x0, w, what, rows=None):
    for p in range(len(case.members)):
        x0_p = x0[p] if x0.ndim == 3 else x0
        w_p = None if w is None else (w[p] if w.ndim == 3 else w)
        if rows is not None:
            x0_p, w_p = x0_p[rows], None if w_p is None else w_p[:, rows]
        want = fhl.oracle_closed_loop(case, p, J[p], x0_p, w_p)
        for a, b, name in zip(got, want, NAMES):
            a_p = a[p] if rows is None else a[p][:, rows]
            assert same(a_p, b), (what, p, name)


# ----------------------------------------------------------------------------------------------------------------------
# parity

@pytest.mark.parametrize('timed', (True, False), ids=('time-indexed', 'one per member'))
@pytest.mark.parametrize('case', fhl.PARITY, ids=repr)
def test_simulate_lookahead_equals_the_solo_calls_and_the_oracle(case, timed):
    fam = fhl.family(case)
    J = cost_to_go(case.name, timed)
    P, T, d, tile = len(fam), case.n_steps, len(fam.dims), fhl.tile(case)
    for B in (1, tile + 1, 2 * tile + 3):
        x0, w = fhl.starts(case, B), fhl.noise(case, B)
        got = fam.simulate_lookahead(J, x0, w, n_steps=T, t0=case.t0)
        assert [a.shape for a in got] == [(P, T + 1, B, d), (P, T, B, fam.nu), (P, T, B), (P, T, B)]
        assert all(a.dtype == fam.dtype for a in got)
        info = fam.backend_info
        assert (info['kernel'], info['lookahead_path'], info['lookahead_box']) == ('family', 'device', 'device'), info
        assert info['horizon']['timed'] == timed and info['horizon']['time_specialized'] == case.int_time
        _sim_against_solo(got, case, J, x0, w, (case, B))
        _sim_against_oracle(got, case, J, x0, w, (case, B))
        assert not np.isnan(got[3]).any()
    # the shared (B, d) and w forms, and the single-x0 form
    B = tile + 1
    x0, w = fhl.starts(case, B)[0], fhl.noise(case, B)
    w = None if w is None else w[0]
    got = fam.simulate_lookahead(J, x0, w, n_steps=T, t0=case.t0)
    _sim_against_solo(got, case, J, x0, w, (case, 'shared'))
    one = fam.simulate_lookahead(J, x0[0], None if w is None else w[:, 0], n_steps=T, t0=case.t0)
    assert [a.shape for a in one] == [(P, T + 1, d), (P, T, fam.nu), (P, T), (P, T)]
    for a, b, name in zip(one, got, NAMES):
        assert same(a, b[:, :, 0]), (case, 'single', name)
    fam.close()


@pytest.mark.parametrize('occupancy', (True, False), ids=('occupancy', 'plain'))
@pytest.mark.parametrize('case', fhl.STOCHASTIC, ids=repr)
def test_monte_carlo_equals_the_solo_calls_and_the_oracle(case, occupancy):
    fam = fhl.family(case)
    B = fhl.tile(case) + 1
    x0 = fhl.starts(case, B)
    kw = dict(n_burn=N_BURN, occupancy=occupancy, traj_offset=OFFSET, t0=case.t0)
    for timed in (True, False):
        J = cost_to_go(case.name, timed)
        res = fam.monte_carlo_lookahead_horizon(J, x0, case.n_steps, seed=SEED, **kw)
        assert res.path == 'device' and res.seeds == (SEED,) * len(fam) and fam.backend_info['lookahead_box'] == 'device'
        assert res.cost_sum.shape == (len(fam), B) and res.cost_sum.dtype == fam.dtype
        for p, s in enumerate(case.solvers()):
            ref = s.monte_carlo_lookahead(J[p], x0[p], case.n_steps, seed=SEED, **kw)
            assert s.backend_info['lookahead_path'] == _path(case)
            _same_result(res[p], ref, (case, timed, p))
            want = fhl.oracle_monte_carlo(case, p, J[p], x0[p], N_BURN, occupancy=occupancy)
            mlc.check(res[p], want, '{} member {}'.format(case, p), occupancy=occupancy)
        if not timed and not case.int_time:
            _same_result(fam.monte_carlo_lookahead(J, x0, case.n_steps, seed=SEED, **kw), res, (case, 'monte_carlo_lookahead'))
    fam.close()


# ----------------------------------------------------------------------------------------------------------------------
# mapping and cap: the oracle alone

@pytest.mark.parametrize('P', flc.MAPPING_P)
def test_every_mapping_of_members_to_xcds(P):
    case = fhl.MAPPING[P]
    fam = fhl.family(case)
    J = cost_to_go(case.name)
    x0, w = fhl.starts(case, fhl.B_MAPPING), fhl.noise(case, fhl.B_MAPPING)
    got = fam.simulate_lookahead(J, x0, w)
    _sim_against_oracle(got, case, J, x0, w, case)
    res = fam.monte_carlo_lookahead_horizon(J, x0, case.n_steps, seed=SEED, n_burn=1, occupancy=True, traj_offset=OFFSET)
    for p in range(P):
        mlc.check(res[p], fhl.oracle_monte_carlo(case, p, J[p], x0[p], 1), '{} member {}'.format(case, p))
    fam.close()


def test_a_batch_past_the_grid_bound():
    case = fhl.CAP
    fam = fhl.family(case)
    P, T = len(fam), case.n_steps
    cus = nat.device_info(0)['compute_units']
    B = flc.cap_batch(cus)
    assert P * -(-B // 4) > 8 * cus and B % 4 == 1
    J = cost_to_go(case.name)
    # every row carries one of a few distinct trajectories: a trajectory is a function of its own inputs
    pick = lc.repeated_rows(B, 7)
    x0_7, w_7 = fhl.starts(case, 7), fhl.noise(case, 7)
    got = fam.simulate_lookahead(J, x0_7[:, pick], w_7[:, :, pick])
    few = fam.simulate_lookahead(J, x0_7, w_7)
    _sim_against_oracle(few, case, J, x0_7, w_7, 'cap')
    for a, b, name in zip(got, few, NAMES):
        assert same(a, np.ascontiguousarray(b[:, :, pick])), name
    # the Monte Carlo loop: the whole batch equals its parts below the bound, the first and the last rows the oracle's
    x = x0_7[:, pick]
    run = lambda lo, hi: fam.monte_carlo_lookahead_horizon(J, x[:, lo:hi], T, seed=SEED, n_burn=1, occupancy=True,
                                                           traj_offset=OFFSET + lo)
    big = run(0, B)
    assert int(big.occupancy.sum()) == P * B * (T - 1)
    cuts = (0, B // 3, B // 3 + 131, B)
    parts = [run(lo, hi) for lo, hi in zip(cuts[:-1], cuts[1:])]
    for name in ('cost_sum', 'n_outside', 'x_final'):
        assert same(np.concatenate([getattr(q, name) for q in parts], axis=1), getattr(big, name)), name
    assert same(sum(q.occupancy for q in parts), big.occupancy)
    for rows in (slice(0, 6), slice(B - 9, B)):
        for p in range(P):
            want = fhl.oracle_monte_carlo(case, p, J[p], x[p][rows], 1, traj_offset=OFFSET + rows.start, occupancy=False)
            one = big[p]
            assert same(one.cost_sum[rows], want[0]) and same(one.n_outside[rows], want[1]) and same(one.x_final[rows], want[2]), p
    fam.close()


# ----------------------------------------------------------------------------------------------------------------------
# cuts, laws, seeds, no lattice, deterministic

def test_no_cut_changes_a_bit():
    case = fhl.CUTS
    fam = fhl.family(case)
    P, T, S, rs = len(fam), case.n_steps, int(np.prod(fam.dims)), fam.dtype.itemsize
    J = cost_to_go(case.name)
    B = 21
    x0, w = fhl.starts(case, B), fhl.noise(case, B)
    kw = dict(seed=SEED, n_burn=N_BURN, occupancy=True)
    sim = fam.simulate_lookahead(J, x0, w)
    assert fam.backend_info['horizon'] == dict(members=P, n_traj=B, n_steps=T, timed=True, time_specialized=False, chunks=1,
                                               step_chunks=1, launches=1)
    _sim_against_solo(sim, case, J, x0, w, 'cuts')
    whole = fam.monte_carlo_lookahead_horizon(J, x0, T, traj_offset=OFFSET, **kw)
    for p, s in enumerate(case.solvers()):
        _same_result(whole[p], s.monte_carlo_lookahead(J[p], x0[p], T, traj_offset=OFFSET, **kw), ('cuts', p))

    def check(what, chunks, spl):
        got = fam.simulate_lookahead(J, x0, w)
        info = fam.backend_info['horizon']
        assert (info['step_chunks'], info['launches']) == (len(chunks), fhl.launches(chunks)), (what, info)
        for a, b, name in zip(got, sim, NAMES):
            assert same(a, b), (what, name)
        res = fam.monte_carlo_lookahead_horizon(J, x0, T, traj_offset=OFFSET, **kw)
        info = fam.backend_info['horizon']
        assert (info['step_chunks'], info['launches']) == (len(chunks), fhl.launches(chunks, spl)), (what, info)
        for name in FIELDS:
            assert same(getattr(res, name), getattr(whole, name)), (what, name)
    # cost-to-go chunks of 1 step, 2 steps and all steps
    for steps in (1, 2, T):
        fam.horizon_chunk_bytes = steps * P * S * rs + 8
        chunks = fhl.step_chunks(P, S, rs, T, fam.horizon_chunk_bytes)
        assert len(chunks) == -(-T // steps)
        check(('chunk', steps), chunks, fam.steps_per_launch)
        for spl in (1, 2, 3, T):
            fam.steps_per_launch = spl
            check(('chunk', steps, 'spl', spl), chunks, spl)
            del fam.steps_per_launch
    del fam.horizon_chunk_bytes
    # a batch split over two calls by traj_offset
    lo = fam.monte_carlo_lookahead_horizon(J, x0[:, :8], T, traj_offset=OFFSET, **kw)
    hi = fam.monte_carlo_lookahead_horizon(J, x0[:, 8:], T, traj_offset=OFFSET + 8, **kw)
    for name in ('cost_sum', 'n_outside', 'x_final'):
        assert same(np.concatenate([getattr(lo, name), getattr(hi, name)], axis=1), getattr(whole, name)), name
    assert same(lo.occupancy + hi.occupancy, whole.occupancy)
    # member chunks 3 + 2, in both calls
    n_box = fam.backend_info['box_constants']
    fam.chunk_bytes = flc.chunk_bytes_for(fam, 3, fhl.mc_extra_bytes(fam, B, 3, True, T, 1, n_box))
    res = fam.monte_carlo_lookahead_horizon(J, x0, T, traj_offset=OFFSET, **kw)
    assert fam.backend_info['chunks'] == 2 and fam.backend_info['horizon']['step_chunks'] == 2
    for name in FIELDS:
        assert same(getattr(res, name), getattr(whole, name)), ('member chunks', name)
    fam.chunk_bytes = flc.chunk_bytes_for(fam, 3, fhl.sim_extra_bytes(fam, B, T, T, 1, n_box))
    got = fam.simulate_lookahead(J, x0, w)
    assert fam.backend_info['chunks'] == 2
    for a, b, name in zip(got, sim, NAMES):
        assert same(a, b), ('member chunks', name)
    fam.close()


def test_the_plant_draws_from_the_callers_law_and_the_backup_keeps_the_members_own():
    case = fhl.AR1_64
    fam = fhl.family(case)
    J = cost_to_go(case.name)
    B, T = 9, case.n_steps
    x0 = fhl.starts(case, B)
    kw = dict(n_burn=N_BURN, occupancy=True, traj_offset=OFFSET)
    laws = flc.member_laws()
    seeds = (SEED, SEED + 1, SEED + 2)
    res = fam.monte_carlo_lookahead_horizon(J, x0, T, seed=seeds, law=laws, **kw)
    assert res.seeds == seeds
    for p, s in enumerate(case.solvers()):
        # (the solo call sums its backup over the solver's own law whatever `law` is: equal bits say the family did too)
        _same_result(res[p], s.monte_carlo_lookahead(J[p], x0[p], T, seed=seeds[p], law=laws[p], **kw), ('laws', p))
        mlc.check(res[p], fhl.oracle_monte_carlo(case, p, J[p], x0[p], N_BURN, seed=seeds[p], law=laws[p]), 'laws member {}'.format(p))
    own = fam.monte_carlo_lookahead_horizon(J, x0, T, seed=seeds, **kw)
    assert not same(own.cost_sum, res.cost_sum)
    fam.close()


def test_a_state_without_a_lattice():
    case = fhl.NO_LATTICE
    fam = fhl.family(case)
    J = cost_to_go(case.name)
    B, row, T = 9, fhl.NAN_ROW, case.n_steps
    x0, w = fhl.starts(case, B), fhl.noise(case, B)
    x0[:, row] = lc.NAN_STATE
    keep = np.flatnonzero(np.arange(B) != row)
    got = fam.simulate_lookahead(J, x0, w)
    x, u, g, q = got
    assert same(x[:, 0, row], x0[:, row]) and np.isnan(x[:, 1:, row]).all()
    assert np.isnan(u[:, :, row]).all() and np.isnan(g[:, :, row]).all() and np.isnan(q[:, :, row]).all()
    assert not any(np.isnan(a[:, :, keep]).any() for a in got)
    _sim_against_oracle(got, case, J, x0, w, 'no lattice', rows=keep)
    res = fam.monte_carlo_lookahead_horizon(J, x0, T, seed=SEED, n_burn=N_BURN, occupancy=True, traj_offset=OFFSET)
    assert np.isnan(res.cost_sum[:, row]).all() and (res.n_outside[:, row] == T - N_BURN).all()
    for p in range(len(fam)):
        mlc.check(res[p], fhl.oracle_monte_carlo(case, p, J[p], x0[p], N_BURN, nan_rows=(row,)), 'no lattice member {}'.format(p))
    fam.close()


@pytest.mark.parametrize('case', (fhl.DETERMINISTIC, fhl.PV), ids=repr)
def test_deterministic_families_run_the_closed_loop_and_have_nothing_to_draw(case):
    fam = fhl.family(case)
    J = cost_to_go(case.name)
    B = 9
    x0 = fhl.starts(case, B)
    got = fam.simulate_lookahead(J, x0, n_steps=case.n_steps, t0=case.t0)
    assert fam.W == 0 and fam.backend_info['horizon']['time_specialized'] == case.int_time
    _sim_against_solo(got, case, J, x0, None, case)
    _sim_against_oracle(got, case, J, x0, None, case)
    assert min(len(np.unique(mlc.bits(u_p))) for u_p in got[1]) >= 3
    with pytest.raises(ValueError) as err:
        fam.monte_carlo_lookahead_horizon(J, x0, case.n_steps)
    assert 'member 0' in str(err.value) and 'nothing to draw' in str(err.value)
    fam.close()
