"""DPSolver.monte_carlo_lookahead on the device (kernel sdp_montecarlo_lookahead, csrc/sdp_lookahead_kernel.h) against
the yardstick of tests/mc_lookahead_cases.py -- the pinned oracle chained step by step on `monte_carlo_draws`, reduced
in numpy -- bit for bit: every stochastic case of tests/lookahead_cases.py on both paths, sampling laws around the
two branches of the index search, every way of cutting a run, a batch past the grid cap, the NaN box, and the replay
through simulate_lookahead.  A closed loop of the oracle is computed once per case and shared; nothing loops over a
failing step or tries it again."""
import functools

import numpy as np
import pytest

import lookahead_cases as lc
import mc_lookahead_cases as mlc
from stodynprog_amd import _native as nat

pytestmark = pytest.mark.gpu

SEED, OFFSET = mlc.SEED, mlc.OFFSET


@functools.lru_cache(maxsize=None)
def reference(name):
    """(x0, x, g) of a case for its largest batch: the oracle's closed loop on the draws of (SEED, OFFSET + row)"""
    case = lc.BY_NAME[name]
    s = case.solver()
    t0, T = mlc.horizon(case)
    B = max(case.batches + (mlc.past_a_workgroup(case),))
    x0 = lc.start_states(case, s, B)
    x, g = mlc.closed_loop(case, s, lc.cost_to_go(s), x0, T, t0=t0)
    for a in (x0, x, g):
        a.setflags(write=False)
    return x0, x, g


@pytest.mark.parametrize('case', mlc.STOCHASTIC, ids=repr)
def test_parity_with_the_oracle_on_both_paths(case):
    s = case.solver()
    t0, T = mlc.horizon(case)
    J_next = lc.cost_to_go(s)
    x0, x, g = reference(case.name)
    for B in case.batches + (mlc.past_a_workgroup(case),):
        rows = np.arange(B)
        for n_burn in mlc.N_BURNS:
            want = mlc.reduce(s, x, g, n_burn, rows)
            for occupancy in (True, False):
                for path in (None, 'host'):
                    res = s.monte_carlo_lookahead(J_next, x0[:B], T, seed=SEED, n_burn=n_burn, occupancy=occupancy,
                                                  traj_offset=OFFSET, t0=t0, path=path)
                    ran = 'host' if path == 'host' else case.path
                    assert res.path == ran and s.backend_info['lookahead_path'] == ran, (case, path, s.backend_info)
                    assert res.cost_sum.dtype == s.dtype and res.x_final.dtype == s.dtype
                    mlc.check(res, want, (case, B, n_burn, path), occupancy)


def _law_case(n, seed):
    rng = np.random.default_rng(seed)
    p = rng.random(n) + 0.05
    return np.linspace(-0.3, 0.3, n), p / p.sum()


@pytest.mark.parametrize('n', [63, 64, 65, 97])
def test_sampling_laws_around_the_branches_of_the_index_search(n):
    case = lc.BY_NAME['lanes 8']
    s = case.solver()
    T, B = lc.T_SIM, 33
    J_next = lc.cost_to_go(s)
    law = _law_case(n, n)
    x0 = lc.start_states(case, s, B)
    x, g = mlc.closed_loop(case, s, J_next, x0, T, law=law)
    res = s.monte_carlo_lookahead(J_next, x0, T, seed=SEED, n_burn=1, law=law, occupancy=True, traj_offset=OFFSET)
    assert res.path == 'device'
    mlc.check(res, mlc.reduce(s, x, g, 1), ('law of', n))


def test_the_law_of_the_plant_is_not_the_law_of_the_backup():
    case = lc.BY_NAME['lanes 8']
    s = case.solver()
    T, B = lc.T_SIM, 33
    J_next = lc.cost_to_go(s)
    x0 = lc.start_states(case, s, B)
    grid, proba = np.asarray(s.perturb_grid[0]), np.asarray(s.perturb_proba[0])
    for what, law in (('reversed', (grid[::-1].copy(), proba[::-1].copy())), ('five times as wide', (5. * grid, proba))):
        x, g = mlc.closed_loop(case, s, J_next, x0, T, law=law)
        want = mlc.reduce(s, x, g, 0)
        res = s.monte_carlo_lookahead(J_next, x0, T, seed=SEED, law=law, occupancy=True, traj_offset=OFFSET)
        mlc.check(res, want, what)
        if what != 'reversed':
            assert want[1].sum() > 0 and res.n_outside.sum() > 0       # the plant leaves the grid


@pytest.mark.parametrize('name', ['symbolic time', 'searev f32'])
def test_cuts_change_no_bit(name):
    case = lc.BY_NAME[name]
    s = case.solver()
    T, t0, B = lc.T_SIM, 1, 37
    J_all = np.stack([lc.cost_to_go(s, k) for k in range(T + 2)])
    x0 = lc.start_states(case, s, B)
    # t0 > 0: the cost-to-go of step k is J_all[t0 + k], the Philox step stays k
    x, g = mlc.closed_loop(case, s, J_all, x0, T, t0=t0)
    want = mlc.reduce(s, x, g, 2)
    run = lambda rows=slice(None), off=OFFSET: s.monte_carlo_lookahead(
        J_all, x0[rows], T, seed=SEED, n_burn=2, occupancy=True, traj_offset=off, t0=t0)
    whole = run()
    assert whole.path == 'device'
    mlc.check(whole, want, (name, 'whole'))
    step_bytes = lc.n_nodes(s) * s.dtype.itemsize
    for chunk in (1, 3):
        for spl in (1, 3, T, 1024):
            s.horizon_chunk_bytes, s.steps_per_launch = chunk * step_bytes, spl
            mlc.check(run(), want, (name, chunk, spl))
    # two calls of half a batch, the trajectory ids carried by traj_offset: the rows of one call, and the occupancies add
    h = B // 2
    first, second = run(slice(0, h)), run(slice(h, B), OFFSET + h)
    assert mlc.same(np.concatenate([first.cost_sum, second.cost_sum]), whole.cost_sum)
    assert mlc.same(np.concatenate([first.n_outside, second.n_outside]), whole.n_outside)
    assert mlc.same(np.concatenate([first.x_final, second.x_final]), whole.x_final)
    assert mlc.same(first.occupancy + second.occupancy, whole.occupancy)
    with pytest.raises(ValueError):
        s.monte_carlo_lookahead(J_all, x0, T, t0=3)


def test_a_batch_past_the_grid_cap():
    case = lc.BY_NAME['lanes 64']
    s = case.solver()
    T = 3
    cus = nat.device_info(0)['compute_units']
    B = cus * 8 * 4 + 33                                                # 4 trajectories a workgroup, cus * 8 workgroups
    J_next = lc.cost_to_go(s)
    x0 = lc.start_states(case, s, B)
    run = lambda lo, hi: s.monte_carlo_lookahead(J_next, x0[lo:hi], T, seed=SEED, n_burn=1, occupancy=True,
                                                 traj_offset=OFFSET + lo)
    big = run(0, B)
    assert big.path == 'device' and int(big.occupancy.sum()) == B * (T - 1)
    cuts = (0, B // 3, B // 3 + 1031, B)
    parts = [run(lo, hi) for lo, hi in zip(cuts[:-1], cuts[1:])]
    assert mlc.same(np.concatenate([p.cost_sum for p in parts]), big.cost_sum)
    assert mlc.same(np.concatenate([p.n_outside for p in parts]), big.n_outside)
    assert mlc.same(np.concatenate([p.x_final for p in parts]), big.x_final)
    assert mlc.same(sum(p.occupancy for p in parts), big.occupancy)
    # the tail -- the trajectories of the second trip through the tiles -- against the oracle
    tail = B - 40
    x, g = mlc.closed_loop(case, s, J_next, x0[tail:], T, traj_offset=OFFSET + tail)
    acc, n_out, x_final, _ = mlc.reduce(s, x, g, 1, occupancy=False)
    assert mlc.same(big.cost_sum[tail:], acc) and mlc.same(big.n_outside[tail:], n_out)
    assert mlc.same(big.x_final[tail:], x_final)


@pytest.mark.parametrize('case', mlc.NAN_CASES, ids=repr)
def test_a_start_without_a_lattice_goes_nan_and_stays(case):
    s = case.solver()
    T, B, row = lc.T_SIM, 9, 3
    J_next = lc.cost_to_go(s)
    x0 = lc.start_states(case, s, B)
    x0[row] = lc.NAN_STATE
    x, g = mlc.closed_loop(case, s, J_next, x0, T, nan_rows=(row,))
    for n_burn in mlc.N_BURNS:
        want = mlc.reduce(s, x, g, n_burn)
        for path in (None, 'host'):
            res = s.monte_carlo_lookahead(J_next, x0, T, seed=SEED, n_burn=n_burn, occupancy=True, traj_offset=OFFSET,
                                          path=path)
            assert res.path == ('host' if path else 'device')
            mlc.check(res, want, (case, n_burn, path))                  # (the other rows are untouched)
            assert np.isnan(res.cost_sum[row]) and np.isnan(res.x_final[row]).all()
            assert res.n_outside[row] == T - max(n_burn, 1)            # x_0 is inside the grid, every later state is NaN
            assert not np.isnan(np.delete(res.cost_sum, row)).any()


def _replay(s, J_next, x0, T, seed, n_burn, law=None):
    """simulate_lookahead on the draws, reduced on the host"""
    _, w = s.monte_carlo_draws(seed, len(x0), T, law=law)
    x, _, g, _ = s.simulate_lookahead(J_next, x0, w, n_steps=T)
    assert s.backend_info['lookahead_path'] == 'device'
    return mlc.reduce(s, x, g, n_burn)


def test_it_is_simulate_lookahead_on_the_draws_searev():
    case = lc.BY_NAME['searev']
    s = case.solver()
    T, B = 8, 70
    J_next = lc.cost_to_go(s)
    x0 = lc.start_states(case, s, B)
    res = s.monte_carlo_lookahead(J_next, x0, T, seed=SEED, n_burn=2, occupancy=True)
    assert res.path == 'device'
    mlc.check(res, _replay(s, J_next, x0, T, SEED, 2), 'searev')


def test_it_is_simulate_lookahead_on_the_draws_two_variables_and_a_joint_law():
    case = lc.BY_NAME['two_inflows']
    s = case.solver()
    T, B = 8, 6
    J_next = lc.cost_to_go(s)
    x0 = lc.start_states(case, s, B)
    res = s.monte_carlo_lookahead(J_next, x0, T, seed=SEED, n_burn=2, occupancy=True)
    mlc.check(res, _replay(s, J_next, x0, T, SEED, 2), 'the flat product law')
    # a joint law that is no product: the two inflows move together
    a, b = (np.asarray(g, dtype=float) for g in s.perturb_grid)
    values = np.array([[a[0], a[-1], a[len(a) // 2], a[0]], [b[0], b[-1], b[0], b[-1]]])
    law = (values, np.array([0.4, 0.4, 0.1, 0.1]))
    res = s.monte_carlo_lookahead(J_next, x0, T, seed=SEED, n_burn=2, law=law, occupancy=True)
    assert res.path == 'device'
    mlc.check(res, _replay(s, J_next, x0, T, SEED, 2, law), 'a joint law')
