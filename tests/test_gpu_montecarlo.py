"""DPSolver.monte_carlo (kernel sdp_montecarlo: the closed loop with the perturbations drawn on the device, reduced per
trajectory) against what the merged code already computes: the draws from their numpy definition
(monte_carlo_draws), the trajectories from DPSolver.simulate (pinned on the reference's loop by
tests/test_gpu_simulate.py), the reductions sequentially in numpy in the problem's reals.  Everything is compared
with np.array_equal: no tolerance."""
import contextlib
import io

import numpy as np
import pytest

import fp32_cases
import policies as P
from conftest import golden
from stodynprog_amd import SysDescription, DPSolver, models, _native as nat

pytestmark = pytest.mark.gpu


def _quiet(f, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all='ignore'):
        return f(*a, **kw)


def _close(s):
    for k in [k for k in s._cache if k[0] == 'problem']:
        s._cache.pop(k).close()


def _nodes(x, state_grid, dt):
    """the occupancy's node of every state of x (B, d), restated point by point in scalars of the problem's reals
    (not stodynprog_amd.montecarlo.nearest_nodes, which the product's host path uses): position
    p = (x - first) / (last - first) * (n - 1), cell = trunc(p) clamped to [0, n - 2] (a position that does not fit
    32 bits, or NaN: cell 0), lam = p - cell, node = cell + (lam >= 0.5) clamped to n - 1"""
    out = np.zeros(x.shape, dtype=np.int64)
    for k, axis in enumerate(state_grid):
        n = len(axis)
        first, nm1 = dt(axis[0]), dt(n - 1)
        span = dt(axis[-1]) - first
        for b in range(x.shape[0]):
            p = (dt(x[b, k]) - first) / span * nm1
            assert type(p) is dt
            cell = min(max(int(p), 0), n - 2) if abs(p) < 2.0 ** 31 else 0
            lam = p - dt(cell)
            out[b, k] = min(cell + (1 if lam >= dt(0.5) else 0), n - 1)
    return out


def _reduce(s, x, g, n_burn, occupancy, dt=None):
    """the kernel's reductions from states x (T+1, B, d) and costs g (T, B), step by step"""
    dt = np.dtype(s.dtype if dt is None else dt).type
    T, B = g.shape
    lo = np.array([a[0] for a in s.state_grid]).astype(dt)
    hi = np.array([a[-1] for a in s.state_grid]).astype(dt)
    acc = np.zeros(B, dtype=s.dtype)
    n_out = np.zeros(B, dtype=np.int64)
    occ = np.zeros(s._state_grid_shape, dtype=np.int64) if occupancy else None
    with np.errstate(all='ignore'):
        for k in range(n_burn, T):
            acc = acc + g[k].astype(s.dtype)                      # one rounded add per step, k ascending
            n_out += ~((x[k] >= lo) & (x[k] <= hi)).all(axis=1)
            if occ is not None:
                np.add.at(occ, tuple(_nodes(x[k], s.state_grid, dt).T), 1)
    return acc, n_out, x[T], occ


def _replay(s, pol, x0, T, seed, n_burn=0, law=None, traj_offset=0, t0=0, occupancy=True):
    x0 = np.atleast_2d(np.asarray(x0, dtype=float))
    _, w = s.monte_carlo_draws(seed, x0.shape[0], T, law=law, traj_offset=traj_offset)
    x, u, g = _quiet(s.simulate, pol, x0, w, t0=t0)
    assert x.dtype == s.dtype and g.dtype == s.dtype
    return _reduce(s, x, g, n_burn, occupancy)


def _eq(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(((a == b) | ((a != a) & (b != b))).all())


def _same(res, ref, what, n_counted=None):
    acc, n_out, x_final, occ = ref
    assert _eq(res.cost_sum, acc), (what, 'cost_sum', int((res.cost_sum != acc).sum()))
    assert _eq(res.x_final, x_final), (what, 'x_final')
    assert res.n_outside.dtype == np.int64 and np.array_equal(res.n_outside, n_out), (what, 'n_outside')
    if occ is not None:
        assert res.occupancy.dtype == np.int64 and res.occupancy.shape == occ.shape
        assert np.array_equal(res.occupancy, occ), (what, 'occupancy', int((res.occupancy != occ).sum()))
        if n_counted is not None:
            assert int(res.occupancy.sum()) == n_counted
    assert np.array_equal(res.cost_mean, res.cost_sum.astype(np.float64) / (res.n_steps - res.n_burn))


def _starts(s, B, rng, margin=0.0):
    lo = np.array([g[0] for g in s.state_grid])
    hi = np.array([g[-1] for g in s.state_grid])
    return lo + (hi - lo) * rng.uniform(-margin, 1 + margin, (B, len(lo)))


def _inventory():
    s = models.inventory()[1]
    pol = _quiet(s.value_iteration, np.zeros(s._state_grid_shape), report_time=False)[1]
    return s, pol


def _ar1():
    s = models.storage_ar1()[1]
    pol = _quiet(s.value_iteration, np.zeros(s._state_grid_shape), report_time=False)[1]
    return s, pol


def _searev():
    s = models.searev()[1]
    return s, golden('g4_searev')['committed_policy']


def _fp32():
    case = [c for c in fp32_cases.CASES if c.name == 'ar1_33x20'][0]
    s = case.solver(case.runs[1])
    assert s.dtype == np.float32
    return s, P.policy(s, 'smooth', seed=3)


MODELS = {'inventory': _inventory, 'storage_ar1': _ar1, 'searev': _searev, 'fp32 ar1_33x20': _fp32}


@pytest.mark.timeout(600)
@pytest.mark.parametrize('name', sorted(MODELS))
def test_parity_with_simulate(gpu, name):
    s, pol = MODELS[name]()
    rng = np.random.default_rng(len(name))
    T = 40
    grid, proba = s.perturb_grid[0], s.perturb_proba[0]
    fine = (np.linspace(grid[0], grid[-1], 97), np.full(97, 1.0 / 97))       # above the branch-free count: the search
    try:
        for B, n_burn, law, seed, off in ((1, 0, None, 0, 0), (63, 0, None, 1, 0), (64, 5, None, 2, 1000),
                                          (200, 13, None, 0x123456789abcdef, (1 << 33) + 7),
                                          (130, 3, fine, 4, 0), (65, 39, (grid[::-1], proba), 5, 3)):
            x0 = _starts(s, B, rng)
            res = _quiet(s.monte_carlo, pol, x0, T, seed=seed, n_burn=n_burn, law=law, occupancy=True,
                         traj_offset=off)
            assert res.path == 'device' and s.backend_info['mode'] == 'traced'
            assert res.cost_sum.dtype == s.dtype and res.x_final.shape == x0.shape
            ref = _replay(s, pol, x0, T, seed, n_burn, law, off)
            _same(res, ref, '{} B={} n_burn={}'.format(name, B, n_burn), B * (T - n_burn))
            # without the occupancy: the same reductions
            bare = _quiet(s.monte_carlo, pol, x0, T, seed=seed, n_burn=n_burn, law=law, traj_offset=off)
            assert bare.occupancy is None
            _same(bare, ref[:3] + (None,), '{} B={} without occupancy'.format(name, B))
        # one start state for the whole batch
        one = _quiet(s.monte_carlo, pol, x0[0], T, seed=8, n_traj=70, occupancy=True)
        _same(one, _replay(s, pol, np.broadcast_to(x0[0], (70, x0.shape[1])), T, 8), name + ' one start', 70 * T)
        assert one.mean == one.cost_mean.mean() and one.stderr == one.cost_mean.std(ddof=1) / np.sqrt(70)
    finally:
        _close(s)


@pytest.mark.timeout(600)
def test_invariance_to_launches_and_batch_splits(gpu):
    s, pol = _ar1()
    rng = np.random.default_rng(21)
    B, T = 301, 29
    x0 = _starts(s, B, rng)
    try:
        kw = dict(seed=77, n_burn=4, occupancy=True, traj_offset=12)
        runs = {}
        for spl in (1, 7, T, 1024):
            s.steps_per_launch = spl
            runs[spl] = _quiet(s.monte_carlo, pol, x0, T, **kw)
        ref = _replay(s, pol, x0, T, 77, 4, None, 12)
        for spl, res in runs.items():
            _same(res, ref, 'steps_per_launch = {}'.format(spl), B * (T - 4))
        # two calls of half the batch against one call
        h = B // 2
        a = _quiet(s.monte_carlo, pol, x0[:h], T, **kw)
        b = _quiet(s.monte_carlo, pol, x0[h:], T, **dict(kw, traj_offset=12 + h))
        whole = runs[1024]
        assert _eq(np.concatenate([a.cost_sum, b.cost_sum]), whole.cost_sum)
        assert _eq(np.concatenate([a.x_final, b.x_final]), whole.x_final)
        assert np.array_equal(np.concatenate([a.n_outside, b.n_outside]), whole.n_outside)
        assert np.array_equal(a.occupancy + b.occupancy, whole.occupancy)
    finally:
        _close(s)


@pytest.mark.timeout(600)
def test_batch_past_the_grid_cap(gpu):
    """more trajectories than the launch holds lanes (sdp_problem_montecarlo caps the grid at cus * 8 workgroups of
    256): the grid-stride loop reaches every one, with the draws of its own id"""
    cus = int(nat.device_info(0)['compute_units'])
    cap = cus * 8 * 256
    B, T = cap + 333, 6
    s, pol = _inventory()
    rng = np.random.default_rng(5)
    x0 = _starts(s, B, rng)
    try:
        big = _quiet(s.monte_carlo, pol, x0, T, seed=31, n_burn=1, occupancy=True, traj_offset=50)
        assert int(big.occupancy.sum()) == B * (T - 1)
        for lo, hi in ((0, 700), (cap - 450, cap + 333), (cap // 2, cap // 2 + 65)):
            part = _quiet(s.monte_carlo, pol, x0[lo:hi], T, seed=31, n_burn=1, traj_offset=50 + lo)
            assert _eq(part.cost_sum, big.cost_sum[lo:hi]), (lo, hi)
            assert _eq(part.x_final, big.x_final[lo:hi]) and np.array_equal(part.n_outside, big.n_outside[lo:hi])
        _same(_quiet(s.monte_carlo, pol, x0[cap - 450:], T, seed=31, n_burn=1, occupancy=True,
                     traj_offset=50 + cap - 450),
              _replay(s, pol, x0[cap - 450:], T, 31, 1, None, 50 + cap - 450), 'tail of the batch')
    finally:
        _close(s)


@pytest.mark.timeout(300)
def test_states_outside_the_grid_are_counted(gpu):
    s, pol = _ar1()
    rng = np.random.default_rng(8)
    B, T = 257, 50
    grid, proba = s.perturb_grid[0], s.perturb_proba[0]
    try:
        # start states outside the grid
        x0 = _starts(s, B, rng, margin=0.3)
        res = _quiet(s.monte_carlo, pol, x0, T, seed=2, occupancy=True)
        ref = _replay(s, pol, x0, T, 2)
        _same(res, ref, 'starts outside', B * T)
        lo = np.array([g[0] for g in s.state_grid])
        hi = np.array([g[-1] for g in s.state_grid])
        started_out = ~((x0 >= lo) & (x0 <= hi)).all(axis=1)
        assert started_out.any() and (res.n_outside[started_out] >= 1).all()
        # inside at the start, pushed out by a law five times as wide
        x0 = _starts(s, B, rng)
        wide = (5.0 * grid, proba)
        res = _quiet(s.monte_carlo, pol, x0, T, seed=3, n_burn=2, law=wide, occupancy=True)
        _same(res, _replay(s, pol, x0, T, 3, 2, wide), 'leaves the grid', B * (T - 2))
        assert (res.n_outside > 0).any() and res.n_outside.max() <= T - 2
    finally:
        _close(s)


def _branchy():
    sysd = SysDescription((1, 1, 1), name='branchy')

    def dyn(x, u, w):
        return (np.array([xi + ui if xi > 0 else xi - ui for xi, ui in zip(np.atleast_1d(x), np.atleast_1d(u))]) + w,)
    sysd.dyn = dyn
    sysd.cost = lambda x, u, w: x * x + u * u + 0 * w
    sysd.control_box = lambda x: ((-1., 1.),)
    sysd.perturb_laws = [models.NormalLaw(0, 0.1)]
    s = DPSolver(sysd)
    s.discretize_state(-2, 2, 9)
    s.discretize_perturb(-0.2, 0.2, 3)
    return s


@pytest.mark.timeout(300)
def test_untraceable_model_takes_the_host_path(gpu):
    s = _branchy()
    pol = (0.1 * s.state_grid[0])[:, None]
    rng = np.random.default_rng(1)
    B, T, n_burn = 37, 150, 20                   # more steps than one block of the host loop
    x0 = _starts(s, B, rng, margin=0.2)
    res = _quiet(s.monte_carlo, pol, x0, T, seed=6, n_burn=n_burn, occupancy=True, traj_offset=9)
    assert res.path == 'host'
    _, w = s.monte_carlo_draws(6, B, T, traj_offset=9)
    x, u, g = _quiet(s._simulate_host, pol, x0, w, T, 0)
    _same(res, _reduce(s, x, g, n_burn, True, dt=np.float64), 'host path', B * (T - n_burn))


@pytest.mark.timeout(600)
def test_two_seeds_agree_within_their_standard_errors(gpu):
    """storage-AR1, 4096 trajectories of 2000 steps, 500 of them burn-in: the batch means of two seeds differ by at
    most 6 joint standard errors, sqrt(se1^2 + se2^2) -- the margin comes from the samples themselves"""
    s, pol = _ar1()
    x0 = np.array([0.5 * (g[0] + g[-1]) for g in s.state_grid])
    try:
        a = _quiet(s.monte_carlo, pol, x0, 2000, seed=1, n_burn=500, n_traj=4096)
        b = _quiet(s.monte_carlo, pol, x0, 2000, seed=2, n_burn=500, n_traj=4096)
    finally:
        _close(s)
    joint = np.sqrt(a.stderr ** 2 + b.stderr ** 2)
    print('seed 1: {!r}\nseed 2: {!r}\n|difference| = {:.6g} = {:.3f} joint standard errors ({:.6g})'.format(
        a, b, abs(a.mean - b.mean), abs(a.mean - b.mean) / joint, joint))
    assert np.isfinite(a.mean) and np.isfinite(b.mean) and joint > 0
    assert not np.array_equal(a.cost_sum, b.cost_sum)
    assert abs(a.mean - b.mean) <= 6.0 * joint


@pytest.mark.timeout(300)
def test_entry_point_refuses_bad_arguments(gpu):
    s, pol = _inventory()
    try:
        with pytest.raises(ValueError):
            s.steps_per_launch = 0
            s.monte_carlo(pol, np.zeros(1), 5, n_traj=3)
    finally:
        s.steps_per_launch = 1024
        _close(s)
