"""The draws of DPSolver.monte_carlo as defined in numpy (stodynprog_amd/montecarlo.py): Philox4x32-10 known
answers, the uniform and the index rule, dependence on (seed, id, step) alone, frequencies, and the argument
errors that need no GPU.  The kernel is pinned against this definition by tests/test_gpu_montecarlo.py."""
import numpy as np
import pytest

from stodynprog_amd import SysDescription, DPSolver, models
from stodynprog_amd import montecarlo as mc

# counter words 0..3, key words 0..1 -> output words 0..3 (Random123 known-answer vectors)
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]
LAW9 = np.array([0.02, 0.08, 0.15, 0.2, 0.1, 0.2, 0.15, 0.06, 0.04])


def _philox_scalar(counter, key):
    """Philox4x32-10 once more, in Python integers"""
    c, k = list(counter), list(key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xffffffff, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xffffffff]
        k = [(k[0] + 0x9E3779B9) & 0xffffffff, (k[1] + 0xBB67AE85) & 0xffffffff]
    return tuple(c)


@pytest.mark.parametrize('counter, key, out', KAT)
def test_philox_known_answers(counter, key, out):
    assert tuple(int(x) for x in mc.philox4x32_10(counter, key)) == out
    assert _philox_scalar(counter, key) == out


def test_philox_is_vectorised_word_by_word():
    rng = np.random.default_rng(0)
    words = rng.integers(0, 1 << 32, (6, 50), dtype=np.uint64)
    got = mc.philox4x32_10(words[:4], words[4:])
    for i in range(50):
        ref = _philox_scalar([int(w) for w in words[:4, i]], [int(w) for w in words[4:, i]])
        assert tuple(int(g[i]) for g in got) == ref


def test_uniform_is_53_bits_of_words_0_and_1():
    seed, ids, steps = 0x1234567890abcdef, np.arange(5, 12), np.arange(100, 140)
    u = mc.uniforms(seed, ids, steps)
    assert u.shape == (40, 7) and u.dtype == np.float64
    assert (u >= 0).all() and (u < 1).all()
    for k in (0, 17, 39):
        for b in (0, 6):
            r = _philox_scalar((int(ids[b]), 0, int(steps[k]), 0), (seed & 0xffffffff, seed >> 32))
            assert u[k, b] == ((r[0] >> 5) * 2.0 ** 26 + (r[1] >> 6)) * 2.0 ** -53
    # the extreme words: 0 and the largest double below 1
    assert ((0 >> 5) * 2.0 ** 26 + (0 >> 6)) * 2.0 ** -53 == 0.0
    assert ((0xffffffff >> 5) * 2.0 ** 26 + (0xffffffff >> 6)) * 2.0 ** -53 == 1.0 - 2.0 ** -53


def test_index_is_searchsorted_on_the_running_sum():
    seed, ids, steps = 11, np.arange(300), np.arange(200)
    u = mc.uniforms(seed, ids, steps)
    for proba in (LAW9, np.array([0.5, 0.5]), np.array([0.25, 0., 0.25, 0.5]), np.full(100, 0.01)):
        c = np.zeros(len(proba))
        acc = 0.0
        for i, p in enumerate(proba):           # sequential float64 running sum
            acc = acc + p
            c[i] = acc
        assert np.array_equal(c, mc.cumulative(proba))
        idx = mc.draws(seed, ids, steps, proba)
        assert idx.dtype == np.int32 and idx.shape == (200, 300)
        assert np.array_equal(idx, np.searchsorted(c[:-1], u, 'right'))
        count = (u[..., None] >= c[:-1]).sum(-1)               # j = #{ i in [0, W-2] : u >= c_i }
        assert np.array_equal(idx, count)
        assert idx.min() >= 0 and idx.max() <= len(proba) - 1


def test_single_point_law_and_the_clamp():
    assert not mc.draws(3, np.arange(50), np.arange(40), [1.0]).any()
    # the last index is the clamp: a running sum that ends below 1 (within 1e-9) still draws W - 1 at most
    p = np.array([0.5, 0.5 - 4e-10])
    idx = mc.draws(3, np.arange(100), np.arange(100), p)
    assert set(np.unique(idx)) == {0, 1}


def test_interior_zero_probability_point_is_never_drawn():
    p = np.array([0.3, 0.0, 0.2, 0.0, 0.0, 0.5])
    idx = mc.draws(5, np.arange(1000), np.arange(1000), p)          # 10^6 draws
    assert idx.size == 10 ** 6
    assert set(np.unique(idx)) == {0, 2, 5}


def test_a_draw_depends_on_seed_id_and_step_only():
    seed = 0xdeadbeefcafe
    ids, steps = np.arange(40, 140), np.arange(7, 67)
    full = mc.draws(seed, ids, steps, LAW9)
    # any sub-block of ids and steps
    assert np.array_equal(mc.draws(seed, ids[13:57], steps[20:41], LAW9), full[20:41, 13:57])
    assert np.array_equal(mc.draws(seed, ids[::3], steps[::-7], LAW9), full[::-7, ::3])
    assert np.array_equal(mc.draws(seed, [ids[99]], [steps[0]], LAW9), full[:1, 99:])
    # another seed: another table
    assert not np.array_equal(mc.draws(seed + 1, ids, steps, LAW9), full)
    assert not np.array_equal(mc.draws(seed + (1 << 32), ids, steps, LAW9), full)
    # a batch split with traj_offset (no GPU: the draws of the public method)
    _, s = models.storage_ar1()
    whole, w = s.monte_carlo_draws(seed, 100, 30)
    a, wa = s.monte_carlo_draws(seed, 37, 30, traj_offset=0)
    b, wb = s.monte_carlo_draws(seed, 63, 30, traj_offset=37)
    assert np.array_equal(np.hstack([a, b]), whole) and np.array_equal(np.hstack([wa, wb]), w)
    assert np.array_equal(w, s.perturb_grid[0][whole]) and w.dtype == np.float64
    assert np.array_equal(whole, mc.draws(seed, np.arange(100), np.arange(30), s.perturb_proba[0]))
    late = mc.draws(seed, np.arange(100), np.arange(20, 30), s.perturb_proba[0])
    assert np.array_equal(late, whole[20:])


def test_ids_and_steps_above_2_to_32_use_the_high_words():
    seed = 9
    ids = np.array([5, 5 + (1 << 32), 5 + (7 << 32), (1 << 64) - 1], dtype=np.uint64)
    steps = np.array([3, 3 + (1 << 32), (1 << 63) + 3], dtype=np.uint64)
    u = mc.uniforms(seed, ids, steps)
    assert len(np.unique(u)) == u.size                       # the high words matter
    for k, st in enumerate(steps):
        for b, i in enumerate(ids):
            r = _philox_scalar((int(i) & 0xffffffff, int(i) >> 32, int(st) & 0xffffffff, int(st) >> 32), (seed, 0))
            assert u[k, b] == ((r[0] >> 5) * 2.0 ** 26 + (r[1] >> 6)) * 2.0 ** -53
    _, s = models.storage_ar1()
    hi, _ = s.monte_carlo_draws(seed, 3, 4, traj_offset=(1 << 40) + 1)
    assert np.array_equal(hi, mc.draws(seed, (1 << 40) + 1 + np.arange(3, dtype=np.uint64), np.arange(4),
                                       s.perturb_proba[0]))


@pytest.mark.parametrize('seed', [0, 1, 20261017, 0xfeedfacefeedface])
def test_frequencies_of_a_nine_point_law(seed):
    """10^6 draws: Pearson's chi-square with 8 degrees of freedom below 50.7, its 1e-7 upper quantile (a correct
    generator fails one seed in 10^7; the seeds are fixed, the test is deterministic)"""
    idx = mc.draws(seed, np.arange(1000), np.arange(1000), LAW9)
    observed = np.bincount(idx.ravel(), minlength=9)
    expected = LAW9 * idx.size
    chi2 = float(((observed - expected) ** 2 / expected).sum())
    print('seed {}: chi2 = {:.3f}'.format(seed, chi2))
    assert chi2 < 50.7, (seed, chi2, observed)


def test_proba_is_validated():
    ids, steps = np.arange(3), np.arange(3)
    for bad in ([0.5, 0.6], [0.5, 0.4], [-0.1, 1.1], [np.nan, 1.0], [np.inf, 0.0], [], [[0.5, 0.5]],
                np.full(mc.MAX_LAW_POINTS + 1, 1.0 / (mc.MAX_LAW_POINTS + 1))):
        with pytest.raises(ValueError):
            mc.draws(0, ids, steps, bad)
    mc.draws(0, ids, steps, np.full(mc.MAX_LAW_POINTS, 1.0 / mc.MAX_LAW_POINTS))
    mc.draws(0, ids, steps, [0.5, 0.5 + 5e-10])
    for bad_seed in (-1, 1 << 64):
        with pytest.raises(ValueError):
            mc.draws(bad_seed, ids, steps, [1.0])
    with pytest.raises(ValueError):
        mc.draws(0, [-1], steps, [1.0])
    with pytest.raises(ValueError):
        mc.draws(0, [0.5], steps, [1.0])


def _deterministic():
    s = SysDescription((1, 1, 0), name='deterministic')
    s.dyn = lambda x, u: (x + u,)
    s.cost = lambda x, u: x * x
    s.control_box = lambda x: ((-1., 1.),)
    solver = DPSolver(s)
    solver.discretize_state(-1, 1, 5)
    solver.control_steps = (0.5,)
    return solver


def test_argument_errors_need_no_gpu():
    d = _deterministic()
    with pytest.raises(ValueError, match='simulate'):
        d.monte_carlo(np.zeros((5, 1)), [0.], 10, n_traj=4)
    with pytest.raises(ValueError, match='simulate'):
        d.monte_carlo_draws(0, 4, 10)
    _, s = models.storage_ar1()
    pol = np.zeros(s._state_grid_shape + (2,))
    x0 = np.zeros(2)
    with pytest.raises(ValueError):
        s.monte_carlo(pol[..., :1], x0, 10, n_traj=4)                # policy shape
    with pytest.raises(ValueError):
        s.monte_carlo(pol, x0, 10)                                    # one start state, no n_traj
    with pytest.raises(ValueError):
        s.monte_carlo(pol, np.zeros(3), 10, n_traj=4)                 # state dimension
    with pytest.raises(ValueError):
        s.monte_carlo(pol, np.zeros((4, 3)), 10)
    with pytest.raises(ValueError):
        s.monte_carlo(pol, np.zeros((4, 2)), 10, n_traj=5)            # n_traj against the batch
    with pytest.raises(ValueError):
        s.monte_carlo(pol, x0, 0, n_traj=4)
    with pytest.raises(ValueError):
        s.monte_carlo(pol, x0, 10, n_burn=10, n_traj=4)               # nothing left to average
    with pytest.raises(ValueError):
        s.monte_carlo(pol, x0, 10, n_burn=-1, n_traj=4)
    with pytest.raises(ValueError):
        s.monte_carlo(pol, x0, 10, n_traj=0)
    with pytest.raises(ValueError):
        s.monte_carlo(pol, x0, 10, n_traj=4, seed=-1)
    with pytest.raises(ValueError):
        s.monte_carlo(pol, x0, 10, n_traj=4, traj_offset=-1)
    with pytest.raises(ValueError):
        s.monte_carlo(pol, x0, 10, n_traj=4, law=([0., 1.], [0.5, 0.6]))
    with pytest.raises(ValueError):
        s.monte_carlo(pol, x0, 10, n_traj=4, law=([0., 1., 2.], [0.5, 0.5]))
    with pytest.raises(ValueError):
        s.monte_carlo(pol, x0, 10, n_traj=4, law=(np.zeros(5000), np.full(5000, 1 / 5000.)))

    class TwoRanks(object):
        is_device, nranks, rank = True, 2, 0
    s.comm = TwoRanks()
    with pytest.raises(NotImplementedError):
        s.monte_carlo(pol, x0, 10, n_traj=4)


def test_result_statistics():
    cost_sum = np.array([10., 14., 12., 20.], dtype=np.float32)
    r = mc.MonteCarloResult(cost_sum, np.zeros(4, dtype=np.int64), np.zeros((4, 2), dtype=np.float32), None,
                            n_steps=12, n_burn=2, seed=3, traj_offset=0, t0=0, path='device')
    assert r.cost_mean.dtype == np.float64 and np.array_equal(r.cost_mean, cost_sum.astype(float) / 10.0)
    assert r.mean == r.cost_mean.mean() and r.stderr == r.cost_mean.std(ddof=1) / 2.0
    assert (r.n_traj, r.n_steps, r.n_burn, r.seed) == (4, 12, 2, 3)
    one = mc.MonteCarloResult(cost_sum[:1], np.zeros(1, dtype=np.int64), np.zeros((1, 2)), None, 12, 2, 3, 0, 0, 'host')
    assert np.isnan(one.stderr)


def test_nearest_node_rule():
    """hand-computed points: node = cell + (lam >= 0.5), the cell clamped to [0, n-2] and lam not clamped"""
    grid = (np.linspace(0., 4., 9), np.array([0., 0.7]))
    x = np.array([[0.0, 0.0], [0.24, 0.34], [0.25, 0.36], [4.0, 0.7], [9.0, 5.0], [-3.0, -1.0], [np.nan, 0.1]])
    n = mc.nearest_nodes(x, grid, np.float64)
    assert n.tolist() == [[0, 0], [0, 0], [1, 1], [8, 1], [8, 1], [0, 0], [0, 0]]
    # axis of 9 nodes half a unit apart: positions are exact in both reals, so lam is exactly 0.5 at the odd quarters
    axis = (np.linspace(0., 4., 9),)
    pts = np.array([0.25, 0.75, 1.25, 3.75, 0.2499, 0.7501, 3.5, 3.74, 3.76, 4.25, 4.24, -0.25, -0.26, 1e30, -1e30,
                    np.inf, -np.inf])[:, None]
    want = [1, 2, 3, 8, 0, 2, 7, 7, 8, 8, 8, 0, 0, 0, 0, 0, 0]
    #  4.25: cell 7 (clamped), lam 1.5 -> 8;  -0.25: cell 0, lam -0.5 -> 0;  a position of 2^31 and more (or NaN)
    #  truncates like x86 to INT_MIN, clamped to cell 0, with lam = the position itself: 1e30 and +inf -> node 1
    want[13] = want[15] = 1
    for dt in (np.float64, np.float32):
        assert mc.nearest_nodes(pts, axis, dt)[:, 0].tolist() == want, dt
    # 4-byte reals round the position before the comparison: 0.7 / 2.8 * 4 is 1.0000000000000002 in 8 bytes and exactly
    # 1 in 4; just below a half-way point the two reals disagree
    axis = (np.linspace(0., 1., 11),)
    below = np.array([[np.nextafter(np.float32(0.05), np.float32(0))]], dtype=np.float64)     # 0.05f rounds up to p = 0.5
    assert mc.nearest_nodes(np.array([[0.05]]), axis, np.float64).tolist() == [[1]]
    p32 = (np.float32(below[0, 0]) - np.float32(0)) / np.float32(1) * np.float32(10)
    assert mc.nearest_nodes(below, axis, np.float32).tolist() == [[1 if p32 >= np.float32(0.5) else 0]]
