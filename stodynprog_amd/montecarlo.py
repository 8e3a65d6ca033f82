"""The perturbation draws of `DPSolver.monte_carlo`, as a definition in numpy.

The kernel `sdp_montecarlo` (csrc/sdp_mc_kernel.h) implements exactly this and the tests pin it:
what `convergence.py` is to the stopping rule, this module is to the draws.

One draw per (trajectory, step), a function of `(seed, id, step)` and nothing else:

    key     = (seed & 0xffffffff, seed >> 32)
    counter = (id & 0xffffffff, id >> 32, step & 0xffffffff, step >> 32)
    r0, r1, _, _ = Philox4x32-10(counter, key)          (Salmon et al., Random123)
    u = ((r0 >> 5) * 2**26 + (r1 >> 6)) * 2**-53          a double in [0, 1)
    j = #{ i in [0, W-2] : u >= c_i }                     c = sequential float64 running sum of proba
      = np.searchsorted(c[:-1], u, 'right')
    w = grid[j]

`id = traj_offset + row` is the 64-bit trajectory id and `step` the 64-bit absolute step index, so
the batch size, the launch grid, the number of launches and how a batch is split over calls cannot
change a draw.  The last index is the clamp (u >= c_{W-2} gives W-1 whatever c_{W-1} is); a point of
zero probability that is not the last one has c_i == c_{i-1} and is never drawn.
"""
import numpy as np

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57          # round multipliers
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85          # key increments
MAX_LAW_POINTS = 4096                                  # the cumulative table and the values live in LDS
_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """Philox4x32-10.  counter: 4 arrays (or ints) of 32-bit words, key: 2; returns the 4 output
    words as uint32 arrays of the broadcast shape."""
    c = [np.asarray(x, dtype=np.uint64) & _M32 for x in counter]
    k = [np.asarray(x, dtype=np.uint64) & _M32 for x in key]
    c = list(np.broadcast_arrays(*(c + k)))
    c, k = c[:4], c[4:]
    m0, m1 = np.uint64(PHILOX_M0), np.uint64(PHILOX_M1)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]                   # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & _M32,
             (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & _M32]
        k = [(k[0] + np.uint64(PHILOX_W0)) & _M32, (k[1] + np.uint64(PHILOX_W1)) & _M32]
    return tuple(x.astype(np.uint32) for x in c)


def _u64(a, what):
    a = np.asarray(a)
    if a.dtype != object and a.dtype.kind not in 'iu':
        raise ValueError('{} must be integers'.format(what))
    if a.dtype == object:                              # Python ints beyond int64
        flat = [int(v) for v in a.ravel()]
        if any(v < 0 or v >= 1 << 64 for v in flat):
            raise ValueError('{} must lie in [0, 2**64)'.format(what))
        return np.array(flat, dtype=np.uint64).reshape(a.shape)
    if a.dtype.kind == 'i' and a.size and a.min() < 0:
        raise ValueError('{} must not be negative'.format(what))
    return a.astype(np.uint64)


def check_seed(seed):
    seed = int(seed)
    if not 0 <= seed < 1 << 64:
        raise ValueError('seed must lie in [0, 2**64)')
    return seed


def uniforms(seed, ids, steps):
    """u[k, b] of step steps[k] and trajectory ids[b]: float64 in [0, 1), shape (T, B)."""
    seed = check_seed(seed)
    ids = np.atleast_1d(_u64(ids, 'ids'))[None, :]
    steps = np.atleast_1d(_u64(steps, 'steps'))[:, None]
    sh = np.uint64(32)
    r0, r1, _, _ = philox4x32_10((ids & _M32, ids >> sh, steps & _M32, steps >> sh),
                                 (seed & 0xFFFFFFFF, seed >> 32))
    hi = (r0 >> np.uint32(5)).astype(np.float64)
    lo = (r1 >> np.uint32(6)).astype(np.float64)
    return (hi * 67108864.0 + lo) * (1.0 / 9007199254740992.0)


def check_proba(proba):
    """the law's probabilities as a float64 vector: non-negative, finite, sum within 1e-9 of 1"""
    p = np.array(proba, dtype=np.float64)
    if p.ndim != 1 or p.size < 1:
        raise ValueError('proba must be a non-empty vector')
    if p.size > MAX_LAW_POINTS:
        raise ValueError('a law of {} points: at most {}'.format(p.size, MAX_LAW_POINTS))
    if not np.all(np.isfinite(p)):
        raise ValueError('proba must be finite')
    if np.any(p < 0):
        raise ValueError('proba must not be negative')
    if abs(float(cumulative(p)[-1]) - 1.0) > 1e-9:
        raise ValueError('proba must sum to 1 (within 1e-9), not {!r}'.format(float(cumulative(p)[-1])))
    return p


def cumulative(proba):
    """c_i = c_{i-1} + p_i, sequentially in float64 (np.cumsum of a 1-D float64 array is that loop)"""
    return np.cumsum(np.asarray(proba, dtype=np.float64))


def index_of(u, proba):
    """the drawn index for uniforms u: searchsorted(c[:-1], u, 'right'), the last index the clamp"""
    c = cumulative(proba)
    return np.searchsorted(c[:-1], u, side='right').astype(np.int32)


def draws(seed, ids, steps, proba):
    """(T, B) int32 indices into the law for trajectory ids `ids` (B,) and absolute steps `steps` (T,)."""
    p = check_proba(proba)
    return index_of(uniforms(seed, ids, steps), p)


def check_law(grid, proba):
    p = check_proba(proba)
    g = np.array(grid, dtype=np.float64)
    if g.shape != p.shape:
        raise ValueError('law: grid of shape {} but proba of shape {}'.format(g.shape, p.shape))
    return g, p


class MonteCarloResult(object):
    """What `DPSolver.monte_carlo` returns: per-trajectory reductions and the batch statistics.

    cost_sum (B,)   sum of g_k over the steps k >= n_burn, accumulated in the problem's reals
    cost_mean (B,)  cost_sum / (n_steps - n_burn), float64
    n_outside (B,)  steps k >= n_burn whose x_k lay outside the state grid (or was NaN)
    x_final (B, d)  state after the last step
    occupancy       visits per grid node (state dims, int64) or None
    mean, stderr    of cost_mean over the batch (float64, ddof=1; stderr is NaN for B = 1)
    """

    def __init__(self, cost_sum, n_outside, x_final, occupancy, n_steps, n_burn, seed, traj_offset, t0, path):
        self.cost_sum, self.n_outside, self.x_final, self.occupancy = cost_sum, n_outside, x_final, occupancy
        self.n_steps, self.n_burn, self.seed, self.traj_offset, self.t0 = n_steps, n_burn, seed, traj_offset, t0
        self.n_traj = cost_sum.shape[0]
        self.path = path                                # 'device' or 'host'
        self.cost_mean = cost_sum.astype(np.float64) / float(n_steps - n_burn)
        self.mean = float(self.cost_mean.mean())
        self.stderr = (float(self.cost_mean.std(ddof=1) / np.sqrt(self.n_traj)) if self.n_traj > 1
                       else float('nan'))

    def __repr__(self):
        return ('MonteCarloResult(mean={:.6g} +- {:.3g}, n_traj={}, n_steps={}, n_burn={}, seed={}, '
                'outside={})').format(self.mean, self.stderr, self.n_traj, self.n_steps, self.n_burn,
                                      self.seed, int(self.n_outside.sum()))


class FamilyMonteCarloResult(object):
    """What `SolverFamily.monte_carlo` returns: the fields of `MonteCarloResult` stacked on a leading member axis.

    cost_sum (P, B), cost_mean (P, B), n_outside (P, B), x_final (P, B, d), occupancy (P,) + state dims or None,
    mean (P,), stderr (P,); `seeds` holds the seed of every member.  len(res) == P and res[p] is the
    `MonteCarloResult` of member p: its mean and stderr are those of the solo call, bit for bit.
    Members that ran with one seed and the same trajectory ids saw the same uniform draws (common random numbers):
    `paired(p, q)` is the mean and the standard error of their per-trajectory difference.
    """

    def __init__(self, cost_sum, n_outside, x_final, occupancy, n_steps, n_burn, seeds, traj_offset, t0, path):
        self.cost_sum, self.n_outside, self.x_final, self.occupancy = cost_sum, n_outside, x_final, occupancy
        self.n_steps, self.n_burn, self.traj_offset, self.t0 = n_steps, n_burn, traj_offset, t0
        self.seeds = tuple(int(s) for s in seeds)
        self.n_members, self.n_traj = cost_sum.shape
        if len(self.seeds) != self.n_members:
            raise ValueError('{} seeds for {} members'.format(len(self.seeds), self.n_members))
        self.path = path
        self._members = [MonteCarloResult(cost_sum[p], n_outside[p], x_final[p],
                                          None if occupancy is None else occupancy[p], n_steps, n_burn, self.seeds[p],
                                          traj_offset, t0, path) for p in range(self.n_members)]
        self.cost_mean = cost_sum.astype(np.float64) / float(n_steps - n_burn)
        self.mean = np.array([m.mean for m in self._members], dtype=np.float64)
        self.stderr = np.array([m.stderr for m in self._members], dtype=np.float64)

    def __len__(self):
        return self.n_members

    def __getitem__(self, p):
        return self._members[p]

    def paired(self, p, q):
        """(mean, stderr) of cost_mean[p] - cost_mean[q] over the batch, float64, ddof=1 (stderr NaN for B = 1).
        Only members that ran with the same seed are paired."""
        if self.seeds[p] != self.seeds[q]:
            raise ValueError('members {} and {} ran with different seeds ({} and {}): their trajectories are not '
                             'paired'.format(p, q, self.seeds[p], self.seeds[q]))
        diff = self.cost_mean[p] - self.cost_mean[q]
        stderr = float(diff.std(ddof=1) / np.sqrt(self.n_traj)) if self.n_traj > 1 else float('nan')
        return float(diff.mean()), stderr

    def __repr__(self):
        return 'FamilyMonteCarloResult({} members, n_traj={}, n_steps={}, n_burn={}, mean={})'.format(
            self.n_members, self.n_traj, self.n_steps, self.n_burn, np.array2string(self.mean, precision=6))


def nearest_nodes(x, state_grid, dtype):
    """Per axis, the grid node the occupancy counts for states x (..., d): the cell and weight of the
    policy lookup (multilinear_cython.pyx:75-81, in the problem's reals), node = cell + (lam >= 0.5),
    clamped to [0, n-1].  Returns int64 indices (..., d)."""
    dt = np.dtype(dtype).type
    x = np.asarray(x, dtype=dt)
    out = np.empty(x.shape, dtype=np.int64)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        for k, axis in enumerate(state_grid):
            n = len(axis)
            smin, smax = dt(axis[0]), dt(axis[-1])
            p = ((x[..., k] - smin) / dt(smax - smin)) * dt(n - 1)
            ok = np.abs(p) < 2147483648.0                   # x86 truncation: NaN / out of range -> INT_MIN, clamped to 0
            q = np.where(ok, np.trunc(np.where(ok, p, 0)), -2147483648.0).astype(np.int64)
            q = np.maximum(np.minimum(q, n - 2), 0)
            lam = p - q.astype(dt)
            out[..., k] = np.clip(q + (lam >= dt(0.5)), 0, n - 1)
    return out
