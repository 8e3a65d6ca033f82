"""The transition operator of a policy and the propagation of state distributions, as a definition in numpy.

What `montecarlo.py` is to the draws and `perturb.py` to the flat law, this module is to
`DPSolver.transition_operator`: the kernel `sdp_transitions` (csrc/sdp_trans_kernel.h) and the library's
`sdp_transop` (csrc/sdp_hip.hip: the stable sort by target, `k_push`) give the bits of the functions below, and
models that cannot be traced build their entries HERE and hand them to the library (`sdp_transop_from_coo`).

Under a fixed policy the backup of `eval_policy` is affine in the cost-to-go,

    (P J)(s) + gbar(s),     (P J)(s) = sum_j P[j] * interp(J)(dyn(x_s, pol[s], w_j)),

the Markov chain on the grid that the solver actually solves.  Its transpose moves a state distribution one step
forward, mu' = P^T mu.  Written out over the 2^d vertices of the multilinear interpolation, P has exactly
W * 2^d entries per node.

Entries.  Node ids are flat, in the reference's C order.  For every node s, u = pol[s] (a grid node: nothing is
interpolated); for every point j of the flat law (`perturb.product_law` for several variables; W = 1, P = [1] for a
deterministic system) x' = dyn(x_s, u, wtab[:, j]) and g_j = cost(..), the callables evaluated on arrays of the
problem's reals.  Per axis k the cell q_k, lam_k and oml_k = 1 - lam_k are those of `sdp_locate_axis`
(csrc/sdp_device.h; oracle/vi_numpy.py:mlinterp_np restates the same lines): p = (x' - smin) / (smax - smin) *
(n - 1), q = clamp(trunc(p), 0, n - 2), lam = p - q.  The cast truncates, the index is clamped, lam is NOT: a NaN
next state gives cell 0 and NaN weights, which propagate.  For every vertex v in {0,1}^d, axis 0 the most
significant bit (the order of itertools.product((0, 1), repeat=d)), one entry:

    target  t   = sum_k M_k (q_k + v_k)
    source  s
    value       = (((f_0 f_1) ..) f_{d-1}) P[j]        f_k = lam_k if v_k else oml_k; one rounded multiply per product

in the emission order (s, j, v) ascending: nnz = S W 2^d exactly; duplicate targets and zero values stay separate
entries.  Mean cost: gbar[s], acc = 0; acc = acc + g_j P[j], j ascending -- the sweep's own two roundings.

Outside the grid.  The reference's interpolation extrapolates, and so does this operator: where the model leaves the
grid, lam is below 0 or above 1 and weights are negative or above 1.  Every source's weights still sum to 1 (up to
rounding), and P^T is the exact adjoint of what `eval_policy` computes -- <mu, P J> = <P^T mu, J> -- which is the
point: nothing is clamped.  A distribution pushed through such an operator can have negative entries.

CSR of P^T: the entries stably sorted by target (within a row they keep the emission order); indptr int64 [S + 1],
indices = the sources, int32, data = the values.  One push: out[t], acc = 0; acc = acc + data[k] * mu[indices[k]]
for k ascending through the row -- one rounded multiply and one rounded add per entry, an empty row gives +0.  That is
np.add.at(out, tgt, val * mu[src]) on the emission-ordered arrays.

Stationary iteration: mu_0 given, or the uniform 1 / S computed in the problem's reals; mu_{k+1} = push(mu_k); after
push number check_every, 2 check_every, .. and after push number n_max, delta = max |mu_{k+1} - mu_k| =
max(dmax, -dmin) of `convergence.diff_stats` (order-independent; NaN never converges); the iteration stops at the
first checked delta <= tol, or at n_max.  No renormalisation and no damping: a periodic chain does not converge and
returns converged = False.

Over a horizon.  Under a time-indexed policy (what `bellman_recursion` returns) or a non-stationary model every step has
its own operator: step k = 0 .. T - 1 of a run that starts at time index t0 is `entries(solver, pol_k, t0 + k)`, pol_k
the policy slice pol[t0 + k] (a stationary policy: the same array at every step) -- `chain_entries`; nothing about one
step is defined again.  The chain mu_0 given, mu_{k+1} = push(P_k^T, mu_k) -- `propagate` -- is the forward pass of a
finite-horizon problem without sampling noise: the distribution of the state at every step, the expected cost
<mu_k, gbar_k> of every step, and their total.  With J_T = J_fin and J_k = gbar_k + P_k J_{k+1}, the backward pass of
`eval_policy` step by step,

    <mu_0, J_0> = sum_k <mu_k, gbar_k> + <mu_T, J_fin>

because <mu_k, P_k J_{k+1}> = <P_k^T mu_k, J_{k+1}> = <mu_{k+1}, J_{k+1}>: exact in exact arithmetic, since nothing is
clamped (P_k^T is the exact adjoint where the model leaves the grid, too).  `DPSolver.horizon_operator` builds the
operators of all steps in one device call (kernel `sdp_transitions_h`, csrc/sdp_trans_horizon_kernel.h; the library's
`sdp_chainop`) and gives the bits of `chain_entries`, `csr` and `propagate`.
"""
import collections
import itertools

import numpy as np

from . import convergence as conv
from . import perturb

_I32_MIN = -2 ** 31

Entries = collections.namedtuple('Entries', 'tgt src val mean_cost S W V')
Stationary = collections.namedtuple('Stationary', 'mu n_done converged delta average_cost mass')
Propagation = collections.namedtuple('Propagation', 'mu step_cost terminal_cost total_cost mass')


class FamilyStationary(object):
    """What `FamilyTransitionOperator.stationary` returns (stodynprog_amd/family.py): the fields of `Stationary`
    stacked on a leading member axis.

    mu (P,) + dims, n_done (P,) int, converged (P,) bool, delta (P,), average_cost (P,) float64 (NaN for an operator
    without mean costs), mass (P,) in the problem's reals.  len(res) == P and res[p] is the `Stationary` of member p:
    what `finish` makes of the member's last iterate, as the solo call does."""

    def __init__(self, mu, n_done, delta, tol, mean_cost=None):
        mu = np.asarray(mu)
        self._members = [finish(mu[p], n_done[p], delta[p], tol, None if mean_cost is None else mean_cost[p])
                         for p in range(mu.shape[0])]
        self.mu = mu
        self.n_done = np.array([m.n_done for m in self._members], dtype=np.int64)
        self.converged = np.array([m.converged for m in self._members], dtype=bool)
        self.delta = np.array([m.delta for m in self._members], dtype=np.float64)
        self.average_cost = np.array([np.nan if m.average_cost is None else m.average_cost for m in self._members],
                                     dtype=np.float64)
        self.mass = np.array([m.mass for m in self._members], dtype=mu.dtype)

    def __len__(self):
        return len(self._members)

    def __getitem__(self, p):
        return self._members[p]

    def __repr__(self):
        return 'FamilyStationary({} members, n_done={}, converged={})'.format(len(self), self.n_done.tolist(),
                                                                           self.converged.tolist())


def operator_bytes(nnz, S, itemsize):
    """bytes of an operator of nnz entries on S nodes: values, sources and the row pointers"""
    return int(nnz) * (int(itemsize) + 4) + 8 * (int(S) + 1)


def flat_law(perturb_grid, perturb_proba, dtype):
    """(wtab (m, W), P (W,)) in the problem's reals: one variable's grid and weights, the product law of several
    (`perturb.product_law`), or -- a deterministic system -- no variable and the single weight 1"""
    dt = np.dtype(dtype)
    if not len(perturb_grid):
        return np.zeros((0, 1), dtype=dt), np.ones(1, dtype=dt)
    if len(perturb_grid) == 1:
        return (np.ascontiguousarray(perturb_grid[0], dtype=dt).reshape(1, -1),
                np.ascontiguousarray(perturb_proba[0], dtype=dt).ravel())
    return perturb.product_law(perturb_grid, perturb_proba, dt)


def locate(axis, x_next):
    """(q, lam, oml) of `sdp_locate_axis` along one axis (`axis`: its points in the problem's reals)"""
    dt = axis.dtype.type
    n = len(axis)
    with np.errstate(all='ignore'):
        sn = (x_next - axis[0]) / (axis[-1] - axis[0])
        p = sn * dt(n - 1)
        ok = np.abs(p) < dt(2147483648.0)
        t = np.where(ok, p, dt(0)).astype(np.int64)                 # C truncation
        t = np.where(ok, t, _I32_MIN)                               # NaN and out-of-range values: INT_MIN, then the clamp
        q = np.maximum(np.minimum(t, n - 2), 0)
        lam = p - q.astype(dt)
        oml = dt(1) - lam
    return q, lam, oml


def model_on_grid(solver, pol, t_k=None, time_index='real'):
    """(x_next [d] arrays (S, W), g (S, W), wtab, P): the callables on every (node, law point) under the policy, on
    arrays of the problem's reals (a result of a wider type is rounded once)"""
    dt = np.dtype(solver.dtype)
    axes = [np.ascontiguousarray(g, dtype=dt) for g in solver.state_grid]
    shape = tuple(len(a) for a in axes)
    S = int(np.prod(shape))
    d, nu = len(shape), len(solver.sys.control)
    pol = np.asarray(pol)
    if pol.shape != shape + (nu,):
        raise ValueError('pol must have shape {}, not {}'.format(shape + (nu,), pol.shape))
    pol = pol.astype(dt, copy=False).reshape(S, nu)
    wtab, P = flat_law(solver.perturb_grid, solver.perturb_proba, dt)
    W = P.size
    ind = np.unravel_index(np.arange(S), shape)
    args = tuple(a[i].reshape(S, 1) for a, i in zip(axes, ind))
    args += tuple(pol[:, c].reshape(S, 1) for c in range(nu))
    args += tuple(wtab[i] for i in range(wtab.shape[0]))
    with np.errstate(all='ignore'):
        if solver.sys.stationnary:
            x_next = solver.sys.dyn(*args, **solver.sys.params)
            g = solver.sys.cost(*args, **solver.sys.params)
        else:
            # the time index as the model is traced: 'real', a scalar of the problem's reals (the kernel's `t`: a symbolic
            # index), or 'int', the concrete index (callables that look data up, `data[k]`, are traced for the step alone,
            # and the host paths hand over an int)
            t = int(0 if t_k is None else t_k) if time_index == 'int' else dt.type(0 if t_k is None else t_k)
            x_next = solver.sys.dyn(t, *args, **solver.sys.params)
            g = solver.sys.cost(t, *args, **solver.sys.params)
    if len(x_next) != d:
        raise ValueError('dyn returns {} next state variables, the grid has {}'.format(len(x_next), d))
    x_next = [np.broadcast_to(np.asarray(v, dtype=dt), (S, W)) for v in x_next]
    g = np.broadcast_to(np.asarray(g, dtype=dt), (S, W))
    return x_next, g, axes, wtab, P


def entries(solver, pol, t_k=None, time_index='real'):
    """The entries of the transition operator of `pol` in emission order and the mean cost (module text):
    Entries(tgt int32 [nnz], src int32 [nnz], val [nnz], mean_cost [S], S, W, V = 2^d).  time_index: how a
    non-stationary model gets t_k, 'real' (a scalar of the problem's reals, as a trace with a symbolic index evaluates it)
    or 'int' (as a trace for the one step does, and as the host paths call the callables)."""
    if time_index not in ('real', 'int'):
        raise ValueError("time_index must be 'real' or 'int'")
    x_next, g, axes, wtab, P = model_on_grid(solver, pol, t_k, time_index)
    dt = P.dtype
    shape = tuple(len(a) for a in axes)
    S, W, d = int(np.prod(shape)), P.size, len(shape)
    V = 1 << d
    M = [1] * d
    for k in range(d - 2, -1, -1):
        M[k] = M[k + 1] * shape[k + 1]
    cells = [locate(axes[k], x_next[k]) for k in range(d)]
    tgt = np.empty((S, W, V), dtype=np.int64)
    val = np.empty((S, W, V), dtype=dt)
    with np.errstate(all='ignore'):
        for v, bits in enumerate(itertools.product((0, 1), repeat=d)):
            node = np.zeros((S, W), dtype=np.int64)
            f = None
            for k in range(d):
                q, lam, oml = cells[k]
                node = node + M[k] * (q + bits[k])
                fk = lam if bits[k] else oml
                f = fk if f is None else f * fk
            tgt[:, :, v] = node
            val[:, :, v] = f * P[None, :]
        acc = np.zeros(S, dtype=dt)
        for j in range(W):
            acc = acc + g[:, j] * P[j]
    src = np.broadcast_to(np.arange(S, dtype=np.int32)[:, None, None], (S, W, V))
    return Entries(tgt.reshape(-1).astype(np.int32), np.ascontiguousarray(src).reshape(-1), val.reshape(-1),
                   acc, S, W, V)


def check_coo(S, tgt, src):
    """ValueError for entries whose target or source is not a node of [0, S)"""
    S = int(S)
    if S < 1:
        raise ValueError('an operator needs at least one node, not S = {}'.format(S))
    tgt, src = np.asarray(tgt), np.asarray(src)
    if tgt.shape != src.shape or tgt.ndim != 1:
        raise ValueError('tgt and src must be vectors of one length')
    for name, a in (('target', tgt), ('source', src)):
        if a.size and (a.min() < 0 or a.max() >= S):
            raise ValueError('{} index outside [0, {})'.format(name, S))


def csr(S, tgt, src, val):
    """(indptr int64 [S + 1], indices int32, data) of P^T: the entries stably sorted by target"""
    check_coo(S, tgt, src)
    tgt = np.asarray(tgt, dtype=np.int64)
    order = np.argsort(tgt, kind='stable')
    indptr = np.zeros(int(S) + 1, dtype=np.int64)
    np.cumsum(np.bincount(tgt, minlength=int(S)), out=indptr[1:])
    return indptr, np.asarray(src)[order].astype(np.int32), np.ascontiguousarray(np.asarray(val)[order])


def push(op, mu, n_steps=1):
    """n_steps pushes of `mu` (flat or of grid shape) through op = (indptr, indices, data): per row the sequential
    sum acc = 0; acc = acc + data[k] * mu[indices[k]], k ascending, in the type of `data`"""
    indptr, indices, data = op
    dt = data.dtype
    S = len(indptr) - 1
    mu = np.asarray(mu)
    shape = mu.shape
    cur = mu.astype(dt, copy=False).reshape(-1)
    if cur.size != S:
        raise ValueError('mu has {} entries, the operator {} nodes'.format(cur.size, S))
    rows = np.repeat(np.arange(S), np.diff(indptr))
    for _ in range(int(n_steps)):
        with np.errstate(all='ignore'):
            out = np.zeros(S, dtype=dt)
            np.add.at(out, rows, data * cur[indices])        # unbuffered: one add per entry, in the order given
        cur = out
    return cur.reshape(shape)


def push_row_by_row(op, mu):
    """one push as the text states it, a Python loop over rows and entries (what `push` is checked against)"""
    indptr, indices, data = op
    dt = data.dtype.type
    mu = np.asarray(mu, dtype=data.dtype).reshape(-1)
    out = np.zeros(len(indptr) - 1, dtype=data.dtype)
    with np.errstate(all='ignore'):
        for t in range(len(out)):
            acc = dt(0)
            for k in range(indptr[t], indptr[t + 1]):
                acc = acc + data[k] * mu[indices[k]]
            out[t] = acc
    return out


def max_abs_diff(a, b):
    """delta = max |a - b| = max(dmax, -dmin) of `convergence.diff_stats`; NaN if any difference is"""
    dmin, dmax = conv.diff_stats(a, b)
    return max(dmax, -dmin) if dmin == dmin else float('nan')


def uniform(S, dtype):
    dt = np.dtype(dtype).type
    return np.full(int(S), dt(1) / dt(S), dtype=dtype)


def stationary(op, mean_cost=None, mu0=None, tol=1e-12, n_max=10000, check_every=10):
    """The power iteration of the module text on op = (indptr, indices, data).  Returns Stationary(mu, n_done,
    converged, delta, average_cost, mass); average_cost = dot(mu, mean_cost) in float64 arithmetic of numpy (not
    bit-pinned; None without mean_cost), mass = mu.sum()."""
    tol, check_every = conv.validate(tol, check_every)
    n_max = int(n_max)
    if n_max < 1:
        raise ValueError('n_max must be at least 1')
    dt = op[2].dtype
    S = len(op[0]) - 1
    mu = uniform(S, dt) if mu0 is None else np.asarray(mu0).astype(dt, copy=False).reshape(-1)
    delta, done = float('nan'), 0
    for k in range(1, n_max + 1):
        new = push(op, mu)
        done = k
        checked = conv.is_check(k, n_max, check_every)
        if checked:
            delta = max_abs_diff(new, mu)
        mu = new
        if checked and delta <= tol:
            break
    return finish(mu, done, delta, tol, mean_cost)


def finish(mu, n_done, delta, tol, mean_cost):
    """the record `stationary` returns, from the last iterate"""
    with np.errstate(all='ignore'):
        avg = None if mean_cost is None else float(np.dot(mu.ravel(), np.asarray(mean_cost).ravel()))
        mass = mu.sum()
    return Stationary(mu, int(n_done), bool(delta <= tol), float(delta), avg, mass)


def chain_entries(solver, pol, n_steps, t0=0, time_index='real'):
    """The `Entries` of the steps k = 0 .. n_steps - 1 of a horizon that starts at time index t0 (module text): step k is
    `entries(solver, pol_k, t0 + k, time_index)` with pol_k = pol[t0 + k] for a time-indexed policy, shape
    (T_pol,) + dims + (nu,), and pol itself for a stationary one."""
    pol = np.asarray(pol)
    timed = pol.ndim == len(solver.state_grid) + 2
    n_steps = int(n_steps)
    if timed and (int(t0) != t0 or t0 < 0 or t0 + n_steps > pol.shape[0]):
        raise ValueError('t0 = {} and n_steps = {} need the policy steps {} .. {}: the policy has shape {}'.format(
            t0, n_steps, t0, t0 + n_steps - 1, pol.shape))
    return [entries(solver, pol[int(t0) + k] if timed else pol, t0 + k, time_index) for k in range(n_steps)]


def propagate(ops, mean_costs, mu0, J_fin=None):
    """mu0 pushed through the chain of operators ops[k] = (indptr, indices, data), k = 0 .. T - 1 (module text):
    mu[0] = mu0 in the reals of the operators, mu[k + 1] = push(ops[k], mu[k], 1).  mu0 has the grid's shape `dims`, or
    (B,) + dims for a batch; mean_costs[k] is gbar of step k (grid shape or flat), J_fin a terminal cost on the grid.

    Returns Propagation(mu, step_cost, terminal_cost, total_cost, mass): mu (T + 1,) + dims or (T + 1, B) + dims, the time
    axis first; step_cost[k] = dot(mu[k], mean_costs[k]), shape (T[, B]); terminal_cost = dot(mu[T], J_fin), or 0;
    total_cost their sum; mass[k] = mu[k].sum(), shape (T + 1[, B]).  The dot products are float64 arithmetic of numpy
    (not bit-pinned, as `finish` treats average_cost); mu is."""
    T = len(ops)
    if T < 1 or len(mean_costs) != T:
        raise ValueError('{} operators and {} mean costs: a chain has at least one step and one mean cost per step'.format(
            T, len(mean_costs)))
    dt = ops[0][2].dtype
    S = len(ops[0][0]) - 1
    mu0 = np.asarray(mu0)
    if mu0.size == 0 or mu0.size % S or (mu0.size != S and (mu0.ndim < 2 or mu0[0].size != S)):
        raise ValueError('mu0 of shape {} is neither one vector of the operators\' {} nodes nor a batch of them'.format(
            mu0.shape, S))
    batch = mu0.size != S
    mu = np.empty((T + 1,) + mu0.shape, dtype=dt)
    mu[0] = mu0
    for k in range(T):
        if batch:
            for b in range(mu0.shape[0]):
                mu[k + 1, b] = push(ops[k], mu[k, b], 1)
        else:
            mu[k + 1] = push(ops[k], mu[k], 1)
    return finish_chain(mu, mean_costs, J_fin, batch)


def finish_chain(mu, mean_costs, J_fin, batch):
    """the record `propagate` returns, from the distributions of all steps"""
    T = mu.shape[0] - 1
    lead = mu.shape[:2] if batch else mu.shape[:1]
    flat = mu.reshape(lead + (-1,)).astype(np.float64)
    with np.errstate(all='ignore'):
        step_cost = np.stack([flat[k] @ np.asarray(mean_costs[k], dtype=np.float64).ravel() for k in range(T)])
        terminal = (flat[T] @ np.asarray(J_fin, dtype=np.float64).ravel() if J_fin is not None
                    else np.zeros(lead[1:], dtype=np.float64))
        total = step_cost.sum(axis=0) + terminal
        mass = mu.reshape(lead + (-1,)).sum(axis=-1)
    return Propagation(mu, step_cost, terminal, total, mass)
