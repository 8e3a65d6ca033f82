"""One-step lookahead at arbitrary states, as a definition in numpy.

What `forward.py` is to the transition operator, this module is to `DPSolver.lookahead` and
`DPSolver.simulate_lookahead`: the kernels `sdp_lookahead` and `sdp_simulate_lookahead`
(csrc/sdp_lookahead_kernel.h) give the bits of the functions below, and the host path of the solver is checked
against them.  The operation is the reference's `_value_at_state_vect(x_k, J_next_interp)` (stodynprog.py:639-691)
-- the body of the sweep -- at a state that need not be a grid node:

    (J_opt, u_opt, idx) = min / argmin over u of  E_w[ g(x, u, w) + J_next(f(x, u, w)) ]

For one state `x` of a batch, in the problem's reals `dt` (a 4-byte problem rounds the state to float32 ONCE and
every step below starts from that value):

Box.  `control_box(x)` in float64 -- the time index first for a time-dependent system; a 4-byte state is widened
first, so the box is that of the state the kernel holds.

Lattice.  `DPSolver._box_lattice`'s rule, operator for operator, in float64: n_interv = (hi - lo) / step; if
n_interv < 0.1 one point at (lo + hi) / 2; otherwise n = ceil(n_interv) + 1.  Then ONE rounding of lo and hi to
`dt`.  The points are those of `sdp_load_box` / `sdp_control_value` (csrc/sdp_sweep_kernel.h), which is
numpy.linspace's arithmetic: delta = hi - lo, step = delta / (n - 1), u_i = i * step + lo, the last point hi itself
(a zero step: u_i = (i / (n - 1)) * delta + lo).

Backup.  Per lattice point, in C order (control 0 slowest): acc = 0; acc = acc + (g + J_next(f)) * P[j], j
ascending over the law -- the flat law of `perturb.py` for several perturbation variables; a deterministic system
is g + J_next(f) itself.  The callables run on arrays of `dt`; J_next is the multilinear interpolation of
`sdp_interp_point` with every operator in `dt` (`forward.locate` and the lerp tree, last axis innermost).  It
EXTRAPOLATES outside the grid, as it does everywhere else: nothing is clamped.  The argmin takes the first
occurrence and the first NaN wins (numpy.argmin).

No valid lattice.  A state whose box has a non-finite end, or whose lattice total reaches 2^31, has none:
J_opt = NaN, u_opt = NaN, idx = -1 (the reference raises from int(ceil(nan)) there).

The closed loop is that step followed by the model's own step: x_{k+1} = dyn(x_k, u_opt, w_k) and
g_k = cost(x_k, u_opt, w_k), formed exactly as `simulate` forms them, and q_k = J_opt, the minimised expected
value.  With a time-indexed cost-to-go of shape (T_J,) + state_dims, step k of a call that starts at t0 looks
ahead into J_next[t0 + k].

`monte_carlo_lookahead` is that closed loop on the draws of `montecarlo.draws`, reduced per trajectory: the definition
of `DPSolver.monte_carlo_lookahead` and of kernel `sdp_montecarlo_lookahead`.
"""
import numpy as np

from . import forward

MAX_LATTICE = 2 ** 31


def lattice(control_box, params, control_steps, x, t_k, dtype):
    """(lo, hi, n) of the control lattices of the states `x` (B, d) -- arrays (nu, B), lo and hi rounded once to
    `dtype`, n int32 -- by scalar calls of `control_box` in float64.  A state without a valid lattice has n = 0 in
    every control (and NaN ends)."""
    dt = np.dtype(dtype)
    x = np.asarray(x, dtype=float)
    B = x.shape[0]
    nu = len(control_steps)
    lo = np.empty((nu, B))
    hi = np.empty((nu, B))
    lead = () if t_k is None else (t_k,)
    for b in range(B):
        box = control_box(*(lead + tuple(x[b])), **params)
        for c, (a, z) in enumerate(box):
            lo[c, b], hi[c, b] = a, z
    return lattice_of_ends(lo, hi, control_steps, dt)


def lattice_of_ends(lo, hi, control_steps, dtype):
    """the lattice rule on arrays of box ends (nu, B) in float64: (lo, hi, n) as `lattice` returns them"""
    dt = np.dtype(dtype)
    lo = np.array(lo, dtype=float)
    hi = np.array(hi, dtype=float)
    n = np.zeros(lo.shape, dtype=np.int64)
    with np.errstate(all='ignore'):
        finite = np.all(np.isfinite(lo) & np.isfinite(hi), axis=0)
        for c in range(lo.shape[0]):
            n_interv = (hi[c] - lo[c]) / control_steps[c]
            single = n_interv < 0.1
            npts = np.where(single, 1., np.ceil(np.where(single, 0., n_interv)) + 1)
            finite &= np.isfinite(npts) & (npts < MAX_LATTICE)
            n[c] = np.where(finite, npts, 0).astype(np.int64)
            mid = (lo[c] + hi[c]) / 2
            lo[c] = np.where(single, mid, lo[c])
            hi[c] = np.where(single, mid, hi[c])
        valid = finite & (np.prod(n, axis=0, dtype=float) < MAX_LATTICE)
    n[:, ~valid] = 0
    lo[:, ~valid] = np.nan
    hi[:, ~valid] = np.nan
    return lo.astype(dt), hi.astype(dt), n.astype(np.int32)


def control_points(lo, hi, n):
    """the points of one control of one state (`sdp_load_box` / `sdp_control_value`); lo, hi: scalars of the reals"""
    dt = type(lo)
    n = int(n)
    if n == 1:
        return np.array([lo], dtype=dt)
    with np.errstate(all='ignore'):
        delta = hi - lo
        step = delta / dt(n - 1)
        k = np.arange(n).astype(dt)
        u = (k / dt(n - 1)) * delta + lo if step == dt(0) else k * step + lo
    u[n - 1] = hi
    return u


def interpolate(axes, values, x_next):
    """J_next at the points `x_next` (d arrays of one shape): `sdp_interp_point` with every operator in the reals of
    `values` (flat, C order); `axes`: the grid's axes in those reals"""
    d = len(axes)
    dt = values.dtype.type
    loc = [forward.locate(axes[k], np.asarray(x_next[k], dtype=dt)) for k in range(d)]
    M = [1] * d
    for k in range(d - 2, -1, -1):
        M[k] = M[k + 1] * len(axes[k + 1])

    def rec(k, base):
        q, lam, oml = loc[k]
        if k == d - 1:
            lo, hi = values[base + M[k] * q], values[base + M[k] * (q + 1)]
        else:
            lo, hi = rec(k + 1, base + M[k] * q), rec(k + 1, base + M[k] * (q + 1))
        return oml * lo + lam * hi

    with np.errstate(all='ignore'):
        return rec(0, np.zeros(np.shape(loc[0][0]), dtype=np.int64))


def _time_arg(t_k, dt, time_index):
    if time_index == 'int':
        return int(t_k)
    return t_k if dt == np.float64 else dt.type(t_k)


def lookahead(solver, J_next, x, t_k=None, time_index='real'):
    """(J_opt (B,), u_opt (B, nu), idx (B,) int32) at the states `x` (B, d) for the discretisation and callables
    of `solver`, with `J_next` on the state grid.  time_index: how a time-dependent model gets t_k, as in
    `forward.entries` ('int': models that look data up as data[k])."""
    sd = solver.sys
    dt = np.dtype(solver.dtype)
    axes = [np.ascontiguousarray(g, dtype=dt) for g in solver.state_grid]
    shape = tuple(len(a) for a in axes)
    values = np.ascontiguousarray(J_next, dtype=dt).reshape(-1)
    if values.size != int(np.prod(shape)):
        raise ValueError('J_next must have shape {}, not {}'.format(shape, np.shape(J_next)))
    x = np.atleast_2d(np.asarray(x, dtype=float)).astype(dt)            # the one rounding of the state
    B, nu = x.shape[0], len(sd.control)
    t_box = None if t_k is None else (int(t_k) if time_index == 'int' else t_k)
    lo, hi, n = lattice(sd.control_box, sd.params, solver.control_steps, x.astype(float), t_box, dt)
    wtab, P = forward.flat_law(solver.perturb_grid, solver.perturb_proba, dt)
    stochastic = len(solver.perturb_grid) > 0
    J = np.full(B, np.nan, dtype=dt)
    u = np.full((B, nu), np.nan, dtype=dt)
    idx = np.full(B, -1, dtype=np.int32)
    lead = () if t_k is None else (_time_arg(t_k, dt, time_index),)
    for b in range(B):
        if n[0, b] == 0:
            continue
        dims = tuple(int(v) for v in n[:, b])
        grids = [control_points(lo[c, b], hi[c, b], n[c, b]) for c in range(nu)]
        mesh = [g.reshape((1,) * c + (-1,) + (1,) * (nu - c)) for c, g in enumerate(grids)]
        args = lead + tuple(x[b]) + tuple(mesh) + tuple(wtab[i] for i in range(wtab.shape[0]))
        with np.errstate(all='ignore'):
            x_next = sd.dyn(*args, **sd.params)
            g = sd.cost(*args, **sd.params)
            full = dims + (P.size,)
            x_next = [np.broadcast_to(np.asarray(v, dtype=dt), full) for v in x_next]
            cell = np.broadcast_to(np.asarray(g, dtype=dt), full) + interpolate(axes, values, x_next)
            if stochastic:
                acc = np.zeros(dims, dtype=dt)
                for j in range(P.size):
                    acc = acc + cell[..., j] * P[j]
            else:
                acc = np.array(cell[..., 0], dtype=dt)
        flat = int(acc.argmin())
        ind = np.unravel_index(flat, dims)
        J[b] = acc[ind]
        u[b] = [grids[c][ind[c]] for c in range(nu)]
        idx[b] = flat
    return J, u, idx


def model_step(solver, x, u, w, t_k=None, time_index='real'):
    """(x_next (B, d), g (B,)): the model's own step at the states x (B, d), controls u (B, nu) and perturbations
    w (m, B) -- the callables on arrays of the problem's reals, one element per trajectory, as `simulate` forms them"""
    sd = solver.sys
    dt = np.dtype(solver.dtype)
    x = np.asarray(x, dtype=dt)
    u = np.asarray(u, dtype=dt)
    args = tuple(x[:, i] for i in range(x.shape[1])) + tuple(u[:, c] for c in range(u.shape[1]))
    if w is not None:
        args += tuple(np.asarray(wi, dtype=dt) for wi in w)
    if t_k is not None:
        args = (_time_arg(t_k, dt, time_index),) + args
    with np.errstate(all='ignore'):
        xn = sd.dyn(*args, **sd.params)
        g = sd.cost(*args, **sd.params)
    B = x.shape[0]
    xn = np.stack([np.broadcast_to(np.asarray(v, dtype=dt), (B,)) for v in xn], axis=1)
    return xn, np.array(np.broadcast_to(np.asarray(g, dtype=dt), (B,)))


def check_horizon(J_next, shape, n_steps, t0):
    """(J_next as an array, whether it has a leading time axis); a ValueError for a shape that is neither, or for
    steps t0 .. t0 + n_steps - 1 that the time-indexed cost-to-go does not have"""
    J_next = np.asarray(J_next)
    if J_next.shape == tuple(shape):
        return J_next, False
    if J_next.ndim == len(shape) + 1 and J_next.shape[1:] == tuple(shape):
        if int(t0) != t0:
            raise ValueError('t0 = {} must be an integer to index a time-indexed cost-to-go'.format(t0))
        if t0 < 0 or t0 + n_steps > J_next.shape[0]:
            raise ValueError('t0 = {} and n_steps = {} need the cost-to-go steps {} .. {}: J_next has T_J = {}'.format(
                t0, n_steps, t0, t0 + n_steps - 1, J_next.shape[0]))
        return J_next, True
    raise ValueError('J_next must have shape {} (one cost-to-go) or (T_J,) + {} (a time-indexed one), not {}'.format(
        tuple(shape), tuple(shape), J_next.shape))


def simulate_lookahead(solver, J_next, x0, w, n_steps, t0=0, time_index='real', step=None):
    """The closed loop under lookahead controls: x (T + 1, B, d), u (T, B, nu), g (T, B), q (T, B) in the problem's
    reals.  x0: (B, d); w: (T, m, B) or None.  `step`: the lookahead of one step, (J_k, x, t) -> (J_opt, u_opt, idx)
    (default: `lookahead` above)."""
    dt = np.dtype(solver.dtype)
    shape = tuple(len(g) for g in solver.state_grid)
    T = int(n_steps)
    J_next, timed = check_horizon(J_next, shape, T, t0)
    x0 = np.atleast_2d(np.asarray(x0, dtype=float))
    B, d = x0.shape
    nu = len(solver.sys.control)
    x = np.zeros((T + 1, B, d), dtype=dt)
    u = np.zeros((T, B, nu), dtype=dt)
    g = np.zeros((T, B), dtype=dt)
    q = np.zeros((T, B), dtype=dt)
    x[0] = x0.astype(dt)
    if step is None:
        step = lambda J_k, x_k, t_k: lookahead(solver, J_k, x_k, t_k, time_index)
    for k in range(T):
        t_k = None if solver.sys.stationnary else t0 + k
        J_k = J_next[int(t0) + k] if timed else J_next
        q[k], u[k], _ = step(J_k, x[k], t_k)
        x[k + 1], g[k] = model_step(solver, x[k], u[k], None if w is None else w[k], t_k, time_index)
    return x, u, g, q


def monte_carlo_lookahead(solver, J_next, x0, n_steps, seed, n_burn, ids, law_grid, law_proba, occupancy=False, t0=0,
                          time_index='real', step=None, block=64):
    """Monte Carlo evaluation under lookahead controls, as a definition (kernel `sdp_montecarlo_lookahead`):
    (cost_sum (B,), n_outside (B,) int64, x_final (B, d), occupancy (state dims, int64) or None).

    Composed of existing definitions only.  Draws: `montecarlo.draws(seed, ids, steps, law_proba)` with the Philox
    counter's step k, the step of the call, and w = law_grid.astype(dt)[idx] (several variables: the column idx of
    the joint table (m, n)).  Steps: `simulate_lookahead`'s -- the box at the carried state in float64, the lattice
    rule with one rounding, the sequential expectation on the solver's OWN flat law, first-occurrence argmin, then
    dyn / cost at u_opt and the drawn w.  Reductions over the steps k >= n_burn, with x_k the state BEFORE the step in
    the problem's reals: acc = acc + g_k (one rounded add, k ascending), n_outside counts the x_k outside the grid or
    NaN, occupancy counts `montecarlo.nearest_nodes(x_k)`; x_final = x_T.

    (law_grid, law_proba) is the law the PLANT draws from; the expectation inside the backup always uses the solver's
    discretised law.  A state without a valid lattice gets u = NaN: the state goes NaN and stays, acc becomes NaN and
    every later counted step is outside -- nothing is special-cased.  `step`: the lookahead of one step, as in
    `simulate_lookahead`; `block`: steps drawn at a time (it changes no bit)."""
    from . import montecarlo as mc
    dt = np.dtype(solver.dtype)
    dims = tuple(len(g) for g in solver.state_grid)
    T, n_burn = int(n_steps), int(n_burn)
    J_next, timed = check_horizon(J_next, dims, T, t0)
    x = np.atleast_2d(np.asarray(x0, dtype=float)).astype(dt)
    B = x.shape[0]
    ids = np.asarray(ids)
    smin = np.array([dt.type(g[0]) for g in solver.state_grid], dtype=dt)
    smax = np.array([dt.type(g[-1]) for g in solver.state_grid], dtype=dt)
    wgrid = np.asarray(law_grid).astype(dt)
    acc = np.zeros(B, dtype=dt)
    n_out = np.zeros(B, dtype=np.int64)
    occ = np.zeros(dims, dtype=np.int64) if occupancy else None
    for k0 in range(0, T, int(block)):
        n = min(int(block), T - k0)
        idx = mc.draws(seed, ids, np.arange(k0, k0 + n, dtype=np.uint64), law_proba)
        w = wgrid[idx][:, None, :] if wgrid.ndim == 1 else np.moveaxis(wgrid[:, idx], 0, 1)       # (n, m, B)
        xs, _, g, _ = simulate_lookahead(solver, J_next, x, w, n, t0 + k0, time_index, step=step)
        for i in range(n):
            if k0 + i < n_burn:
                continue
            with np.errstate(all='ignore'):
                acc = acc + g[i]
                n_out += ~np.all((xs[i] >= smin) & (xs[i] <= smax), axis=1)
            if occ is not None:
                np.add.at(occ, tuple(mc.nearest_nodes(xs[i], solver.state_grid, dt).T), 1)
        x = xs[n]
    return acc, n_out, x, occ
