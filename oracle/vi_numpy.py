"""numpy restatement of the reference's value-iteration path, with the user's
Python callables evaluated exactly the way the reference evaluates them.

TEST INFRASTRUCTURE ONLY (see oracle/sdp_oracle.c header).  Slow by design:
one Python iteration per state node, like stodynprog/stodynprog.py:511-515.

Every function cites the reference lines it follows (paths relative to the
reference checkout: sdp.py = stodynprog/stodynprog.py, pyx =
stodynprog/dolointerpolation/multilinear_cython.pyx).

Pinning: tests/test_oracle.py checks this module against tests/golden/*.npz,
which tests/golden/make_golden.py produced by importing the real reference.
"""
import itertools

import numpy as np

_I32_MIN = -2 ** 31


def mlinterp_np(smin, smax, orders, values, s, wide=True):
    """pyx:17-49 dispatcher + pyx:51-300 point kernels, vectorised over points.

    Each numpy operator below is one IEEE operation per element, in the order
    of the Cython source, so results are bit-identical to the compiled
    reference for float32 and float64.

    wide=False: the lerp tree in the type of `values` from top to bottom -- what the sweep
    kernels evaluate (csrc/sdp_device.h: sdp_interp_point<real, D, wide = real>); the cell and
    lam are the same lines.  For float64 values the two forms are the same operations.
    """
    values = np.ascontiguousarray(values)
    dt = values.dtype.type
    s = np.ascontiguousarray(s, dtype=dt)
    d, n_s = s.shape
    if d < 1 or d > 4:
        raise Exception("Can't interpolate in dimension strictly greater than 5")  # pyx:47
    orders = [int(o) for o in orders]
    q, lam = [], []
    for k in range(d):
        sn = (s[k] - dt(smin[k])) / (dt(smax[k]) - dt(smin[k]))        # pyx:75
        p = sn * dt(orders[k] - 1)
        with np.errstate(invalid='ignore'):
            ok = np.abs(p) < dt(2147483648.0)
            t = np.where(ok, p, dt(0)).astype(np.int64)                # C truncation
        t = np.where(ok, t, _I32_MIN)                                  # x86 cvtt* indefinite
        qk = np.maximum(np.minimum(t, orders[k] - 2), 0)               # pyx:78
        q.append(qk)
        lam.append(p - qk.astype(dt))                                  # pyx:81
    M = [1] * d
    for k in range(d - 2, -1, -1):
        M[k] = M[k + 1] * orders[k + 1]
    out = np.zeros((values.shape[0], n_s), dtype=dt)
    # Cython emits the `1` of `(1-lam_k)` as the C double literal 1.0
    # (pyx:88,140,208,300), so in the float specialisation the lerp tree is
    # evaluated in double -- except the innermost `lam*v` product, float x
    # float -- and rounded to float once, on the store.
    lam64 = [l.astype(np.float64) for l in lam]
    # wide=False: oml = (real)1 - lam (sdp_device.h:sdp_locate_axis), then per axis, last axis
    # innermost, `oml * lo + lam * hi` with every operator in `dt` (sdp_device.h:SdpLerp)
    oml = [dt(1) - l for l in lam]
    for v in range(values.shape[0]):
        V = values[v]

        def rec_narrow(k, base):
            if k == d - 1:
                lo = V[base + M[k] * q[k]]
                hi = V[base + M[k] * (q[k] + 1)]
            else:
                lo = rec_narrow(k + 1, base + M[k] * q[k])
                hi = rec_narrow(k + 1, base + M[k] * (q[k] + 1))
            return oml[k] * lo + lam[k] * hi
        if not wide:
            out[v] = rec_narrow(0, np.zeros(n_s, dtype=np.int64))
            continue

        def rec(k, base):
            if k == d - 1:
                lo = V[base + M[k] * q[k]]
                hi = V[base + M[k] * (q[k] + 1)]
                return (1.0 - lam64[k]) * lo.astype(np.float64) + (lam[k] * hi).astype(np.float64)
            lo = rec(k + 1, base + M[k] * q[k])
            hi = rec(k + 1, base + M[k] * (q[k] + 1))
            return (1.0 - lam64[k]) * lo + lam64[k] * hi
        out[v] = rec(0, np.zeros(n_s, dtype=np.int64)).astype(dt)
    return out


class Interp:
    """sdp.py:255-290 (MlinInterpolator) on top of mlinterp_np."""

    def __init__(self, *x_grid):
        self.ndim = len(x_grid)
        self._xmin = np.array([x[0] for x in x_grid], dtype=float)     # sdp.py:263
        self._xmax = np.array([x[-1] for x in x_grid], dtype=float)    # sdp.py:264
        self._xshape = np.array([len(x) for x in x_grid], dtype=np.int64)
        self.values = None

    def set_values(self, values):
        assert values.shape == tuple(self._xshape)
        self.values = np.ascontiguousarray(np.atleast_2d(values.ravel()), dtype=float)

    def __call__(self, *x_interp):
        x_mesh = np.broadcast_arrays(*x_interp)                         # sdp.py:281
        shape = x_mesh[0].shape
        x_stack = np.vstack([x.astype(float).ravel() for x in x_mesh])  # sdp.py:283
        a = mlinterp_np(self._xmin, self._xmax, self._xshape, self.values, x_stack)
        return a.reshape(shape)


class Spec:
    """Plain container for a discretised problem (what DPSolver holds)."""

    def __init__(self, dyn, cost, control_box, state_grid, perturb_grid, perturb_proba,
                 control_steps, params=None, stationnary=True):
        self.dyn, self.cost, self.control_box = dyn, cost, control_box
        self.state_grid = [np.asarray(g, dtype=float) for g in state_grid]
        self.perturb_grid = [np.asarray(g, dtype=float) for g in perturb_grid]
        self.perturb_proba = [np.asarray(g, dtype=float) for g in perturb_proba]
        self.control_steps = tuple(control_steps)
        self.params = params or {}
        self.stationnary = stationnary
        self.shape = tuple(len(g) for g in self.state_grid)
        self.ref_ind = tuple(n // 2 for n in self.shape)                # sdp.py:384

    @classmethod
    def from_solver(cls, dpsolv):
        s = dpsolv.sys
        return cls(s.dyn, s.cost, s.control_box, dpsolv.state_grid, dpsolv.perturb_grid,
                   dpsolv.perturb_proba, dpsolv.control_steps, s.params, s.stationnary)


def control_grids(spec, state_k, t_k=None):
    """sdp.py:432-463."""
    if t_k is not None:
        state_k = (t_k,) + tuple(state_k)
    intervals = spec.control_box(*state_k, **spec.params)               # sdp.py:440
    grids, dims = [], []
    for (u_min, u_max), step in zip(intervals, spec.control_steps):
        width = u_max - u_min
        n_interv = width / step                                         # sdp.py:447
        if n_interv < 0.1:
            npts = 1
            u_grid = np.array([(u_min + u_max) / 2])                    # sdp.py:453
        else:
            npts = int(np.ceil(n_interv) + 1)                           # sdp.py:457
            u_grid = np.linspace(u_min, u_max, npts)
        grids.append(u_grid)
        dims.append(npts)
    return grids, tuple(dims)


def backup_node(spec, x_k, J_next_interp, t_k=None, full=False, dtype=None):
    """sdp.py:639-691 (_value_at_state_vect) plus index and margin.

    `dtype` given: the direct kernel's definition in that type (`backup_node_real`; J_next_interp
    is then an InterpReal)."""
    if dtype is not None:
        return backup_node_real(spec, x_k, J_next_interp, t_k, full)
    u_grids, control_dims = control_grids(spec, x_k, t_k)
    nb_control = len(u_grids)
    for i in range(nb_control):
        u_grids[i] = u_grids[i].reshape((1,) * i + (-1,) + (1,) * (nb_control - i))
    nb_perturb = len(spec.perturb_grid)
    args = tuple(x_k) + tuple(u_grids) + tuple(spec.perturb_grid)       # sdp.py:668
    if t_k is not None:
        args = (t_k,) + args
    x_next = spec.dyn(*args, **spec.params)                             # sdp.py:674
    g_k_grid = spec.cost(*args, **spec.params)                          # sdp.py:676
    J_k_grid = g_k_grid + J_next_interp(*x_next)                        # sdp.py:677
    if nb_perturb == 0:
        J = J_k_grid
    else:
        # sdp.py:681 uses np.inner (BLAS, summation order not source-defined);
        # the restatement sums sequentially in w order like the HIP kernel.
        w_proba = spec.perturb_proba[0]
        Jb = np.broadcast_to(J_k_grid, control_dims + (len(w_proba),))
        J = np.zeros(control_dims)
        for w in range(len(w_proba)):
            J = J + Jb[..., w] * w_proba[w]
    J = np.asarray(J, dtype=float).reshape(control_dims)
    flat = int(J.argmin())                                              # sdp.py:686
    ind_opt = np.unravel_index(flat, control_dims)
    J_opt = J[ind_opt]
    u_opt = [u_grids[i].flatten()[ind_opt[i]] for i in range(nb_control)]
    Jr = J.ravel()
    if Jr.size > 1:
        margin = np.partition(Jr, 1)[1] - Jr[flat] if not np.isnan(Jr).any() else 0.0
    else:
        margin = np.inf
    if full:
        return J_opt, u_opt, flat, margin, J
    return J_opt, u_opt, flat, margin


def value_iteration(spec, J_next, rel_dp=False, t_k=None, nodes=None, dtype=None):
    """sdp.py:466-534.  Returns (J_k | (J_k, J_ref)), pol_k, idx_k, margin_k.

    `nodes`: optional iterable of flat C-order node ids; then 1-D outputs for
    those nodes only (used for sampled parity on big grids).

    `dtype`: None is the reference's path in float64, the code below.  np.float32 or np.float64
    is the direct kernel's definition restated in that type (`value_iteration_real`): J and the
    policy come back in `dtype`.
    """
    if dtype is not None:
        return value_iteration_real(spec, J_next, dtype, rel_dp, t_k, nodes)
    if rel_dp:
        J_next, _ = J_next
        assert J_next[spec.ref_ind] == 0.                               # sdp.py:488
    interp = Interp(*spec.state_grid)
    interp.set_values(np.asarray(J_next, dtype=float))
    nu = len(spec.control_steps)
    if nodes is not None:
        nodes = np.asarray(nodes, dtype=np.int64)
        J = np.zeros(len(nodes)); pol = np.zeros((len(nodes), nu))
        idx = np.zeros(len(nodes), dtype=np.int64); mar = np.zeros(len(nodes))
        for n, flat in enumerate(nodes):
            ind = np.unravel_index(flat, spec.shape)
            x_k = tuple(g[i] for g, i in zip(spec.state_grid, ind))
            J[n], pol[n], idx[n], mar[n] = backup_node(spec, x_k, interp, t_k)
        return J, pol, idx, mar
    J_k = np.zeros(spec.shape)
    pol_k = np.zeros(spec.shape + (nu,))
    idx_k = np.zeros(spec.shape, dtype=np.int64)
    mar_k = np.zeros(spec.shape)
    state_ind = itertools.product(*[range(n) for n in spec.shape])      # sdp.py:480
    for ind_x, x_k in zip(state_ind, itertools.product(*spec.state_grid)):
        J_k[ind_x], pol_k[ind_x], idx_k[ind_x], mar_k[ind_x] = \
            backup_node(spec, x_k, interp, t_k)
    if rel_dp:
        J_ref = J_k[spec.ref_ind]                                       # sdp.py:524
        J_k -= J_ref
        return (J_k, J_ref), pol_k, idx_k, mar_k
    return J_k, pol_k, idx_k, mar_k


def eval_policy(spec, pol, n_iter, rel_dp=False, J_zero=None, J_ref_full=False, nodes=None, dtype=None,
                t_k=None):
    """sdp.py:693-775 with the expectation summed sequentially in w order.

    `nodes`: optional flat C-order node ids; then one step (n_iter == 1, no rel_dp) at those nodes only, a 1-D
    result (the same operations per node as the whole grid: sampled parity on big grids).

    `dtype`: None is the reference's path in float64, the code below; a type is the fixed-policy kernel's definition
    restated in it (`eval_policy_real`; `t_k` is the time index of a non-stationary model there)."""
    if dtype is not None:
        return eval_policy_real(spec, pol, n_iter, dtype, rel_dp, J_zero, J_ref_full, nodes, t_k)
    assert t_k is None
    if nodes is not None:
        assert n_iter == 1 and not rel_dp
        nodes = np.asarray(nodes, dtype=np.int64)
        ind = np.unravel_index(nodes, spec.shape)
        interp = Interp(*spec.state_grid)
        interp.set_values(np.zeros(spec.shape) if J_zero is None else J_zero)
        args = tuple(g[i].reshape(-1, 1) for g, i in zip(spec.state_grid, ind))
        args = args + tuple(pol[ind + (c,)].reshape(-1, 1) for c in range(pol.shape[-1])) + (spec.perturb_grid[0],)
        x_next = spec.dyn(*args, **spec.params)
        g = spec.cost(*args, **spec.params)
        J_k_grid = np.broadcast_to(g + interp(*x_next), (len(nodes), len(spec.perturb_grid[0])))
        J = np.zeros(len(nodes))
        for w in range(len(spec.perturb_proba[0])):
            J = J + J_k_grid[:, w] * spec.perturb_proba[0][w]
        return J
    dims = spec.shape
    nb_state = len(dims)
    J_pol = np.zeros(dims) if J_zero is None else J_zero
    J_ref = np.zeros(n_iter)
    nb_control = pol.shape[-1]
    w_k = spec.perturb_grid[0]
    w_proba = spec.perturb_proba[0]
    state_grid = tuple(np.reshape(spec.state_grid[i], (1,) * i + (-1,) + (1,) * (nb_state - i))
                       for i in range(nb_state))                        # sdp.py:732-739
    for k in range(n_iter):
        interp = Interp(*spec.state_grid)
        interp.set_values(J_pol)
        u_k = [pol[..., i].reshape(dims + (1,)) for i in range(nb_control)]
        args = state_grid + tuple(u_k) + (w_k,)
        x_next = spec.dyn(*args, **spec.params)
        g = spec.cost(*args, **spec.params)
        J_k_grid = np.broadcast_to(g + interp(*x_next), dims + (len(w_k),))
        J_pol = np.zeros(dims)
        for w in range(len(w_proba)):
            J_pol = J_pol + J_k_grid[..., w] * w_proba[w]
        if rel_dp:
            J_ref[k] = J_pol[spec.ref_ind]                              # sdp.py:761
            J_pol -= J_ref[k]
    if rel_dp:
        return J_pol, (J_ref if J_ref_full else J_ref[-1])
    return J_pol


# ---------------------------------------------------------------------------------------------------------------
# The definition the direct kernel implements (stodynprog_amd/csrc/sdp_sweep_kernel.h with sdp_device.h), restated
# in one real type `dt`.  The sweep kernels are compiled with -ffp-contract=off -fno-fast-math: one IEEE operation
# per source operator, and so is every numpy operator on arrays of `dt`.  Each line cites the kernel line it follows
# (sweep.h = csrc/sdp_sweep_kernel.h, device.h = csrc/sdp_device.h, solver.py = stodynprog_amd/solver.py).
#
# In float64 these are the operations of the reference's path above: the lattice is numpy.linspace's own arithmetic
# (step = delta / (n - 1), y = arange(n) * step + start, y[-1] = stop), the lerp tree is in double either way.
# In float32 it is what nothing else in this module states: constants rounded ONCE from the solver's float64 values,
# the callables on float32 arrays (numpy >= 2: Python float constants are weak), the whole tree in float32.
# ---------------------------------------------------------------------------------------------------------------
class InterpReal:
    """J_next on the state grid as the sweep kernels read it: axes rounded once to `dt` (solver.py:_create_problem),
    smin = axes[0], smax = axes[-1] in `dt` (sweep.h:sdp_grid_from_args), the pure-`dt` tree
    (sweep.h:sdp_expected_cost -> device.h:sdp_interp_point<real, D, wide = real>)."""

    def __init__(self, spec, values, dtype):
        self.dt = dt = np.dtype(dtype).type
        self.axes = [np.ascontiguousarray(g, dtype=dt) for g in spec.state_grid]      # solver.py:_create_problem
        self.smin = [a[0] for a in self.axes]                                         # sweep.h:sdp_grid_from_args
        self.smax = [a[-1] for a in self.axes]
        self.orders = [len(a) for a in self.axes]
        values = np.asarray(values)
        assert values.dtype == dt, (values.dtype, dt)           # (the caller rounds: DPSolver casts J_next once)
        self.values = np.ascontiguousarray(values).reshape(1, -1)

    def __call__(self, *x_next):
        dt = self.dt
        for v in x_next:            # a wider result would be rounded twice; a Python float is weak and may pass
            assert not isinstance(v, (np.ndarray, np.generic)) or v.dtype == dt, (v.dtype, dt)
        x_mesh = np.broadcast_arrays(*[np.asarray(v, dtype=dt) for v in x_next])
        shape = x_mesh[0].shape
        s = np.vstack([x.ravel() for x in x_mesh])
        # (the power-of-two spans' product with the reciprocal, device.h:sdp_div_span, is the true division's bits:
        # stated as the division here, so that claim is checked too)
        return mlinterp_np(self.smin, self.smax, self.orders, self.values, s, wide=False).reshape(shape)


def control_lattice_real(spec, x_k, t_k, dt):
    """Per control (lo, hi, n) as the host hands them to the kernel and the points the kernel makes of them.

    solver.py:_box_lattice (the reference's control_grids, sdp.py:446-457) in float64: n from the width and the step
    hint; a single point is the centre, stored as lo = hi.  Then ONE rounding of lo and hi to `dt`
    (solver.py:_create_problem).  Points: sweep.h:sdp_load_box / sdp_control_value."""
    state = tuple(x_k) if t_k is None else (t_k,) + tuple(x_k)
    intervals = spec.control_box(*state, **spec.params)                             # float64, as the host calls it
    grids, dims = [], []
    with np.errstate(all='ignore'):
        for (u_min, u_max), hint in zip(intervals, spec.control_steps):
            n_interv = (u_max - u_min) / hint                                       # solver.py:_box_lattice
            if n_interv < 0.1:
                n = 1
                lo = hi = dt((u_min + u_max) / 2)
            else:
                n = int(np.ceil(n_interv) + 1)
                lo, hi = dt(u_min), dt(u_max)
            if n == 1:
                u = np.array([lo], dtype=dt)                                        # sdp_control_value: n == 1 -> lo
            else:
                delta = hi - lo                                                     # sdp_load_box: delta
                step = delta / dt(n - 1)                                            # sdp_load_box: step
                k = np.arange(n).astype(dt)                                         # (sdp_real)k
                if step == dt(0):                                                   # sdp_control_value: step == 0
                    u = (k / dt(n - 1)) * delta + lo
                else:
                    u = k * step + lo                                               # sdp_control_value: k * step + lo
                u[n - 1] = hi                                                       # sdp_control_value: last point
            assert u.dtype == dt
            grids.append(u)
            dims.append(n)
    return grids, tuple(dims)


def _check_real(values, dt):
    """every result of a callable is of type `dt` (or a weak Python number): a wider one would be rounded twice"""
    for v in values:
        assert not isinstance(v, (np.ndarray, np.generic)) or v.dtype == dt, \
            'the model returns {} from {} arguments'.format(v.dtype, np.dtype(dt))


def _expectation_real(spec, J_cell, shape, dt):
    """sweep.h:sdp_expected_cost: acc = 0; acc = acc + jc * p_w for w ascending, every operator in `dt`; a deterministic
    system is g + J(f) itself.  J_cell: shape + (W,) (broadcastable)."""
    if len(spec.perturb_grid) == 0:
        return np.array(np.broadcast_to(J_cell, shape + (1,))[..., 0], dtype=dt)     # (the w axis has length 1)
    proba = np.ascontiguousarray(spec.perturb_proba[0], dtype=dt)                  # solver.py:_create_problem
    Jb = np.broadcast_to(J_cell, shape + (len(proba),))
    acc = np.zeros(shape, dtype=dt)
    for w in range(len(proba)):
        acc = acc + Jb[..., w] * proba[w]
    assert acc.dtype == dt
    return acc


def backup_node_real(spec, x_k, interp, t_k=None, full=False):
    """One node of sweep.h:sdp_sweep.  x_k: the node's float64 coordinates (the box is the host's, in float64; the
    kernel reads the axes rounded to `dt`: sdp_node_coords)."""
    dt = interp.dt
    u_grids, control_dims = control_lattice_real(spec, x_k, t_k, dt)
    nb_control = len(u_grids)
    u_mesh = [u.reshape((1,) * i + (-1,) + (1,) * (nb_control - i)) for i, u in enumerate(u_grids)]   # C order, control 0 slowest
    args = tuple(dt(x) for x in x_k) + tuple(u_mesh)                                # sdp_node_coords
    if len(spec.perturb_grid):
        args = args + (np.ascontiguousarray(spec.perturb_grid[0], dtype=dt),)       # solver.py:_create_problem
    if t_k is not None:
        args = (dt(t_k),) + args                                                    # sdp_sweep: t = (sdp_real)a.t_k
    x_next = spec.dyn(*args, **spec.params)
    g = spec.cost(*args, **spec.params)
    _check_real(tuple(x_next) + (g,), dt)
    J_cell = g + interp(*x_next)                                                    # sdp_expected_cost: jc = g + interp
    J = _expectation_real(spec, J_cell, control_dims, dt)
    flat = int(J.argmin())          # first occurrence, the first NaN wins (device.h:sdp_better_seq / sdp_better_idx)
    ind_opt = np.unravel_index(flat, control_dims)
    J_opt = J[ind_opt]
    u_opt = [u_grids[i][ind_opt[i]] for i in range(nb_control)]                     # sdp_controls_at(box, ibest)
    Jr = J.ravel()
    if Jr.size > 1:
        margin = float(np.partition(Jr, 1)[1] - Jr[flat]) if not np.isnan(Jr).any() else 0.0
    else:
        margin = np.inf
    if full:
        return J_opt, u_opt, flat, margin, J
    return J_opt, u_opt, flat, margin


def value_iteration_real(spec, J_next, dtype, rel_dp=False, t_k=None, nodes=None):
    """sweep.h:sdp_sweep on every node (or on `nodes`).  J_next is rounded to `dtype` once, as DPSolver does
    (solver.py:_DeviceProblem.set_value); J and the policy come back in `dtype`, the margin in float64."""
    dt = np.dtype(dtype).type
    if rel_dp:
        J_next, _ = J_next
    interp = InterpReal(spec, np.asarray(J_next).astype(dt, copy=False), dt)
    if rel_dp:
        assert interp.values[0, np.ravel_multi_index(spec.ref_ind, spec.shape)] == 0.
    nu = len(spec.control_steps)
    whole = nodes is None
    nodes = np.arange(int(np.prod(spec.shape))) if whole else np.asarray(nodes, dtype=np.int64)
    J = np.zeros(len(nodes), dtype=dt); pol = np.zeros((len(nodes), nu), dtype=dt)
    idx = np.zeros(len(nodes), dtype=np.int64); mar = np.zeros(len(nodes))
    for n, flat in enumerate(nodes):
        ind = np.unravel_index(flat, spec.shape)
        x_k = tuple(g[i] for g, i in zip(spec.state_grid, ind))
        J[n], pol[n], idx[n], mar[n] = backup_node_real(spec, x_k, interp, t_k)
    if not whole:
        assert not rel_dp
        return J, pol, idx, mar
    J, pol = J.reshape(spec.shape), pol.reshape(spec.shape + (nu,))
    idx, mar = idx.reshape(spec.shape), mar.reshape(spec.shape)
    if rel_dp:
        J_ref = J[spec.ref_ind]
        return (J - J_ref, float(J_ref)), pol, idx, mar                            # one subtraction in `dt` per node
    return J, pol, idx, mar


def eval_policy_real(spec, pol, n_iter, dtype, rel_dp=False, J_zero=None, J_ref_full=False, nodes=None, t_k=None):
    """sweep.h:sdp_evalpol, n_iter times.  The policy and J_zero are rounded to `dtype` once
    (solver.py:_DeviceProblem.set_policy / set_value).  Relative DP: step k reads every vertex as V - V[ref], ONE
    rounding per vertex before the lerp (device.h:SdpLerp<.., SHIFT = true>) -- the bits of the reference's in-place
    `J_pol -= J_ref[k]` (sdp.py:760-762) done in `dtype`, which is how it is stated here; J_ref per step is V[ref]."""
    dt = np.dtype(dtype).type
    dims = spec.shape
    nb_state = len(dims)
    pol = np.asarray(pol).astype(dt, copy=False)
    nb_control = pol.shape[-1]
    J_pol = np.zeros(dims, dtype=dt) if J_zero is None else np.asarray(J_zero).astype(dt, copy=False)
    axes = [np.ascontiguousarray(g, dtype=dt) for g in spec.state_grid]            # sdp_node_coords
    if nodes is not None:
        assert n_iter == 1 and not rel_dp
        ind = np.unravel_index(np.asarray(nodes, dtype=np.int64), dims)
        out_dims = (len(nodes),)
        x = tuple(a[i].reshape(-1, 1) for a, i in zip(axes, ind))
        u = tuple(pol[ind + (c,)].reshape(-1, 1) for c in range(nb_control))
    else:
        out_dims = dims
        x = tuple(np.reshape(axes[i], (1,) * i + (-1,) + (1,) * (nb_state - i)) for i in range(nb_state))
        u = tuple(pol[..., c].reshape(dims + (1,)) for c in range(nb_control))
    args = x + u
    if len(spec.perturb_grid):
        args = args + (np.ascontiguousarray(spec.perturb_grid[0], dtype=dt),)
    if t_k is not None:
        args = (dt(t_k),) + args
    J_ref = np.zeros(n_iter)
    for k in range(n_iter):
        interp = InterpReal(spec, J_pol, dt)
        x_next = spec.dyn(*args, **spec.params)
        g = spec.cost(*args, **spec.params)
        _check_real(tuple(x_next) + (g,), dt)
        J_pol = _expectation_real(spec, g + interp(*x_next), out_dims, dt)          # sdp_expected_cost<SHIFT>
        if rel_dp:
            J_ref[k] = J_pol[spec.ref_ind]
            J_pol = J_pol - J_pol[spec.ref_ind]                                     # SdpLerp<.., SHIFT = true>
    if rel_dp:
        return J_pol, (J_ref if J_ref_full else J_ref[-1])
    return J_pol


def simulate(spec, pol, x0, w, T, t0=0, dtype=np.float64):
    """The closed loop of the reference's examples (examples/20 Searev storage control/storage_control.py:242-251):

        for k in range(T):
            u[k] = [interp_on_state(pol[..., c])(*x[k]) for c in range(nb_control)]
            x[k+1] = dyn(*x[k], *u[k], w[k])

    batched over B trajectories.  The policy lookup is mlinterp_np (the compiled reference's bits in float32 and
    float64); dyn and cost run on numpy arrays of `dtype`, one element per trajectory (numpy >= 2: Python float
    constants are weak, so 4-byte arithmetic stays in float32).  A non-stationary model gets the time index t0 + k
    first, as a scalar of `dtype`.

    pol: state_dims + (nb_control,); x0: (B, nb_state); w: (>= T, B), or None for a deterministic model.
    Returns x (T+1, B, nb_state), u (T, B, nb_control), g (T, B), all of `dtype`."""
    dt = np.dtype(dtype).type
    pol = np.asarray(pol)
    x0 = np.atleast_2d(np.asarray(x0, dtype=float))
    B, d = x0.shape
    nu = pol.shape[-1]
    assert pol.shape == spec.shape + (nu,) and d == len(spec.shape)
    smin = [g[0] for g in spec.state_grid]
    smax = [g[-1] for g in spec.state_grid]
    values = np.ascontiguousarray(np.moveaxis(pol, -1, 0).reshape(nu, -1), dtype=dt)
    x = np.zeros((T + 1, B, d), dtype=dt)
    u = np.zeros((T, B, nu), dtype=dt)
    g = np.zeros((T, B), dtype=dt)
    x[0] = x0.astype(dt)
    for k in range(T):
        u[k] = mlinterp_np(smin, smax, spec.shape, values, x[k].T).T                # storage_control.py:246
        args = tuple(x[k, :, i] for i in range(d)) + tuple(u[k, :, c] for c in range(nu))
        if w is not None:
            args = args + (np.asarray(w[k], dtype=dt),)
        if not spec.stationnary:
            args = (dt(t0 + k),) + args
        xn = spec.dyn(*args, **spec.params)                                         # storage_control.py:248
        gk = spec.cost(*args, **spec.params)
        for v in tuple(xn) + (gk,):         # (a wider result would be rounded twice on the store)
            assert not isinstance(v, np.ndarray) or v.dtype == dt, (v.dtype, dt)
        for i in range(d):
            x[k + 1, :, i] = xn[i]
        g[k] = gk
    return x, u, g
