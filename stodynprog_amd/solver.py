"""Dynamic-programming solver: the drop-in `DPSolver` class.

Host-side mirror of the reference's solver API (reference
stodynprog/stodynprog.py:317-876).  The discretisation helpers stay in numpy
(same operators as the reference, so grids and weights are bit-identical); the
sweeps run on the GPU:

  value_iteration / bellman_recursion
      -> sdp_problem_vi_sweep   (fused node x control x perturbation backup)
  eval_policy / policy_iteration
      -> sdp_problem_eval_policy (device-resident fixed-policy backups)
  interp_on_state(...)(coords)
      -> sdp_mlinterp_f64 / _f32

The user's `dyn` and `cost` callables are traced once (trace.py) and compiled
into the sweep kernel (codegen.py).  Callables that cannot be traced are
evaluated on the host exactly as the reference does and only the gather /
expectation / argmin runs on the device (sdp_tab_backup, "tabulated mode").
There is no CPU compute fallback: without the HIP library and a GPU every
sweep raises.
"""
from __future__ import division, print_function
import ctypes as C
import itertools
from datetime import datetime

import numpy as np

from . import _native as nat
from . import codegen
from . import convergence as conv
from . import forward
from . import montecarlo as mc
from . import perturb
from .interp import MlinInterpolator
from .trace import TraceError, trace_model, trace_box, callable_fingerprint, _fp_value, _NoFingerprint

__all__ = ['DPSolver', 'TransitionOperator']


class _DeviceProblem(object):
    """Owner of one sdp_problem handle (include/sdp_hip.h)."""

    def __init__(self, desc_arrays, module_path, dtype, shape, nu, W, lanes, box_per_node,
                 node_range, comm=None, slab_bounds=None, layout=0, staged=None, col_seg_nodes=0, n_perturb=0):
        self._keep = desc_arrays            # host arrays referenced by the descriptor
        self.layout = int(layout)
        self.dtype = np.dtype(dtype)
        self.shape = tuple(shape)
        self.S = int(np.prod(shape))
        self.nu = nu
        # shape of the per-node arrays as the device stores them
        self.dev_shape = (self.shape[1:] + self.shape[:1]
                          if self.layout == nat.LAYOUT_COLUMNS else self.shape)
        d = nat.sdp_problem_desc()
        d.dtype = nat.np_real(dtype)
        d.d, d.nu, d.W = len(shape), nu, W
        for k, n in enumerate(shape):
            d.orders[k] = n
            d.axes[k] = desc_arrays['axes'][k].ctypes.data
        if W > 0:
            d.wgrid = desc_arrays['wgrid'].ctypes.data
            d.proba = desc_arrays['proba'].ctypes.data
        d.box_per_node = int(box_per_node)
        d.lanes_per_node = int(lanes)
        d.layout = int(layout)
        d.col_seg_nodes = int(col_seg_nodes)
        d.n_perturb = int(n_perturb)            # 0: "1 when W > 0"; 2..4: wgrid is [n_perturb][W], the flat law
        d.variant = nat.VARIANT_STAGED if staged else nat.VARIANT_DIRECT
        if staged:
            for k, n in enumerate(staged['tile']):
                d.tile[k] = int(n)
        d.box_lo = desc_arrays['box_lo'].ctypes.data
        d.box_hi = desc_arrays['box_hi'].ctypes.data
        d.box_n = desc_arrays['box_n'].ctypes.data
        d.node_begin, d.node_end = node_range
        d.module_path = module_path.encode()
        h = C.c_void_p()
        rc = nat.lib().sdp_problem_create(C.byref(d), C.byref(h))
        if comm is not None and comm.nranks > 1:
            # What follows (attaching the communicator, mapping the peers' buffers, need lists) is collective, and so
            # is what the caller does about a failure (DPSolver._problem re-plans without the reduced-array sweep when
            # the device memory does not suffice): the ranks agree HERE whether every one of them has its problem --
            # all go on or all raise (advisor, round 4: one rank out of memory left the others in a collective)
            why = None if rc == 0 else nat.lib().sdp_last_error().decode(errors='replace')
            if comm.allreduce_max(0.0 if rc == 0 else 1.0) > 0:
                if rc == 0:
                    nat.lib().sdp_problem_destroy(h)
                    raise MemoryError('another rank could not create its problem (out of device memory there?)')
                if rc != -4:
                    raise nat._ERR.get(rc, RuntimeError)(why)
                raise MemoryError(why)
        else:
            nat.check(rc)
        self.h = h
        self.node_range = tuple(node_range)
        self.parts = None
        # sharded: what DPSolver._set_exchange_lists keeps up to date -- the need lists of a sparse exchange, the lead
        # halo -- and the bits of the constants they were made from
        self.sparse_needs = self.lead_halo = False
        self.lists_of = None
        if comm is not None:
            # slab_bounds: [n_phases][nranks+1] partition (dist.phase_partition)
            self.parts = np.ascontiguousarray(slab_bounds, dtype=np.int64)
            nat.check(nat.lib().sdp_problem_attach_comm(self.h, comm.handle,
                                                        int(self.parts.shape[0]),
                                                        nat.ptr(self.parts)))

    def close(self):
        if getattr(self, 'h', None):
            nat.lib().sdp_problem_destroy(self.h)
            self.h = None

    def unmap_peers(self):
        """first half of tearing down a sharded problem: the peers' buffers leave this process (every rank does
        this, then a barrier, then close(): memory a peer still maps must not be freed under it)"""
        if getattr(self, 'h', None):
            nat.check(nat.lib().sdp_problem_disable_peer_exchange(self.h))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # per-node arrays cross the C API in the reference's C order; the library
    # keeps them axis-0-fastest on the device when the column kernels are used.
    # These two helpers express that order in numpy (host-side gather, tests).
    def _to_device_order(self, A, extra=(), dtype=None):
        A = np.asarray(A, dtype=dtype or self.dtype).reshape(self.shape + extra)
        if self.layout == nat.LAYOUT_COLUMNS:
            A = np.moveaxis(A, 0, len(self.shape) - 1)
        return np.ascontiguousarray(A)

    def _from_device_order(self, A, extra=()):
        if self.layout == nat.LAYOUT_COLUMNS:
            A = A.reshape(self.shape[1:] + self.shape[:1] + extra)
            A = np.moveaxis(A, len(self.shape) - 1, 0)
        return np.ascontiguousarray(A).reshape(self.shape + extra)

    def set_value(self, V):
        assert np.size(V) == self.S
        V = np.ascontiguousarray(V, dtype=self.dtype)       # reference order; the library converts
        nat.check(nat.lib().sdp_problem_set_value(self.h, nat.ptr(V)))

    def set_policy(self, pol):
        assert np.size(pol) == self.S * self.nu
        pol = np.ascontiguousarray(pol, dtype=self.dtype)
        nat.check(nat.lib().sdp_problem_set_policy(self.h, nat.ptr(pol)))

    def set_params(self, values):
        """lifted model constants of the launches that follow (sdp_problem_set_params)"""
        values = np.ascontiguousarray(values, dtype=self.dtype)
        nat.check(nat.lib().sdp_problem_set_params(self.h, nat.ptr(values), int(values.size)))

    def sweep(self, t_k=0.0, rel_dp=False, ref_index=0):
        ref = C.c_double(0.0)
        nat.check(nat.lib().sdp_problem_vi_sweep(self.h, float(t_k), int(bool(rel_dp)),
                                                 int(ref_index), C.byref(ref)))
        return ref.value

    def eval_policy(self, n_iter, rel_dp=False, ref_index=0):
        refs = np.zeros(max(int(n_iter), 1))
        nat.check(nat.lib().sdp_problem_eval_policy(self.h, int(n_iter), int(bool(rel_dp)),
                                                    int(ref_index), nat.ptr(refs)))
        return refs[:int(n_iter)]

    def until(self, evalpol, n_max, rel_dp, ref_index, check_every, tol):
        """the loop of `sweep` + `swap` (evalpol False) or of `eval_policy` (True) with the convergence check inside
        the library (sdp_problem_vi_until / sdp_problem_eval_policy_until).  Returns (sweeps done, checked sweeps,
        [n_checks][2] dmin / dmax, reference costs of the sweeps done)"""
        schedule = conv.check_schedule(int(n_max), int(check_every))
        stats = np.zeros((len(schedule), 2))
        refs = np.zeros(int(n_max))
        n_done = C.c_int32(0)
        fn = nat.lib().sdp_problem_eval_policy_until if evalpol else nat.lib().sdp_problem_vi_until
        nat.check(fn(self.h, int(n_max), int(bool(rel_dp)), int(ref_index), int(check_every), float(tol),
                     C.byref(n_done), nat.ptr(stats), nat.ptr(refs)))
        n = n_done.value
        checked = [k for k in schedule if k <= n]
        return n, checked, stats[:len(checked)], refs[:n]

    def backup_host(self, V, t_k=0.0, rel_dp=False, ref_index=0, overlap=True):
        """value_iteration's device work with host arrays in and out in ONE library call
        (sdp_problem_backup_host): upload, sweep, relative-DP shift, download of J and of
        the policy values, one synchronisation.  Large outputs live in page-locked memory
        (ordinary writable ndarrays for the caller) so the copies run at PCIe rate; fed
        back as the next J_next they upload at that rate too.  The lattice indices stay
        on the device until asked for (get_index)."""
        V = np.ascontiguousarray(V, dtype=self.dtype)
        big = self.S * self.dtype.itemsize >= (1 << 20)
        new = nat.pinned_empty if big else np.empty
        J = new(self.shape, self.dtype)
        pol = new(self.shape + (self.nu,), self.dtype)
        ref = C.c_double(0.0)
        nat.check(nat.lib().sdp_problem_set_host_overlap(self.h, int(bool(overlap))))
        nat.check(nat.lib().sdp_problem_backup_host(self.h, nat.ptr(V), float(t_k), int(bool(rel_dp)),
                                                    int(ref_index), nat.ptr(J), nat.ptr(pol), None,
                                                    C.byref(ref)))
        return J, pol, ref.value

    def get_index(self):
        idx = np.empty(self.shape, dtype=np.int32)
        nat.check(nat.lib().sdp_problem_get_policy(self.h, None, nat.ptr(idx)))
        return idx

    def swap(self):
        nat.check(nat.lib().sdp_problem_swap(self.h))

    def complete(self):
        """sparse peer exchange: make J complete on every rank (collective; no-op otherwise)"""
        nat.check(nat.lib().sdp_problem_complete_value(self.h))

    def get_value(self):
        J = np.empty(self.shape, dtype=self.dtype)
        nat.check(nat.lib().sdp_problem_get_value(self.h, nat.ptr(J)))
        return J

    def get_policy(self):
        pol = np.empty(self.shape + (self.nu,), dtype=self.dtype)
        idx = np.empty(self.shape, dtype=np.int32)
        nat.check(nat.lib().sdp_problem_get_policy(self.h, nat.ptr(pol), nat.ptr(idx)))
        return pol, idx

    def last_kernel_ms(self):
        ms = C.c_double(0.0)
        nat.check(nat.lib().sdp_problem_last_kernel_ms(self.h, C.byref(ms)))
        return ms.value

    def bench_sweeps(self, reps, rel_dp=False, ref_index=0):
        loop, kern = C.c_double(0.0), C.c_double(0.0)
        nat.check(nat.lib().sdp_problem_bench_sweeps(self.h, int(reps), int(bool(rel_dp)),
                                                     int(ref_index), C.byref(loop),
                                                     C.byref(kern)))
        return loop.value, kern.value


class TransitionOperator(object):
    """The transition operator of a policy on the device (`DPSolver.transition_operator`): P^T as a CSR matrix in
    device memory, owner of one sdp_transop handle (include/sdp_hip.h).  `stodynprog_amd.forward` is the definition
    of every number it returns.  NOT in the reference API.

    shape     : the state grid's
    nnz       : entries, S W 2^d
    mean_cost : gbar, the expected cost of one step from every node (grid shape)
    path      : 'device' (entries from kernel sdp_transitions) or 'host' (callables evaluated on the host, entries
                uploaded: models that cannot be traced)"""

    def __init__(self, handle, shape, dtype, nnz, mean_cost, path):
        self.h = handle
        self.shape = tuple(shape)
        self.dtype = np.dtype(dtype)
        self.S = int(np.prod(self.shape))
        self.nnz = int(nnz)
        self.mean_cost = mean_cost
        self.path = path
        self.nbytes = forward.operator_bytes(self.nnz, self.S, self.dtype.itemsize)
        self.info = dict(nnz=self.nnz, bytes=self.nbytes, path=path)
        entries_ms, sort_ms = C.c_double(0.0), C.c_double(0.0)
        nat.check(nat.lib().sdp_transop_build_ms(self.h, C.byref(entries_ms), C.byref(sort_ms)))
        self.info.update(build_ms=entries_ms.value + sort_ms.value, entries_ms=entries_ms.value, sort_ms=sort_ms.value)

    @classmethod
    def from_coo(cls, shape, tgt, src, val, mean_cost=None, path='host'):
        """the operator of host-given entries in emission order (sdp_transop_from_coo): tgt, src node ids, val reals
        (their type is the operator's)"""
        nat.require_gpu()
        shape = tuple(int(n) for n in np.atleast_1d(shape))
        S = int(np.prod(shape))
        val = np.ascontiguousarray(val)
        tgt = np.ascontiguousarray(tgt, dtype=np.int32)
        src = np.ascontiguousarray(src, dtype=np.int32)
        if not (tgt.shape == src.shape == val.shape and tgt.ndim == 1):
            raise ValueError('tgt, src and val must be vectors of one length')
        h = C.c_void_p()
        nat.check(nat.lib().sdp_transop_from_coo(nat.np_real(val.dtype), S, tgt.size, nat.ptr(tgt), nat.ptr(src),
                                                 nat.ptr(val), C.byref(h)))
        return cls(h, shape, val.dtype, tgt.size, mean_cost, path)

    def close(self):
        if getattr(self, 'h', None):
            nat.lib().sdp_transop_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _handle(self):
        if not self.h:
            raise ValueError('the operator is closed')
        return self.h

    def _vector(self, mu):
        mu = np.asarray(mu)
        if mu.size != self.S:
            raise ValueError('mu has {} entries, the grid {} nodes'.format(mu.size, self.S))
        return np.ascontiguousarray(mu, dtype=self.dtype).reshape(-1)

    def _kernel_ms(self):
        ms = C.c_double(0.0)
        nat.check(nat.lib().sdp_transop_last_kernel_ms(self._handle(), C.byref(ms)))
        return ms.value

    def push(self, mu, n_steps=1):
        """mu after n_steps steps under the policy, (P^T)^n mu: an array of grid shape in the problem's dtype.  The
        steps run back to back on the device."""
        n_steps = int(n_steps)
        if n_steps < 0:
            raise ValueError('n_steps must not be negative')
        nat.check(nat.lib().sdp_transop_push(self._handle(), nat.ptr(self._vector(mu)), n_steps))
        self.info.update(push_ms=self._kernel_ms(), pushes=n_steps)
        out = np.empty(self.S, dtype=self.dtype)
        nat.check(nat.lib().sdp_transop_get(self.h, nat.ptr(out)))
        return out.reshape(self.shape)

    def stationary(self, mu0=None, tol=1e-12, n_max=10000, check_every=10):
        """Power iteration mu <- P^T mu from mu0 (default: uniform) until max |mu_{k+1} - mu_k| <= tol at a checked
        push (every check_every-th and the n_max-th), without renormalisation or damping (`forward.stationary` is the
        definition).  Returns a `forward.Stationary` record: mu (grid shape), n_done, converged, delta,
        average_cost = dot(mu, mean_cost) (computed on the host) and mass = mu.sum()."""
        tol, check_every = conv.validate(tol, check_every)
        n_max = int(n_max)
        if n_max < 1:
            raise ValueError('n_max must be at least 1')
        mu0 = forward.uniform(self.S, self.dtype) if mu0 is None else self._vector(mu0)
        nat.check(nat.lib().sdp_transop_push(self._handle(), nat.ptr(mu0), 0))
        n_done, delta = C.c_int32(0), C.c_double(0.0)
        nat.check(nat.lib().sdp_transop_push_until(self.h, n_max, check_every, tol, C.byref(n_done), C.byref(delta)))
        self.info.update(push_ms=self._kernel_ms(), pushes=n_done.value)
        mu = np.empty(self.S, dtype=self.dtype)
        nat.check(nat.lib().sdp_transop_get(self.h, nat.ptr(mu)))
        return forward.finish(mu.reshape(self.shape), n_done.value, delta.value, tol, self.mean_cost)

    def set_long_rows(self, min_entries):
        """Which rows a push gives to a whole wave instead of one lane: those of `min_entries` entries or more (the
        build sets 8; 0: every row to one lane).  A tuning and measuring knob (tools/forward_times.py): both paths add a
        row's products in entry order, so no result depends on it."""
        nat.check(nat.lib().sdp_transop_set_long_rows(self._handle(), int(min_entries)))
        self.info['long_rows_from'] = int(min_entries)

    def tocsr(self):
        """(indptr int64 [S + 1], indices int32 [nnz], data [nnz]) of P^T, e.g. for scipy.sparse.csr_matrix"""
        indptr = np.empty(self.S + 1, dtype=np.int64)
        indices = np.empty(self.nnz, dtype=np.int32)
        data = np.empty(self.nnz, dtype=self.dtype)
        nat.check(nat.lib().sdp_transop_get_csr(self._handle(), nat.ptr(indptr), nat.ptr(indices), nat.ptr(data)))
        return indptr, indices, data


class HorizonOperator(object):
    """The transition operators of the steps of a horizon on the device (`DPSolver.horizon_operator`): step k is the
    operator of the policy slice of time index t0 + k, and `propagate` pushes state distributions through the chain
    mu_{k+1} = P_k^T mu_k.  `stodynprog_amd.forward` (`chain_entries`, `csr`, `propagate`) is the definition of every
    number it returns.  NOT in the reference API.

    shape     : the state grid's
    n_steps   : steps of the chain
    nnz       : entries of all steps, n_steps S W 2^d
    mean_cost : gbar of every step, shape (n_steps,) + shape
    path      : 'device' (the entries of all steps of a part from ONE launch of kernel sdp_transitions_h and one sort:
                a sdp_chainop handle per part) or 'host' (callables evaluated on the host step by step, a solo
                `TransitionOperator` per step: models the horizon kernels do not run)
    parts     : the runs of steps (first, count) that each are one device operator; the distribution is handed from
                part to part on the host, and no cut changes a bit"""

    # Steps per part.  None: as many as the library's limits allow (plan_parts); a test sets a small number to reach the
    # cut at a tiny size.
    part_steps = None
    MAX_ROWS = (1 << 31) - 1           # rows of one device operator: 32-bit row ids
    MAX_ENTRIES = (1 << 32) - 1        # .. and its entries: 32-bit entry positions
    MAX_BATCH = 65535                  # vectors of one device call (the grid's second dimension)

    @classmethod
    def plan_parts(cls, n_steps, S, nnz_step, part_steps=None):
        """the runs (first, count) a horizon of n_steps steps is cut into: `part_steps` steps each (the last one what is
        left), by default the most that keep a part within MAX_ROWS rows and MAX_ENTRIES entries"""
        run = min(cls.MAX_ROWS // int(S), cls.MAX_ENTRIES // int(nnz_step)) if part_steps is None else int(part_steps)
        if run < 1:
            raise ValueError('a part of a horizon holds at least one step: part_steps = {}, or one step of {} rows and {} '
                             'entries is beyond {} rows or {} entries'.format(part_steps, S, nnz_step, cls.MAX_ROWS,
                                                                            cls.MAX_ENTRIES))
        return [(k, min(run, int(n_steps) - k)) for k in range(0, int(n_steps), run)]

    def __init__(self, shape, dtype, n_steps, nnz_step, path, parts, handles, mean_cost, times):
        self.shape = tuple(shape)
        self.dtype = np.dtype(dtype)
        self.S = int(np.prod(self.shape))
        self.n_steps = int(n_steps)
        self.nnz_step = int(nnz_step)
        self.nnz = self.n_steps * self.nnz_step
        self.path = path
        self.parts = list(parts)
        self._h = list(handles)            # device: a sdp_chainop per part; host: a TransitionOperator per step
        self.mean_cost = mean_cost
        self.nbytes = self.n_steps * forward.operator_bytes(self.nnz_step, self.S, self.dtype.itemsize)
        self.info = dict(path=path, n_steps=self.n_steps, parts=len(self.parts), nnz=self.nnz, bytes=self.nbytes,
                         entries_ms=times[0], sort_ms=times[1])

    def close(self):
        handles, self._h = getattr(self, '_h', None) or [], []
        for h in handles:
            if self.path == 'device':
                nat.lib().sdp_chainop_destroy(h)
            else:
                h.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _handles(self):
        if not self._h:
            raise ValueError('the operator is closed')
        return self._h

    def vectors(self, mu0):
        """(mu0 as [B][S] in the operator's reals, whether it is a batch)"""
        return _horizon_vectors(mu0, self.shape, self.dtype)

    def propagate(self, mu0, J_fin=None):
        """mu0 -- shape `shape`, or (B,) + shape for a batch -- pushed through the chain: a `forward.Propagation` record
        with mu (n_steps + 1[, B]) + shape, step_cost (n_steps[, B]), terminal_cost = dot(mu[-1], J_fin) or 0,
        total_cost and mass.  The vectors stay on the device between the steps of a part."""
        handles = self._handles()
        cur, batch = self.vectors(mu0)
        B = cur.shape[0]
        if J_fin is not None and np.shape(J_fin) != self.shape:
            raise ValueError('J_fin must have the shape of the grid, {}, not {}'.format(self.shape, np.shape(J_fin)))
        mu = np.empty((self.n_steps + 1, B, self.S), dtype=self.dtype)
        mu[0] = cur
        push_ms = 0.0
        if self.path == 'device':
            for h, (first, count) in zip(handles, self.parts):
                for b0 in range(0, B, self.MAX_BATCH):
                    b1 = min(B, b0 + self.MAX_BATCH)
                    start = np.ascontiguousarray(mu[first, b0:b1])
                    out = np.empty((count + 1, b1 - b0, self.S), dtype=self.dtype)
                    nat.check(nat.lib().sdp_chainop_propagate(h, b1 - b0, nat.ptr(start), nat.ptr(out)))
                    mu[first + 1:first + count + 1, b0:b1] = out[1:]
                    push_ms += _chainop_times(h)[2]
        else:
            for k, op in enumerate(handles):
                for b in range(B):
                    mu[k + 1, b] = op.push(mu[k, b], 1).reshape(-1)
                    push_ms += op.info['push_ms']
        self.info['push_ms'] = push_ms
        mu = mu.reshape((self.n_steps + 1, B) + self.shape)
        return forward.finish_chain(mu if batch else mu[:, 0], self.mean_cost, J_fin, batch)

    def tocsr(self, k):
        """(indptr int64 [S + 1], indices int32, data) of step k's P^T: what `transition_operator(pol_k, t0 + k).tocsr()`
        gives"""
        k = int(k)
        if not 0 <= k < self.n_steps:
            raise ValueError('step {} outside [0, {})'.format(k, self.n_steps))
        handles = self._handles()
        if self.path != 'device':
            return handles[k].tocsr()
        for h, (first, count) in zip(handles, self.parts):
            if first <= k < first + count:
                indptr = np.empty(self.S + 1, dtype=np.int64)
                indices = np.empty(self.nnz_step, dtype=np.int32)
                data = np.empty(self.nnz_step, dtype=self.dtype)
                nat.check(nat.lib().sdp_chainop_get_csr(h, k - first, nat.ptr(indptr), nat.ptr(indices), nat.ptr(data)))
                return indptr, indices, data


def _horizon_vectors(mu0, shape, dtype):
    """mu0 of shape `shape` or (B,) + shape as ([B][S] in `dtype`, whether it is a batch); a ValueError names the shapes"""
    mu0 = np.asarray(mu0)
    shape = tuple(shape)
    if mu0.shape == shape:
        return np.ascontiguousarray(mu0, dtype=dtype).reshape(1, -1), False
    if mu0.ndim == len(shape) + 1 and mu0.shape[1:] == shape and mu0.shape[0] >= 1:
        return np.ascontiguousarray(mu0, dtype=dtype).reshape(mu0.shape[0], -1), True
    raise ValueError('mu0 must have shape {} (one distribution) or (B,) + {} (a batch), not {}'.format(shape, shape, mu0.shape))


def _chainop_times(h):
    entries_ms, sort_ms, push_ms = C.c_double(0.0), C.c_double(0.0), C.c_double(0.0)
    nat.check(nat.lib().sdp_chainop_times(h, C.byref(entries_ms), C.byref(sort_ms), C.byref(push_ms)))
    return entries_ms.value, sort_ms.value, push_ms.value


class DPSolver(object):
    # Diagnostic / A-B switches of the generated kernels (codegen.DEBUG_NAMES): None in the product.
    # Tests and tools/ set a dict here (on an instance, or on the class for a block of solvers);
    # nothing is ever read from the environment.  A radius scale below 1, say, voids the
    # bit-identity guarantee -- which is why it takes an explicit assignment to get one.
    debug_defines = None
    # value_iteration with host arrays in and out on one GPU (sdp_problem_backup_host): True sends the finished
    # rows of a phase to the host under the next phase's kernel (grids of 8 MiB and more), False runs one launch
    # and then the downloads.  Same arrays either way.
    host_overlap = True
    # a control_box callback that cannot be traced (its table is made by scalar calls at every node, like the reference's):
    # 'sample' re-checks the cached table at 24 nodes per call, 'every node' rebuilds it on every call (stodynprog.py:440)
    box_recheck = 'sample'
    # dyn, cost and control_box are traced again on a call only when their fingerprint changed (trace.callable_fingerprint:
    # code, defaults, closure cells and the globals they name, by value; callables that have none are traced on every call);
    # False: trace on every call, as rounds 1-5 did
    trace_cache = True
    # monte_carlo: a run of n_steps is cut into kernel launches of at most this many steps (the state stays on the
    # device between them; the draws are keyed by the absolute step, so the cut changes no bit).  The default is an
    # estimate (a few microseconds per step and lane): no launch has been timed yet.
    steps_per_launch = 1024
    # .. and the host loop of untraceable models draws and keeps this many steps at a time
    MC_HOST_BLOCK = 64
    # simulate / monte_carlo under a time-indexed policy: the policy goes to the device in chunks of whole steps of at
    # most this many bytes (a step larger than that is a chunk of its own; the state stays on the device between the
    # chunks, so the cut changes no bit)
    horizon_chunk_bytes = 256 << 20
    # transition_operator: the most bytes an operator may take on the device (values, sources and row pointers,
    # forward.operator_bytes; the build needs about three times that for a moment).  A cap, not a tuning knob: beyond
    # it the call raises before anything is allocated
    TRANSITION_MAX_BYTES = 2 << 30
    _debug_after_create = None
    STAGED_MIN_NODES = 32768          # 'auto': grids of at most this many nodes run the direct kernel, not the staged tiles (see _kernel_plan_now);
    STAGED_MIN_WORK = 1024            #         up to 4 x as many where a node has this many control x perturbation points or more
    PERCONTROL_MIN_NODES = 32768      # 'auto': .. and grids of fewer nodes than this the direct kernel rather than a table per control
    LINE_MIN_CELLS = 1 << 20          # 'auto': one state variable, x' = a(x, u) +- b(w): the filtered line kernel from this many lattice cells per sweep

    def __init__(self, sys, dtype=np.float64, comm=None):
        """Dynamic Programming solver for stochastic dynamic control of `sys`
        (a `SysDescription`).  Implements value iteration, policy evaluation,
        policy iteration and finite-horizon Bellman recursion on an AMD GPU.

        New (optional) arguments, absent from the reference:
        dtype : arithmetic type of the sweep, float64 (default) or float32
        comm  : a `stodynprog_amd.dist.Communicator` to shard the outer state
                axis over several GPUs (one process per GPU)
        """
        self.sys = sys
        self.state_grid = [[0.] for s in self.sys.state]
        self.perturb_grid = [[0.] for p in self.sys.perturb]
        self.perturb_proba = [[1.] for p in self.sys.perturb]
        self.control_steps = (1.,) * len(self.sys.control)
        self.dtype = np.dtype(dtype)
        self.comm = comm
        # 'auto': column kernel for storage-separable models whose table fits LDS, else the
        # LDS-staged tile kernel; 'column' / 'staged' / 'generic' (one global load per
        # vertex, the first kernel) force a family.  All give the same bits.
        self.kernel = 'auto'
        self.comm_phases = 4               # multi-GPU: phases per backup (comm/compute overlap)
        # multi-GPU: how the J rows of a phase reach the other ranks -- 'rccl': in-place all-gather;
        # 'peer': every rank writes its rows straight into the others' buffers (HIP IPC mappings,
        # device-to-device copies over xGMI, no compute units); 'direct': the backup kernel itself
        # stores every J it computes into the buffers of the ranks that read it (xGMI stores spread
        # over the whole sweep: one launch and one rendezvous per backup, nothing left to copy).
        # Both fall back to 'rccl' when the buffers cannot be mapped (backend_info['exchange'] tells
        # which one runs)
        self.comm_exchange = 'rccl'
        self.comm_taper = False            # multi-GPU: shrinking phases (smallest gather exposed)
        # 'peer' / 'direct' exchange only: every rank owns one slab of columns and is sent only the rows
        # of J its own backups read (computed from the model: the cells its trailing next states fall
        # in) -- for a contracting exogenous process a fraction of the array.  J is completed on every
        # rank when the host asks for it.  Full-table column kernels (all filter forms), stationary systems.
        self.comm_sparse = False
        # (every kernel performs the reference's floating-point operations in the reference's order; the opt-in
        # 'fused' arithmetic of rounds 1-5 -- J within ~1e-15, 6.6 ms per benchmark sweep -- went in round 6, when the
        # exact kernel with the certified filter ran the same sweep in 1.05 ms)
        # column kernel: decide all but the near-minimal controls of a node on
        # a table reduced over the perturbation (rigorous error radius) and evaluate only the
        # survivors with the reference's operations -- same bits, ~W times less work per control
        # (csrc/sdp_colfilter_kernel.h, SdpColFilter).  False: every control the long way.
        self.certified_filter = True
        self._cache = {}
        self._idx_cache = None             # see last_policy_index
        self._idx_source = None
        self.backend_info = {}
        # what the last value_iterations / eval_policy / policy_iteration call made with `tol` did
        # (convergence.SweepConvergence / PolicyIterationConvergence); None after a call without `tol`
        self.last_convergence = None

    @property
    def last_policy_index(self):
        """flat C-order index into the control lattice of the optimal control of every
        node, from the last sweep (int32, shape of the state grid).  After a
        value_iteration call the indices stay on the device and are fetched on first
        access (the reference returns control VALUES only, stodynprog.py:530-533)."""
        if self._idx_cache is None and self._idx_source is not None:
            prob, self._idx_source = self._idx_source, None
            if prob.h:
                self._idx_cache = prob.get_index()
        return self._idx_cache

    @last_policy_index.setter
    def last_policy_index(self, value):
        self._idx_cache, self._idx_source = value, None

    # ------------------------------------------------------------------ grids
    def discretize_perturb(self, *linspace_args):
        """create a regular discrete grid for each perturbation variable;
        grids go to `self.perturb_grid` (may also be set manually), the
        probability weights to `self.perturb_proba` (reference sdp.py:335-362)."""
        assert len(linspace_args) == len(self.sys.perturb) * 3
        self.perturb_grid = []
        self.perturb_proba = []
        for i in range(len(self.sys.perturb)):
            grid_wi = np.linspace(*linspace_args[i * 3:i * 3 + 3])
            law = self.sys.perturb_laws[i]
            if self.sys.perturb_types[i] == 'continuous':
                proba_wi = law.pdf(grid_wi)
                proba_wi /= proba_wi.sum()
            else:
                proba_wi = law.pmf(grid_wi)
                assert np.allclose(proba_wi.sum(), 1.)
            self.perturb_grid.append(grid_wi)
            self.perturb_proba.append(proba_wi)
        return self.perturb_grid, self.perturb_proba

    def discretize_state(self, *linspace_args):
        """create a regular discrete grid for each state variable, stored in
        `self.state_grid` (reference sdp.py:364-389)."""
        assert len(linspace_args) == len(self.sys.state) * 3
        self.state_grid = [np.linspace(*linspace_args[i * 3:i * 3 + 3])
                           for i in range(len(self.sys.state))]
        shape = tuple(len(g) for g in self.state_grid)
        self._state_grid_shape = shape
        # reference state of the relative DP algorithm: the middle of the grid
        self._state_ref_ind = tuple(n // 2 for n in shape)
        self._state_ref = tuple(g[i] for g, i in zip(self.state_grid, self._state_ref_ind))
        return self.state_grid

    @property
    def state_grid_full(self):
        """broadcasted state grid (self.state_grid is flat)"""
        d = len(self.state_grid)
        parts = []
        for i, g in enumerate(self.state_grid):
            shape = [1] * d
            shape[i] = -1
            parts.append(np.asarray(g).reshape(shape))
        return np.broadcast_arrays(*parts)

    def interp_on_state(self, A):
        """returns an interpolating function of array A, assumed to be given
        on the state grid (reference sdp.py:405-430)."""
        expect_shape = self._state_grid_shape
        if A.shape != expect_shape:
            raise ValueError('array `A` should be of shape {:s}, not {:s}'.format(
                str(expect_shape), str(A.shape)))
        if len(expect_shape) <= 5:
            A_interp = MlinInterpolator(*self.state_grid)
            A_interp.set_values(A)
            return A_interp
        raise NotImplementedError('interpolation for state dimension >5'
                                  ' is not implemented.')

    def _check_state_array(self, A):
        expect_shape = self._state_grid_shape
        if A.shape != expect_shape:
            raise ValueError('array `A` should be of shape {:s}, not {:s}'.format(
                str(expect_shape), str(A.shape)))

    def control_grids(self, state_k, t_k=None):
        """grid on the box of admissible controls at state `state_k`, using
        self.control_steps as hints (reference sdp.py:432-463).
        Returns (list of 1-D arrays, tuple of their lengths)."""
        if t_k is not None:
            state_k = (t_k,) + tuple(state_k)
        intervals = self.sys.control_box(*state_k, **self.sys.params)
        grids, dims = [], []
        for (u_min, u_max), step in zip(intervals, self.control_steps):
            n_interv = (u_max - u_min) / step
            if n_interv < 0.1:
                npts = 1
                u_grid = np.array([(u_min + u_max) / 2])
            else:
                npts = int(np.ceil(n_interv) + 1)
                u_grid = np.linspace(u_min, u_max, npts)
            grids.append(u_grid)
            dims.append(npts)
        return grids, tuple(dims)

    # ------------------------------------------------- host-side preparation
    def _shape(self):
        return tuple(len(g) for g in self.state_grid)

    def _trace_box_now(self, t_k=None):
        """The control_box callback traced for ONE call (trace.trace_box): a TracedBox whose whole-grid evaluation is,
        node for node, what the reference's scalar calls return (stodynprog.py:438-440) -- or a TraceError, and the
        table is then made by those scalar calls themselves.  Traced afresh on every call, like dyn and cost: data the
        callback reads (a rated power in a closure, a module-level capacity) are constants of the DAG, so data that
        changed show up as a changed signature.  A time index (t_k not None) is traced as a symbol, or failing that as
        the concrete step (`data[k]`)."""
        sd = self.sys
        nx, nu = len(sd.state), len(sd.control)
        try:
            tb = trace_box(sd.control_box, nx, nu, sd.params, stationnary=t_k is None)
        except TraceError as e:
            if t_k is None:
                return e
            try:
                tb = trace_box(sd.control_box, nx, nu, sd.params, stationnary=False, t_value=t_k)
            except TraceError:
                return e
        bad = tb.inexact_ops()
        if bad:
            return TraceError('control_box uses operations whose whole-grid evaluation need not repeat the scalar call '
                              'bit for bit: {}'.format(', '.join(bad)))
        return tb

    def _box_from_trace(self, tb, t_k=None):
        """(lo, hi) of shape (nu, S) -- (nu, 1) when the box ignores the state -- from a traced box, on the open grid"""
        shape = self._shape()
        d = len(shape)
        S = int(np.prod(shape))
        nu = len(self.sys.control)
        open_grid = [np.asarray(g, dtype=float).reshape((1,) * k + (-1,) + (1,) * (d - k - 1))
                     for k, g in enumerate(self.state_grid)]
        ends = tb.evaluate(open_grid, t_k)
        constant = all(np.ndim(a) == 0 and np.ndim(b) == 0 for a, b in ends)
        cols = 1 if constant else S
        lo_v = np.empty((nu, cols))
        hi_v = np.empty((nu, cols))
        for c, (a, b) in enumerate(ends):
            if constant:
                lo_v[c, 0], hi_v[c, 0] = a, b
            else:
                lo_v[c] = np.broadcast_to(a, shape).ravel()
                hi_v[c] = np.broadcast_to(b, shape).ravel()
        return lo_v, hi_v

    def _box_table(self, t_k=None, traced=None):
        """control_grids() for every node at once: (lo, hi, n) arrays of shape (nu, S) -- (nu, 1) when the box ignores
        the state -- with the same numpy operators as control_grids (sdp.py:432-463).

        The ends of the boxes come from the callback's TRACE evaluated on the whole grid (`_trace_box_now`): per node
        the same IEEE operations as the reference's scalar call, so the table is exact at every node by construction
        -- no sampling.  (As a check of the tracer itself the corners and the centre of the grid are compared with
        scalar calls whenever a table is built.)  A callback that cannot be traced is called node by node, as the
        reference does."""
        shape = self._shape()
        S = int(np.prod(shape))
        nu = len(self.sys.control)
        params = self.sys.params
        lead = () if t_k is None else (t_k,)
        tb = self._trace_box_now(t_k) if traced is None else traced
        self._box_mode = None           # how the table was made: 'traced', or None (node by node)
        self._box_sig = None
        lo = hi = None
        if not isinstance(tb, TraceError):
            lo, hi = self._box_from_trace(tb, t_k)
            anchors = sorted({int(np.ravel_multi_index(ind, shape))
                              for ind in itertools.product(*[(0, n - 1) for n in shape])} | {S // 2})
            for flat in anchors:
                ind = np.unravel_index(flat, shape)
                x = tuple(g[i] for g, i in zip(self.state_grid, ind))
                col = flat if lo.shape[1] > 1 else 0
                for c, (a, b) in enumerate(self.sys.control_box(*(lead + x), **params)):
                    if not (_same(lo[c, col], a) and _same(hi[c, col], b)):
                        raise AssertionError('the traced control_box differs from the callback at node {}: the callback is '
                                             'not a pure function of its arguments, or the tracer is wrong'.format(ind))
            self._box_mode = 'traced'
            self._box_sig = tb.signature()
        else:
            lo = np.empty((nu, S))
            hi = np.empty((nu, S))
            for flat, x in enumerate(itertools.product(*self.state_grid)):
                box = self.sys.control_box(*(lead + x), **params)
                for c, (a, b) in enumerate(box):
                    lo[c, flat] = a
                    hi[c, flat] = b
        return self._box_lattice(lo, hi)

    def _box_lattice(self, lo, hi):
        """(lo, hi, n) of the control lattice from the ends of the boxes, with control_grids' operators (sdp.py:446-453)"""
        nu = len(self.sys.control)
        n = np.empty(lo.shape, dtype=np.int32)
        with np.errstate(all='ignore'):
            for c in range(nu):
                step = self.control_steps[c]
                n_interv = (hi[c] - lo[c]) / step                   # sdp.py:446-447
                single = n_interv < 0.1                              # sdp.py:449
                npts = np.where(single, 1, np.ceil(np.where(single, 0., n_interv)) + 1)
                n[c] = npts.astype(np.int32)
                mid = (lo[c] + hi[c]) / 2                            # sdp.py:453
                lo[c] = np.where(single, mid, lo[c])
                hi[c] = np.where(single, mid, hi[c])
        return lo, hi, n

    def _fingerprint(self, t_k):
        s = self.sys
        # the callables themselves (hashed by identity and kept alive by the cache
        # key, so a recycled id() can never alias a stale entry)
        parts = [s.dyn, s.cost, s.control_box, _params_key(s.params),
                 tuple(float(x) for x in self.control_steps), str(self.dtype), t_k,
                 id(self.comm), self.comm_phases, self.comm_taper, self.comm_exchange,
                 getattr(self, 'comm_sparse', False), self.kernel,
                 getattr(self, 'certified_filter', True),
                 tuple(sorted((codegen.check_debug(self.debug_defines) or {}).items()))]
        for g in list(self.state_grid) + list(self.perturb_grid) + list(self.perturb_proba):
            parts.append(np.asarray(g, dtype=float).tobytes())
        # the tuple itself is the cache key (not its hash): the callables stay alive as
        # long as the entry does, so a recycled id() can never alias a stale entry
        return tuple(parts)

    def _traced(self):
        key = ('trace', self.sys.dyn, self.sys.cost, repr(sorted(self.sys.params.items())))
        if key not in self._cache:
            s = self.sys
            try:
                model = trace_model(s.dyn, s.cost, len(s.state), len(s.control),
                                    len(s.perturb), s.params, s.stationnary)
            except TraceError as e:
                model = e
            self._cache[key] = model
        return self._cache[key]

    def _trace_now(self, t_k=None):
        """Trace the callables for ONE call (value_iteration, a step of
        bellman_recursion, eval_policy).  Traced afresh every time, like the
        reference evaluates the callables at call time (stodynprog.py:674-676):
        module-level data they read may have changed since the last call.

        A time-dependent system whose callables need a concrete time index
        (`data[k]`) cannot be traced with a symbolic k; it is traced for the
        step `t_k` alone and the constants of the step are lifted into kernel
        parameters (trace.TracedModel.lift_constants), so the steps of a
        horizon share one code object.  Returns a TracedModel or a TraceError."""
        s = self.sys
        # (round 6: a callable whose FINGERPRINT -- code, defaults, closure cells and the globals it names, by value -- is
        # what it was at the last call traces to the same graph: the trace is kept.  No fingerprint (an object, a large
        # array, a module of the user's in sight): traced afresh, as before.  trace.callable_fingerprint)
        # A time-dependent system traced with a SYMBOLIC time index gives the same graph at every step: one kept trace
        # serves the whole horizon.  A trace for one concrete step (t_value) is not kept, nor is the failure of one: the
        # next step may trace where this one did not.
        fp = callable_fingerprint(s.dyn, s.cost, s.params) if self.trace_cache else None
        key = ('trace now', s.stationnary)
        if fp is not None:
            kept = self._cache.get(key)
            if kept is not None and kept[0] == fp:
                return kept[1]
        model = self._trace_now_uncached(t_k)
        if fp is not None and (s.stationnary or (not isinstance(model, TraceError) and model.t_value is None)):
            self._cache[key] = (fp, model)
        return model

    def _trace_now_uncached(self, t_k=None):
        s = self.sys
        try:
            model = trace_model(s.dyn, s.cost, len(s.state), len(s.control), len(s.perturb),
                                s.params, s.stationnary)
            # Constants stay literals in the generated source (the compiler folds
            # them) until the SAME expression structure shows up with other values
            # -- a parameter study looping over a cost coefficient, say; from then on
            # they are lifted too, so the study compiles at most two code objects.
            key = ('struct', model.structure_key())
            bits = np.asarray(model.param_values(), dtype=float).tobytes()
            seen = self._cache.setdefault(key, dict(bits=bits, lifted=False))
            if not seen['lifted'] and seen['bits'] != bits:
                seen['lifted'] = True
            if seen['lifted']:
                model.lift_constants()
            return model
        except TraceError as e:
            if s.stationnary or t_k is None:
                return e
            try:
                model = trace_model(s.dyn, s.cost, len(s.state), len(s.control),
                                    len(s.perturb), s.params, s.stationnary, t_value=int(t_k))
            except TraceError:
                return e
            model.lift_constants()
            return model

    def _check_supported(self):
        m = len(self.perturb_grid)
        if m > perturb.MAX_PERTURB:
            raise NotImplementedError('{} perturbation variables: at most {} are supported (the reference stops at '
                                      'one, sdp.py:664-666)'.format(m, perturb.MAX_PERTURB))
        if m > 1 and self.comm is not None:
            raise NotImplementedError('several perturbation variables run on one GPU (no communicator)')
        d = len(self.state_grid)
        if d > 5:
            raise NotImplementedError('interpolation for state dimension >5'
                                      ' is not implemented.')
        if d > 4:
            raise Exception("Can't interpolate in dimension strictly greater than 5")

    def _box_plan(self, box_t=None):
        """Control-box table of the current discretisation, cached.

        The reference calls control_box at every node of every sweep (stodynprog.py:440), so data the callback reads (a
        rated power in a closure, a module-level capacity) may change between two calls.  The callback is therefore
        TRACED AGAIN on every call -- as dyn and cost are --: what it reads are constants of its DAG, and the cached
        table stays exactly as long as the new trace has the structure and the constants of the one the table was made
        from (`TracedBox.signature`): a proof for every node, not a probe of some.  Only a callback that cannot be traced
        (its table was made by scalar calls at every node) is re-checked by scalar calls at `n_probe` nodes -- the
        corners, the centre and a different sample every time -- which is all a cached table of an opaque callable can
        offer; `DPSolver.box_recheck = 'every node'` rebuilds such a table on every call instead, as the reference does."""
        key = ('box', self._fingerprint(box_t))
        bp = self._cache.get(key)
        # (a callback whose fingerprint is what it was when the table was made would trace to the same graph: no trace)
        fp = callable_fingerprint(self.sys.control_box, self.sys.params) if self.trace_cache else None
        if bp is not None and fp is not None and bp.get('fp') == fp and bp.get('sig') is not None:
            return bp
        tb = self._trace_box_now(box_t)
        if bp is not None:
            if not isinstance(tb, TraceError):
                if bp.get('sig') != tb.signature():
                    bp = None                   # the callback reads data that changed (or is no longer what it was): rebuild
                else:
                    bp['fp'] = fp               # (the same graph under another fingerprint: data it does not depend on)
            elif bp.get('sig') is not None or self.box_recheck == 'every node' or not self._box_still_valid(bp, box_t):
                bp = None
        if bp is None:
            lo, hi, n = self._box_table(box_t, traced=tb)
            per_node = not (np.all(lo == lo[:, :1]) and np.all(hi == hi[:, :1])
                            and np.all(n == n[:, :1]))
            max_u = int(np.prod(n.astype(np.int64), axis=0).max())
            if max_u >= 2 ** 31:
                raise ValueError('control lattice too large')
            if not per_node:
                lo, hi, n = lo[:, :1], hi[:, :1], n[:, :1]
            lo, hi, n = (np.ascontiguousarray(a) for a in (lo, hi, n))
            digest = hash((lo.tobytes(), hi.tobytes(), n.tobytes()))
            bp = dict(lo=lo, hi=hi, n=n, per_node=per_node, max_u=max_u,
                      lanes=codegen.lanes_for(max_u), digest=digest, mode=getattr(self, '_box_mode', None),
                      sig=getattr(self, '_box_sig', None), fp=fp)
            if box_t is not None:           # one table per time step: keep only the latest
                for k in [k for k in self._cache if k[0] == 'box']:
                    del self._cache[k]
            self._cache[key] = bp
        return bp

    def _box_still_valid(self, bp, box_t, n_probe=21):
        """A table made by scalar calls at every node (the callback could not be traced): the callback again at
        `n_probe` nodes plus the corners and the centre, compared with the table; any difference rebuilds it."""
        shape = self._shape()
        S = int(np.prod(shape))
        lo, hi, n = bp['lo'], bp['hi'], bp['n']
        self._box_probe_round = getattr(self, '_box_probe_round', 0) + 1
        rng = np.random.default_rng(self._box_probe_round)
        probe = set(rng.integers(0, S, size=min(S, n_probe)).tolist())
        probe.update([0, S - 1, S // 2])
        lead = () if box_t is None else (box_t,)
        try:
            for flat in probe:
                ind = np.unravel_index(flat, shape)
                x = tuple(g[i] for g, i in zip(self.state_grid, ind))
                box = self.sys.control_box(*(lead + x), **self.sys.params)
                col = flat if bp['per_node'] else 0
                for c, (a, b) in enumerate(box):
                    a, b = float(a), float(b)
                    with np.errstate(all='ignore'):
                        n_interv = (b - a) / self.control_steps[c]
                    if n_interv < 0.1:
                        a = b = (a + b) / 2
                        npts = 1
                    else:
                        npts = int(np.ceil(n_interv) + 1)
                    if not (_same(lo[c, col], a) and _same(hi[c, col], b) and n[c, col] == npts):
                        return False
        except Exception:
            return False
        return True

    def _kernel_plan(self, box_t=None, model=None):
        """Everything that determines the model code object of the current
        discretisation (no GPU needed): control-box table, lanes per node,
        kernel family, generated source.  `model`: the trace to plan for
        (default: the cached symbolic trace of `_traced`)."""
        if model is None:
            model = self._traced()
        if isinstance(model, TraceError):
            raise model
        shape = self._shape()
        dt = self.dtype
        bp = self._box_plan(box_t)
        lanes = bp['lanes']
        debug = codegen.check_debug(self.debug_defines)
        W = self._law_points()
        # The callables are traced afresh on every call (_trace_now), but a trace with the structure and the constants
        # of the last one plans -- and generates -- the same unit: the plan is kept (the source text of a call was a
        # fifth of a millisecond, as much as the kernels of the reference's own problem sizes).
        # (a trace that was kept -- trace_cache -- keeps what it contributes to the key, too)
        mk = getattr(model, '_plan_key', None)
        if mk is None or mk[0] != (model.param_index is not None):
            mk = (model.param_index is not None, model.structure_key(), np.asarray(model.param_values(), dtype=float).tobytes())
            try:
                model._plan_key = mk
            except AttributeError:
                pass
        memo = ('plan', self._fingerprint(None), bp['digest'], None if box_t is None else float(box_t),
                mk[1], mk[2], model.param_index is not None, model.t_value, bool(self._cache.get('no_lead')))
        kept = self._cache.get(memo)
        if kept is not None:
            return dict(kept, model=model)
        plan = self._kernel_plan_now(box_t, model, bp, lanes, debug, W)
        plan['_memo'] = memo
        for k in [k for k in self._cache if k[0] == 'plan' and k[1:4] != memo[1:4]]:
            del self._cache[k]                  # (another discretisation / box table: its plans are never asked for again)
        self._cache[memo] = plan
        return plan

    def _plans_direct_exchange(self):
        """whether _problem may turn the direct exchange on (the kernels then store J into the other ranks): only
        such a unit carries the peer stores"""
        return bool(self.comm is not None and self.comm.is_device and 1 < self.comm.nranks <= 8
                    and self.comm_exchange == 'direct')

    def _kernel_plan_now(self, box_t, model, bp, lanes, debug, W):
        shape = self._shape()
        dt = self.dtype
        # storage-separable models on a grid whose (W x N0) table fits the LDS of
        # a CU run the column kernels, with per-node arrays stored axis-0-fastest
        if self.kernel not in ('auto', 'generic', 'column', 'staged', 'lead', 'line'):
            raise ValueError("kernel must be 'auto', 'column', 'lead', 'line', 'staged' or 'generic'")
        if model.n_perturb >= 2:
            return self._multiw_plan(model, bp, lanes, debug, W)
        certified = getattr(self, 'certified_filter', True)
        col_family = self.kernel in ('auto', 'column')
        S_nodes = int(np.prod(shape))
        # A lattice that changes with the time index gets a control table with room to spare (a capacity, checked by
        # the library as controls <= capacity), so that the steps of a horizon keep sharing one code object.
        n_controls = bp['max_u'] if box_t is None else 1 << max(int(bp['max_u']) - 1, 0).bit_length()
        col_args = (model, dt, shape, W, n_controls)
        # the column family, first form: the table of a column fits the LDS of a CU (codegen.column_table_unit)
        unit = None
        if col_family and model.storage_separable:
            unit = codegen.column_table_unit(*col_args, box=bp, axis=self.state_grid[0], certified_filter=certified, debug=debug)
        # several controlled state variables next to an exogenous process: the node-order sweep with the
        # certified filter on an array reduced over w (csrc/sdp_lead_kernel.h); one GPU for now
        # (one stock whose table does not fit LDS too: measured 5.9 ms against 12.7 ms of the row-window
        # column kernel at 1024 x 128 x 128 x 64 x 32, tools/window_vs_lead.py)
        lead_axes, lead_perm = 0, None
        if (unit is None and self.kernel in ('auto', 'lead') and W > 0 and not self._cache.get('no_lead')
                and (self.comm is None or self.comm.is_device) and certified):
            lead_axes = codegen.lead_filter_applies(
                model, dt, 1 if (self.kernel == 'lead' or model.storage_separable) else 2, debug)
            # the stocks need not be listed first (the order of the state variables is the user's, reference
            # stodynprog.py:119-131): the filter then works on a permuted view of the axes, the second pass keeps the
            # reference's own axis order
            if not lead_axes:
                lead_axes, lead_perm = codegen.lead_order(model, dt, debug) or (0, None)
        if self.kernel == 'lead' and not lead_axes:
            raise ValueError("kernel = 'lead' needs controlled state variables next to an exogenous process, "
                             'a perturbation that reaches only that process, 8-byte reals and the certified '
                             'filter (several GPUs: a device communicator)')
        if lead_axes:
            lanes = 1                                     # one lane per node, the control loop in-lane
        # second form: a table per control, provided the nodes of a column share their control values (box independent
        # of x0) -- codegen.column_percontrol_unit
        # (on a grid of fewer than PERCONTROL_MIN_NODES nodes the direct kernel is faster than a table per control: 16^3
        # 0.160 / 0.036 ms, 24^3 0.224 / 0.101 ms, 32^3 0.242 / 0.251 ms, 48^3 0.46 / 0.95 ms -- round 5)
        if (unit is None and not lead_axes and col_family
                and (self.kernel == 'column' or S_nodes >= self.PERCONTROL_MIN_NODES)
                and self._box_constant_along_axis0(bp, shape)):
            unit = codegen.column_percontrol_unit(*col_args, debug=debug)
        # third form: the W x N0 table exceeds the LDS of a CU -- a window of rows per segment of the column
        if unit is None and not lead_axes and col_family and model.storage_separable:
            unit = codegen.column_window_unit(*col_args, reach_rows=self._lead_reach_rows(model, bp, box_t), debug=debug)
        column = unit is not None
        per_control = column and unit.form == 'table per control'
        if (not column or per_control) and not lead_perm and self.kernel in ('auto', 'column'):
            k = model.separable_axis_hint()
            if k is not None and not self._cache.get('hinted'):
                self._cache['hinted'] = True
                import warnings
                warnings.warn('state variable "{}" is the only one driven by the control: listing it '
                              'FIRST in dyn/cost/control_box (and in discretize_state) lets the fast '
                              'column kernel run this model'.format(self.sys.state[k]))
        if self.kernel == 'column' and not column:
            raise ValueError('the column kernel needs a storage-separable model whose '
                             'table fits in LDS')
        staged = None
        # The staged kernel gives a node to a thread, the direct one to `lanes` of them: below ~1e5 nodes the staged tiles
        # do not fill the chip and the value array sits in the caches anyway.  Measured in round 5 (staged / direct):
        # 1-D inventory 600 nodes x 257 controls x 16 w 0.95 / 0.023 ms, 4096 x 1025 x 32 6.9 / 0.23 ms, 65 536 x 1025 x 16
        # 7.8 / 3.3 ms, 262 144 x 257 x 16 5.0 / 4.2 ms; control-coupled 3-D 16^3 0.85 / 0.037 ms, 32^3 0.87 / 0.25 ms,
        # 40^3 0.88 / 0.46 ms, 48^3 0.92 / 0.88 ms, 64^3 1.42 / 2.05 ms; coupled 2-D, 65 controls x 9 w: 128^2 0.196 / 0.069 ms,
        # 256^2 0.218 / 0.288 ms, 512^2 0.34 / 1.26 ms; the same with 1025 controls: 256^2 3.04 / 1.46 ms, 512^2 4.5 / 5.9 ms.
        # So the direct kernel for one state variable, for grids of at most STAGED_MIN_NODES nodes, and up to four times
        # that where a node has STAGED_MIN_WORK control x perturbation points or more (few threads with long loops).
        small = (len(shape) == 1 or S_nodes <= self.STAGED_MIN_NODES
                 or (S_nodes <= 4 * self.STAGED_MIN_NODES and bp['max_u'] * max(W, 1) >= self.STAGED_MIN_WORK))
        if not column and not lead_axes and (self.kernel == 'staged' or (self.kernel == 'auto' and not small)):
            key = ('staged', model.structure_key(), bp['digest'], str(dt), shape, W, _dbg_key(debug))
            staged = self._cache.get(key)
            if staged is None:
                staged = codegen.staged_config(model, self.state_grid, self.perturb_grid, bp, dt,
                                               0.0 if box_t is None else float(box_t), debug=debug)
                self._cache[key] = staged
        # ONE state variable with the perturbation in its sums (`x + u - w`): the certified filter on the shifted lattice with
        # the value array itself as the table (csrc/sdp_line_kernel.h; one GPU).  Two launches per sweep, so only where
        # there is work to save: LINE_MIN_CELLS lattice cells per sweep (below that the direct kernel takes microseconds).
        line = 0
        if (len(shape) == 1 and self.kernel in ('auto', 'line') and self.comm is None and W > 0 and staged is None
                and certified and box_t is None
                and model.t_value is None and model.param_index is None
                and (self.kernel == 'line' or S_nodes * int(bp['max_u']) * W >= self.LINE_MIN_CELLS)
                and codegen.line_filter_applies(model, dt, W, debug)):
            line = W
            # lanes = slices of the control lattice per wave (csrc/sdp_line_kernel.h: a workgroup's four waves share a tile of
            # 64 / lanes consecutive nodes): enough of them to fill the chip (8192 waves), at least 8 controls per slice,
            # and a tile's (node, perturbation point) items within the kernel's LDS table of terms (2048)
            pow2 = lambda v: 1 << max(int(np.ceil(np.log2(max(v, 1)))), 0)
            need = pow2(W * 64 / 2048.)
            want = min(pow2(131072. / S_nodes), max(1 << int(np.floor(np.log2(max(bp['max_u'] / 32., 1)))), 1))
            lanes = int(min(64, max(need, want)))
        if self.kernel == 'line' and not line:
            raise ValueError("kernel = 'line' needs one state variable whose perturbation enters x' through final sums "
                             "(x + u - w), a cost that does not see it, 8-byte reals, a stationary system, the certified "
                             'filter, one GPU')
        # (what the unit holds beside the direct kernels: codegen.translation_unit)
        family = unit or staged or line or ((lead_axes, lead_perm) if lead_axes else None)
        source = codegen.translation_unit(model, dt, lanes, family, debug=debug, peer_stores=self._plans_direct_exchange())
        window = (unit.threads, unit.lds_bytes, unit.window_rows, unit.seg_nodes) if column and unit.form == 'row window' else None
        return dict(model=model, source=source, column=column, unit=unit, lanes=lanes, staged=staged,
                    filtered=bool((column and unit.filtered) or lead_axes or line),
                    lead_axes=lead_axes, lead_perm=lead_perm, line=bool(line),
                    window=window, per_control=per_control, col_seg_nodes=unit.seg_nodes if column else 0,
                    per_node=bp['per_node'], lo=bp['lo'], hi=bp['hi'], n=bp['n'],
                    max_u=bp['max_u'], W=W, box_digest=bp['digest'], box_mode=bp.get('mode'))

    def _multiw_plan(self, model, bp, lanes, debug, W):
        """the plan of a system with SEVERAL perturbation variables: the node-order kernels of
        csrc/sdp_multiw_kernel.h on the flat law of `perturb.product_law`, planned before any other family (the fast
        families -- column, lead, line, staged -- take one variable)"""
        self._check_supported()
        if self.kernel not in ('auto', 'generic'):
            raise ValueError("kernel = '{}' takes one perturbation variable: a system of {} runs the direct node-order "
                             "kernel (kernel = 'auto' or 'generic')".format(self.kernel, model.n_perturb))
        source = codegen.translation_unit(model, self.dtype, lanes, None, debug=debug)
        return dict(model=model, source=source, column=False, unit=None, lanes=lanes, staged=None, filtered=False,
                    lead_axes=0, lead_perm=None, line=False, window=None, per_control=False, col_seg_nodes=0,
                    per_node=bp['per_node'], lo=bp['lo'], hi=bp['hi'], n=bp['n'],
                    max_u=bp['max_u'], W=W, box_digest=bp['digest'], box_mode=bp.get('mode'))

    def _law_points(self):
        """points of the (flat) perturbation law: W_1 .. W_m; 0 for a deterministic system"""
        return int(np.prod([len(g) for g in self.perturb_grid], dtype=np.int64)) if self.perturb_grid else 0

    def _flat_law(self):
        """The law the backups sum over, as the callables see it: (one array of W values per perturbation variable,
        float64 probabilities [W] or None, W).  One variable: its grid and weights as they are; several: the flat
        product law of `perturb.product_law` (C order, last variable fastest)."""
        if not self.perturb_grid:
            return (), None, 0
        if len(self.perturb_grid) == 1:
            return (tuple(self.perturb_grid), np.ascontiguousarray(self.perturb_proba[0], dtype=float),
                    len(self.perturb_grid[0]))
        wtab, P = perturb.product_law(self.perturb_grid, self.perturb_proba)
        return tuple(wtab), P, int(P.size)

    @staticmethod
    def _box_constant_along_axis0(bp, shape):
        """do all nodes of every column along axis 0 have the same control box?"""
        if not bp['per_node']:
            return True
        n0 = shape[0]
        for arr in (bp['lo'], bp['hi'], bp['n']):
            a = arr.reshape(arr.shape[0], n0, -1)
            if not (a == a[:, :1, :]).all():
                return False
        return True

    def _lead_reach_rows(self, model, bp, box_t=None, n_samples=4096, around=False):
        """Rows of axis 0 the controls (and perturbation points) of ONE node span:
        max over sampled nodes of the distance, in grid rows, between the next
        values of the leading state variable at the ends of the node's control
        lattice -- the same prediction the windowed column kernel makes per unit."""
        from .trace import evaluate
        shape = self._shape()
        S = int(np.prod(shape))
        rng = np.random.default_rng(7)
        flat = np.unique(np.concatenate([rng.integers(0, S, size=min(S, n_samples)), [0, S - 1]]))
        idx = np.unravel_index(flat, shape)
        x = [np.asarray(g, dtype=float)[i] for g, i in zip(self.state_grid, idx)]
        col = flat if bp['per_node'] else np.zeros_like(flat)
        nu = len(self.sys.control)
        ends = []
        for first in (True, False):
            ends.append([bp['lo'][c, col] if first else bp['hi'][c, col] for c in range(nu)])
        wg = np.asarray(self.perturb_grid[0], dtype=float) if (self.perturb_grid and model.n_perturb) else None
        ws = [None] if wg is None else ([wg[0], wg[-1]] if model.lead_depends_on_w else [wg[0]])
        g0 = np.asarray(self.state_grid[0], dtype=float)
        rows = []
        for u in ends:
            for w in ws:
                with np.errstate(all='ignore'):
                    xn, _ = evaluate(model, x, u, [] if w is None else [w],
                                     0.0 if box_t is None else float(box_t))
                p = (np.asarray(xn[0], dtype=float) - g0[0]) / (g0[-1] - g0[0]) * (len(g0) - 1)
                rows.append(np.clip(np.nan_to_num(p, nan=0.0, posinf=1e9, neginf=-1e9), 0, len(g0) - 2))
        rows = np.array([np.broadcast_to(r, flat.shape) for r in rows])
        if around:          # farthest row from the node's own, either side
            return int(np.ceil(np.abs(rows - idx[0][None, :]).max())) + 1
        return int(np.ceil((rows.max(axis=0) - rows.min(axis=0)).max())) + 1

    def _problem(self, t_k=None, model=None):
        """Device problem for the current discretisation and callables.  The
        handle is reused from call to call (and from time step to time step)
        as long as the generated source and the control-box table are the
        same; lifted constants are re-sent on every call."""
        self._check_supported()
        box_t = None if self.sys.stationnary else t_k
        if model is None:
            model = self._trace_now(t_k)
        if isinstance(model, TraceError):
            raise model
        plan = self._kernel_plan(box_t, model)
        # (the key of the unit's source: a hash of the text and of the kernel headers -- once per plan, not per call)
        skey = plan.get('_source_key')
        if skey is None:
            skey = codegen.source_key(plan['source'])
            kept_plan = self._cache.get(plan.get('_memo'))
            if kept_plan is not None:
                kept_plan['_source_key'] = skey
        fp = ('problem', self._fingerprint(None), plan['box_digest'], skey)
        prob = self._cache.get(fp)
        if prob is None:
            try:
                prob = self._create_problem(fp, plan)
            except MemoryError:
                # the reduced-array sweep keeps two more arrays of the size of the grid (the reduced array and a
                # plane-major copy of the cost-to-go): where they no longer fit, the families that need no extra
                # memory take over (row window / table per control / staged tiles) -- slower, same bits
                if not plan.get('lead_axes') or self.kernel == 'lead':
                    raise
                import warnings
                warnings.warn('not enough device memory for the reduced-array sweep (2 extra arrays of the grid\'s '
                              'size): using the kernels that need none')
                self._cache['no_lead'] = True
                plan = self._kernel_plan(box_t, model)
                fp = ('problem', self._fingerprint(None), plan['box_digest'], codegen.source_key(plan['source']))
                prob = self._create_problem(fp, plan)
        if model.param_index is not None:
            prob.set_params(model.param_values())
            if prob.lists_of is not None and prob.lists_of != np.asarray(model.param_values(), dtype=float).tobytes():
                self._set_exchange_lists(prob, model, plan)
        self.backend_info = dict(prob.info, time_specialized=model.t_value is not None,
                                 lifted_constants=len(model.param_index or ()),
                                 # how the table of admissible boxes was made: 'traced' (the callback's DAG on the whole grid: exact
                                 # at every node by construction) or 'node by node' (scalar calls, like the reference)
                                 box_mode=plan.get('box_mode') or 'node by node')
        return prob

    def _create_problem(self, fp, plan):
        nat.require_gpu()
        model, source, column, lanes = plan['model'], plan['source'], plan['column'], plan['lanes']
        per_node, lo, hi, n, max_u, W = (plan[k] for k in ('per_node', 'lo', 'hi', 'n', 'max_u', 'W'))
        shape = self._shape()
        S = int(np.prod(shape))
        dt = self.dtype
        layout = nat.LAYOUT_COLUMNS if column else nat.LAYOUT_NODES
        arrays = dict(
            axes=[np.ascontiguousarray(g, dtype=dt) for g in self.state_grid],
            box_lo=np.ascontiguousarray(lo, dtype=dt),
            box_hi=np.ascontiguousarray(hi, dtype=dt),
            box_n=np.ascontiguousarray(n, dtype=np.int32))
        if W and model.n_perturb >= 2:
            # (the flat law, rounded ONCE to the problem's reals: perturb.product_law)
            arrays['wgrid'], arrays['proba'] = perturb.product_law(self.perturb_grid, self.perturb_proba, dt)
        elif W:
            arrays['wgrid'] = np.ascontiguousarray(self.perturb_grid[0], dtype=dt)
            arrays['proba'] = np.ascontiguousarray(self.perturb_proba[0], dtype=dt)
        module = nat.compile_model(source)
        # slabs: whole hyperplanes of the outermost axis of the device layout
        dev_shape = (shape[1:] + shape[:1]) if column else shape
        if self.comm is not None and self.comm.is_device:
            # RCCL: the library shares out phases of the node range and overlaps
            # each phase's all-gather with the next phase's kernel
            from .dist import phase_partition, slab_partition
            unit = shape[0] if column else 1
            bounds = phase_partition(S // unit, unit, self.comm.nranks, self.comm_phases,
                                     self.comm_taper)
            sparse = ((getattr(self, 'comm_sparse', False) or self.comm_exchange == 'sendrecv')
                      and self.comm_exchange in ('peer', 'direct', 'sendrecv')
                      and self.comm.nranks > 1 and column and not plan['per_control']
                      and not plan['window'] and model.storage_separable and self.sys.stationnary
                      and len(shape) >= 2)
            if sparse:
                dense_bounds = bounds
                bounds = slab_partition(S // unit, unit, self.comm.nranks, self.comm_phases)
            elif plan.get('lead_axes'):
                # reduced-array sweep: a rank reduces what its nodes read -- its own rows of the first
                # stock and a few around them -- so it gets ONE slab of whole rows
                row = int(np.prod(shape[1:])) if shape[0] >= self.comm.nranks else 1
                bounds = slab_partition(S // row, row, self.comm.nranks, self.comm_phases)
            node_range = (0, S)
        elif self.comm is not None:
            bounds = self.comm.slab_bounds(dev_shape)
            node_range = (int(bounds[self.comm.rank]), int(bounds[self.comm.rank + 1]))
        else:
            bounds, node_range = None, (0, S)
        # drop other cached problems: they hold large device buffers (indices of the last
        # sweep that nobody has looked at yet are fetched first)
        if self._idx_source is not None:
            self.last_policy_index
        old = [k for k in self._cache if k[0] == 'problem']
        if old and self.comm is not None and self.comm.is_device and self.comm.nranks > 1:
            # peer exchange: the other ranks may have this rank's old buffers mapped (HIP IPC).  Every
            # rank first closes ITS mappings, then all meet, and only then are the buffers freed -- a
            # freed buffer that is still mapped elsewhere poisons the export of the next one
            # allocated at its address (hipIpcGetMemHandle: invalid argument, seen with 8 ranks).
            for k in old:
                if self._cache[k].h:
                    nat.check(nat.lib().sdp_problem_attach_comm(self._cache[k].h, None, 0, None))
            self.comm.barrier()
        for k in old:
            self._cache.pop(k).close()
        prob = _DeviceProblem(arrays, module, dt, shape, len(self.sys.control), W, lanes,
                              per_node, node_range,
                              self.comm if (self.comm is not None and self.comm.is_device) else None,
                              bounds, layout, plan['staged'], plan['col_seg_nodes'],
                              n_perturb=model.n_perturb if model.n_perturb >= 2 else 0)
        self._cache[fp] = prob
        if self._debug_after_create is not None:        # (tools/host_phase_stress.py: poison the fresh buffers)
            self._debug_after_create(prob)
        exchange = None
        if self.comm is not None and self.comm.is_device and self.comm.nranks > 1:
            exchange = 'rccl'
            if self.comm_exchange in ('peer', 'direct'):
                try:                                        # collective: all ranks succeed or none
                    nat.check(nat.lib().sdp_problem_enable_peer_exchange(prob.h))
                    exchange = 'peer'
                except RuntimeError as e:
                    # only the outcome the ranks AGREED on is a reason to fall back (all of them
                    # do); anything else is this rank's problem alone and must not be papered over
                    if 'peer exchange not available' not in str(e):
                        raise
                    import warnings
                    warnings.warn('peer exchange unavailable, using the RCCL all-gather: {}'.format(e))
                    prob.peer_failure = str(e)
                    if sparse:                              # back to interleaved phases for the gathers
                        prob.parts = np.ascontiguousarray(dense_bounds, dtype=np.int64)
                        nat.check(nat.lib().sdp_problem_attach_comm(prob.h, self.comm.handle,
                                                                    int(prob.parts.shape[0]), nat.ptr(prob.parts)))
                if exchange == 'peer' and sparse:
                    prob.sparse_needs = True
                    exchange = 'peer-sparse'
                if exchange.startswith('peer') and self.comm_exchange == 'direct':
                    if self.comm.nranks <= 8:
                        nat.check(nat.lib().sdp_problem_set_direct_exchange(prob.h, 1))
                        exchange = exchange.replace('peer', 'direct')
                    else:
                        import warnings
                        warnings.warn('the direct exchange serves the (at most 8) GPUs of one node: peer copies instead')
            elif self.comm_exchange == 'sendrecv':
                # the sparse exchange through the collective library alone: grouped ncclSend / ncclRecv of the bounding
                # range of what each rank reads (csrc/sdp_hip.hip, sendrecv_phase); where the model gives no need lists
                # it is the RCCL all-gather
                if sparse:
                    nat.check(nat.lib().sdp_problem_set_sendrecv_exchange(prob.h, 1))
                    prob.sparse_needs = True
                    exchange = 'sendrecv'
            elif self.comm_exchange != 'rccl':
                raise ValueError("comm_exchange must be 'rccl', 'sendrecv', 'peer' or 'direct'")
        prob.lead_halo = bool(plan.get('lead_axes') and self.comm is not None and self.comm.is_device
                              and self.comm.nranks > 1)
        self._set_exchange_lists(prob, model, plan)
        prob.info = dict(plan_info(plan), mode='traced', exchange=exchange, module=module,
                         bit_exact_model=model.bit_exact,
                         inexact_ops=model.inexact_ops(),
                         # diagnostic switches this code object was built with (None in the product)
                         debug_defines=codegen.check_debug(self.debug_defines))
        return prob

    def _set_exchange_lists(self, prob, model, plan):
        """What the sharded exchanges predict from the model: the need lists of the sparse exchanges (the rows of J
        each rank reads) and the lead halo of the reduced-array sweep (the rows of the first stock a node's controls
        reach; sampled: the kernel notices a node that reaches further and evaluates it from the value array itself).
        Both depend on the values of the model's constants, and a problem of lifted constants serves every value: they
        are made again when a call brings other values (DPSolver._problem), on every rank alike -- every rank computes
        every rank's list from the same model, so the lists agree."""
        if not (prob.sparse_needs or prob.lead_halo):
            return
        if prob.lists_of is not None:
            # (the library takes new lists only while J and V are whole: rows another rank sent under the old lists
            # must not be read under the new ones.  Collective, like the calls of every rank that lead here)
            prob.complete()
            prob.swap()
            prob.complete()
            prob.swap()
        if prob.sparse_needs:
            off, ranges = self._peer_needs(model, prob.parts, prob.shape)
            nat.check(nat.lib().sdp_problem_set_peer_needs(prob.h, nat.ptr(off), nat.ptr(ranges)))
            prob.need_fraction = float((ranges[:, 1] - ranges[:, 0]).sum()) / prob.S / self.comm.nranks
        if prob.lead_halo:
            nat.check(nat.lib().sdp_problem_set_lead_halo(prob.h, self._lead_reach_rows(model, plan, None, around=True) + 1))
        # (the constants the lists were made from: a trace of literal constants has a source, and so a problem, of its own)
        prob.lists_of = (np.asarray(model.param_values(), dtype=float).tobytes() if model.param_index is not None
                         else b'')

    def _peer_needs(self, model, parts, shape):
        """For the sparse peer exchange: per rank the node ranges (device order, whole columns) of
        the cost-to-go array its backups READ -- the 2^(d-1) vertex columns of the cell each
        perturbation point sends each of its columns to, one more cell on every side (the device
        locates the cells itself; a next state on a cell boundary may round the other way there),
        and the column of the relative-DP reference node.  Returns (offsets[nranks+1], ranges[:, 2])."""
        from .trace import evaluate
        from .dist import intervals_of
        n0, trail = shape[0], shape[1:]
        nranks = parts.shape[1] - 1
        grids = [np.asarray(g, dtype=float) for g in self.state_grid]
        wg = (np.asarray(self.perturb_grid[0], dtype=float)
              if (self.perturb_grid and model.n_perturb) else None)
        ws = [None] if wg is None else list(wg)
        n_cols = int(np.prod(trail))
        idx = np.unravel_index(np.arange(n_cols), trail)
        xcols = [grids[k + 1][idx[k]] for k in range(len(trail))]
        owner = np.empty(n_cols, dtype=np.int64)
        for r in range(nranks):
            for ph in range(parts.shape[0]):
                owner[parts[ph, r] // n0:parts[ph, r + 1] // n0] = r
        nu = len(self.sys.control)
        u0 = [np.zeros(n_cols) for _ in range(nu)]
        x0 = np.full(n_cols, grids[0][0])
        cells = []
        for w in ws:
            with np.errstate(all='ignore'):
                xn, _ = evaluate(model, [x0] + xcols, u0, [] if w is None else [np.full(n_cols, w)], 0.0)
            q = []
            for k, g in enumerate(grids[1:]):
                nk = len(g)
                p = (np.broadcast_to(np.asarray(xn[k + 1], dtype=float), (n_cols,)) - g[0]) / (g[-1] - g[0]) * (nk - 1)
                p = np.nan_to_num(p, nan=0.0, posinf=0.0, neginf=0.0)
                p = np.where(np.abs(p) < 2147483648.0, p, 0.0)        # sdp_trunc_i32
                q.append(np.clip(np.trunc(p).astype(np.int64), 0, nk - 2))
            cells.append(q)
        ref_col = int(np.ravel_multi_index(self._state_ref_ind[1:], trail)) if len(trail) else 0
        offs, out = [0], []
        span = (-1, 0, 1, 2)
        for r in range(nranks):
            mine = owner == r
            need = np.zeros(trail, dtype=bool)
            for q in cells:
                for delta in np.ndindex(*([len(span)] * len(trail))):
                    at = tuple(np.clip(q[k][mine] + span[delta[k]], 0, trail[k] - 1) for k in range(len(trail)))
                    need[at] = True
            need = need.reshape(-1)
            need[ref_col] = True
            need[mine] = False                               # its own rows never travel
            iv = intervals_of(need) * n0
            out.append(iv)
            offs.append(offs[-1] + len(iv))
        ranges = (np.concatenate(out) if out else np.zeros((0, 2))).astype(np.int64).reshape(-1, 2)
        if not len(ranges):
            ranges = np.zeros((1, 2), dtype=np.int64)        # (a valid pointer for the C call)
        return np.ascontiguousarray(offs, dtype=np.int64), np.ascontiguousarray(ranges)

    def _ref_flat(self, prob=None):
        """flat C-order index of the relative-DP reference node (sdp.py:384)"""
        return int(np.ravel_multi_index(self._state_ref_ind, self._shape()))

    # ------------------------------------------------------------ value iteration
    def value_iteration(self, J_next, rel_dp=False, report_time=True):
        """solve one DP step on the entire state space grid, given the
        cost-to-go array `J_next` discretized over the state space grid
        (reference sdp.py:466-534).

        If rel_dp is True, J_next should be a (J_next, J_ref) tuple.

        Returns (J_k, pol_k); J_k is a tuple (J_diff, J_ref) if `rel_dp` is True.
        pol_k holds the optimal control VALUES, shape state_dims + (nb_control,).
        """
        t_start = datetime.now()
        ref_ind = self._state_ref_ind if rel_dp else None
        if rel_dp:
            J_next, J_ref = J_next
            # the cost-to-go must be a *differential* cost, zero at the reference state
            assert J_next[ref_ind] == 0.
        J_next = np.asarray(J_next)
        self._check_state_array(J_next)         # same ValueError as interp_on_state (sdp.py:412-415)
        if report_time:
            print('value iteration...', end='')
        J_k, pol_k, J_ref = self._backup(J_next, None, rel_dp)
        exec_time = (datetime.now() - t_start).total_seconds()
        if report_time:
            print('\rvalue iteration run in {:.2f} s'.format(exec_time))
        if rel_dp:
            J_k = J_k, J_ref
        return J_k, pol_k

    def value_iterations(self, J_next, n_iter, rel_dp=False, report_time=True, J_ref_full=False, tol=None,
                         check_every=1):
        """`n_iter` successive calls of `value_iteration`, each fed with the
        result of the previous one -- the loop every user of the reference
        writes by hand (doc/example_inventory.py:98-109, AR1 notebook) -- but
        with the cost-to-go kept on the device between sweeps: one upload, one
        download.  NOT in the reference API.  Same results, bit for bit, as

            for k in range(n_iter): J, pol = self.value_iteration(J, rel_dp)

        Returns (J_k, pol_k) of the last sweep; J_k is (J_diff, J_ref) with
        `rel_dp` (J_ref: last reference cost, or all of them if J_ref_full).

        tol: stop at the first checked sweep whose span max(d) - min(d) of
        d = J_k - J_{k-1} is <= tol (stodynprog_amd.convergence); `n_iter` is then
        the maximum number of sweeps, checked are sweeps check_every, 2 check_every,
        ... and the last allowed one.  The result equals the call with n_iter = the
        sweeps run; self.last_convergence tells what the checks found."""
        t_start = datetime.now()
        assert n_iter >= 1
        if tol is not None:
            tol, check_every = conv.validate(tol, check_every)
        self.last_convergence = None
        if rel_dp:
            J_next, J_ref = J_next
            assert J_next[self._state_ref_ind] == 0.
        J_next = np.asarray(J_next)
        self._check_state_array(J_next)
        host_comm = self.comm is not None and not self.comm.is_device
        refs = np.zeros(n_iter)
        model = self._trace_now(None)
        checks = []
        if isinstance(model, TraceError) or host_comm:
            J_k = J_next                    # host callbacks / host exchange: sweep by sweep
            for k in range(n_iter):
                J_prev = J_k
                J_k, pol_k, r = self._backup(J_k, None, rel_dp)
                refs[k] = 0.0 if r is None else r
                if tol is not None and self._host_check(checks, k + 1, n_iter, check_every, tol, J_k, J_prev):
                    break
            n_done = k + 1
        else:
            prob = self._problem(None, model)
            prob.set_value(J_next)
            ref_flat = self._ref_flat(prob) if rel_dp else 0
            if tol is None:
                for k in range(n_iter):
                    if k:
                        prob.swap()             # J of the previous sweep becomes J_next
                    refs[k] = prob.sweep(0.0, rel_dp, ref_flat)
                n_done = n_iter
            else:
                n_done, checked, stats, r = prob.until(False, n_iter, rel_dp, ref_flat, check_every, tol)
                refs[:n_done] = r
                checks = [(k, a, b) for k, (a, b) in zip(checked, stats)]
            J_k = prob.get_value()
            pol_k, self.last_policy_index = prob.get_policy()
        refs = refs[:n_done]
        if tol is not None:
            self.last_convergence = self._sweep_record(tol, check_every, n_done, checks, refs, rel_dp)
        if report_time:
            exec_time = (datetime.now() - t_start).total_seconds()
            print('{:d} value iterations run in {:.2f} s'.format(n_done, exec_time))
        if rel_dp:
            return (J_k, refs if J_ref_full else refs[-1]), pol_k
        return J_k, pol_k

    @staticmethod
    def _host_check(checks, k, n_iter, check_every, tol, J_k, J_prev):
        """the convergence check of the loops that hold full host arrays every sweep: after sweep k (1-based) when it
        is a checked one, appends (k, dmin, dmax) to `checks`; True when the loop stops here"""
        if not conv.is_check(k, n_iter, check_every):
            return False
        J_k = np.asarray(J_k)
        dmin, dmax = conv.diff_stats(J_k, J_prev, J_k.dtype)
        checks.append((k, dmin, dmax))
        return conv.converged(dmin, dmax, tol)

    @staticmethod
    def _sweep_record(tol, check_every, n_done, checks, refs, rel_dp):
        checked = [c[0] for c in checks]
        return conv.SweepConvergence(tol, check_every, n_done, checked, [c[1] for c in checks],
                                     [c[2] for c in checks],
                                     [refs[k - 1] for k in checked] if rel_dp else None)

    def _backup(self, J_next, t_k, rel_dp):
        """One sweep: fused kernel when the model is traceable, else tabulated."""
        model = self._trace_now(t_k)
        if isinstance(model, TraceError):
            return self._backup_tabulated(J_next, t_k, rel_dp)
        prob = self._problem(t_k, model)
        if self.comm is None:
            # single GPU: one library call, arrays through page-locked memory
            J_k, pol_k, J_ref = prob.backup_host(J_next, 0.0 if t_k is None else t_k, rel_dp,
                                                 self._ref_flat(prob) if rel_dp else 0,
                                                 overlap=self.host_overlap)
            self._idx_cache, self._idx_source = None, prob
            return J_k, pol_k, J_ref
        prob.set_value(J_next)
        # with a host-side (gloo) communicator the slabs are exchanged through
        # host memory after the sweep; with RCCL the library does it on device
        host_comm = self.comm is not None and not self.comm.is_device
        J_ref = prob.sweep(0.0 if t_k is None else t_k, rel_dp and not host_comm,
                           self._ref_flat(prob) if rel_dp else 0)
        J_k = prob.get_value()
        if host_comm:
            Jd = prob._to_device_order(J_k).reshape(-1)
            self.comm.all_gather_slabs(Jd, self.comm.slab_bounds(prob.dev_shape))
            J_k = prob._from_device_order(Jd)
            if rel_dp:
                J_ref = J_k[self._state_ref_ind]              # sdp.py:523-525
                J_k -= J_ref
        pol_k, idx = prob.get_policy()
        if host_comm:
            # every rank returns the complete policy, like the single-process call
            nu = len(self.sys.control)
            bounds = self.comm.slab_bounds(prob.dev_shape)
            pd = prob._to_device_order(pol_k, (nu,)).reshape(-1)
            self.comm.all_gather_slabs(pd, bounds * nu)
            pol_k = prob._from_device_order(pd, (nu,))
            idd = prob._to_device_order(idx, (), np.asarray(idx).dtype).reshape(-1)
            self.comm.all_gather_slabs(idd, bounds)
            idx = prob._from_device_order(idd)
        self.last_policy_index = idx
        return J_k, pol_k, J_ref

    def _backup_tabulated(self, J_next, t_k, rel_dp, chunk_cells=4_000_000):
        """Tabulated mode: callbacks evaluated on the host node by node exactly
        like reference sdp.py:651-676; gather + expectation + argmin on the
        device (sdp_tab_backup)."""
        nat.require_gpu()
        self._check_supported()
        shape = self._shape()
        S = int(np.prod(shape))
        nu = len(self.sys.control)
        w_args, proba, W = self._flat_law()
        d = len(shape)
        smin = np.array([g[0] for g in self.state_grid], dtype=float)
        smax = np.array([g[-1] for g in self.state_grid], dtype=float)
        orders = np.array(shape, dtype=np.int64)
        V = np.ascontiguousarray(J_next, dtype=float)
        h = C.c_void_p()
        nat.check(nat.lib().sdp_tab_create(d, nat.ptr(smin), nat.ptr(smax), nat.ptr(orders),
                                           nat.ptr(V), C.byref(h)))
        self.backend_info = dict(mode='tabulated', reason=str(self._trace_now(None)))
        J_k = np.zeros(S)
        idx_k = np.zeros(S, dtype=np.int64)
        pol_k = np.zeros((S, nu))
        try:
            batch = []          # (flat, u_grids, dims, x_next[d, cells], g[cells])
            cells = 0

            def flush():
                nonlocal batch, cells
                if not batch:
                    return
                off = np.zeros(len(batch) + 1, dtype=np.int64)
                for i, b in enumerate(batch):
                    off[i + 1] = off[i] + b[4].size
                xn = np.ascontiguousarray(np.concatenate([b[3] for b in batch], axis=1))
                g = np.ascontiguousarray(np.concatenate([b[4] for b in batch]))
                Jb = np.zeros(len(batch))
                ib = np.zeros(len(batch), dtype=np.int64)
                nat.check(nat.lib().sdp_tab_backup(h, len(batch), nat.ptr(off), W,
                                                   nat.ptr(proba), nat.ptr(xn), nat.ptr(g),
                                                   nat.ptr(Jb), nat.ptr(ib)))
                for (flat, u_grids, dims, _, _), Jv, iv in zip(batch, Jb, ib):
                    J_k[flat] = Jv
                    idx_k[flat] = iv
                    ind = np.unravel_index(iv, dims)
                    pol_k[flat] = [u_grids[c].ravel()[ind[c]] for c in range(nu)]
                batch, cells = [], 0

            # one rule in every path (traced or not): the callables of a STATIONARY system
            # are never handed a time index.  (The reference's bellman_recursion passes t_k
            # regardless, sdp.py:582, and so raises TypeError on a stationary system.)
            if self.sys.stationnary:
                t_k = None
            for flat, x_k in enumerate(itertools.product(*self.state_grid)):
                u_grids, dims = self.control_grids(x_k, t_k)
                # (the control meshes keep the axis of the perturbation, of length 1 for a deterministic system)
                lattice = dims + (W or 1,)
                for i in range(nu):
                    u_grids[i] = u_grids[i].reshape((1,) * i + (-1,) + (1,) * (nu - i))
                args = tuple(x_k) + tuple(u_grids) + w_args
                if t_k is not None:
                    args = (t_k,) + args
                x_next = self.sys.dyn(*args, **self.sys.params)
                g_grid = self.sys.cost(*args, **self.sys.params)
                xn = np.vstack([np.broadcast_to(np.asarray(x, dtype=float), lattice).ravel()
                                for x in x_next])
                gg = np.broadcast_to(np.asarray(g_grid, dtype=float), lattice).ravel()
                batch.append((flat, u_grids, dims, xn, gg))
                cells += gg.size
                if cells >= chunk_cells:
                    flush()
            flush()
        finally:
            nat.lib().sdp_tab_destroy(h)
        J_k = J_k.reshape(shape)
        J_ref = 0.0
        if rel_dp:
            J_ref = J_k[self._state_ref_ind]
            J_k -= J_ref
        self.last_policy_index = idx_k.reshape(shape).astype(np.int32)
        return J_k, pol_k.reshape(shape + (nu,)), J_ref

    def bellman_recursion(self, t_fin, J_fin, t_ini=0, report_time=True):
        """solve the Bellman backward recursion of a *finite horizon problem*
        from `t_fin` (positive int) down to `t_ini` (reference sdp.py:536-591).
        Supports non-stationnary problems.  Returns (J, pol) with a leading
        time axis."""
        t_start = datetime.now()
        state_dims = tuple(len(grid) for grid in self.state_grid)
        nb_control = len(self.sys.control)
        stationnary = self.sys.stationnary
        print('time-dependent problem: {:s}'.format('no' if stationnary else 'yes'))
        assert t_ini == 0       # t_ini > 0 not tested (as in the reference)
        J = np.zeros((t_fin - t_ini,) + state_dims)
        pol = np.zeros((t_fin - t_ini,) + state_dims + (nb_control,))
        if report_time:
            print('bellman recursion...', end='')
        for t_k in range(t_ini, t_fin)[::-1]:
            print('\rtk = {:3d}...'.format(t_k), end='')
            k = t_k - t_ini
            J_next = J_fin if t_k == (t_fin - 1) else J[k + 1]
            self._check_state_array(np.asarray(J_next))
            # the callables get t_k when the system is time dependent (see _backup_tabulated)
            J[k], pol[k], _ = self._backup(np.asarray(J_next), t_k, False)
        exec_time = (datetime.now() - t_start).total_seconds()
        if report_time:
            print('\rvalue iteration run in {:.2f} s'.format(exec_time))
        return J, pol

    # ----------------------------------------------------- per-node entry points
    def _node_lattice(self, x_k, t_k):
        u_grids, dims = self.control_grids(x_k, t_k)
        nu = len(u_grids)
        for i in range(nu):
            u_grids[i] = u_grids[i].reshape((1,) * i + (-1,) + (1,) * (nu - i))
        args = tuple(x_k) + tuple(u_grids) + self._flat_law()[0]
        if t_k is not None:
            args = (t_k,) + args
        return u_grids, dims, args

    def _value_at_state_vect(self, x_k, J_next_interp, t_k=None):
        """optimal cost and control at one state point `x_k` (reference
        sdp.py:639-691): callbacks on the host, gather / expectation / argmin
        on the device.  Returns (J_xk_opt, u_xk_opt)."""
        u_grids, dims, args = self._node_lattice(x_k, t_k)
        nu = len(u_grids)
        _, proba, W = self._flat_law()
        lattice = dims + (W or 1,)          # (as in _backup_tabulated)
        x_next = self.sys.dyn(*args, **self.sys.params)
        g_grid = self.sys.cost(*args, **self.sys.params)
        xn = np.ascontiguousarray(np.vstack(
            [np.broadcast_to(np.asarray(x, dtype=float), lattice).ravel() for x in x_next]))
        gg = np.ascontiguousarray(np.broadcast_to(np.asarray(g_grid, dtype=float), lattice).ravel())
        # the interpolator's values go to the device once (handle cached on the object,
        # dropped by set_values), not once per node
        from .interp import device_tab
        tab = device_tab(J_next_interp)
        off = np.array([0, gg.size], dtype=np.int64)
        Jb = np.zeros(1)
        ib = np.zeros(1, dtype=np.int64)
        nat.check(nat.lib().sdp_tab_backup(tab.h, 1, nat.ptr(off), W, nat.ptr(proba),
                                           nat.ptr(xn), nat.ptr(gg), nat.ptr(Jb),
                                           nat.ptr(ib)))
        ind_opt = np.unravel_index(int(ib[0]), dims)
        u_opt = [u_grids[i].flatten()[ind_opt[i]] for i in range(nu)]
        return (Jb[0], u_opt)

    def _value_at_state_loop(self, x_k, J_next_interp):
        """same result as `_value_at_state_vect` (the reference's iterative
        variant, sdp.py:594-636, keeps the first minimum as well)."""
        J, u = self._value_at_state_vect(x_k, J_next_interp)
        return (J, tuple(u))

    # ------------------------------------------------------------ one-step lookahead at arbitrary states
    def _lookahead_refusals(self, path):
        """what lookahead and simulate_lookahead refuse before anything is traced or allocated"""
        if self.comm is not None and self.comm.nranks > 1:
            raise NotImplementedError('lookahead at arbitrary states runs on one GPU')
        if path not in (None, 'device', 'host'):
            raise ValueError("path must be None, 'device' or 'host', not {!r}".format(path))
        self._check_supported()

    def _lookahead_unit(self, t_k):
        """(device problem of the lookahead unit or None, traced box or TraceError, traced model or TraceError) for
        the time index t_k (None: a stationary system).  The unit is a direct-family unit whatever `self.kernel`
        says (codegen.lookahead_unit), with `lanes_for` the largest lattice of the grid's nodes; it carries its own
        box function when control_box traces with a symbolic time index.  A model that does not trace has no unit."""
        box_t = None if self.sys.stationnary else t_k
        model = self._trace_now(t_k)
        tb = self._trace_box_now(box_t)
        if isinstance(model, TraceError):
            return None, tb, model
        bp = self._box_plan(box_t)
        box = tb if (not isinstance(tb, TraceError) and tb.t_value is None) else None
        debug = codegen.check_debug(self.debug_defines)
        source = codegen.lookahead_unit(model, self.dtype, bp['lanes'], box, debug=debug)
        key = ('lookahead', self._fingerprint(None), bp['lanes'], source)
        prob = self._cache.get(key)
        if prob is None:
            nat.require_gpu()
            for k in [k for k in self._cache if k[0] == 'lookahead']:
                self._cache.pop(k).close()
            shape, dt, nu = self._shape(), self.dtype, len(self.sys.control)
            W = self._law_points()
            arrays = dict(axes=[np.ascontiguousarray(g, dtype=dt) for g in self.state_grid],
                          # (the sweep kernels of the unit are not launched: a one-point box stands in for theirs)
                          box_lo=np.zeros((nu, 1), dtype=dt), box_hi=np.zeros((nu, 1), dtype=dt),
                          box_n=np.ones((nu, 1), dtype=np.int32))
            if W and model.n_perturb >= 2:
                arrays['wgrid'], arrays['proba'] = perturb.product_law(self.perturb_grid, self.perturb_proba, dt)
            elif W:
                arrays['wgrid'] = np.ascontiguousarray(self.perturb_grid[0], dtype=dt)
                arrays['proba'] = np.ascontiguousarray(self.perturb_proba[0], dtype=dt)
            module = nat.compile_model(source)
            prob = _DeviceProblem(arrays, module, dt, shape, nu, W, bp['lanes'], False, (0, int(np.prod(shape))),
                                  n_perturb=model.n_perturb if model.n_perturb >= 2 else 0)
            prob.look_box = box is not None
            prob.info = dict(module=module, lanes=bp['lanes'])
            self._cache[key] = prob
        if model.param_index is not None:
            prob.set_params(model.param_values())
        return prob, tb, model

    def _lookahead_boxes(self, tb, x, t_k):
        """host-made lattices (lo, hi, n) of shape (nu, B) at the states x (B, d), already in the problem's reals:
        the traced box evaluated on the batch, or scalar calls where control_box does not trace"""
        from . import lookahead as la
        xd = np.asarray(x, dtype=float)
        box_t = None if self.sys.stationnary else t_k
        if isinstance(tb, TraceError):
            return la.lattice(self.sys.control_box, self.sys.params, self.control_steps, xd, box_t, self.dtype)
        B, nu = xd.shape[0], len(self.sys.control)
        ends = tb.evaluate([xd[:, i] for i in range(xd.shape[1])], box_t)
        lo = np.empty((nu, B))
        hi = np.empty((nu, B))
        for c, (a, b) in enumerate(ends):
            lo[c], hi[c] = a, b
        return la.lattice_of_ends(lo, hi, self.control_steps, self.dtype)

    def _lookahead_step(self, J_k, x, t_k, path):
        """one lookahead of a batch: J_k on the grid, x (B, d) in the problem's reals.  Returns (J_opt, u_opt (B, nu),
        idx) and leaves in backend_info how it was done."""
        dt = self.dtype
        B, d = x.shape
        nu = len(self.sys.control)
        prob, tb, model = self._lookahead_unit(t_k)
        if prob is None:
            out = self._lookahead_tabulated(J_k, x, t_k, tb)
            self.backend_info = dict(mode='tabulated', reason=str(model), lookahead_path='host', lookahead_box='host')
            return out
        device_box = path != 'host' and prob.look_box
        V = np.ascontiguousarray(J_k, dtype=dt)
        x_d = np.ascontiguousarray(x.T, dtype=dt)                               # [d][B]
        lo = hi = n = None
        steps = np.ascontiguousarray(self.control_steps, dtype=float)
        if not device_box:
            lo, hi, n = (np.ascontiguousarray(a) for a in self._lookahead_boxes(tb, x, t_k))
        J = np.empty(B, dtype=dt)
        u = np.empty((nu, B), dtype=dt)
        idx = np.empty(B, dtype=np.int32)
        nat.check(nat.lib().sdp_problem_lookahead(prob.h, nat.ptr(V), B, nat.ptr(x_d), nat.ptr(lo), nat.ptr(hi), nat.ptr(n),
                                                  nat.ptr(steps), 0.0 if t_k is None else float(t_k),
                                                  nat.ptr(J), nat.ptr(u), nat.ptr(idx)))
        self.backend_info = dict(prob.info, mode='traced', kernel='lookahead', lookahead_path='host' if path == 'host' else 'device',
                                 lookahead_box='device' if device_box else 'host',
                                 time_specialized=model.t_value is not None, lifted_constants=len(model.param_index or ()))
        self._lookahead_prob = prob
        return J, np.ascontiguousarray(u.T), idx

    def _lookahead_tabulated(self, J_k, x, t_k, tb):
        """a model that does not trace: the callables on the host for the whole batch, ONE sdp_tab_backup call with
        all states' cells (what `_value_at_state_vect` does for one state; in float64, like the tabulated sweep)"""
        from . import lookahead as la
        nat.require_gpu()
        B, d = x.shape
        nu = len(self.sys.control)
        w_args, proba, W = self._flat_law()
        xd = np.asarray(x, dtype=float)
        lo, hi, n = self._lookahead_boxes(tb, x, t_k)
        lo, hi = lo.astype(float), hi.astype(float)
        lead = () if (t_k is None or self.sys.stationnary) else (t_k,)
        J = np.full(B, np.nan)
        u = np.full((B, nu), np.nan)
        idx = np.full(B, -1, dtype=np.int32)
        live = [b for b in range(B) if n[0, b] > 0]
        if not live:
            return J.astype(self.dtype), u.astype(self.dtype), idx
        grids, cells_x, cells_g = [], [], []
        off = np.zeros(len(live) + 1, dtype=np.int64)
        for i, b in enumerate(live):
            dims = tuple(int(v) for v in n[:, b])
            ug = [la.control_points(lo[c, b], hi[c, b], n[c, b]) for c in range(nu)]
            mesh = [g.reshape((1,) * c + (-1,) + (1,) * (nu - c)) for c, g in enumerate(ug)]
            args = lead + tuple(xd[b]) + tuple(mesh) + tuple(w_args)
            lattice = dims + (W or 1,)          # (as in _backup_tabulated)
            x_next = self.sys.dyn(*args, **self.sys.params)
            g_grid = self.sys.cost(*args, **self.sys.params)
            cells_x.append(np.vstack([np.broadcast_to(np.asarray(v, dtype=float), lattice).ravel() for v in x_next]))
            cells_g.append(np.broadcast_to(np.asarray(g_grid, dtype=float), lattice).ravel())
            grids.append((ug, dims))
            off[i + 1] = off[i] + cells_g[-1].size
        xn = np.ascontiguousarray(np.concatenate(cells_x, axis=1))
        gg = np.ascontiguousarray(np.concatenate(cells_g))
        shape = self._shape()
        smin = np.array([g[0] for g in self.state_grid], dtype=float)
        smax = np.array([g[-1] for g in self.state_grid], dtype=float)
        orders = np.array(shape, dtype=np.int64)
        V = np.ascontiguousarray(J_k, dtype=float)
        h = C.c_void_p()
        nat.check(nat.lib().sdp_tab_create(len(shape), nat.ptr(smin), nat.ptr(smax), nat.ptr(orders), nat.ptr(V), C.byref(h)))
        try:
            Jb = np.zeros(len(live))
            ib = np.zeros(len(live), dtype=np.int64)
            nat.check(nat.lib().sdp_tab_backup(h, len(live), nat.ptr(off), W, nat.ptr(proba), nat.ptr(xn), nat.ptr(gg),
                                               nat.ptr(Jb), nat.ptr(ib)))
        finally:
            nat.lib().sdp_tab_destroy(h)
        for i, b in enumerate(live):
            ug, dims = grids[i]
            ind = np.unravel_index(int(ib[i]), dims)
            J[b], idx[b] = Jb[i], ib[i]
            u[b] = [ug[c][ind[c]] for c in range(nu)]
        return J.astype(self.dtype), u.astype(self.dtype), idx

    def _lookahead_time(self, t_k):
        if self.sys.stationnary:
            return None
        if t_k is None:
            raise ValueError('a time-dependent system needs the time index t_k')
        return t_k

    def lookahead(self, J_next, x, t_k=None, path=None):
        """Optimal cost and control at ARBITRARY states, for a batch: at every state of `x`

            (J_opt, u_opt, idx) = min / argmin over u of  E_w[ cost(x, u, w) + J_next(dyn(x, u, w)) ]

        over the control lattice of the state -- the reference's `_value_at_state_vect(x_k, J_next_interp)`
        (stodynprog.py:639-691), the body of its sweep, at states that need not be grid nodes, in ONE device call
        for the batch (kernel sdp_lookahead).  NOT in the reference API.  The definition, operator for operator, is
        `stodynprog_amd/lookahead.py`: the box is control_box at the state in float64, the lattice control_grids'
        rule, the expectation the sweep's sequential sum, first-occurrence argmin; J_next extrapolates outside the
        grid, nothing is clamped.  At a grid node the result is value_iteration's J, policy and
        last_policy_index of that node.

        J_next : cost-to-go on the state grid
        x      : state(s), shape (nb_state,) or (B, nb_state); a 4-byte solver rounds them once
        t_k    : time index (non-stationary systems)
        path   : None / 'device': the lattice is made on the device where control_box traces (else by the host);
                 'host': the lattice always comes from the host's evaluation of control_box (the same bits)

        Returns (J_opt (B,), u_opt (B, nb_control), idx (B,) int32).  A state whose box has a non-finite end, or
        whose lattice would have 2^31 points or more, gives NaN, NaN, -1 (the reference raises there).
        backend_info['lookahead_path'] tells 'device' or 'host', ['lookahead_box'] where the lattice was made; a
        model that does not trace takes the host path (callables on the host, one sdp_tab_backup call)."""
        self._lookahead_refusals(path)
        shape = self._shape()
        J_next = np.asarray(J_next)
        if J_next.shape != shape:
            raise ValueError('J_next must have shape {}, not {}'.format(shape, J_next.shape))
        x = np.atleast_2d(np.asarray(x, dtype=float))
        if x.ndim != 2 or x.shape[1] != len(shape):
            raise ValueError('x must have shape ({0},) or (B, {0}), not {1}'.format(len(shape), np.shape(x)))
        t_k = self._lookahead_time(t_k)
        x = x.astype(self.dtype)
        if x.shape[0] == 0:
            return (np.zeros(0, dtype=self.dtype), np.zeros((0, len(self.sys.control)), dtype=self.dtype),
                    np.zeros(0, dtype=np.int32))
        return self._lookahead_step(J_next, x, t_k, path)

    def simulate_lookahead(self, J_next, x0, w=None, n_steps=None, t0=0, path=None):
        """Closed-loop trajectories under LOOKAHEAD controls: at the state the plant is in, the control is

            u_k = argmin over u of  E_w[ cost(x_k, u, w) + J_next(dyn(x_k, u, w)) ]        (`lookahead`)

        followed by the model's own step, x_{k+1} = dyn(x_k, u_k, w_k), g_k = cost(x_k, u_k, w_k), formed as
        `simulate` forms them -- how online control is run in practice, where `simulate` interpolates a tabulated
        policy between nodes (a control that need not be admissible at the state in between).  The whole run is one
        device call (kernel sdp_simulate_lookahead).  NOT in the reference API.

        J_next : cost-to-go on the state grid, or a TIME-INDEXED one of shape (T_J,) + state_dims: step k of the
                 call looks ahead into J_next[t0 + k].  From bellman_recursion's output (J, pol) with final cost
                 J_fin that is `np.concatenate([J[1:], J_fin[None]])`: step k decides with the cost-to-go of k + 1.
        x0, w, n_steps, t0 : as `simulate` (several perturbation variables and the single-trajectory form included)
        path   : None / 'device', or 'host': the loop on the host, one lookahead call per step and the callables
                 for the model's step (what also serves models that do not trace or are traced per step, `data[k]`)

        Returns (x, u, g, q): x, u, g with `simulate`'s shapes, q (T[, B]) the minimised expected value of every
        step.  backend_info['lookahead_path'] tells 'device' or 'host'."""
        from . import lookahead as la
        self._lookahead_refusals(path)
        dims = self._shape()
        d, nu = len(dims), len(self.sys.control)
        x0 = np.asarray(x0, dtype=float)
        single = x0.ndim == 1
        x0 = np.atleast_2d(x0)
        if x0.ndim != 2 or x0.shape[1] != d:
            raise ValueError('x0 must have shape ({0},) or (B, {0}), not {1}'.format(d, x0.shape))
        B = x0.shape[0]
        n_w = len(self.sys.perturb)
        if n_w:
            if w is None:
                raise ValueError('a stochastic system needs the perturbation sequence(s) w')
            w = np.asarray(w, dtype=float)
            if n_w >= 2:
                w = w[:, :, None] if w.ndim == 2 else w
                if w.ndim != 3 or w.shape[1] != n_w:
                    raise ValueError('w must have shape (T, {0}) or (T, {0}, B), not {1}'.format(n_w, w.shape))
            else:
                w = w.reshape(-1, 1) if w.ndim == 1 else w
                if w.ndim != 2:
                    raise ValueError('w must have shape (T,) or (T, B), not {}'.format(w.shape))
                w = w[:, None, :]
            T = w.shape[0] if n_steps is None else int(n_steps)
            if w.shape[-1] != B or w.shape[0] < T:
                raise ValueError('w of shape {} does not give {} steps of {} trajectories'.format(w.shape, T, B))
            w = w[:T]                                                              # (T, m, B)
        else:
            if n_steps is None:
                raise ValueError('give n_steps for a deterministic system')
            T, w = int(n_steps), None
        J_next, timed = la.check_horizon(J_next, dims, T, t0)
        dt = self.dtype
        t_trace = None if self.sys.stationnary else t0
        prob, tb, model = self._lookahead_unit(t_trace)
        on_device = (path != 'host' and prob is not None and prob.look_box
                     and model.t_value is None and model.param_index is None)
        if on_device:
            V = np.ascontiguousarray(J_next[int(t0):int(t0) + T] if timed else J_next, dtype=dt)
            x0_d = np.ascontiguousarray(x0.T, dtype=dt)                             # [d][B]
            w_d = None if w is None else np.ascontiguousarray(w if n_w >= 2 else w[:, 0], dtype=dt)
            steps = np.ascontiguousarray(self.control_steps, dtype=float)
            x = np.empty((T + 1, d, B), dtype=dt)
            u = np.empty((T, nu, B), dtype=dt)
            g = np.empty((T, B), dtype=dt)
            q = np.empty((T, B), dtype=dt)
            nat.check(nat.lib().sdp_problem_simulate_lookahead(
                prob.h, T if timed else 0, nat.ptr(V), int(self.horizon_chunk_bytes), B, T, nat.ptr(x0_d), nat.ptr(w_d),
                nat.ptr(steps), float(t0), nat.ptr(x), nat.ptr(u), nat.ptr(g), nat.ptr(q)))
            x, u = np.ascontiguousarray(np.moveaxis(x, 1, 2)), np.ascontiguousarray(np.moveaxis(u, 1, 2))
            self.backend_info = dict(prob.info, mode='traced', kernel='lookahead', lookahead_path='device', lookahead_box='device')
            self._lookahead_prob = prob
        else:
            # the callables see the time index as `simulate`'s host loop hands it over where the model is traced per
            # step or not at all (an int: `data[k]`), as the kernels do where the trace is symbolic (a real)
            time_index = 'real' if (not isinstance(model, TraceError) and model.t_value is None) else 'int'
            step = lambda J_k, x_k, t_k: self._lookahead_step(J_k, x_k, t_k, 'host')
            x, u, g, q = la.simulate_lookahead(self, J_next, x0, w, T, t0, time_index, step=step)
            self.backend_info = dict(getattr(self, 'backend_info', None) or {}, lookahead_path='host')
        if single:
            return x[:, 0], u[:, 0], g[:, 0], q[:, 0]
        return x, u, g, q

    # ------------------------------------------------------------ policy evaluation
    def eval_policy(self, pol, n_iter, rel_dp=False, J_zero=None,
                    report_time=True, J_ref_full=False, tol=None, check_every=1):
        """evaluate the policy `pol`: cost of each state after `n_iter` steps
        (reference sdp.py:693-775).  If rel_dp is True the relative DP
        algorithm is used.

        Returns J_pol (array of shape self._state_grid_shape), or
        (J_pol, J_ref) if `rel_dp` is True (J_ref: the last reference cost,
        or all of them when J_ref_full).

        tol, check_every: stop early, as in `value_iterations` (n_iter is then the
        maximum; J_ref_full gives the references of the iterations run).
        """
        t_start = datetime.now()
        if tol is not None:
            tol, check_every = conv.validate(tol, check_every)
            if n_iter < 1:
                raise ValueError('eval_policy with tol needs n_iter >= 1, not {!r}'.format(n_iter))
        self.last_convergence = None
        state_dims = self._state_grid_shape
        if J_zero is None:
            J_zero = np.zeros(state_dims)
        assert J_zero.shape == state_dims
        nb_control = len(self.sys.control)
        assert pol.shape == state_dims + (nb_control,)
        t_pol = None if self.sys.stationnary else 0
        model = self._trace_now(t_pol)
        if isinstance(model, TraceError):
            return self._eval_policy_tabulated(pol, n_iter, rel_dp, J_zero, report_time,
                                               J_ref_full, t_start, tol, check_every)
        prob = self._problem(t_pol, model)
        prob.set_value(J_zero)
        prob.set_policy(pol)
        for k in range(n_iter):
            # progress line of the reference; the iterations themselves run in one device call
            print('\rpolicy evaluation: iter. {:d}/{:d}'.format(k, n_iter), end='')
        checks = []
        if self.comm is not None and not self.comm.is_device:
            # host-side (gloo) communicator: one device call per iteration, the
            # slabs meet in host memory in between (test path; RCCL stays on device)
            bounds = self.comm.slab_bounds(prob.dev_shape)
            J_pol, J_ref = np.asarray(J_zero, dtype=self.dtype), np.zeros(n_iter)
            for k in range(n_iter):
                if k:
                    prob.set_value(J_pol)
                prob.eval_policy(1, False, 0)
                Jd = prob._to_device_order(prob.get_value()).reshape(-1)
                self.comm.all_gather_slabs(Jd, bounds)
                J_prev, J_pol = J_pol, prob._from_device_order(Jd)
                if rel_dp:
                    J_ref[k] = J_pol[self._state_ref_ind]          # sdp.py:757-760
                    J_pol -= J_pol[self._state_ref_ind]
                if tol is not None and self._host_check(checks, k + 1, n_iter, check_every, tol, J_pol, J_prev):
                    break
            if tol is not None:
                J_ref = J_ref[:k + 1]
        elif tol is None:
            J_ref = prob.eval_policy(n_iter, rel_dp, self._ref_flat(prob) if rel_dp else 0)
            J_pol = prob.get_value()
        else:
            n_done, checked, stats, J_ref = prob.until(True, n_iter, rel_dp, self._ref_flat(prob) if rel_dp else 0,
                                                       check_every, tol)
            checks = [(k, a, b) for k, (a, b) in zip(checked, stats)]
            J_pol = prob.get_value()
        if tol is not None:
            self.last_convergence = self._sweep_record(tol, check_every, len(J_ref), checks, J_ref, rel_dp)
        exec_time = (datetime.now() - t_start).total_seconds()
        if report_time:
            print('\rpolicy evaluation run in {:.2f} s     '.format(exec_time))
        if rel_dp:
            if not J_ref_full:
                J_ref = J_ref[-1]
            return J_pol, J_ref
        return J_pol

    def _eval_policy_tabulated(self, pol, n_iter, rel_dp, J_zero, report_time, J_ref_full,
                               t_start, tol=None, check_every=1):
        """eval_policy for callables that cannot be traced: dyn and cost are
        evaluated on the host over the whole (S x W) lattice exactly as the
        reference does (sdp.py:732-754, once: they do not change between
        iterations), the interpolation + expectation of every iteration run on
        the device (sdp_tab_backup with one control per node)."""
        nat.require_gpu()
        self._check_supported()
        dims = self._state_grid_shape
        d = len(dims)
        S = int(np.prod(dims))
        nu = len(self.sys.control)
        w_args, proba, W = self._flat_law()
        if not W:           # (this path has always read perturb_grid[0])
            raise NotImplementedError('eval_policy of a deterministic system whose callables cannot be traced')
        state_grid = tuple(np.reshape(self.state_grid[i], (1,) * i + (-1,) + (1,) * (d - i))
                           for i in range(d))
        u_k = [pol[..., i].reshape(dims + (1,)) for i in range(nu)]
        args = state_grid + tuple(u_k) + w_args
        if not self.sys.stationnary:
            args = (0,) + args                  # like the traced path: time index 0
        x_next = self.sys.dyn(*args, **self.sys.params)
        g = self.sys.cost(*args, **self.sys.params)
        lattice = dims + (W,)
        xn = np.ascontiguousarray(np.vstack(
            [np.broadcast_to(np.asarray(x, dtype=float), lattice).ravel() for x in x_next]))
        gg = np.ascontiguousarray(np.broadcast_to(np.asarray(g, dtype=float), lattice).ravel())
        off = np.arange(S + 1, dtype=np.int64) * W
        smin = np.array([gr[0] for gr in self.state_grid], dtype=float)
        smax = np.array([gr[-1] for gr in self.state_grid], dtype=float)
        orders = np.array(dims, dtype=np.int64)
        self.backend_info = dict(mode='tabulated', reason=str(self._trace_now(None)))
        J_pol = np.ascontiguousarray(J_zero, dtype=float)
        J_ref = np.zeros(n_iter)
        idx = np.zeros(S, dtype=np.int64)
        checks = []
        for k in range(n_iter):
            J_prev = J_pol
            print('\rpolicy evaluation: iter. {:d}/{:d}'.format(k, n_iter), end='')
            h = C.c_void_p()
            nat.check(nat.lib().sdp_tab_create(d, nat.ptr(smin), nat.ptr(smax), nat.ptr(orders),
                                               nat.ptr(J_pol), C.byref(h)))
            try:
                J_new = np.zeros(S)
                nat.check(nat.lib().sdp_tab_backup(h, S, nat.ptr(off), W, nat.ptr(proba),
                                                   nat.ptr(xn), nat.ptr(gg), nat.ptr(J_new),
                                                   nat.ptr(idx)))
            finally:
                nat.lib().sdp_tab_destroy(h)
            J_pol = J_new.reshape(dims)
            if rel_dp:
                J_ref[k] = J_pol[self._state_ref_ind]               # sdp.py:760-762
                J_pol -= J_ref[k]
            if tol is not None and self._host_check(checks, k + 1, n_iter, check_every, tol, J_pol, J_prev):
                break
        if tol is not None:
            J_ref = J_ref[:k + 1]
        if tol is not None:
            self.last_convergence = self._sweep_record(tol, check_every, len(J_ref), checks, J_ref, rel_dp)
        exec_time = (datetime.now() - t_start).total_seconds()
        if report_time:
            print('\rpolicy evaluation run in {:.2f} s     '.format(exec_time))
        if rel_dp:
            return J_pol, (J_ref if J_ref_full else J_ref[-1])
        return J_pol

    def policy_iteration(self, pol_init, n_val, n_pol=1, rel_dp=False, tol=None, check_every=1):
        """policy iteration algorithm (reference sdp.py:777-812).

        pol_init : initial policy to evaluate
        n_val : number of value iterations to evaluate the policy
        n_pol : number of policy iterations (default to 1)
        tol, check_every : (not in the reference) every evaluation stops at `tol` as in
              `eval_policy` (n_val is its maximum), and the loop ends early when an
              improvement step returns exactly the policy it was given;
              self.last_convergence then holds one record per evaluation

        Returns (J_pol, pol); J_pol is a tuple (J_diff, J_ref) if rel_dp.
        """
        if tol is not None:
            tol, check_every = conv.validate(tol, check_every)
        ev = dict(tol=tol, check_every=check_every) if tol is not None else {}
        evaluations = []
        pol = pol_init
        J_pol = self.eval_policy(pol, n_val, rel_dp, **ev)
        evaluations.append(self.last_convergence)
        if rel_dp:
            J_diff, J_ref = J_pol
            print('ref policy cost: {:g}'.format(J_ref))
        stable, n_improvements = False, 0
        for k in range(n_pol):
            print('policy iteration {:d}/{:d}'.format(k + 1, n_pol))
            _, pol_new = self.value_iteration(J_pol, rel_dp=rel_dp)
            n_improvements += 1
            if tol is not None and np.array_equal(pol_new, pol):
                stable, pol = True, pol_new     # J_pol is already the evaluation of this policy
                break
            pol = pol_new
            J_pol = self.eval_policy(pol, n_val, rel_dp, **ev)
            evaluations.append(self.last_convergence)
            if rel_dp:
                J_ref = J_pol[1]
                print('ref policy cost: {:g}'.format(J_ref))
        self.last_convergence = (conv.PolicyIterationConvergence(evaluations, n_improvements, stable)
                                 if tol is not None else None)
        return J_pol, pol

    # ------------------------------------------------------------ closed-loop simulation
    def simulate(self, pol, x0, w=None, n_steps=None, t0=0):
        """Closed-loop trajectories under the policy `pol` -- the loop every example of the
        reference writes by hand (examples/20 Searev storage control/
        storage_control.py:242-251):

            for k in range(T):
                u[k] = [self.interp_on_state(pol[..., c])(*x[k]) for c in range(nb_control)]
                x[k+1] = sys.dyn(*x[k], *u[k], w[k])

        run for a BATCH of trajectories on the GPU without a host round trip per step
        (kernel sdp_simulate: policy lookup by multilinear interpolation + the traced
        dynamics).  NOT in the reference API.

        pol : policy array on the state grid, shape state_dims + (nb_control,)
              (as returned by value_iteration / policy_iteration), or a TIME-INDEXED policy of shape
              (T_pol,) + state_dims + (nb_control,) (as returned by bellman_recursion with t_ini = 0): step k
              of the call runs at time index t0 + k with the controls of pol[t0 + k] (kernel
              sdp_simulate_h; also on a stationary system: a receding schedule)
        x0  : start state(s), shape (nb_state,) or (B, nb_state)
        w   : perturbation sequence(s), shape (T,) or (T, B); None for a deterministic
              system (then give n_steps); m >= 2 perturbation variables: (T, m) or (T, m, B)
        t0  : time index of the first step (non-stationary systems)

        Returns (x, u, g): states (T+1, [B,] nb_state), controls (T, [B,] nb_control) and
        instantaneous costs (T[, B]).  Same bits as the hand-written loop when the
        model is `bit_exact` (backend_info)."""
        dims = self._state_grid_shape
        d, nu = len(dims), len(self.sys.control)
        pol, timed = self._check_policy_shape(pol)
        x0 = np.asarray(x0, dtype=float)
        single = x0.ndim == 1
        x0 = np.atleast_2d(x0)
        assert x0.shape[1] == d
        B = x0.shape[0]
        n_w = len(self.sys.perturb)
        if n_w:
            assert w is not None, 'a stochastic system needs the perturbation sequence(s) w'
            w = np.asarray(w, dtype=float)
            if n_w >= 2:
                w = w[:, :, None] if w.ndim == 2 else w
                assert w.ndim == 3 and w.shape[1] == n_w, 'w must have shape (T, {0}) or (T, {0}, B)'.format(n_w)
            else:
                w = w.reshape(-1, 1) if w.ndim == 1 else w
            assert w.shape[-1] == B
            T = w.shape[0] if n_steps is None else int(n_steps)
            assert w.shape[0] >= T
        else:
            assert n_steps is not None, 'give n_steps for a deterministic system'
            T = int(n_steps)
        self._check_horizon(pol, timed, T, t0)
        t_trace = None if self.sys.stationnary else t0
        model = self._trace_now(t_trace)
        table = self._horizon_table(model, timed, T, t0)
        if table is not None:
            # a time-indexed policy, or a model traced step by step (`data[k]`): one device call with the policy slice
            # and the constants of every step
            prob = self._problem(t_trace, model)
            self.backend_info['horizon_path'] = 'device'
            dt = self.dtype
            pol_d = self._horizon_policy(pol, timed, T, t0)                          # [T][nu][S]
            x0_d = np.ascontiguousarray(x0.T, dtype=dt)                             # [d][B]
            w_d = np.ascontiguousarray(w[:T], dtype=dt) if n_w else None            # [T][B]; several variables: [T][m][B]
            x = np.empty((T + 1, d, B), dtype=dt)
            u = np.empty((T, nu, B), dtype=dt)
            g = np.empty((T, B), dtype=dt)
            nat.check(nat.lib().sdp_problem_simulate_h(prob.h, T, nat.ptr(pol_d), nat.ptr(table), table.shape[1],
                                                       int(self.horizon_chunk_bytes), B, T, nat.ptr(x0_d), nat.ptr(w_d),
                                                       float(t0), nat.ptr(x), nat.ptr(u), nat.ptr(g)))
            x, u = np.moveaxis(x, 1, 2), np.moveaxis(u, 1, 2)
        elif isinstance(model, TraceError) or (model.t_value is not None):
            x, u, g = self._simulate_host(pol, x0, w, T, t0)
            self.backend_info = dict(getattr(self, 'backend_info', None) or {}, horizon_path='host')
        else:
            prob = self._problem(t_trace, model)
            dt = self.dtype
            pol_d = np.ascontiguousarray(np.moveaxis(pol, -1, 0), dtype=dt)        # [nu][S]
            x0_d = np.ascontiguousarray(x0.T, dtype=dt)                             # [d][B]
            w_d = np.ascontiguousarray(w[:T], dtype=dt) if n_w else None            # [T][B]; several variables: [T][m][B]
            x = np.empty((T + 1, d, B), dtype=dt)
            u = np.empty((T, nu, B), dtype=dt)
            g = np.empty((T, B), dtype=dt)
            nat.check(nat.lib().sdp_problem_simulate(prob.h, nat.ptr(pol_d), B, T, nat.ptr(x0_d),
                                                     nat.ptr(w_d), float(t0), nat.ptr(x), nat.ptr(u),
                                                     nat.ptr(g)))
            x, u = np.moveaxis(x, 1, 2), np.moveaxis(u, 1, 2)
        if single:
            return x[:, 0], u[:, 0], g[:, 0]
        return np.ascontiguousarray(x), np.ascontiguousarray(u), g

    def _check_policy_shape(self, pol):
        """(pol as an array, whether it has a leading time axis); a ValueError names the two shapes accepted"""
        dims = self._state_grid_shape
        nu = len(self.sys.control)
        pol = np.asarray(pol)
        if pol.shape == dims + (nu,):
            return pol, False
        if pol.ndim == len(dims) + 2 and pol.shape[1:] == dims + (nu,):
            return pol, True
        raise ValueError('pol must have shape {} (a stationary policy) or (T_pol,) + {} (a time-indexed one), not {}'.format(
            dims + (nu,), dims + (nu,), pol.shape))

    def _check_horizon(self, pol, timed, n_steps, t0):
        """the steps t0 .. t0 + n_steps - 1 of a time-indexed policy exist; such a run takes one GPU"""
        if not timed:
            return
        if int(t0) != t0:
            raise ValueError('t0 = {} must be an integer to index a time-indexed policy'.format(t0))
        if t0 < 0 or t0 + n_steps > pol.shape[0]:
            raise ValueError('t0 = {} and n_steps = {} need the policy steps {} .. {}: the policy has T_pol = {}'.format(
                t0, n_steps, t0, t0 + n_steps - 1, pol.shape[0]))
        if self.comm is not None and self.comm.nranks > 1:
            raise NotImplementedError('a time-indexed policy runs on one GPU')

    def _horizon_models(self, n_steps, t0):
        """the traces of the steps t0 .. t0 + n_steps - 1 of a system whose callables need a concrete time index
        (trace_model(.., t_value=t)), or None when a step does not trace"""
        s = self.sys
        out = []
        for t in range(int(t0), int(t0) + int(n_steps)):
            try:
                out.append(trace_model(s.dyn, s.cost, len(s.state), len(s.control), len(s.perturb), s.params,
                                       s.stationnary, t_value=t))
            except TraceError:
                return None
        return out

    def _horizon_table(self, model, timed, n_steps, t0):
        """The lifted constants of every step of a device run over a horizon, as an array (n_steps, n_params) in the
        problem's reals (rounded once, as set_params does), or None when the run is not one for the horizon kernels:
        a stationary policy on a model with a symbolic trace (kernels sdp_simulate / sdp_montecarlo), or a model that the host loop runs --
        no trace, a step that does not trace, or steps whose traces differ in structure (structure_key: the
        operators, the interpolation tables, the number of constants)."""
        if isinstance(model, TraceError):
            return None
        if model.t_value is None:
            if not timed:
                return None
            row = model.param_values() if model.param_index is not None else []
            return np.ascontiguousarray(np.tile(np.asarray(row, dtype=float), (n_steps, 1)), dtype=self.dtype).reshape(n_steps, len(row))
        if n_steps < 1 or int(t0) != t0 or (self.comm is not None and self.comm.nranks > 1):
            return None
        steps = self._horizon_models(n_steps, t0)
        if steps is None:
            return None
        key = model.structure_key()
        if any(m.structure_key() != key for m in steps):
            return None
        rows = [m.param_values() for m in steps]
        return np.ascontiguousarray(np.asarray(rows, dtype=float).reshape(n_steps, len(model.param_index)), dtype=self.dtype)

    def _horizon_policy(self, pol, timed, n_steps, t0):
        """the policy slices of the steps t0 .. t0 + n_steps - 1 as [n_steps][nu][S] in the problem's reals"""
        if timed:
            part = np.moveaxis(pol[int(t0):int(t0) + n_steps], -1, 1)
        else:
            part = np.broadcast_to(np.moveaxis(pol, -1, 0), (n_steps,) + pol.shape[-1:] + pol.shape[:-1])
        return np.ascontiguousarray(part, dtype=self.dtype)

    def _simulate_host(self, pol, x0, w, T, t0):
        """the reference's loop as written (callables on the host, one interpolator call
        per step, batched over the trajectories): models that cannot be traced"""
        d, nu = len(self._state_grid_shape), len(self.sys.control)
        B = x0.shape[0]
        timed = pol.ndim == d + 2          # a time-indexed policy: per step the interpolators of pol[t0 + k]
        if not timed:
            laws = [self.interp_on_state(np.ascontiguousarray(pol[..., c])) for c in range(nu)]
        x = np.zeros((T + 1, B, d))
        u = np.zeros((T, B, nu))
        g = np.zeros((T, B))
        x[0] = x0
        for k in range(T):
            xs = tuple(x[k, :, i] for i in range(d))
            if timed:
                laws = [self.interp_on_state(np.ascontiguousarray(pol[t0 + k][..., c])) for c in range(nu)]
            for c in range(nu):
                u[k, :, c] = laws[c](*xs)
            args = xs + tuple(u[k, :, c] for c in range(nu)) + (
                () if w is None else ((w[k],) if w.ndim == 2 else tuple(w[k])))       # (several variables: w is (T, m, B))
            if not self.sys.stationnary:
                args = (t0 + k,) + args
            xn = self.sys.dyn(*args, **self.sys.params)
            for i in range(d):
                x[k + 1, :, i] = xn[i]
            g[k] = self.sys.cost(*args, **self.sys.params)
        return x, u, g

    # ------------------------------------------------------------ Monte Carlo policy evaluation
    def _mc_law(self, law):
        if not self.sys.stochastic:
            raise ValueError('a deterministic system has nothing to draw: use simulate(pol, x0, n_steps=...)')
        m = len(self.sys.perturb)
        if m == 1:
            if law is None:
                law = (self.perturb_grid[0], self.perturb_proba[0])
            if len(law) != 2:
                raise ValueError('law must be (grid, proba)')
            return mc.check_law(*law)
        # several variables: ONE draw per step indexes a joint law, values (m, n) and proba (n,) -- by default the
        # flat product law the DP optimised against (stodynprog_amd.perturb)
        self._check_supported()
        if law is None:
            law = perturb.product_law(self.perturb_grid, self.perturb_proba)
        if len(law) != 2:
            raise ValueError('law must be (values of shape ({}, n), proba of shape (n,))'.format(m))
        n = np.size(law[1])
        need = perturb.mc_table_bytes(n, m, self.dtype.itemsize)
        if n <= mc.MAX_LAW_POINTS and need > perturb.MC_TABLE_BYTES:
            raise ValueError('a law of {} points of {} variables needs a draw table of {} bytes: at most {} (the LDS the '
                             'Monte Carlo kernel may ask for)'.format(n, m, need, perturb.MC_TABLE_BYTES))
        return perturb.check_joint_law(law[0], law[1], m)

    @staticmethod
    def _mc_ids(n_traj, traj_offset):
        n_traj, traj_offset = int(n_traj), int(traj_offset)
        if n_traj < 1:
            raise ValueError('n_traj must be at least 1')
        if traj_offset < 0 or traj_offset + n_traj > 1 << 64:
            raise ValueError('trajectory ids must lie in [0, 2**64)')
        return np.arange(n_traj, dtype=np.uint64) + np.uint64(traj_offset)

    def monte_carlo_draws(self, seed, n_traj, n_steps, law=None, traj_offset=0):
        """The perturbations `monte_carlo` draws on the device, from their definition in numpy
        (`stodynprog_amd.montecarlo`): trajectories traj_offset .. traj_offset + n_traj - 1, steps
        0 .. n_steps - 1.  Returns (indices, w): (n_steps, n_traj) int32 indices
        into the law and the values law_grid[indices] in the problem's reals, so that
        `simulate(pol, x0, w)` replays the run (m >= 2 perturbation variables: w is
        (n_steps, m, n_traj), the columns of the joint law).  NOT in the reference API."""
        grid, proba = self._mc_law(law)
        n_steps = int(n_steps)
        if n_steps < 0:
            raise ValueError('n_steps must not be negative')
        ids = self._mc_ids(n_traj, traj_offset)
        steps = np.arange(n_steps, dtype=np.uint64)
        idx = mc.draws(seed, ids, steps, proba)
        if grid.ndim == 2:
            return idx, np.ascontiguousarray(np.moveaxis(grid.astype(self.dtype)[:, idx], 0, 1))
        return idx, grid.astype(self.dtype)[idx]

    def monte_carlo(self, pol, x0, n_steps, seed=0, n_burn=0, n_traj=None, law=None, occupancy=False,
                    traj_offset=0, t0=0):
        """Monte Carlo evaluation of the policy `pol`: the closed loop of `simulate` for a batch of
        trajectories, with every step's perturbation drawn ON THE DEVICE from the discretised law and
        only per-trajectory reductions coming back -- the `cost.mean()` at the end of the
        reference's examples (examples/20 Searev storage control/storage_control.py:197-265)
        without T x B reals up and (T+1) d B + T nu B + T B reals down.  NOT in the reference API.

        pol      : policy array, shape state_dims + (nb_control,), or a time-indexed policy of shape
                   (T_pol,) + state_dims + (nb_control,): step k takes the controls of pol[t0 + k], as in `simulate`
        x0       : start state (nb_state,) -- then give n_traj -- or one per trajectory (B, nb_state)
        n_steps  : steps per trajectory
        seed     : the run is a function of (seed, trajectory id, step) alone (Philox4x32-10, see
                   `stodynprog_amd.montecarlo`): batch size, launch configuration and how a batch is
                   split over calls (traj_offset = id of row 0) do not change a bit
        n_burn   : the first n_burn steps advance the state but enter no reduction
        law      : (grid, proba) of the perturbation, at most 4096 points; default: the solver's
                   own perturb_grid / perturb_proba, the chain the DP optimised against.
                   m >= 2 perturbation variables: (values (m, n), proba (n,)), a JOINT law (it need
                   not be a product; default: the flat product law of stodynprog_amd.perturb)
        occupancy: also count, per grid node, the visits of the node nearest to x_k (k >= n_burn)
        t0       : time index of the first step (non-stationary systems)

        Returns a `montecarlo.MonteCarloResult`: cost_sum, cost_mean, n_outside, x_final,
        occupancy, mean, stderr.  Models that `simulate` runs on the host (untraceable ones) run
        the same host loop here, fed by `montecarlo.draws`."""
        dims = self._state_grid_shape
        d, nu = len(dims), len(self.sys.control)
        grid, proba = self._mc_law(law)
        if self.comm is not None and self.comm.nranks > 1:
            raise NotImplementedError('monte_carlo runs on one GPU')
        pol, timed = self._check_policy_shape(pol)
        x0 = np.asarray(x0, dtype=float)
        if x0.ndim == 1:
            if x0.shape != (d,):
                raise ValueError('x0 must have shape ({},) or (B, {})'.format(d, d))
            if n_traj is None:
                raise ValueError('give n_traj with a single start state')
            x0 = np.broadcast_to(x0, (int(n_traj), d))
        elif x0.ndim != 2 or x0.shape[1] != d:
            raise ValueError('x0 must have shape ({},) or (B, {})'.format(d, d))
        elif n_traj is not None and int(n_traj) != x0.shape[0]:
            raise ValueError('n_traj = {} but x0 holds {} start states'.format(n_traj, x0.shape[0]))
        B = x0.shape[0]
        n_steps, n_burn = int(n_steps), int(n_burn)
        if n_steps < 1 or not 0 <= n_burn < n_steps:
            raise ValueError('need n_steps >= 1 and 0 <= n_burn < n_steps')
        seed = mc.check_seed(seed)
        ids = self._mc_ids(B, traj_offset)
        spl = int(self.steps_per_launch)
        if spl < 1:
            raise ValueError('steps_per_launch must be at least 1')
        dt = self.dtype
        self._check_horizon(pol, timed, n_steps, t0)
        t_trace = None if self.sys.stationnary else t0
        model = self._trace_now(t_trace)
        table = self._horizon_table(model, timed, n_steps, t0)
        if table is not None:
            prob = self._problem(t_trace, model)
            self.backend_info['horizon_path'] = 'device'
            pol_d = self._horizon_policy(pol, timed, n_steps, t0)                   # [T][nu][S]
            x0_d = np.ascontiguousarray(x0.T, dtype=dt)                             # [d][B]
            cum = np.ascontiguousarray(mc.cumulative(proba))
            law_d = np.ascontiguousarray(grid, dtype=dt)                            # [n]; several variables: [m][n]
            cost_sum = np.empty(B, dtype=dt)
            n_out = np.empty(B, dtype=np.int64)
            x_final = np.empty((d, B), dtype=dt)
            occ = np.empty(int(np.prod(dims)), dtype=np.uint64) if occupancy else None
            nat.check(nat.lib().sdp_problem_montecarlo_h(
                prob.h, n_steps, nat.ptr(pol_d), nat.ptr(table), table.shape[1], int(self.horizon_chunk_bytes), B,
                n_steps, n_burn, seed, int(traj_offset), nat.ptr(x0_d), nat.ptr(cum), len(proba), nat.ptr(law_d),
                float(t0), spl, nat.ptr(cost_sum), nat.ptr(n_out), nat.ptr(x_final), nat.ptr(occ)))
            x_final = np.ascontiguousarray(x_final.T)
            if occ is not None:
                occ = occ.astype(np.int64).reshape(dims)
            path = 'device'
        elif isinstance(model, TraceError) or (model.t_value is not None):
            cost_sum, n_out, x_final, occ = self._monte_carlo_host(pol, x0, n_steps, n_burn, seed, ids, grid, proba,
                                                                   occupancy, t0)
            path = 'host'
            self.backend_info = dict(getattr(self, 'backend_info', None) or {}, horizon_path='host')
        else:
            prob = self._problem(t_trace, model)
            pol_d = np.ascontiguousarray(np.moveaxis(pol, -1, 0), dtype=dt)        # [nu][S]
            x0_d = np.ascontiguousarray(x0.T, dtype=dt)                             # [d][B]
            cum = np.ascontiguousarray(mc.cumulative(proba))
            law_d = np.ascontiguousarray(grid, dtype=dt)                            # [n]; several variables: [m][n]
            cost_sum = np.empty(B, dtype=dt)
            n_out = np.empty(B, dtype=np.int64)
            x_final = np.empty((d, B), dtype=dt)
            occ = np.empty(int(np.prod(dims)), dtype=np.uint64) if occupancy else None
            nat.check(nat.lib().sdp_problem_montecarlo(
                prob.h, nat.ptr(pol_d), B, n_steps, n_burn, seed, int(traj_offset), nat.ptr(x0_d), nat.ptr(cum),
                len(proba), nat.ptr(law_d), float(t0), spl, nat.ptr(cost_sum), nat.ptr(n_out), nat.ptr(x_final),
                nat.ptr(occ)))
            x_final = np.ascontiguousarray(x_final.T)
            if occ is not None:
                occ = occ.astype(np.int64).reshape(dims)
            path = 'device'
        return mc.MonteCarloResult(cost_sum, n_out, x_final, occ, n_steps, n_burn, seed, int(traj_offset), t0, path)

    def _monte_carlo_host(self, pol, x0, n_steps, n_burn, seed, ids, grid, proba, occupancy, t0):
        """the reductions of the kernel in numpy over `_simulate_host`, a block of steps at a time"""
        dims = self._state_grid_shape
        dt = self.dtype
        B = x0.shape[0]
        smin = np.array([g[0] for g in self.state_grid], dtype=float)
        smax = np.array([g[-1] for g in self.state_grid], dtype=float)
        x = np.array(x0, dtype=float)
        acc = np.zeros(B, dtype=dt)
        n_out = np.zeros(B, dtype=np.int64)
        occ = np.zeros(dims, dtype=np.int64) if occupancy else None
        wgrid = grid.astype(dt)
        for k0 in range(0, n_steps, self.MC_HOST_BLOCK):
            n = min(self.MC_HOST_BLOCK, n_steps - k0)
            steps = np.arange(k0, k0 + n, dtype=np.uint64)
            idx = mc.draws(seed, ids, steps, proba)
            w = (wgrid[idx] if wgrid.ndim == 1 else np.moveaxis(wgrid[:, idx], 0, 1)).astype(float)
            xs, _, g = self._simulate_host(pol, x, w, n, t0 + k0)
            for i in range(n):
                if k0 + i < n_burn:
                    continue
                acc = acc + g[i].astype(dt)
                n_out += ~np.all((xs[i] >= smin) & (xs[i] <= smax), axis=1)
                if occ is not None:
                    np.add.at(occ, tuple(mc.nearest_nodes(xs[i], self.state_grid, np.float64).T), 1)   # (host states are float64)
            x = xs[n]
        return acc, n_out, x.astype(dt), occ

    def monte_carlo_lookahead(self, J_next, x0, n_steps, seed=0, n_burn=0, n_traj=None, law=None, occupancy=False,
                              traj_offset=0, t0=0, path=None):
        """Monte Carlo evaluation of a COST-TO-GO under lookahead controls: the closed loop of `simulate_lookahead`
        for a batch of trajectories -- at the state the plant is in, u_k = argmin over u of
        E_w[cost(x_k, u, w) + J_next(dyn(x_k, u, w))], then the model's own step -- with every step's perturbation
        drawn ON THE DEVICE and only per-trajectory reductions coming back (kernel sdp_montecarlo_lookahead).  It is
        to `simulate_lookahead` what `monte_carlo` is to `simulate`: no tabulated policy, no T x B reals up and no
        (T+1) d B + T nu B + 2 T B reals down.  NOT in the reference API.  The definition is
        `stodynprog_amd.lookahead.monte_carlo_lookahead`.

        J_next   : cost-to-go on the state grid, or a time-indexed one of shape (T_J,) + state_dims read at t0 + k
                   (as `simulate_lookahead`)
        x0, n_traj, n_steps, seed, n_burn, traj_offset, occupancy, t0 : as `monte_carlo`
        law      : the law the PLANT draws from, with `monte_carlo`'s meaning and checks (several perturbation
                   variables: a joint table (m, n)); default: the solver's own.  The expectation INSIDE the backup
                   always runs over the solver's own discretised law, whatever `law` is: a controller can be scored
                   against a law it was not optimised for.
        path     : None / 'device', or 'host' (as `simulate_lookahead`: one lookahead call per step, the draws of
                   `montecarlo.draws` and the reductions in numpy, MC_HOST_BLOCK steps at a time; what also serves
                   `data[k]` models and models that do not trace)

        A state whose box has no valid lattice gets u = NaN: its trajectory's state and cost_sum go NaN and every
        later counted step is outside.  Returns a `montecarlo.MonteCarloResult`; its `path` and
        backend_info['lookahead_path'] tell 'device' or 'host'."""
        from . import lookahead as la
        if not self.sys.stochastic:
            raise ValueError('a deterministic system has nothing to draw: use simulate_lookahead(J_next, x0, n_steps=...)')
        self._lookahead_refusals(path)
        dims = self._shape()
        d = len(dims)
        grid, proba = self._mc_law(law)
        x0 = np.asarray(x0, dtype=float)
        if x0.ndim == 1:
            if x0.shape != (d,):
                raise ValueError('x0 must have shape ({},) or (B, {})'.format(d, d))
            if n_traj is None:
                raise ValueError('give n_traj with a single start state')
            x0 = np.broadcast_to(x0, (int(n_traj), d))
        elif x0.ndim != 2 or x0.shape[1] != d:
            raise ValueError('x0 must have shape ({},) or (B, {})'.format(d, d))
        elif n_traj is not None and int(n_traj) != x0.shape[0]:
            raise ValueError('n_traj = {} but x0 holds {} start states'.format(n_traj, x0.shape[0]))
        B = x0.shape[0]
        n_steps, n_burn = int(n_steps), int(n_burn)
        if n_steps < 1 or not 0 <= n_burn < n_steps:
            raise ValueError('need n_steps >= 1 and 0 <= n_burn < n_steps')
        seed = mc.check_seed(seed)
        ids = self._mc_ids(B, traj_offset)
        spl = int(self.steps_per_launch)
        if spl < 1:
            raise ValueError('steps_per_launch must be at least 1')
        J_next, timed = la.check_horizon(J_next, dims, n_steps, t0)
        dt = self.dtype
        t_trace = None if self.sys.stationnary else t0
        prob, tb, model = self._lookahead_unit(t_trace)
        on_device = (path != 'host' and prob is not None and prob.look_box
                     and model.t_value is None and model.param_index is None)
        if on_device:
            V = np.ascontiguousarray(J_next[int(t0):int(t0) + n_steps] if timed else J_next, dtype=dt)
            x0_d = np.ascontiguousarray(x0.T, dtype=dt)                             # [d][B]
            cum = np.ascontiguousarray(mc.cumulative(proba))
            law_d = np.ascontiguousarray(grid, dtype=dt)                            # [n]; several variables: [m][n]
            steps = np.ascontiguousarray(self.control_steps, dtype=float)
            cost_sum = np.empty(B, dtype=dt)
            n_out = np.empty(B, dtype=np.int64)
            x_final = np.empty((d, B), dtype=dt)
            occ = np.empty(int(np.prod(dims)), dtype=np.uint64) if occupancy else None
            nat.check(nat.lib().sdp_problem_montecarlo_lookahead(
                prob.h, n_steps if timed else 0, nat.ptr(V), int(self.horizon_chunk_bytes), B, n_steps, n_burn, seed,
                int(traj_offset), nat.ptr(x0_d), nat.ptr(cum), len(proba), nat.ptr(law_d), nat.ptr(steps), float(t0), spl,
                nat.ptr(cost_sum), nat.ptr(n_out), nat.ptr(x_final), nat.ptr(occ)))
            x_final = np.ascontiguousarray(x_final.T)
            if occ is not None:
                occ = occ.astype(np.int64).reshape(dims)
            self.backend_info = dict(prob.info, mode='traced', kernel='lookahead', lookahead_path='device', lookahead_box='device')
            self._lookahead_prob = prob
            ran = 'device'
        else:
            time_index = 'real' if (not isinstance(model, TraceError) and model.t_value is None) else 'int'
            step = lambda J_k, x_k, t_k: self._lookahead_step(J_k, x_k, t_k, 'host')
            cost_sum, n_out, x_final, occ = la.monte_carlo_lookahead(
                self, J_next, x0, n_steps, seed, n_burn, ids, grid, proba, bool(occupancy), t0, time_index, step=step,
                block=self.MC_HOST_BLOCK)
            self.backend_info = dict(getattr(self, 'backend_info', None) or {}, lookahead_path='host')
            ran = 'host'
        return mc.MonteCarloResult(cost_sum, n_out, x_final, occ, n_steps, n_burn, seed, int(traj_offset), t0, ran)

    # ------------------------------------------------------------ state distributions under a policy
    def _transition_size(self):
        """(S, nnz, bytes) of the transition operator of the current discretisation"""
        shape = self._shape()
        S = int(np.prod(shape))
        nnz = S * max(self._law_points(), 1) * (1 << len(shape))
        return S, nnz, forward.operator_bytes(nnz, S, self.dtype.itemsize)

    def transition_operator(self, pol, t_k=None):
        """The Markov chain on the grid that `eval_policy(pol, ..)` implies, as an operator on state distributions:
        (P J)(s) = sum_w p_w interp(J)(dyn(x_s, pol[s], w)) is the linear part of one evaluation step, and the
        `TransitionOperator` returned applies its transpose, mu' = P^T mu, on the device.  NOT in the reference API.

        pol : policy array, shape state_dims + (nb_control,), as for eval_policy
        t_k : time index of a non-stationary system (as in `control_grids`; default 0, like eval_policy)

        `stodynprog_amd.forward` defines every entry.  The interpolation extrapolates: where the model leaves the
        grid, weights are negative or above 1 (each source's weights still sum to 1) -- nothing is clamped, so that
        P^T is the exact adjoint of what eval_policy computes.  An operator stores S W 2^d entries;
        DPSolver.TRANSITION_MAX_BYTES (2 GiB) caps it, one GPU only."""
        dims = self._shape()
        nu = len(self.sys.control)
        self._check_supported()
        if self.comm is not None:
            raise NotImplementedError('transition_operator runs on one GPU (no communicator)')
        pol = np.asarray(pol)
        if pol.shape != dims + (nu,):
            raise ValueError('pol must have shape {}, not {}'.format(dims + (nu,), pol.shape))
        S, nnz, nbytes = self._transition_size()
        if nbytes > self.TRANSITION_MAX_BYTES:
            raise ValueError('the transition operator of this grid has nnz = {} entries and takes {} bytes: more than '
                             'DPSolver.TRANSITION_MAX_BYTES = {} bytes'.format(nnz, nbytes, self.TRANSITION_MAX_BYTES))
        if nnz >= 1 << 32:
            raise ValueError('the transition operator of this grid has nnz = {} entries ({} bytes): entry positions are '
                             '32-bit words, at most 2**32 - 1 entries whatever the cap'.format(nnz, nbytes))
        t_trace = None if self.sys.stationnary else (0 if t_k is None else t_k)
        model = self._trace_now(t_trace)
        if isinstance(model, TraceError):
            # callables that cannot be traced: the entries from the definition, on the host
            e = forward.entries(self, pol, t_trace, time_index='int')
            op = TransitionOperator.from_coo(dims, e.tgt, e.src, e.val, e.mean_cost.reshape(dims), 'host')
            self.backend_info = dict(mode='host entries', reason=str(model))
        else:
            prob = self._problem(t_trace, model)
            pol_d = np.ascontiguousarray(pol, dtype=self.dtype)                    # [S][nu]
            h = C.c_void_p()
            nat.check(nat.lib().sdp_transop_create(prob.h, nat.ptr(pol_d), float(0 if t_trace is None else t_trace),
                                                   C.byref(h)))
            gbar = np.empty(dims, dtype=self.dtype)
            nat.check(nat.lib().sdp_transop_get_mean_cost(h, nat.ptr(gbar)))
            op = TransitionOperator(h, dims, self.dtype, nnz, gbar, 'device')
        # (the operator's record: push times are added to it as the operator is used)
        self.backend_info = dict(self.backend_info, transition=op.info)
        return op

    def stationary_distribution(self, pol, t_k=None, **kw):
        """`transition_operator(pol, t_k).stationary(**kw)` in one call: the stationary distribution of the state
        under `pol` (a `forward.Stationary` record: mu, n_done, converged, delta, average_cost, mass)."""
        op = self.transition_operator(pol, t_k)
        try:
            return op.stationary(**kw)
        finally:
            op.close()

    def horizon_operator(self, pol, n_steps=None, t0=0):
        """The transition operators of the steps of a horizon, as one `HorizonOperator`: step k = 0 .. n_steps - 1 is
        `transition_operator(pol_k, t0 + k)` -- its CSR, its mean cost, its push, bit for bit -- with all steps built in
        one device call (kernel sdp_transitions_h and one sort).  `forward.chain_entries` and `forward.propagate` are
        the definition.  NOT in the reference API.

        pol     : a TIME-INDEXED policy of shape (T_pol,) + state_dims + (nb_control,), as bellman_recursion returns
                  (pol_k = pol[t0 + k]; n_steps defaults to T_pol - t0), or a stationary one of shape state_dims +
                  (nb_control,) (pol_k = pol; give n_steps: a non-stationary model, or a receding schedule)
        n_steps : steps of the chain
        t0      : time index of step 0, an integer

        The device path serves every model `simulate` runs a time-indexed policy of on the device (a symbolic time index,
        or `data[k]` steps of one structure with their constants lifted per step); any other model takes the host path:
        per step the entries of the definition, uploaded, and the existing solo operators chained.  The operators take
        n_steps times the bytes of one (`forward.operator_bytes`), capped by DPSolver.TRANSITION_MAX_BYTES: continue a
        longer horizon from mu[-1].  One GPU only."""
        dims = self._shape()
        self._check_supported()
        if self.comm is not None:
            raise NotImplementedError('horizon_operator runs on one GPU (no communicator)')
        pol, timed = self._check_policy_shape(pol)
        if int(t0) != t0:
            raise ValueError('t0 = {} must be an integer: it indexes the steps of a horizon'.format(t0))
        t0 = int(t0)
        if timed and not 0 <= t0 < pol.shape[0]:
            raise ValueError('t0 = {} is outside the time-indexed policy of shape {}: T_pol = {} steps of shape {}'.format(
                t0, pol.shape, pol.shape[0], pol.shape[1:]))
        if n_steps is None:
            if not timed:
                raise ValueError('a stationary policy, shape {}, needs n_steps; a time-indexed one has shape (T_pol,) + {} '
                                 'and runs to its end'.format(pol.shape, pol.shape))
            n_steps = pol.shape[0] - t0
        n_steps = int(n_steps)
        if n_steps < 1:
            raise ValueError('n_steps = {}: a horizon has at least one step'.format(n_steps))
        self._check_horizon(pol, timed, n_steps, t0)
        S, nnz_step, step_bytes = self._transition_size()
        if n_steps * step_bytes > self.TRANSITION_MAX_BYTES:
            raise ValueError('the operators of {} steps have {} entries each and take {} bytes together: more than '
                             'DPSolver.TRANSITION_MAX_BYTES = {} bytes, which n_steps = {} fits (continue from mu[-1])'.format(
                                 n_steps, nnz_step, n_steps * step_bytes, self.TRANSITION_MAX_BYTES,
                                 self.TRANSITION_MAX_BYTES // step_bytes))
        parts = HorizonOperator.plan_parts(n_steps, S, nnz_step, HorizonOperator.part_steps)
        t_trace = None if self.sys.stationnary else t0
        model = self._trace_now(t_trace)
        # (the policy is handed over slice by slice whatever its form: the table of a time-indexed run)
        table = self._horizon_table(model, True, n_steps, t0)
        if table is not None:
            prob = self._problem(t_trace, model)
            pol_d = self._horizon_policy(pol, timed, n_steps, t0)                    # [n_steps][nu][S]
            n_params = table.shape[1]
            handles, times = [], [0.0, 0.0]
            gbar = np.empty((n_steps,) + dims, dtype=self.dtype)
            try:
                for first, count in parts:
                    h = C.c_void_p()
                    rows = np.ascontiguousarray(table[first:first + count]) if n_params else None
                    nat.check(nat.lib().sdp_chainop_create(prob.h, count, nat.ptr(pol_d[first:first + count]), nat.ptr(rows),
                                                           n_params, float(t0 + first), C.byref(h)))
                    handles.append(h)
                    nat.check(nat.lib().sdp_chainop_get_mean_cost(h, nat.ptr(gbar[first:first + count])))
                    ms = _chainop_times(h)
                    times = [times[0] + ms[0], times[1] + ms[1]]
            except Exception:
                for h in handles:
                    nat.lib().sdp_chainop_destroy(h)
                raise
            op = HorizonOperator(dims, self.dtype, n_steps, nnz_step, 'device', parts, handles, gbar, times)
        else:
            # a model the horizon kernels do not run: the entries of every step from the definition, on the host
            steps, times = [], [0.0, 0.0]
            gbar = np.empty((n_steps,) + dims, dtype=self.dtype)
            try:
                for k, e in enumerate(forward.chain_entries(self, pol, n_steps, t0, time_index='int')):
                    steps.append(TransitionOperator.from_coo(dims, e.tgt, e.src, e.val, None, 'host'))
                    gbar[k] = e.mean_cost.reshape(dims)
                    times[1] += steps[-1].info['sort_ms']
            except Exception:
                for o in steps:
                    o.close()
                raise
            op = HorizonOperator(dims, self.dtype, n_steps, nnz_step, 'host', [(k, 1) for k in range(n_steps)], steps, gbar,
                                 times)
        self.backend_info = dict(getattr(self, 'backend_info', None) or {}, horizon_operator=op.info)
        return op

    def propagate(self, pol, mu0, n_steps=None, t0=0, J_fin=None):
        """`horizon_operator(pol, n_steps, t0).propagate(mu0, J_fin)` in one call: the distribution of the state at every
        step of a horizon from mu0 (shape state_dims, or (B,) + state_dims), the expected cost of every step and their
        total (a `forward.Propagation` record)."""
        _horizon_vectors(mu0, self._shape(), self.dtype)
        op = self.horizon_operator(pol, n_steps, t0)
        try:
            return op.propagate(mu0, J_fin)
        finally:
            op.close()

    # ------------------------------------------------------------------ reporting
    def print_summary(self):
        """summary information about the state of the SDP solver
        (reference sdp.py:814-875)"""
        print('SDP solver for system "{}"'.format(self.sys.name))

        def describe(names, grids):
            for name, grid in zip(names, grids):
                if len(grid) > 1:
                    print('  - Δ{:s} = {:g}'.format(name, grid[1] - grid[0]))
                else:
                    print('  - {:s} fixed at {:g}'.format(name, grid[0]))

        size = 'x'.join(str(len(g)) for g in self.state_grid)
        print('* state space discretized on a {:s} points grid'.format(size))
        describe(self.sys.state, self.state_grid)
        if self.sys.stochastic:
            size = 'x'.join(str(len(g)) for g in self.perturb_grid)
            print('* perturbation discretized on a {:s} points grid'.format(size))
            describe(self.sys.perturb, self.perturb_grid)
        cdim = None
        if self.sys.control_box is not None:
            t_k = None if self.sys.stationnary else 0
            _, _, n = self._box_table(t_k)
            cdim = n.T.astype(np.int64)             # (S, nu)
        else:
            print('Warning: sys.control_box is still to be defined!')
        print('* control discretization steps:')
        for i in range(len(self.sys.control)):
            print('  - Δ{:s} = {:g}'.format(self.sys.control[i], self.control_steps[i]))
            if cdim is not None:
                lo_n, hi_n = cdim[:, i].min(), cdim[:, i].max()
                if lo_n != hi_n:
                    print(('    yields [{:,d} to {:,d}] possible values'
                           ' ({:,.1f} on average)').format(lo_n, hi_n, cdim[:, i].mean()))
                else:
                    print('    yields {:,d} possible values'.format(cdim[0, i]))
        if cdim is not None and len(self.sys.control) >= 2:
            tot = np.prod(cdim, axis=1)
            print('  control combinations:'
                  ' [{:,d} to {:,d}] possible values ({:,.1f} on average)'.format(
                      tot.min(), tot.max(), tot.mean()))


def plan_info(plan):
    """The entries of `backend_info` that the plan of `DPSolver._kernel_plan` decides alone (no GPU needed)."""
    model, unit, filtered = plan['model'], plan['unit'], bool(plan['filtered'])
    shifted = bool(unit is not None and unit.shift)
    return dict(
        kernel='column' if plan['column'] else ('staged' if plan['staged'] else
                                                ('lead' if plan['lead_axes'] else ('line' if plan['line'] else 'generic'))),
        controlled_axes=int(plan['lead_axes'] or (1 if plan['column'] else 0)),
        # state variables in the order the filter sees them (stocks first) when they are not listed first
        controlled_order=list(plan['lead_perm']) if plan['lead_perm'] else None,
        staged=plan['staged'],
        row_window=dict(rows=unit.window_rows, segment_nodes=unit.seg_nodes) if plan['window'] else None,
        table_per_control=bool(plan['per_control']),
        certified_filter=filtered,
        # 'shifted lattice': the perturbation reaches x0' through a final sum (SDP_COL_SHIFT; the line kernel)
        filter_form=(None if not filtered else
                     ('shifted lattice' if (shifted or plan['line']) else
                      ('reduced array' if plan['lead_axes'] else 'reduced table'))),
        # x0' = a chain of sums in another nesting than ((a +- b) +- ..), x + (w - u): regrouped for the first pass
        regrouped_sums=bool(filtered and shifted and codegen.shift_chain(model)),
        # the branch and bound's uniform evaluation stage (codegen.uniform_eval_plan): the rows its positions may lie from the
        # reference's -- what the radius pays for -- and the node's share of them that the kernel checks
        uniform_eval=(dict(delta_rows=unit.eval_delta, node_rows=unit.eval_dx, unit_axis=bool(unit.eval_unit_axis))
                      if (unit is not None and unit.eval_delta and unit.uniform) else None),
        lanes_per_node=plan['lanes'], max_controls=plan['max_u'], box_per_node=bool(plan['per_node']),
        # perturbation variables; 2 or more: kernel 'generic' is the family of csrc/sdp_multiw_kernel.h on their flat law
        n_perturb=int(model.n_perturb), perturb_vars=int(model.n_perturb))


def _params_key(params):
    """hashable, untruncated image of a params dict (repr() shortens large arrays); reals by their bits (0.0 == -0.0,
    yet np.copysign tells them apart)"""
    out = []
    for k in sorted(params):
        v = params[k]
        if isinstance(v, np.ndarray):
            out.append((k, v.dtype.str, v.shape, v.tobytes()))
        else:
            try:
                out.append((k, _fp_value(v, 0, [1 << 20])))
            except _NoFingerprint:
                try:
                    hash(v)
                    out.append((k, type(v).__name__, v))
                except TypeError:
                    out.append((k, repr(v)))
    return tuple(out)


def _dbg_key(debug):
    return tuple(sorted(debug.items())) if debug else ()


def _same(a, b):
    a, b = float(a), float(b)
    return a == b or (a != a and b != b)
