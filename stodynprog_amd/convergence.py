"""Convergence test of the sweep loops (DPSolver.value_iterations, eval_policy, policy_iteration with `tol`).

NOT in the reference API: its problems are average-cost (`rel_dp`) or finite-horizon ones, and its users judge
convergence by eye.  One definition serves every layer -- the device reduction of the library (k_diff_stats in
csrc/sdp_hip.hip, sdp_problem_vi_until / sdp_problem_eval_policy_until) gives the bits of `diff_stats` below, and
the loops that hold full host arrays every sweep (host communicator, tabulated callables) call it directly.

Two consecutive cost-to-go arrays a = J^(k), b = J^(k-1) of the loop's sequence (with rel_dp both shifted,
J - J[ref], as the loop returns them; J^(0) is the caller's starting array):

    d = 0                       where a == b   (equal infinities included)
    d = a - b rounded in the problem's real type, otherwise (NaN if either is NaN)

dmin = min d, dmax = max d as float64, both NaN if any d is.  The loop stops after the first checked sweep with
span = dmax - dmin <= tol (float64; NaN never converges) -- the standard rule of undiscounted value iteration: the
span goes to zero with or without rel_dp, where the sup-norm without it grows by the average cost every sweep.

Average-cost (Odoni) bounds: lower = dmin + ref_k, upper = dmax + ref_k with rel_dp (ref_k: the reference cost of
sweep k), dmin and dmax without it.  In exact arithmetic they bracket the optimal average cost per stage (or the
policy's, in eval_policy) of a unichain, aperiodic problem; in floating point, up to the rounding of the sweeps.
"""
import math

import numpy as np

__all__ = ['diff_stats', 'converged', 'check_schedule', 'is_check', 'validate', 'SweepConvergence',
           'PolicyIterationConvergence']


def diff_stats(a, b, dtype=None):
    """(dmin, dmax) of d = a - b (0 where a == b) rounded in `dtype` (default: a's real type), as floats;
    (nan, nan) if any d is NaN.  Never -0.0: a - b is zero only where a == b."""
    a = np.asarray(a)
    dt = np.dtype(dtype) if dtype is not None else (a.dtype if a.dtype.kind == 'f' else np.dtype(np.float64))
    a = a.astype(dt, copy=False)
    b = np.asarray(b).astype(dt, copy=False)
    with np.errstate(invalid='ignore', over='ignore'):
        d = np.where(a == b, dt.type(0), a - b)
    if np.isnan(d).any():
        return float('nan'), float('nan')
    return float(d.min()), float(d.max())


def converged(dmin, dmax, tol):
    """the stopping rule: span = dmax - dmin <= tol, in float64 (False for NaN)"""
    return float(dmax) - float(dmin) <= tol


def is_check(k, n_iter, check_every):
    """is sweep k (1-based) of a loop of at most n_iter sweeps a checked one?"""
    return k % check_every == 0 or k == n_iter


def check_schedule(n_iter, check_every):
    """the checked sweeps of a loop of at most n_iter sweeps: check_every, 2 check_every, ... and n_iter"""
    return [k for k in range(1, n_iter + 1) if is_check(k, n_iter, check_every)]


def validate(tol, check_every):
    """ValueError for a tolerance that is negative or NaN, or a check interval below 1 (before any device call)"""
    try:
        t = float(tol)
    except (TypeError, ValueError):
        raise ValueError('tol must be a number >= 0, not {!r}'.format(tol))
    if math.isnan(t) or t < 0:
        raise ValueError('tol must be a number >= 0, not {!r}'.format(tol))
    if isinstance(check_every, bool) or not isinstance(check_every, (int, np.integer)) or check_every < 1:
        raise ValueError('check_every must be an integer >= 1, not {!r}'.format(check_every))
    return t, int(check_every)


class SweepConvergence(object):
    """What one sweep loop run with `tol` did (DPSolver.last_convergence): n_iter sweeps done, whether the last
    check met the tolerance, and per checked sweep (`checked`, 1-based) dmin, dmax, span and the average-cost
    bounds lower / upper (numpy arrays)."""

    def __init__(self, tol, check_every, n_iter, checked, dmin, dmax, refs=None):
        self.tol = float(tol)
        self.check_every = int(check_every)
        self.n_iter = int(n_iter)
        self.checked = [int(k) for k in checked]
        self.dmin = np.asarray(dmin, dtype=np.float64).reshape(-1)
        self.dmax = np.asarray(dmax, dtype=np.float64).reshape(-1)
        self.span = self.dmax - self.dmin
        ref = np.zeros(len(self.checked)) if refs is None else np.asarray(refs, dtype=np.float64).reshape(-1)
        self.lower = self.dmin + ref
        self.upper = self.dmax + ref
        self.converged = bool(len(self.checked)) and converged(self.dmin[-1], self.dmax[-1], self.tol)

    def __repr__(self):
        last = ', span {:.3g}'.format(self.span[-1]) if len(self.span) else ''
        return 'SweepConvergence(n_iter={}, converged={}, tol={:g}, check_every={}{})'.format(
            self.n_iter, self.converged, self.tol, self.check_every, last)


class PolicyIterationConvergence(object):
    """What DPSolver.policy_iteration with `tol` did: one SweepConvergence per policy evaluation, the number of
    improvement steps, and whether the last one returned exactly the policy it was given"""

    def __init__(self, evaluations, n_improvements, stable):
        self.evaluations = list(evaluations)
        self.n_improvements = int(n_improvements)
        self.stable = bool(stable)

    def __repr__(self):
        return 'PolicyIterationConvergence(evaluations={}, n_improvements={}, stable={})'.format(
            len(self.evaluations), self.n_improvements, self.stable)
