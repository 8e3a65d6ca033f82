#!/usr/bin/env python3
"""The stationary distribution of the state under a policy, without sampling: the forward half of the model the DP
solves.  `transition_operator(pol)` holds the Markov chain that `eval_policy(pol, ..)` implies -- next states
interpolated on the grid, the discretised perturbation law -- as a sparse operator on the device, and
`stationary()` iterates mu <- P^T mu to a fixed point.

The SEAREV storage policy comes from policy_iteration.  Three figures for its average cost per step are printed side
by side: the relative-DP reference cost (the DP's own, with its Odoni bounds), mu* . gbar from the stationary
distribution of the same chain (it must lie within those bounds up to the tolerances: same model, no noise), and the
Monte Carlo mean +- standard error of the continuous-state closed loop (another object: it carries no interpolation of
the value function, and O(1 / sqrt(N)) noise).  Where the model leaves the grid the operator extrapolates like the
reference's interpolation does, so a few entries of mu* may be slightly negative; they are counted."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from stodynprog_amd import models


def main(n_val=200, n_pol=2, grid=(31, 61, 61), n_traj=16384, n_steps=4000, n_burn=1000, verbose=True):
    wec, dpsolv = models.searev(n_E=grid[0], n_S=grid[1], n_A=grid[2])
    (J, r), pol = dpsolv.policy_iteration(models.searev_linear_policy(dpsolv), n_val, n_pol, rel_dp=True)
    dpsolv.eval_policy(pol, 2000, rel_dp=True, tol=1e-9, check_every=10, report_time=False)
    conv = dpsolv.last_convergence
    t = time.perf_counter()
    op = dpsolv.transition_operator(pol)
    rec = op.stationary(tol=1e-12, n_max=20000, check_every=10)
    dt = time.perf_counter() - t
    info = dict(op.info)
    op.close()
    mc = dpsolv.monte_carlo(pol, (models.SEAREV['E_rated'] / 3, 0., 0.), n_steps, seed=0, n_burn=n_burn, n_traj=n_traj)
    if verbose:
        print('operator: {:d} entries, {:.1f} MB, built in {:.2f} ms ({:.2f} ms entries + {:.2f} ms sort)'.format(
            info['nnz'], info['bytes'] / 1e6, info['build_ms'], info['entries_ms'], info['sort_ms']))
        print('stationary distribution: {:d} pushes in {:.2f} s, converged {}, delta {:.2e}, mass {:.12f}, '
              '{:d} negative entries (smallest {:.2e})'.format(rec.n_done, dt, rec.converged, rec.delta, float(rec.mass),
                                                               int((rec.mu < 0).sum()), float(rec.mu.min())))
        print('average cost per step')
        print('  relative DP (eval_policy, Odoni bounds):  [{:.9f}, {:.9f}]'.format(conv.lower[-1], conv.upper[-1]))
        print('  mu* . gbar (stationary distribution):      {:.9f}'.format(rec.average_cost))
        print('  Monte Carlo, {:d} x {:d} steps:          {:.6f} +- {:.6f}'.format(n_traj, n_steps - n_burn, mc.mean, mc.stderr))
        share = rec.mu.sum(axis=(1, 2))
        print('share of time per stored-energy node: ' + ' '.join('{:.3f}'.format(v) for v in share))
    return dict(J_ref=r, lower=conv.lower[-1], upper=conv.upper[-1], stationary=rec, monte_carlo=mc)


if __name__ == '__main__':
    main()
