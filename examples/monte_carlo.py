#!/usr/bin/env python3
"""Monte Carlo evaluation of a policy on the device: the last step of the reference's workflow
(examples/20 Searev storage control/storage_control.py:197-265 draws a perturbation sequence, runs the
closed loop and prints cost.mean()), for a whole batch of trajectories with the draws and the sums on the GPU.

The SEAREV storage policy comes from policy_iteration; its relative-DP reference cost (the average cost per
step the DP itself reports) is printed next to the Monte Carlo mean +- standard error.  The two are NOT
asserted equal: the DP's figure carries the interpolation error of the value function on the grid."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from stodynprog_amd import models


def main(n_val=200, n_pol=2, n_traj=16384, n_steps=4000, n_burn=1000, grid=(31, 61, 61), seed=0, verbose=True):
    wec, dpsolv = models.searev(n_E=grid[0], n_S=grid[1], n_A=grid[2])
    (J, r), pol = dpsolv.policy_iteration(models.searev_linear_policy(dpsolv), n_val, n_pol, rel_dp=True)
    x0 = (models.SEAREV['E_rated'] / 3, 0., 0.)
    t = time.perf_counter()
    res = dpsolv.monte_carlo(pol, x0, n_steps, seed=seed, n_burn=n_burn, n_traj=n_traj, occupancy=True)
    dt = time.perf_counter() - t
    if verbose:
        print('relative-DP reference cost of the policy (eval_policy): {:.6f}'.format(r))
        print('Monte Carlo, {:d} trajectories x {:d} steps ({:d} burn-in) in {:.2f} s: {:.6f} +- {:.6f}'.format(
            n_traj, n_steps, n_burn, dt, res.mean, res.stderr))
        print('steps outside the state grid: {:d} of {:d}'.format(int(res.n_outside.sum()),
                                                                  n_traj * (n_steps - n_burn)))
        occ = res.occupancy.sum(axis=(1, 2)) / float(res.occupancy.sum())
        print('share of time per stored-energy node: ' + ' '.join('{:.3f}'.format(v) for v in occ))
        # the same run is a function of (seed, trajectory id, step): half the batch, bit for bit
        half = dpsolv.monte_carlo(pol, x0, n_steps, seed=seed, n_burn=n_burn, n_traj=n_traj // 2)
        print('first half of the batch on its own: {} the same sums'.format(
            'exactly' if np.array_equal(half.cost_sum, res.cost_sum[:n_traj // 2]) else 'NOT'))
    return dict(J_ref=r, mean=res.mean, stderr=res.stderr, result=res)


if __name__ == '__main__':
    main()
