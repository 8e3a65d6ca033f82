#!/usr/bin/env python3
"""Online control by one-step lookahead, next to the interpolated policy: the SEAREV storage problem.

The reference's closed loop (examples/20 Searev storage control/storage_control.py:242-251) interpolates the
tabulated policy between grid nodes.  The admissible box of the storage power depends on the energy left, so a
control interpolated between two nodes' optima need not be admissible at the state in between.  `simulate_lookahead`
instead takes, at the state the plant is in, argmin_u E[cost + J(next state)] over the box of THAT state, from the same
cost-to-go J.  Both loops run on the same draws (`monte_carlo_draws`); the mean cost per step of each is printed, and
the steps at which the interpolated control lies outside the box at the state are counted."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from stodynprog_amd import models


def main(n_val=200, n_pol=2, n_traj=4096, n_steps=600, n_burn=100, grid=(31, 61, 61), seed=0, verbose=True):
    wec, dpsolv = models.searev(n_E=grid[0], n_S=grid[1], n_A=grid[2])
    (J, r), pol = dpsolv.policy_iteration(models.searev_linear_policy(dpsolv), n_val, n_pol, rel_dp=True)
    x0 = np.tile((models.SEAREV['E_rated'] / 3, 0., 0.), (n_traj, 1))
    _, w = dpsolv.monte_carlo_draws(seed, n_traj, n_steps)
    t = time.perf_counter()
    x_i, u_i, g_i = dpsolv.simulate(pol, x0, w)
    t_i = time.perf_counter() - t
    t = time.perf_counter()
    x_l, u_l, g_l, q_l = dpsolv.simulate_lookahead(J, x0, w)
    t_l = time.perf_counter() - t
    path = dpsolv.backend_info['lookahead_path']
    # the box at the states the interpolated policy visited (wec_box of models.searev, on arrays)
    k = models.SEAREV
    E = x_i[:-1, :, 0]
    lo = np.maximum(-E / (1 + k['a']) / k['dt'], -k['P_rated'])
    hi = np.minimum((k['E_rated'] - E) / (1 - k['a']) / k['dt'], k['P_rated'])
    outside = int(((u_i[..., 0] < lo) | (u_i[..., 0] > hi)).sum())
    mean_i, mean_l = float(g_i[n_burn:].mean()), float(g_l[n_burn:].mean())
    if verbose:
        print('relative-DP reference cost of the policy: {:.6f}'.format(r))
        print('{:d} trajectories x {:d} steps ({:d} burn-in), the same draws:'.format(n_traj, n_steps, n_burn))
        print('  interpolated policy: mean cost {:.6f} per step ({:.2f} s); control outside the box at the state in '
              '{:d} of {:d} steps'.format(mean_i, t_i, outside, n_traj * n_steps))
        print('  one-step lookahead : mean cost {:.6f} per step ({:.2f} s, {} path)'.format(mean_l, t_l, path))
    return dict(J_ref=r, mean_interpolated=mean_i, mean_lookahead=mean_l, outside=outside, path=path)


if __name__ == '__main__':
    main()
