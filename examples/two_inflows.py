#!/usr/bin/env python3
"""Two reservoirs with an inflow innovation each: a system of SEVERAL perturbation variables, which the
reference's interface accepts (`SysDescription((3, 2, 2))`, two laws, `discretize_perturb` with six arguments)
and its sweep does not run (stodynprog.py:666, `# TODO : implement nD perturbation`).

Relative value iteration to a tolerance on the device, then a Monte Carlo evaluation of the policy it returns
with ONE draw per step from the flat product law (stodynprog_amd/perturb.py).  The relative-DP reference cost
and the Monte Carlo mean are printed next to each other and NOT asserted equal: the DP's figure carries the
interpolation error of the value function on the grid."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from stodynprog_amd import models


def main(grid=(24, 24, 12), n_w=(5, 5), n_iter=300, tol=1e-6, n_traj=4096, n_steps=2000, n_burn=500, seed=0,
         verbose=True):
    sysd, dpsolv = models.two_inflows(n_a=grid[0], n_b=grid[1], n_y=grid[2], n_w=n_w)
    if verbose:
        dpsolv.print_summary()
    J0 = np.zeros(grid)
    t = time.perf_counter()
    (J, refs), pol = dpsolv.value_iterations((J0, 0.), n_iter, rel_dp=True, tol=tol, report_time=False)
    t_vi = time.perf_counter() - t
    conv = dpsolv.last_convergence
    x0 = (1.0, 1.0, 0.3)
    t = time.perf_counter()
    res = dpsolv.monte_carlo(pol, x0, n_steps, seed=seed, n_burn=n_burn, n_traj=n_traj)
    t_mc = time.perf_counter() - t
    if verbose:
        info = dpsolv.backend_info
        print('kernel: {} on {} perturbation variables, {} lanes per node'.format(
            info['kernel'], info['perturb_vars'], info['lanes_per_node']))
        print('relative value iteration: {} sweeps in {:.2f} s, reference cost {:.6f}'.format(conv.n_iter, t_vi, refs))
        print('Monte Carlo, {:d} trajectories x {:d} steps ({:d} burn-in) in {:.2f} s: {:.6f} +- {:.6f}'.format(
            n_traj, n_steps, n_burn, t_mc, res.mean, res.stderr))
        print('steps outside the state grid: {:d} of {:d}'.format(int(res.n_outside.sum()), n_traj * (n_steps - n_burn)))
    return dict(J_ref=refs, mean=res.mean, stderr=res.stderr, sweeps=conv.n_iter, result=res)


if __name__ == '__main__':
    main()
