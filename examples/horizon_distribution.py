"""The forward pass of a finite-horizon problem without sampling noise: `DPSolver.horizon_operator` builds the transition
operators of all steps of the horizon in one device call, `propagate` pushes state distributions through them.

Two problems are solved backward with `bellman_recursion` and then run forward under the policy it returns:

  models.finite_horizon   one state, dynamics, cost and admissible controls all depend on the time index; stochastic
  models.pv_storage       a storage smoothing a PV plant over 48 half-hours, the production looked up as data[k];
                          deterministic

each from a point mass and from the uniform distribution on the grid.  Per step the mass, the mean state and the expected
cost are printed, and at the end `total_cost` next to <mu0, J[0]> of the backward pass -- the two agree to rounding, since
the chain is the exact adjoint of the backward recursion (stodynprog_amd/forward.py) -- and, for the stochastic problem,
next to the Monte Carlo mean +- standard error of the closed loop under the same policy.  The closed loop carries sampling
noise and runs off the nodes, where the chain interpolates: the two agree as far as the grid is fine.

    python examples/horizon_distribution.py
"""
import contextlib
import io
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from stodynprog_amd import models           # noqa: E402


def quiet(f, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return f(*a, **kw)


def forward_pass(name, solver, T, n_traj=0):
    dims = tuple(len(g) for g in solver.state_grid)
    x = np.asarray(solver.state_grid[0], dtype=float)
    J_fin = np.zeros(dims)
    J, pol = quiet(solver.bellman_recursion, T, J_fin)
    node = dims[0] // 3
    point = np.zeros(dims)
    point[node] = 1.0
    uniform = np.full(dims, 1.0 / dims[0])
    op = solver.horizon_operator(pol)
    res = op.propagate(np.stack([point, uniform]), J_fin)
    info = solver.backend_info['horizon_operator']
    op.close()
    print('{}: {} nodes, {} steps, {} entries; {} path, build {:.3f} ms (entries {:.3f}, sort {:.3f}), propagate {:.3f} ms'.format(
        name, dims[0], T, info['nnz'], info['path'], info['entries_ms'] + info['sort_ms'], info['entries_ms'], info['sort_ms'],
        info['push_ms']))
    for b, start in enumerate(('point mass at x = {:.3f}'.format(x[node]), 'uniform start')):
        print('  ' + start)
        print('    step      mass   mean state   expected cost')
        for k in range(0, T, max(1, T // 12)):
            print('    {:4d}  {:8.5f}  {:11.5f}  {:14.6f}'.format(k, res.mass[k, b], res.mu[k, b] @ x, res.step_cost[k, b]))
        print('    {:4d}  {:8.5f}  {:11.5f}'.format(T, res.mass[T, b], res.mu[T, b] @ x))
        backward = float((point, uniform)[b].ravel() @ J[0].ravel())
        print('    total_cost = {:.12f}   <mu0, J[0]> = {:.12f}   difference {:.2e}'.format(
            res.total_cost[b], backward, res.total_cost[b] - backward))
        if n_traj:
            if b == 0:
                x0 = np.full((n_traj, 1), x[node])
            else:
                x0 = np.repeat(x, n_traj // dims[0]).reshape(-1, 1)
            mcr = solver.monte_carlo(pol, x0, T, seed=7)
            mean = float(mcr.cost_sum.mean())                       # (of the trajectories' totals over the T steps)
            stderr = float(mcr.cost_sum.std(ddof=1) / np.sqrt(len(x0)))
            print('    Monte Carlo, {} trajectories: {:.6f} +- {:.6f}   (total_cost - mean) / stderr = {:+.2f}'.format(
                len(x0), mean, stderr, (res.total_cost[b] - mean) / stderr))


def main():
    # (a fine grid: the chain is exact for the problem ON THE GRID, the closed loop runs off the nodes; what is left between
    # them is the interpolation of a convex cost, of the order of the square of the grid step)
    forward_pass('finite horizon', models.finite_horizon(n_x=2049)[1], 12, n_traj=2049 * 128)
    forward_pass('PV storage', models.pv_storage()[1], 48)


if __name__ == '__main__':
    main()
