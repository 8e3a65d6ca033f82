#!/usr/bin/env python3
"""Ranking the sizings of a study without sampling noise, as one family: the storage + AR(1) problem over a range of
storage capacities.

examples/sizing_monte_carlo.py scores every capacity's policy by simulation: a mean with a standard error.  The
transition operator of a policy (examples/stationary.py does this for one problem) gives the same number exactly, up to
the discretisation the solver itself works on: the stationary state distribution mu* of the Markov chain on the grid
under the policy, and the average cost mu* . gbar.  Here every capacity is a member of a `SolverFamily`:
`policy_iteration` solves them together, `transition_operator` builds all their operators in one device call and
`stationary` iterates them together, each member stopping at its own push.  The table prints, per capacity, the
stationary average cost next to the relative-DP reference cost of the policy iteration and the Monte Carlo mean of
`fam.monte_carlo`, and how often the storage sits at its bounds under mu*; the loop of solo calls gives the same bits."""
import contextlib
import io
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from stodynprog_amd import SolverFamily, models


def members(capacities, **kw):
    return [models.storage_ar1(E_rated=float(E), **kw)[1] for E in capacities]


def main(capacities=np.linspace(2., 20., 10), n_traj=4096, n_steps=1000, n_burn=100, seed=0, tol=1e-6, verbose=True, **kw):
    kw.setdefault('steps', (0.1, 0.1))
    fam = SolverFamily(members(capacities, **kw))
    pol0 = np.zeros(fam.dims + (fam.nu,))                       # the idle policy, for every member
    (_, J_ref), pol = fam.policy_iteration(pol0, 1000, 8, rel_dp=True, tol=tol, check_every=10)
    t = time.perf_counter()
    op = fam.transition_operator(pol)
    res = op.stationary(tol=1e-12, n_max=5000, check_every=10)
    t_fam = time.perf_counter() - t
    info = dict(op.info)
    op.close()
    # the loop of solo calls: the same bits
    same = True
    t = time.perf_counter()
    for p, s in enumerate(members(capacities, **kw)):
        with contextlib.redirect_stdout(io.StringIO()):
            one = s.stationary_distribution(pol[p], tol=1e-12, n_max=5000, check_every=10)
        same = same and np.array_equal(res.mu[p], one.mu) and res[p].n_done == one.n_done \
            and res[p].average_cost == one.average_cost
    t_solo = time.perf_counter() - t
    # Monte Carlo from a half-full storage, for comparison
    x0 = np.stack([np.broadcast_to([0.5 * E, 0.], (n_traj, 2)) for E in capacities])
    mcr = fam.monte_carlo(pol, x0, n_steps, seed=seed, n_burn=n_burn)
    empty, full = res.mu[:, 0, :].sum(axis=1), res.mu[:, -1, :].sum(axis=1)       # the storage at its bounds
    if verbose:
        print('{:>8s} {:>18s} {:>18s} {:>26s} {:>7s} {:>9s} {:>9s}'.format(
            'E_rated', 'mu* . gbar', 'average cost (DP)', 'Monte Carlo mean +- stderr', 'pushes', 'P(empty)', 'P(full)'))
        for p, E in enumerate(capacities):
            print('{:8.3f} {:18.12g} {:18.12g} {:16.10g} +- {:<8.2g} {:6d}{} {:9.4f} {:9.4f}'.format(
                E, res.average_cost[p], J_ref[p], mcr.mean[p], mcr.stderr[p], int(res.n_done[p]),
                ' ' if res.converged[p] else '*', empty[p], full[p]))
        print('family: {:.3f} s ({} members, {} entries in {} chunk(s), build {:.2f} ms, pushes {:.2f} ms); solo loop: '
              '{:.3f} s; same bits: {}'.format(t_fam, fam.P, info['entries'], info['chunks'], info['build_ms'],
                                               info['push_ms'], t_solo, same))
    fam.close()
    assert same
    return dict(capacities=list(map(float, capacities)), stationary_cost=res.average_cost.tolist(),
                average_cost=[float(r) for r in J_ref], mean=mcr.mean.tolist(), stderr=mcr.stderr.tolist(),
                n_done=res.n_done.tolist(), converged=res.converged.tolist(), empty=empty.tolist(), full=full.tolist(),
                family_s=t_fam, solo_s=t_solo, same_bits=same)


if __name__ == '__main__':
    main()
