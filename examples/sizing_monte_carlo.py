#!/usr/bin/env python3
"""Scoring the policies of a sizing study in closed loop, as one family: the storage + AR(1) problem over a range of
storage capacities.

The study does not end with the policies: each sizing's policy is then simulated and its cost averaged, as
examples/monte_carlo.py does for one problem (and the reference's Searev performance script, a loop of simulations
over its data files).  Here every capacity is a member of a `SolverFamily`: `policy_iteration` solves them together
and `monte_carlo` runs all their trajectories in one device call.  With one seed every member sees the same uniform
draws -- common random numbers -- so the difference between two neighbouring sizings is a PAIRED difference: its
standard error (`res.paired(p, p + 1)`) is printed next to the one two independent runs would have.  The relative-DP
average cost of every capacity stands next to its Monte Carlo mean, and the loop of solo calls gives the same bits."""
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
    # every member starts half full, without a mismatch
    x0 = np.stack([np.broadcast_to([0.5 * E, 0.], (n_traj, 2)) for E in capacities])
    t = time.perf_counter()
    res = fam.monte_carlo(pol, x0, n_steps, seed=seed, n_burn=n_burn)
    t_fam = time.perf_counter() - t
    same = True
    t = time.perf_counter()
    for p, s in enumerate(members(capacities, **kw)):
        with contextlib.redirect_stdout(io.StringIO()):
            one = s.monte_carlo(pol[p], x0[p], n_steps, seed=seed, n_burn=n_burn)
        same = same and all(np.array_equal(getattr(res[p], name), getattr(one, name))
                            for name in ('cost_sum', 'cost_mean', 'n_outside', 'x_final')) \
            and res[p].mean == one.mean and res[p].stderr == one.stderr
    t_solo = time.perf_counter() - t
    paired = [res.paired(p, p + 1) for p in range(fam.P - 1)]
    if verbose:
        print('{:>8s} {:>20s} {:>26s} {:>9s}'.format('E_rated', 'average cost (DP)', 'Monte Carlo mean +- stderr', 'outside'))
        for p, E in enumerate(capacities):
            print('{:8.3f} {:20.12g} {:16.10g} +- {:<8.2g} {:9d}'.format(E, J_ref[p], res.mean[p], res.stderr[p],
                                                                        int(res.n_outside[p].sum())))
        print('{:>19s} {:>28s} {:>18s}'.format('E_rated', 'paired difference +- stderr', 'unpaired stderr'))
        for p, (mean, stderr) in enumerate(paired):
            print('{:8.3f} - {:<8.3f} {:16.10g} +- {:<9.2g} {:18.2g}'.format(
                capacities[p], capacities[p + 1], mean, stderr, float(np.hypot(res.stderr[p], res.stderr[p + 1]))))
        print('family: {:.3f} s ({} members, {} trajectories of {} steps each, {} launch(es)); solo loop: {:.3f} s; '
              'same bits: {}'.format(t_fam, fam.P, n_traj, n_steps, fam.backend_info['monte_carlo']['launches'], t_solo, same))
    assert same
    return dict(capacities=list(map(float, capacities)), average_cost=[float(r) for r in J_ref], mean=res.mean.tolist(),
                stderr=res.stderr.tolist(), paired=paired, family_s=t_fam, solo_s=t_solo, same_bits=same)


if __name__ == '__main__':
    main()
