#!/usr/bin/env python3
"""Ranking the sizings of a study under the controller that would run: the storage + AR(1) problem over a range of
storage capacities, every capacity scored twice with the same draws.

examples/sizing_monte_carlo.py scores each sizing's TABULATED policy, interpolated between the nodes of the grid.
Online control is not run that way: at the state the plant is in, the controller minimises the one-step lookahead
against the cost-to-go over the controls admissible THERE (examples/lookahead_monte_carlo.py, for one problem).  The
members of a sizing study differ in the very constants of `control_box`, so the two scores differ most where the
sizing matters.  Here every capacity is a member of a `SolverFamily`: `value_iterations` solves them together,
`monte_carlo` scores the tabulated policies and `monte_carlo_lookahead` the lookahead controller, each in one device
call, with one seed: every member sees the same uniform draws under both controllers.  Printed: both means per
capacity with the paired difference between the two controllers, and the paired differences between neighbouring
capacities under lookahead.  The first and the last member are run alone as well and give the same bits.

The capacities avoid E_rated == P_rated (4.0) and E_rated == dt (1.0): equal constants of control_box are one node of
its trace, and such a member's box is another structure (the family refuses it with a ValueError that says so)."""
import contextlib
import io
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from stodynprog_amd import SolverFamily, models

CAPACITIES = np.linspace(3., 21., 10)


def members(capacities, **kw):
    return [models.storage_ar1(E_rated=float(E), **kw)[1] for E in capacities]


def main(capacities=CAPACITIES, n_traj=1024, n_steps=300, n_burn=50, seed=0, tol=1e-6, verbose=True, **kw):
    kw.setdefault('steps', (0.1, 0.1))
    fam = SolverFamily(members(capacities, **kw))
    zero = np.zeros(fam.dims)
    (J, J_ref), pol = fam.value_iterations((zero, 0.), 2000, rel_dp=True, tol=tol, check_every=10)
    # every member starts half full, without a mismatch
    x0 = np.stack([np.broadcast_to([0.5 * E, 0.], (n_traj, 2)) for E in capacities])
    tab = fam.monte_carlo(pol, x0, n_steps, seed=seed, n_burn=n_burn)
    t = time.perf_counter()
    look = fam.monte_carlo_lookahead(J, x0, n_steps, seed=seed, n_burn=n_burn)
    t_fam = time.perf_counter() - t
    launches = fam.backend_info['monte_carlo']['launches']
    same = True
    solo = members(capacities, **kw)
    for p in (0, fam.P - 1):
        with contextlib.redirect_stdout(io.StringIO()):
            one = solo[p].monte_carlo_lookahead(J[p], x0[p], n_steps, seed=seed, n_burn=n_burn)
        same = same and one.path == 'device' and one.mean == look[p].mean and one.stderr == look[p].stderr and all(
            np.array_equal(getattr(look[p], name), getattr(one, name)) for name in ('cost_sum', 'n_outside', 'x_final'))
    # the same draws under both controllers: the difference of a member's two scores is a paired one
    gap = tab.cost_mean - look.cost_mean                                    # (P, n_traj)
    gap_mean, gap_err = gap.mean(axis=1), gap.std(axis=1, ddof=1) / np.sqrt(n_traj)
    paired = [look.paired(p, p + 1) for p in range(fam.P - 1)]
    if verbose:
        print('{:>8s} {:>18s} {:>24s} {:>24s} {:>24s}'.format('E_rated', 'average cost (DP)', 'tabulated policy', 'lookahead',
                                                              'tabulated - lookahead'))
        for p, E in enumerate(capacities):
            print('{:8.3f} {:18.10g} {:14.8g} +- {:<7.2g} {:14.8g} +- {:<7.2g} {:14.8g} +- {:<7.2g}'.format(
                E, J_ref[p], tab.mean[p], tab.stderr[p], look.mean[p], look.stderr[p], gap_mean[p], gap_err[p]))
        print('{:>19s} {:>36s} {:>18s}'.format('E_rated', 'lookahead: paired difference +- stderr', 'unpaired stderr'))
        for p, (mean, stderr) in enumerate(paired):
            print('{:8.3f} - {:<8.3f} {:24.10g} +- {:<9.2g} {:18.2g}'.format(
                capacities[p], capacities[p + 1], mean, stderr, float(np.hypot(look.stderr[p], look.stderr[p + 1]))))
        print('lookahead, family: {:.3f} s ({} members, {} trajectories of {} steps each, {} launch(es)); members 0 and {} '
              'alone: same bits: {}'.format(t_fam, fam.P, n_traj, n_steps, launches, fam.P - 1, same))
    assert same
    fam.close()
    return dict(capacities=list(map(float, capacities)), average_cost=[float(r) for r in J_ref], tabulated=tab.mean.tolist(),
                lookahead=look.mean.tolist(), gap=gap_mean.tolist(), gap_stderr=gap_err.tolist(), paired=paired,
                family_s=t_fam, same_bits=same)


if __name__ == '__main__':
    main()
