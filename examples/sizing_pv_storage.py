#!/usr/bin/env python3
"""Sizing the storage of a PV plant over a finite horizon, as one family: the deterministic PV-storage problem of
examples/pv_storage.py (the reference's `det/` example) over a range of storage capacities.

Every capacity is a member of a `SolverFamily`.  `bellman_recursion` runs the backward pass of all of them together, one
family launch per step, and returns a time-indexed policy per member; `simulate` then runs those policies forward from an
empty store in one device call: step k looks its control up in pol[p, k] and evaluates the member's model with the
production data of step k.  The cost of the day per capacity stands next to what the loop of solo `simulate` calls gives
-- the same bits -- and to the cost-to-go the backward pass computed for that start, with both wall times."""
import contextlib
import io
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from stodynprog_amd import SolverFamily, models


def members(capacities, **kw):
    return [models.pv_storage(E_rated=float(E), **kw)[1] for E in capacities]


def main(capacities=np.linspace(1., 4., 64), T=48, verbose=True, **kw):
    fam = SolverFamily(members(capacities, T=T, **kw))
    J, pol = fam.bellman_recursion(T, np.zeros(fam.dims))
    x0 = np.zeros(1)                                            # every member starts with an empty store
    t = time.perf_counter()
    x, u, g = fam.simulate(pol, x0, n_steps=T)                  # (P, T+1, 1), (P, T, 1), (P, T)
    t_fam = time.perf_counter() - t
    cost = np.zeros(fam.P)
    for k in range(T):
        cost = cost + g[:, k]
    same = True
    solo_cost = np.zeros(fam.P)
    t = time.perf_counter()
    for p, s in enumerate(members(capacities, T=T, **kw)):
        with contextlib.redirect_stdout(io.StringIO()):
            x1, u1, g1 = s.simulate(pol[p], x0, n_steps=T)
        same = same and np.array_equal(x1, x[p]) and np.array_equal(u1, u[p]) and np.array_equal(g1, g[p])
        for k in range(T):
            solo_cost[p] = solo_cost[p] + g1[k]
    t_solo = time.perf_counter() - t
    if verbose:
        print('{:>8s} {:>22s} {:>22s} {:>14s} {:>12s}'.format('E_rated', 'cost of the day', 'by the solo loop', 'J[0] at E = 0',
                                                              'fullest store'))
        for p, E in enumerate(capacities):
            print('{:8.3f} {:22.15g} {:22.15g} {:14.8g} {:12.6g}'.format(E, cost[p], solo_cost[p], J[p, 0, 0], x[p].max()))
        print('family: {:.3f} s ({} members, {} steps, {} launch(es)); solo loop: {:.3f} s; same bits: {}'.format(
            t_fam, fam.P, T, fam.backend_info['horizon']['launches'], t_solo, same))
    assert same
    return dict(capacities=list(map(float, capacities)), cost=cost.tolist(), solo_cost=solo_cost.tolist(),
                cost_to_go=J[:, 0, 0].tolist(), family_s=t_fam, solo_s=t_solo, same_bits=same)


if __name__ == '__main__':
    main()
