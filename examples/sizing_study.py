#!/usr/bin/env python3
"""A sizing study as one device call: the storage + AR(1) problem over a range of storage capacities.

The reference's studies are loops over small problems (examples/01 Deterministic storage control/det_storage_perf.py:
11 capacities x 50 inputs; the AR(1) and Searev notebooks sweep E_rated, P_rated and the correlation).  Here every
capacity is a member of a `SolverFamily`: relative value iteration runs to a tolerance for all of them together, a
member leaves the launches when its own span is below `tol`.  The average cost per stage of every capacity (the
relative-DP reference cost of its last sweep) is printed next to what the loop of solo calls gives: the same bits."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from stodynprog_amd import SolverFamily, models


def members(capacities, **kw):
    return [models.storage_ar1(E_rated=float(E), **kw)[1] for E in capacities]


def main(capacities=np.linspace(2., 20., 10), n_iter=500, tol=1e-6, check_every=10, verbose=True, **kw):
    fam = SolverFamily(members(capacities, **kw))
    J0 = np.zeros(fam.dims)
    t = time.perf_counter()
    (J, J_ref), pol = fam.value_iterations((J0, 0.), n_iter, rel_dp=True, tol=tol, check_every=check_every)
    t_fam = time.perf_counter() - t
    records = fam.last_convergence
    solo_ref, same = [], True
    t = time.perf_counter()
    for p, s in enumerate(members(capacities, **kw)):
        (Jp, rp), polp = s.value_iterations((J0, 0.), n_iter, rel_dp=True, report_time=False, tol=tol, check_every=check_every)
        solo_ref.append(rp)
        same = same and np.array_equal(J[p], Jp) and np.array_equal(pol[p], polp) and J_ref[p] == rp \
            and s.last_convergence.n_iter == records[p].n_iter
    t_solo = time.perf_counter() - t
    if verbose:
        print('{:>8s} {:>7s} {:>22s} {:>22s}'.format('E_rated', 'sweeps', 'average cost (family)', 'average cost (solo)'))
        for E, r, a, b in zip(capacities, records, J_ref, solo_ref):
            print('{:8.3f} {:7d} {:22.15g} {:22.15g}'.format(E, r.n_iter, a, b))
        print('family: {:.3f} s in one call ({} members, {} lanes); solo loop: {:.3f} s; same bits: {}'.format(
            t_fam, fam.P, fam.backend_info['lanes'], t_solo, same))
    assert same
    return dict(capacities=list(map(float, capacities)), average_cost=[float(r) for r in J_ref],
                sweeps=[r.n_iter for r in records], family_s=t_fam, solo_s=t_solo, same_bits=same)


if __name__ == '__main__':
    main()
