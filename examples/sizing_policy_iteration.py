#!/usr/bin/env python3
"""Policy iteration of a sizing study as one family: the storage + AR(1) problem over a range of storage capacities.

Policy iteration is how the reference solves its flagship case (examples/20 Searev storage control: evaluate a policy
for hundreds of steps, improve it, repeat).  Here every capacity is a member of a `SolverFamily`: every evaluation runs
to a tolerance for all members together -- a member of this size lives in the LDS of one workgroup for the whole
evaluation --, the improvement is one family sweep, and a member whose improvement returns the policy it was given
leaves the rounds.  The average cost per stage of every capacity (the reference cost of its last evaluation) is printed
next to what the loop of solo calls gives: the same bits."""
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


def main(capacities=np.linspace(2., 20., 10), n_val=500, n_pol=8, tol=1e-6, check_every=10, verbose=True, **kw):
    kw.setdefault('steps', (0.1, 0.1))
    fam = SolverFamily(members(capacities, **kw))
    pol0 = np.zeros(fam.dims + (fam.nu,))                       # the idle policy, for every member
    t = time.perf_counter()
    (J, J_ref), pol = fam.policy_iteration(pol0, n_val, n_pol, rel_dp=True, tol=tol, check_every=check_every)
    t_fam = time.perf_counter() - t
    records = fam.last_convergence
    solo_ref, same = [], True
    t = time.perf_counter()
    for p, s in enumerate(members(capacities, **kw)):
        with contextlib.redirect_stdout(io.StringIO()):         # (the solo progress lines)
            (Jp, rp), polp = s.policy_iteration(pol0, n_val, n_pol, rel_dp=True, tol=tol, check_every=check_every)
        solo_ref.append(rp)
        same = same and np.array_equal(J[p], Jp) and np.array_equal(pol[p], polp) and J_ref[p] == rp \
            and s.last_convergence.n_improvements == records[p].n_improvements
    t_solo = time.perf_counter() - t
    if verbose:
        print('{:>8s} {:>12s} {:>7s} {:>22s} {:>22s}'.format('E_rated', 'improvements', 'stable', 'average cost (family)',
                                                            'average cost (solo)'))
        for E, r, a, b in zip(capacities, records, J_ref, solo_ref):
            print('{:8.3f} {:12d} {:>7s} {:22.15g} {:22.15g}'.format(E, r.n_improvements, str(r.stable), a, b))
        print('family: {:.3f} s ({} members, evaluation {}); solo loop: {:.3f} s; same bits: {}'.format(
            t_fam, fam.P, fam.backend_info['evaluation'], t_solo, same))
    assert same
    return dict(capacities=list(map(float, capacities)), average_cost=[float(r) for r in J_ref],
                improvements=[r.n_improvements for r in records], family_s=t_fam, solo_s=t_solo, same_bits=same)


if __name__ == '__main__':
    main()
