#!/usr/bin/env python3
"""Sizing the storage of a PV plant under the controller that would run: the study of examples/sizing_pv_storage.py
scored under one-step LOOKAHEAD controls.

Every capacity is a member of a `SolverFamily`.  `bellman_recursion` runs the backward pass of all of them once and
returns, per member, a time-indexed cost-to-go and a time-indexed policy.  The forward pass then runs twice from the same
start states, each in one device call: under the tabulated policy (`simulate`: step k interpolates pol[p, k] between the
nodes of the state grid) and under lookahead (`simulate_lookahead`: step k minimises cost + J[p, k + 1] over the
admissible controls AT the state the store is in, with the production data of step k).  The costs of the day per capacity
stand side by side.

The capacities avoid every other constant of the members' control_box (P_rated = 1, 1 +- loss, dt): a member whose
capacity coincides with one of them traces its box with another structure and cannot share the family's box function."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from stodynprog_amd import SolverFamily, models


def main(capacities=np.linspace(1.13, 4.28, 64), T=48, n_start=8, verbose=True, **kw):
    fam = SolverFamily([models.pv_storage(E_rated=float(E), T=T, **kw)[1] for E in capacities])
    J_fin = np.zeros((fam.P,) + fam.dims)
    J, pol = fam.bellman_recursion(T, J_fin)
    J_next = np.concatenate([J[:, 1:], J_fin[:, None]], axis=1)            # step k decides with the cost-to-go of k + 1
    # the same start states for both controllers: the store between empty and half full, per member
    x0 = np.linspace(0., 0.5, n_start)[None, :, None] * np.asarray(capacities, dtype=float)[:, None, None]
    t = time.perf_counter()
    _, _, g_pol = fam.simulate(pol, x0, n_steps=T)                         # (P, T, B)
    t_pol = time.perf_counter() - t
    t = time.perf_counter()
    x, u, g_look, q = fam.simulate_lookahead(J_next, x0, n_steps=T)        # (P, T+1, B, 1), (P, T, B, 1), (P, T, B), (P, T, B)
    t_look = time.perf_counter() - t
    info = fam.backend_info
    cost_pol, cost_look = np.zeros((fam.P, n_start)), np.zeros((fam.P, n_start))
    for k in range(T):
        cost_pol, cost_look = cost_pol + g_pol[:, k], cost_look + g_look[:, k]
    if verbose:
        print('{:>8s} {:>20s} {:>20s} {:>12s} {:>14s}'.format('E_rated', 'tabulated policy', 'lookahead', 'difference', 'J[0] at E = 0'))
        for p, E in enumerate(capacities):
            a, b = cost_pol[p].mean(), cost_look[p].mean()
            print('{:8.3f} {:20.12g} {:20.12g} {:12.4g} {:14.8g}'.format(E, a, b, b - a, J[p, 0, 0]))
        print('mean cost of the day over {} start states; simulate: {:.3f} s, simulate_lookahead: {:.3f} s ({} members, {} steps, '
              '{} launch(es), lanes {}, box {})'.format(n_start, t_pol, t_look, fam.P, T, info['horizon']['launches'], info['lanes'],
                                                         info['lookahead_box']))
    assert not np.isnan(q).any()
    return dict(capacities=list(map(float, capacities)), cost_policy=cost_pol.mean(axis=1).tolist(),
                cost_lookahead=cost_look.mean(axis=1).tolist(), policy_s=t_pol, lookahead_s=t_look)


if __name__ == '__main__':
    main()
