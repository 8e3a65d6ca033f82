"""What scoring a family under lookahead controls in one device call (SolverFamily.monte_carlo_lookahead,
csrc/sdp_family_lookahead_kernel.h) costs against the loop of solo DPSolver.monte_carlo_lookahead calls, written to
profiles/family_lookahead_times.json.

Storage-AR1 on 41 x 61 nodes with a control step of 0.1, 9 perturbation points, 8-byte reals, over 64 storage
capacities: the cost-to-go of `fam.value_iterations` to tol = 1e-6, then n_traj trajectories per member under one
seed, at two batch sizes: 4096 per member, where a solo call already fills the chip, and 256, where it does not.
Two paths:

  solo      the loop of P DPSolver.monte_carlo_lookahead calls in the same process (the only route before the family
            call), units compiled and problems created beforehand
  family    one SolverFamily.monte_carlo_lookahead call

Per path: wall time of the call (perf_counter) and the HIP-event time of its launches (the solo loop's: the sum over
the members).  Also the kernel time of ONE member alone, family of one against solo.  Warm chip: both paths once
before the timed rounds, which also compares their bits; the paths in turn within one process; the median of three
rounds.  The convention of DESIGN.md 5e-5g: the family's kernel time at 4096 per member is at most 1.10 times the sum
of the solo kernels' times -- the same work is expected to cost the same.

    python tools/family_lookahead_times.py [--small] [--out profiles/family_lookahead_times.json]
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stodynprog_amd import SolverFamily, models, _native as nat           # noqa: E402

PROBLEM = dict(steps=(0.1, 0.1))
SMALL = dict(n_E=7, n_P=5, n_w=3, steps=(0.5, 0.1))
TOL = dict(tol=1e-6, check_every=10)
FIELDS = ('cost_sum', 'n_outside', 'x_final')
MEMBERS = 64
BOUND = 1.10


def quiet(f, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all='ignore'):
        return f(*a, **kw)


def capacities(P):
    """no capacity equals P_rated = 4 or dt = 1: equal constants of control_box would be one node of its trace"""
    return np.linspace(2.5, 20.5, P) if P > 1 else np.array([10.])


def members(P, kw):
    return [models.storage_ar1(E_rated=float(E), **kw)[1] for E in capacities(P)]


def measure(P, B, n_steps, rounds, kw):
    fam = SolverFamily(members(P, kw))
    solo = members(P, kw)
    (J, _), _ = fam.value_iterations((np.zeros(fam.dims), 0.), 2000, rel_dp=True, **TOL)
    # every member starts in the middle of its own grid
    x0 = np.stack([np.broadcast_to([0.5 * s.state_grid[0][-1], 0.], (B, 2)) for s in solo])
    run_kw = dict(seed=1, n_burn=n_steps // 10)

    def run_family():
        t = time.perf_counter()
        out = fam.monte_carlo_lookahead(J, x0, n_steps, **run_kw)
        return time.perf_counter() - t, fam.last_kernel_ms(), out

    def run_solo():
        t = time.perf_counter()
        out, ms = [], 0.
        for p, s in enumerate(solo):
            out.append(quiet(s.monte_carlo_lookahead, J[p], x0[p], n_steps, **run_kw))
            ms += s._lookahead_prob.last_kernel_ms()
        return time.perf_counter() - t, ms, out

    # warm-up, and the bits of the two paths
    _, _, a = run_family()
    _, _, each = run_solo()
    same = all(each[p].path == 'device' and np.array_equal(getattr(a[p], name), getattr(each[p], name))
               for p in range(P) for name in FIELDS)
    times = dict(family=[], solo=[])
    for _ in range(rounds):
        for name, run in (('solo', run_solo), ('family', run_family)):
            w, k, _ = run()
            times[name].append((w, k))
    med = lambda x: float(np.median(x))
    row = dict(members=P, n_traj=B, steps=n_steps, n_burn=run_kw['n_burn'], rounds=rounds, same_bits=bool(same),
               launches=fam.backend_info['monte_carlo']['launches'], lanes=fam.backend_info['lanes'],
               mean_cost=[float(m) for m in a.mean[:8]])
    for name, got in times.items():
        row[name + '_wall_s'] = med([g[0] for g in got])
        row[name + '_wall_s_all_rounds'] = [g[0] for g in got]
        row[name + '_kernel_ms'] = med([g[1] for g in got])
        row[name + '_kernel_ms_all_rounds'] = [g[1] for g in got]
    row['family_over_solo_kernel'] = row['family_kernel_ms'] / row['solo_kernel_ms']
    row['solo_over_family_wall'] = row['solo_wall_s'] / row['family_wall_s']
    if P > 1:
        row['paired_0_1'] = list(a.paired(0, 1))
        row['unpaired_stderr_0_1'] = float(np.hypot(a.stderr[0], a.stderr[1]))
    fam.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--small', action='store_true', help='a tiny problem: a rehearsal, not a measurement')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'family_lookahead_times.json'))
    a = ap.parse_args()
    nat.require_gpu()
    nat.check(nat.lib().sdp_set_device(0))
    kw = SMALL if a.small else PROBLEM
    n_steps = 20 if a.small else 200
    one = members(1, kw)[0]
    rows = []
    out = dict(device=nat.device_info(0), small=bool(a.small), real_bytes=8, value_iterations=TOL, grid=list(one._shape()),
               control_steps=list(one.control_steps), law_points=len(one.perturb_grid[0]), seed=1, bound=BOUND, rows=rows)
    sizes = [(3, 300), (3, 40), (1, 300)] if a.small else [(MEMBERS, 4096), (MEMBERS, 256), (1, 4096)]
    for P, B in sizes:
        rows.append(measure(P, B, n_steps, 3, kw))
        print(json.dumps(rows[-1], sort_keys=True), flush=True)
        full = [r for r in rows if r['members'] > 1 and r['n_traj'] == sizes[0][1]]
        if full:
            out['family_over_solo_kernel_at_full_batch'] = full[0]['family_over_solo_kernel']
            out['within_bound'] = bool(full[0]['family_over_solo_kernel'] <= BOUND)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:                    # (after every size: a run cut short keeps what it has)
            json.dump(out, f, indent=1, sort_keys=True)
            f.write('\n')


if __name__ == '__main__':
    main()
