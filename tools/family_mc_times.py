"""What scoring the policies of a family in one device call (SolverFamily.monte_carlo, csrc/sdp_family_mc_kernel.h)
gains over the loop of solo DPSolver.monte_carlo calls, written to profiles/family_mc_times.json.

Storage-AR1 on 41 x 61 nodes with a control step of 0.1, 9 perturbation points, 8-byte reals, over P storage
capacities, P = 1, 8 and 64: the policies of `fam.policy_iteration` to tol = 1e-6, then 4096 trajectories of 1000
steps per member under one seed.  Two paths:

  solo      the loop of P DPSolver.monte_carlo calls in the same process, kernel = 'auto' (what a user's loop runs),
            units compiled and problems created beforehand
  family    one SolverFamily.monte_carlo call

Per path: wall time of the call (perf_counter) and the HIP-event time of its launches (the solo loop's: the sum over
the members).  Warm chip: both paths once before the timed rounds, which also compares their bits; the paths in turn
within one process; the median of three rounds.  At P = 64 the variant with the occupancy counted as well.

    python tools/family_mc_times.py [--small] [--out profiles/family_mc_times.json]
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
FIELDS = ('cost_sum', 'n_outside', 'x_final', 'occupancy')


def quiet(f, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all='ignore'):
        return f(*a, **kw)


def members(P, kw):
    return [models.storage_ar1(E_rated=float(E), **kw)[1] for E in np.linspace(2., 20., P)] if P > 1 else \
        [models.storage_ar1(E_rated=10., **kw)[1]]


def measure(P, B, n_steps, rounds, kw, occupancy):
    fam = SolverFamily(members(P, kw))
    solo = members(P, kw)
    pol0 = np.zeros(fam.dims + (fam.nu,))
    _, pol = fam.policy_iteration(pol0, 1000, 8, True, **TOL)
    # every member starts in the middle of its own grid
    x0 = np.stack([np.broadcast_to([0.5 * s.state_grid[0][-1], 0.], (B, 2)) for s in solo])
    run_kw = dict(seed=1, n_burn=n_steps // 10, occupancy=occupancy)

    def run_family():
        t = time.perf_counter()
        out = fam.monte_carlo(pol, x0, n_steps, **run_kw)
        return time.perf_counter() - t, fam.last_kernel_ms(), out

    def run_solo():
        t = time.perf_counter()
        out, ms = [], 0.
        for p, s in enumerate(solo):
            out.append(quiet(s.monte_carlo, pol[p], x0[p], n_steps, **run_kw))
            ms += s._problem().last_kernel_ms()
        return time.perf_counter() - t, ms, out

    # warm-up, and the bits of the two paths
    _, _, a = run_family()
    _, _, each = run_solo()
    same = all(np.array_equal(getattr(a[p], name), getattr(each[p], name)) for p in range(P) for name in FIELDS
               if getattr(each[p], name) is not None)
    times = dict(family=[], solo=[])
    for _ in range(rounds):
        for name, run in (('solo', run_solo), ('family', run_family)):
            w, k, _ = run()
            times[name].append((w, k))
    med = lambda x: float(np.median(x))
    row = dict(members=P, n_traj=B, steps=n_steps, n_burn=run_kw['n_burn'], occupancy=bool(occupancy), rounds=rounds,
               same_bits=bool(same), launches=fam.backend_info['monte_carlo']['launches'],
               mean_cost=[float(m) for m in a.mean[:8]], solo_kernel=solo[0].backend_info.get('kernel'))
    for name, got in times.items():
        row[name + '_wall_s'] = med([g[0] for g in got])
        row[name + '_wall_s_all_rounds'] = [g[0] for g in got]
        row[name + '_kernel_ms'] = med([g[1] for g in got])
    row['solo_over_family_wall'] = row['solo_wall_s'] / row['family_wall_s']
    row['solo_over_family_kernel'] = row['solo_kernel_ms'] / row['family_kernel_ms']
    if P > 1:
        row['paired_0_1'] = list(a.paired(0, 1))
        row['unpaired_stderr_0_1'] = float(np.hypot(a.stderr[0], a.stderr[1]))
    fam.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--small', action='store_true', help='a tiny problem: a rehearsal, not a measurement')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'family_mc_times.json'))
    a = ap.parse_args()
    nat.require_gpu()
    nat.check(nat.lib().sdp_set_device(0))
    kw = SMALL if a.small else PROBLEM
    B, n_steps = (300, 50) if a.small else (4096, 1000)
    one = members(1, kw)[0]
    rows = []
    out = dict(device=nat.device_info(0), small=bool(a.small), real_bytes=8, policy_iteration=TOL, grid=list(one._shape()),
               control_steps=list(one.control_steps), law_points=len(one.perturb_grid[0]), seed=1, by_members=rows)
    sizes = [(1, False), (3, False), (3, True)] if a.small else [(1, False), (8, False), (64, False), (64, True)]
    for P, occupancy in sizes:
        rows.append(measure(P, B, n_steps, 3, kw, occupancy))
        print(json.dumps(rows[-1], sort_keys=True), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:                    # (after every size: a run cut short keeps what it has)
            json.dump(out, f, indent=1, sort_keys=True)
            f.write('\n')


if __name__ == '__main__':
    main()
