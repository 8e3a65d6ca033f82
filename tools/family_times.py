"""What solving a family of same-shaped problems in one device call (stodynprog_amd.SolverFamily,
csrc/sdp_family_kernel.h) gains over the loop of solo calls, written to profiles/family_times.json.

Storage-AR1 at the reference's published size (41 x 61 nodes, <= 8001 controls, 9 perturbation points, 8-byte reals)
over P storage capacities, 100 sweeps of relative value iteration from zero, for P = 1, 8, 64 and 512 -- and the same
grid with a control step of 0.1 (<= 81 controls), where a sweep of one member is bound by its launch:

  family   one `SolverFamily.value_iterations` call: wall time (tracing, tables, upload, sweeps, download) and the
           HIP-event time of all its launches (sweeps and relative-DP shifts) per member and sweep
  solo     the loop of P `DPSolver.value_iterations` calls in the same process, kernel = 'auto' (what a user's loop
           runs: the column kernel), units compiled and problems created beforehand: wall time, and the HIP-event
           time of a sweep kernel (the last sweep of every call; without the shift kernels) averaged over the members

Warm chip: every path once before the timed rounds, which also checks that the two give the same bits; the paths in
turn within one process; the median of the rounds.

    python tools/family_times.py [--small] [--out profiles/family_times.json]
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


def quiet(f, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all='ignore'):
        return f(*a, **kw)


# the problems measured: the published lattice (a step of 0.001: up to 8001 controls per node, a sweep of one member is
# 142.8 M cells and bound by arithmetic), and the same grid with a step of 0.1 (up to 81 controls: a sweep of one
# member is bound by the launch)
PROBLEMS = dict(published={}, coarse_lattice=dict(steps=(0.1, 0.1)))
SMALL = dict(rehearsal=dict(n_E=7, n_P=5, n_w=3, steps=(0.5, 0.1)))


def members(P, kw):
    return [models.storage_ar1(E_rated=float(E), **kw)[1] for E in np.linspace(2., 20., P)] if P > 1 else \
        [models.storage_ar1(E_rated=10., **kw)[1]]


def measure(P, sweeps, rounds, kw):
    fam = SolverFamily(members(P, kw))
    solo = members(P, kw)
    J0 = np.zeros(fam.dims)

    def run_family():
        t = time.perf_counter()
        out = quiet(fam.value_iterations, (J0, 0.), sweeps, True)
        return time.perf_counter() - t, fam.last_kernel_ms() / (sweeps * P), out

    def run_solo():
        t = time.perf_counter()
        out = [quiet(s.value_iterations, (J0, 0.), sweeps, True, report_time=False) for s in solo]
        wall = time.perf_counter() - t
        kern = float(np.mean([s._problem().last_kernel_ms() for s in solo]))
        return wall, kern, out

    _, _, ((J, refs), pol) = run_family()                           # warm-up, and the bits
    _, _, each = run_solo()
    for p, ((Jp, refp), polp) in enumerate(each):
        assert np.array_equal(J[p], Jp) and np.array_equal(pol[p], polp) and refs[p] == refp, p
    fw, fk, sw, sk = [], [], [], []
    for _ in range(rounds):
        w, k, _ = run_family()
        fw.append(w)
        fk.append(k)
        w, k, _ = run_solo()
        sw.append(w)
        sk.append(k)
    med = lambda x: float(np.median(x))
    info = fam.backend_info
    return dict(members=P, sweeps=sweeps, rounds=rounds, lanes=info['lanes'], chunks=info['chunks'],
                solo_kernel=solo[0].backend_info.get('kernel'), same_bits=True,
                family_wall_s=med(fw), family_wall_s_all_rounds=fw,
                solo_loop_wall_s=med(sw), solo_loop_wall_s_all_rounds=sw,
                solo_over_family_wall=med(sw) / med(fw),
                family_kernel_ms_per_member_sweep=med(fk), family_kernel_ms_per_member_sweep_all_rounds=fk,
                solo_kernel_ms_per_member_sweep=med(sk), solo_kernel_ms_per_member_sweep_all_rounds=sk,
                solo_over_family_kernel=med(sk) / med(fk))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--small', action='store_true', help='a tiny problem: a rehearsal, not a measurement')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'family_times.json'))
    a = ap.parse_args()
    nat.require_gpu()
    nat.check(nat.lib().sdp_set_device(0))
    sweeps = 5 if a.small else 100
    sizes = ((1, 3), (8, 3), (64, 3), (512, 1)) if not a.small else ((1, 2), (8, 2), (17, 1))
    out = dict(device=nat.device_info(0), small=bool(a.small), real_bytes=8, rel_dp=True, problems={})
    for name, kw in (SMALL if a.small else PROBLEMS).items():
        rows = []
        for P, rounds in sizes:
            rows.append(measure(P, sweeps, rounds, kw))
            print(name, json.dumps(rows[-1], sort_keys=True), flush=True)
        one = members(1, kw)[0]
        plan = one._kernel_plan()
        out['problems'][name] = dict(grid=list(one._shape()), law_points=int(plan['W']), max_controls=int(plan['max_u']),
                                     control_steps=list(one.control_steps), by_members=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')


if __name__ == '__main__':
    main()
