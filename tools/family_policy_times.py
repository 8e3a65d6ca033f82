"""What evaluating and iterating policies for a family in one device call (SolverFamily.eval_policy /
policy_iteration, csrc/sdp_family_policy_kernel.h) gains over the loop of solo calls, written to
profiles/family_policy_times.json.

Storage-AR1 on 41 x 61 nodes -- and on 21 x 31, which the resident kernel's workgroup evaluates in one trip -- with a
control step of 0.1 (<= 81 controls), 9 perturbation points, 8-byte reals, over P storage capacities, P = 1, 8 and 64: `eval_policy` of the idle policy for 1000 steps with rel_dp, and
`policy_iteration` from it to tol = 1e-6 (n_val = 1000 at most, checked every 10 steps, n_pol = 5).  Three paths:

  solo      the loop of P DPSolver calls in the same process, kernel = 'auto' (what a user's loop runs), units compiled
            and problems created beforehand
  steps     the family with evaluation = 'steps': one launch of sdp_family_evalpol per step
  resident  the family with evaluation = 'resident': one launch of sdp_family_evalpol_resident per evaluation

Per path: wall time of a call, and for eval_policy the HIP-event time of its launches per member and step.  Warm chip:
every path once before the timed rounds, which also compares the bits of the three; the paths in turn within one
process; the median of three rounds.

    python tools/family_policy_times.py [--small] [--out profiles/family_policy_times.json]
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

# the issue's size, 41 x 61 = 2501 nodes (three trips of the resident kernel's 1024 threads), and a grid of 21 x 31 = 651
# nodes, which a workgroup evaluates in one trip
PROBLEMS = {'41x61': dict(steps=(0.1, 0.1)), '21x31': dict(n_E=21, n_P=31, steps=(0.1, 0.1))}
SMALL = {'7x5': dict(n_E=7, n_P=5, n_w=3, steps=(0.5, 0.1))}
TOL = dict(tol=1e-6, check_every=10)


def quiet(f, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all='ignore'):
        return f(*a, **kw)


def members(P, kw):
    return [models.storage_ar1(E_rated=float(E), **kw)[1] for E in np.linspace(2., 20., P)] if P > 1 else \
        [models.storage_ar1(E_rated=10., **kw)[1]]


def measure(P, n_steps, n_pol, rounds, kw):
    fam = SolverFamily(members(P, kw))
    solo = members(P, kw)
    pol0 = np.zeros(fam.dims + (fam.nu,))

    def family_eval(form):
        fam.evaluation = form
        t = time.perf_counter()
        out = fam.eval_policy(pol0, n_steps, True)
        return time.perf_counter() - t, fam.last_kernel_ms() / (n_steps * P), out

    def solo_eval():
        t = time.perf_counter()
        out = [quiet(s.eval_policy, pol0, n_steps, True, report_time=False) for s in solo]
        wall = time.perf_counter() - t
        return wall, float(np.mean([s._problem().last_kernel_ms() for s in solo])) / n_steps, out

    def family_iteration(form):
        fam.evaluation = form
        t = time.perf_counter()
        out = fam.policy_iteration(pol0, n_steps, n_pol, True, **TOL)
        return time.perf_counter() - t, None, out

    def solo_iteration():
        t = time.perf_counter()
        out = [quiet(s.policy_iteration, pol0, n_steps, n_pol, True, **TOL) for s in solo]
        return time.perf_counter() - t, None, out

    row = dict(members=P, steps=n_steps, rounds=rounds)
    for what, run_family, run_solo in (('eval_policy', family_eval, solo_eval), ('policy_iteration', family_iteration, solo_iteration)):
        # warm-up, and the bits of the three paths
        _, _, a = run_family('steps')
        _, _, b = run_family('resident')
        _, _, each = run_solo()
        if what == 'eval_policy':
            same = np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and all(
                np.array_equal(a[0][p], Jp) and a[1][p] == refp for p, (Jp, refp) in enumerate(each))
        else:
            same = np.array_equal(a[0][0], b[0][0]) and np.array_equal(a[1], b[1]) and all(
                np.array_equal(a[0][0][p], Jp) and a[0][1][p] == refp and np.array_equal(a[1][p], polp)
                for p, ((Jp, refp), polp) in enumerate(each))
            row['policy_iteration_improvements'] = [r.n_improvements for r in fam.last_convergence]
            row['policy_iteration_evaluation_steps'] = [[e.n_iter for e in r.evaluations] for r in fam.last_convergence][:8]
        times = dict(steps=[], resident=[], solo=[])
        for _ in range(rounds):
            for name, run in (('solo', run_solo), ('steps', lambda: run_family('steps')), ('resident', lambda: run_family('resident'))):
                w, k, _ = run()
                times[name].append((w, k))
        med = lambda x: float(np.median(x))
        res = dict(same_bits=bool(same))
        for name, got in times.items():
            res[name + '_wall_s'] = med([g[0] for g in got])
            res[name + '_wall_s_all_rounds'] = [g[0] for g in got]
            if got[0][1] is not None:
                res[name + '_kernel_ms_per_member_step'] = med([g[1] for g in got])
        res['solo_over_steps_wall'] = res['solo_wall_s'] / res['steps_wall_s']
        res['solo_over_resident_wall'] = res['solo_wall_s'] / res['resident_wall_s']
        res['steps_over_resident_wall'] = res['steps_wall_s'] / res['resident_wall_s']
        row[what] = res
    row['solo_kernel'] = solo[0].backend_info.get('kernel')
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--small', action='store_true', help='a tiny problem: a rehearsal, not a measurement')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'family_policy_times.json'))
    a = ap.parse_args()
    nat.require_gpu()
    nat.check(nat.lib().sdp_set_device(0))
    n_steps, n_pol = (20, 2) if a.small else (1000, 5)
    out = dict(device=nat.device_info(0), small=bool(a.small), real_bytes=8, rel_dp=True, tol=TOL, n_pol=n_pol, problems={})
    for name, kw in (SMALL if a.small else PROBLEMS).items():
        one = members(1, kw)[0]
        rows = []
        out['problems'][name] = dict(grid=list(one._shape()), control_steps=list(one.control_steps), by_members=rows)
        for P in ((1, 3) if a.small else (1, 8, 64)):
            rows.append(measure(P, n_steps, n_pol, 3, kw))
            print(name, json.dumps(rows[-1], sort_keys=True), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'w') as f:                    # (after every size: a run cut short keeps what it has)
                json.dump(out, f, indent=1, sort_keys=True)
                f.write('\n')


if __name__ == '__main__':
    main()
