"""What building and iterating the transition operators of a family in one device call
(SolverFamily.transition_operator, csrc/sdp_family_trans_kernel.h, sdp_transop_push_until_members) gains over the loop
of solo DPSolver.transition_operator calls, written to profiles/family_forward_times.json.

Storage-AR1 on 41 x 61 nodes with a control step of 0.1, 9 perturbation points, 8-byte reals, over P storage
capacities, P = 1, 8 and 64, under the policies of `fam.policy_iteration` to tol = 1e-6.  Three steps, each on two
paths -- the loop of P solo calls in the same process, kernel = 'auto' (what a user's loop runs), and one family call:

  build        transition_operator(pol): entries, sort, row pointers, mean costs read back
  push         op.push(mu, 100): 100 steps back to back from a vector of the host's
  stationary   op.stationary(tol = 1e-12, check_every = 10): the power iteration, each member to its own stop

Per step and path: wall time of the call(s) (perf_counter) and the HIP-event time of the launches (the solo loop's: the
sum over the members).  Warm chip: both paths once before the timed rounds, which also compares their bits; the paths
in turn within one process; the median of three rounds.

    python tools/family_forward_times.py [--small] [--out profiles/family_forward_times.json]
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

from stodynprog_amd import SolverFamily, forward, models, _native as nat           # noqa: E402

PROBLEM = dict(steps=(0.1, 0.1))
SMALL = dict(n_E=7, n_P=5, n_w=3, steps=(0.5, 0.1))
TOL = dict(tol=1e-6, check_every=10)
STAT = dict(tol=1e-12, n_max=5000, check_every=10)
PUSHES = 100


def quiet(f, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all='ignore'):
        return f(*a, **kw)


def members(P, kw):
    return [models.storage_ar1(E_rated=float(E), **kw)[1] for E in np.linspace(2., 20., P)] if P > 1 else \
        [models.storage_ar1(E_rated=10., **kw)[1]]


def measure(P, rounds, kw):
    fam = SolverFamily(members(P, kw))
    solo = members(P, kw)
    pol0 = np.zeros(fam.dims + (fam.nu,))
    _, pol = fam.policy_iteration(pol0, 1000, 8, True, **TOL)
    S = int(np.prod(fam.dims))
    mu0 = np.broadcast_to(forward.uniform(S, fam.dtype).reshape(fam.dims), (P,) + fam.dims)

    def run_family():
        out, t = {}, time.perf_counter()
        op = fam.transition_operator(pol)
        out['build'] = (time.perf_counter() - t, op.info['build_ms'])
        t = time.perf_counter()
        pushed = op.push(mu0, PUSHES)
        out['push'] = (time.perf_counter() - t, op.info['push_ms'])
        t = time.perf_counter()
        res = op.stationary(**STAT)
        out['stationary'] = (time.perf_counter() - t, op.info['push_ms'])
        got = ([op.tocsr(p) for p in range(P)], op.mean_cost, pushed, res)
        op.close()
        return out, got

    def run_solo():
        out = dict(build=[0., 0.], push=[0., 0.], stationary=[0., 0.])
        csr, gbar, pushed, res = [], [], [], []
        for p, s in enumerate(solo):
            t = time.perf_counter()
            op = quiet(s.transition_operator, pol[p])
            out['build'][0] += time.perf_counter() - t
            out['build'][1] += op.info['build_ms']
            t = time.perf_counter()
            pushed.append(op.push(mu0[p], PUSHES))
            out['push'][0] += time.perf_counter() - t
            out['push'][1] += op.info['push_ms']
            t = time.perf_counter()
            res.append(op.stationary(**STAT))
            out['stationary'][0] += time.perf_counter() - t
            out['stationary'][1] += op.info['push_ms']
            csr.append(op.tocsr())
            gbar.append(op.mean_cost)
            op.close()
        return {k: tuple(v) for k, v in out.items()}, (csr, gbar, pushed, res)

    # warm-up, and the bits of the two paths
    _, a = run_family()
    _, b = run_solo()
    same = all(np.array_equal(x, y, equal_nan=True) for p in range(P) for x, y in zip(a[0][p], b[0][p])) \
        and all(np.array_equal(a[1][p], b[1][p]) and np.array_equal(a[2][p], b[2][p]) and np.array_equal(a[3].mu[p], b[3][p].mu)
                and a[3][p].n_done == b[3][p].n_done and a[3][p].delta == b[3][p].delta for p in range(P))
    times = dict(family=[], solo=[])
    for _ in range(rounds):
        for name, run in (('solo', run_solo), ('family', run_family)):
            times[name].append(run()[0])
    med = lambda x: float(np.median(x))
    row = dict(members=P, rounds=rounds, same_bits=bool(same), pushes=PUSHES, entries=P * S * max(fam.W, 1) * (1 << len(fam.dims)),
               chunks=fam.backend_info['transition']['chunks'], n_done=[int(n) for n in a[3].n_done],
               converged=[bool(c) for c in a[3].converged], average_cost=[float(c) for c in a[3].average_cost[:8]],
               solo_kernel=solo[0].backend_info.get('kernel'))
    for step in ('build', 'push', 'stationary'):
        for name, got in times.items():
            row['{}_{}_wall_s'.format(step, name)] = med([g[step][0] for g in got])
            row['{}_{}_wall_s_all_rounds'.format(step, name)] = [g[step][0] for g in got]
            row['{}_{}_kernel_ms'.format(step, name)] = med([g[step][1] for g in got])
        row[step + '_solo_over_family_wall'] = row[step + '_solo_wall_s'] / row[step + '_family_wall_s']
        row[step + '_solo_over_family_kernel'] = row[step + '_solo_kernel_ms'] / row[step + '_family_kernel_ms']
    fam.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--small', action='store_true', help='a tiny problem: a rehearsal, not a measurement')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'family_forward_times.json'))
    a = ap.parse_args()
    nat.require_gpu()
    nat.check(nat.lib().sdp_set_device(0))
    kw = SMALL if a.small else PROBLEM
    one = members(1, kw)[0]
    rows = []
    out = dict(device=nat.device_info(0), small=bool(a.small), real_bytes=8, policy_iteration=TOL, stationary=STAT,
               grid=list(one._shape()), control_steps=list(one.control_steps), law_points=len(one.perturb_grid[0]),
               by_members=rows)
    for P in ((1, 3) if a.small else (1, 8, 64)):
        rows.append(measure(P, 3, kw))
        print(json.dumps(rows[-1], sort_keys=True), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:                    # (after every size: a run cut short keeps what it has)
            json.dump(out, f, indent=1, sort_keys=True)
            f.write('\n')


if __name__ == '__main__':
    main()
