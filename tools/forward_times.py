"""What the transition operator of a policy costs (DPSolver.transition_operator: kernel sdp_transitions, the sort into
the CSR of P^T, k_push), written to profiles/forward_times.json.  models.searev() at its own 31 x 61 x 61 grid with 9
perturbation points (8.3e6 entries, 8-byte reals), the heuristic linear policy of the example:

  build      the HIP-event time of kernel sdp_transitions and of the sort + gather + row pointers, each on its own
  push       the time per push over 100 pushes queued back to back (one call, HIP events around the queue), for each
             way of sharing the rows out -- every row to one lane (the first kernel), and a wave per row of at least 64,
             8 (what the build sets) and 1 entries -- and the bytes a push must move, nnz 12 + 8 (S + 1) + 2 x 8 S, as a fraction of the 6.3 TB/s a copy reaches
             
  YARDSTICK  one step of eval_policy on the same problem and policy, in the same process: the adjoint over the same
             cells, with the model evaluated again every time (kernel time per step over 10 steps)

Warm chip (a build, pushes and evaluation steps before the timed ones), three rounds in turn, the median of the rounds.
Accepted: a push takes at most 1.10 x the evaluation step (the pool's boxes differ by 2-4 %).

    python tools/forward_times.py [--small] [--out profiles/forward_times.json]
"""
import argparse
import contextlib
import io
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stodynprog_amd import models, _native as nat           # noqa: E402

COPY_RATE = 6.3e12          # bytes per second of a float4 copy


def quiet(f, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return f(*a, **kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--small', action='store_true', help='a tiny grid: a rehearsal, not a measurement')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'forward_times.json'))
    a = ap.parse_args()
    nat.require_gpu()
    nat.check(nat.lib().sdp_set_device(0))
    grid = (7, 9, 9) if a.small else (31, 61, 61)
    pushes, steps, rounds = (10, 2, 3) if a.small else (100, 10, 3)
    _, s = models.searev(n_E=grid[0], n_S=grid[1], n_A=grid[2])
    pol = models.searev_linear_policy(s)
    S = int(np.prod(grid))
    mu = np.full(grid, 1.0 / S)
    # warm-up: the code object, the buffers, a first build, pushes and evaluation steps
    quiet(s.eval_policy, pol, 2, report_time=False)
    prob = s._problem(None)
    prob.set_value(np.zeros(grid))
    prob.set_policy(pol)
    s.transition_operator(pol).close()
    op = s.transition_operator(pol)
    op.push(mu, 10)
    paths = {'one lane per row': 0, 'a wave per row of 64 entries or more': 64,
             'a wave per row of 8 entries or more (the build sets this)': 8, 'a wave per row that has an entry': 1}
    build, step_ms, path_ms, results = [], [], {k: [] for k in paths}, {}
    for _ in range(rounds):
        again = s.transition_operator(pol)
        build.append(dict(again.info))
        again.close()
        for name, long_from in paths.items():
            op.set_long_rows(long_from)
            op.push(mu, 3)
            results[name] = op.push(mu, pushes)
            path_ms[name].append(op.info['push_ms'] / pushes)
        prob.eval_policy(steps)
        step_ms.append(prob.last_kernel_ms() / steps)
    first = results['one lane per row']
    assert all(np.array_equal(first, r) for r in results.values()), 'the paths differ'
    op.set_long_rows(8)
    push_ms = path_ms['a wave per row of 8 entries or more (the build sets this)']
    rows = np.diff(op.tocsr()[0])
    rec = op.stationary(tol=1e-12, n_max=2000, check_every=10)
    moved = op.nnz * 12 + 8 * (S + 1) + 2 * 8 * S
    push = float(np.median(push_ms))
    step = float(np.median(step_ms))
    out = dict(device=nat.device_info(0), small=bool(a.small), grid=list(grid), nnz=op.nnz, operator_bytes=op.nbytes,
               kernel=s.backend_info['kernel'], rounds=rounds, pushes_per_round=pushes, eval_steps_per_round=steps,
               entries_ms=float(np.median([b['entries_ms'] for b in build])),
               sort_ms=float(np.median([b['sort_ms'] for b in build])),
               build_ms_all_rounds=[[b['entries_ms'], b['sort_ms']] for b in build],
               push_ms=push, push_ms_all_rounds=push_ms,
               push_ms_by_path={k: dict(median=float(np.median(v)), all_rounds=v, over_eval_step=float(np.median(v)) / step)
                                for k, v in path_ms.items()},
               rows_of_8_or_more=int((rows >= 8).sum()), rows_of_64_or_more=int((rows >= 64).sum()), eval_policy_step_ms=step, eval_policy_step_ms_all_rounds=step_ms,
               push_over_eval_step=push / step, accepted_at_most=1.10, accepted=bool(push <= 1.10 * step),
               bytes_per_push=moved, push_bytes_per_second=moved / (push * 1e-3),
               fraction_of_copy_rate=moved / (push * 1e-3) / COPY_RATE,
               rows=dict(longest=int(rows.max()), empty=int((rows == 0).sum()), mean=float(rows.mean())),
               stationary=dict(n_done=rec.n_done, converged=rec.converged, delta=rec.delta, mass=float(rec.mass),
                               average_cost=rec.average_cost, negative_entries=int((rec.mu < 0).sum()),
                               ms=op.info['push_ms']))
    op.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == '__main__':
    main()
