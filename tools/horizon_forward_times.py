"""What building the transition operators of all steps of a horizon in one device call and pushing a batch of
distributions through them on the device (DPSolver.horizon_operator / propagate, csrc/sdp_trans_horizon_kernel.h and the
library's sdp_chainop) takes next to the loop this replaces, written to profiles/horizon_forward_times.json.

  ar1   storage-AR1 on 41 x 61 nodes, 9 perturbation points, T = 200 steps under the time-indexed policy of
        bellman_recursion (a receding schedule on a stationary model)
  pv    models.pv_storage (deterministic, `data[k]` in the cost, 50 nodes), T = 48 steps under its bellman_recursion policy

each with B = 1 and B = 64 initial distributions (point masses).  The yardstick is the loop over k of
`transition_operator(pol[k], t_k=k)`, `push(mu, 1)` for every vector, and `close()`: its wall time (perf_counter) and the
sum of its HIP-event times (backend_info['transition']: build and pushes).  Of the call: the wall time of
`horizon_operator` + `propagate` + `close`, and the HIP-event times of the build (entries, sort) and of the propagate.
Warm chip: both paths once before the timed rounds, which also compares their bits; the paths in turn within one process;
the median of three rounds.

    python tools/horizon_forward_times.py [--small] [--out profiles/horizon_forward_times.json]
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

from stodynprog_amd import models, _native as nat           # noqa: E402


def quiet(f, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all='ignore'):
        return f(*a, **kw)


def workloads(small):
    if small:
        return [('ar1', models.storage_ar1(n_E=7, n_P=5, n_w=3, steps=(0.5, 0.1))[1], 8),
                ('pv', models.pv_storage(T=6, N_E=9, u_step=0.05)[1], 6)]
    return [('ar1', models.storage_ar1(steps=(0.1, 0.1))[1], 200), ('pv', models.pv_storage()[1], 48)]


def starts(dims, B):
    """B point masses spread over the grid"""
    S = int(np.prod(dims))
    mu0 = np.zeros((B, S))
    mu0[np.arange(B), (np.arange(B) * S) // B + S // (2 * B)] = 1.0
    return mu0.reshape((B,) + dims)


def measure(name, s, T, pol, B, rounds):
    dims = tuple(len(g) for g in s.state_grid)
    mu0 = starts(dims, B)

    def run_call():
        t = time.perf_counter()
        op = s.horizon_operator(pol)
        res = op.propagate(mu0)
        op.close()
        return time.perf_counter() - t, dict(s.backend_info['horizon_operator']), res.mu

    def run_loop():
        t = time.perf_counter()
        mu = np.empty((T + 1,) + mu0.shape)
        mu[0] = mu0
        ms = 0.
        for k in range(T):
            op = s.transition_operator(pol[k], t_k=k)
            ms += op.info['build_ms']
            for b in range(B):
                mu[k + 1, b] = op.push(mu[k, b], 1)
                ms += op.info['push_ms']
            op.close()
        return time.perf_counter() - t, ms, mu

    _, _, a = quiet(run_call)                       # warm-up, and the bits of the two paths
    _, _, b = quiet(run_loop)
    same = bool(np.array_equal(a, b))
    assert same, '{} B = {}: the call and the loop differ: nothing to time'.format(name, B)
    call, loop = [], []
    for _ in range(rounds):
        loop.append(quiet(run_loop)[:2])
        call.append(quiet(run_call)[:2])
    med = lambda x: float(np.median(x))
    info = call[-1][1]
    row = dict(case=name, n_steps=T, B=B, nodes=int(np.prod(dims)), rounds=rounds, same_bits=same, path=info['path'],
               parts=info['parts'], nnz=info['nnz'], bytes=info['bytes'],
               call_wall_s=med([c[0] for c in call]), call_wall_s_all_rounds=[c[0] for c in call],
               entries_ms=med([c[1]['entries_ms'] for c in call]), sort_ms=med([c[1]['sort_ms'] for c in call]),
               push_ms=med([c[1]['push_ms'] for c in call]),
               loop_wall_s=med([c[0] for c in loop]), loop_wall_s_all_rounds=[c[0] for c in loop],
               loop_kernel_ms=med([c[1] for c in loop]))
    row['call_kernel_ms'] = row['entries_ms'] + row['sort_ms'] + row['push_ms']
    row['loop_over_call_wall'] = row['loop_wall_s'] / row['call_wall_s']
    row['loop_over_call_kernel'] = row['loop_kernel_ms'] / row['call_kernel_ms']
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--small', action='store_true', help='tiny problems: a rehearsal, not a measurement')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'horizon_forward_times.json'))
    a = ap.parse_args()
    nat.require_gpu()
    nat.check(nat.lib().sdp_set_device(0))
    rows = []
    out = dict(device=nat.device_info(0), small=bool(a.small), real_bytes=8, rows=rows,
               yardstick='the loop of transition_operator(pol[k], t_k=k), push(mu, 1) per vector and close()')
    for name, s, T in workloads(a.small):
        _, pol = quiet(s.bellman_recursion, T, np.zeros(tuple(len(g) for g in s.state_grid)))
        for B in (1, 64):
            rows.append(measure(name, s, T, pol, B, 3))
            print(json.dumps(rows[-1], sort_keys=True), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'w') as f:                    # (after every row: a run cut short keeps what it has)
                json.dump(out, f, indent=1, sort_keys=True)
                f.write('\n')


if __name__ == '__main__':
    main()
