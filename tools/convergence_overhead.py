#!/usr/bin/env python3
"""What the convergence check of `value_iterations(..., tol=...)` costs on the benchmark model (synthetic3d, 256^3,
float64, the column kernel): 50 sweeps without a check against the same 50 sweeps with the check after every sweep
(tol=0, check_every=1) and after every tenth (check_every=10).

Device time: HIP events around the whole loop inside the library -- sdp_problem_bench_sweeps (the sweeps back to back,
no check; it records two more events per sweep) and sdp_problem_vi_until (the same sweeps, the reduction k_diff_stats
and its 24-byte readback at every check; 'last only': one check, after sweep 50).  Wall time: the Python calls,
uploads and downloads included.  Warmed up first; each figure is the median of REPS runs in this one process.  The bytes/s of the reduction kernel itself come from a `rocprofv3 --kernel-trace
--stats` run of this script (it reads J and V once: 2 x 8 x 256^3 bytes).

    python tools/convergence_overhead.py [--out FILE.json]
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from stodynprog_amd import models, _native as nat

N_SWEEPS, REPS = 50, 5


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    nat.require_gpu()
    _, s = models.synthetic3d(N=256)
    V0 = models.synthetic3d_V0(s.state_grid)
    quiet(s.value_iterations, V0, 3)                                     # compile, plan, page in
    prob = [v for k, v in s._cache.items() if k[0] == 'problem'][0]
    prob.set_value(V0)
    prob.bench_sweeps(10)                                                # clocks up

    dev = {'none': [], 'last only': [], 'every 1': [], 'every 10': []}
    wall = {'none': [], 'every 1': [], 'every 10': []}
    done = {}
    for _ in range(REPS):
        prob.set_value(V0)
        loop_ms, _ = prob.bench_sweeps(N_SWEEPS)
        dev['none'].append(loop_ms)
        for name, c in (('last only', N_SWEEPS), ('every 1', 1), ('every 10', 10)):
            prob.set_value(V0)
            n, checked, stats, _ = prob.until(False, N_SWEEPS, False, 0, c, 0.0)
            done[name] = (n, len(checked))
            dev[name].append(prob.last_kernel_ms())
        for name, kw in (('none', {}), ('every 1', dict(tol=0.0)), ('every 10', dict(tol=0.0, check_every=10))):
            t = time.perf_counter()
            quiet(s.value_iterations, V0, N_SWEEPS, **kw)
            wall[name].append((time.perf_counter() - t) * 1e3)
    med = {k: float(np.median(v)) for k, v in dev.items()}
    medw = {k: float(np.median(v)) for k, v in wall.items()}
    base = med['none'] / N_SWEEPS
    res = dict(
        model='synthetic3d N=256 float64', kernel=s.backend_info.get('kernel'), sweeps=N_SWEEPS, reps=REPS,
        device=nat.device_info(0),
        sweeps_and_checks_run={k: dict(sweeps=v[0], checks=v[1]) for k, v in done.items()},
        device_loop_ms_median=med, device_loop_ms_all=dev,
        device_ms_per_sweep={k: v / N_SWEEPS for k, v in med.items()},
        extra_per_sweep_percent={k: 100.0 * (med[k] / N_SWEEPS - base) / base for k in ('every 1', 'every 10')},
        extra_per_sweep_percent_vs_last_only={k: 100.0 * (med[k] - med['last only']) / med['last only']
                                              for k in ('every 1', 'every 10')},
        # (a check after every sweep against one after the last: the same loop, 49 checks apart)
        extra_per_check_us=(med['every 1'] - med['last only']) / (done['every 1'][1] - 1) * 1e3,
        wall_ms_median=medw, wall_ms_all=wall,
        bytes_read_per_check=2 * 8 * 256 ** 3)
    line = json.dumps(res, indent=1)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
