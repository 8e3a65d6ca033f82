"""Times of DPSolver.monte_carlo on the device, written to profiles/montecarlo_times.json.

(a) the same job two ways -- Searev 31x61x61, B trajectories of T steps, the B cost means:
    the route through simulate (host draws + upload + kernel that stores every state, control and cost +
    download + host sum, each part listed) against monte_carlo;
(b) steps per second at a size simulate cannot hold: B = 2^20, occupancy off, on, and on without the in-wave
    combine (a unit built with SDP_MC_COMBINE=0).

Wall time around synchronised calls after a warm-up call; kernel time from the events around the launches
(sdp_problem_last_kernel_ms).  The registers of sdp_montecarlo are read from the code object.

    python tools/montecarlo_times.py [--small] [--out profiles/montecarlo_times.json]
"""
import argparse
import contextlib
import ctypes as C
import io
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stodynprog_amd import models, _native as nat                    # noqa: E402


def quiet(f, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return f(*a, **kw)


def kernel_ms(s):
    prob = [v for k, v in s._cache.items() if k[0] == 'problem'][-1]
    ms = C.c_double(0)
    nat.check(nat.lib().sdp_problem_last_kernel_ms(prob.h, C.byref(ms)))
    return ms.value


def timed(f, reps):
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        res = f()
        out.append(time.perf_counter() - t)
    return res, out


def code_object_notes(s, name='sdp_montecarlo'):
    """registers, LDS and scratch of kernel `name` in the solver's unit, from the code object's notes"""
    path = nat.compile_model(s._kernel_plan()['source'])
    llvm = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(nat.HIPCC))), 'llvm', 'bin')
    elf = path + '.elf.tmp'
    try:
        subprocess.run([os.path.join(llvm, 'clang-offload-bundler'), '--unbundle', '--type=o',
                        '--targets=hipv4-amdgcn-amd-amdhsa--gfx950', '--input=' + path, '--output=' + elf],
                       check=True, capture_output=True)
        notes = subprocess.run([os.path.join(llvm, 'llvm-readelf'), '--notes', elf], check=True, capture_output=True,
                               text=True).stdout
    finally:
        if os.path.exists(elf):
            os.remove(elf)
    for block in notes.split('  - .agpr_count')[1:]:
        if re.search(r'^\s+\.name:\s+{}\s*$'.format(name), block, re.M):
            f = {k: int(v) for k, v in re.findall(r'^\s+(\.[a-z_]+):\s+(\d+)\s*$', block, re.M)}
            return dict(vgprs=f['.vgpr_count'], sgprs=f['.sgpr_count'], scratch_bytes=f['.private_segment_fixed_size'],
                        vgpr_spills=f['.vgpr_spill_count'], static_lds_bytes=f['.group_segment_fixed_size'])
    raise RuntimeError('no kernel {} in {}'.format(name, path))


def same_job(B, T, reps):
    _, s = models.searev()
    pol = np.load(os.path.join(ROOT, 'tests', 'golden', 'g4_searev.npz'))['committed_policy']
    d, nu = 3, 1
    x0 = np.tile([10 / 3., 0., 0.], (B, 1))
    seed = 1

    def route():
        t0 = time.perf_counter()
        _, w = s.monte_carlo_draws(seed, B, T)
        t1 = time.perf_counter()
        x, u, g = quiet(s.simulate, pol, x0, w)
        t2 = time.perf_counter()
        acc = np.zeros(B)
        for k in range(T):
            acc = acc + g[k]
        t3 = time.perf_counter()
        return acc, (t1 - t0, t2 - t1, t3 - t2)

    route()                                                            # warm-up (code object, buffers)
    parts = []
    for _ in range(reps):
        acc, p = route()
        parts.append(p)
    quiet(s.monte_carlo, pol, x0, T, seed=seed)
    res, walls = timed(lambda: quiet(s.monte_carlo, pol, x0, T, seed=seed), reps)
    kms = kernel_ms(s)
    assert np.array_equal(res.cost_sum, acc), 'the two routes disagree'
    best = min(parts, key=sum)
    item = np.dtype(s.dtype).itemsize
    out = dict(model='searev 31x61x61', B=B, T=T, reps=reps,
               simulate_route_s=dict(host_draws=best[0], simulate_call=best[1], host_sum=best[2], total=sum(best)),
               simulate_call_all_s=[p[1] for p in parts],
               monte_carlo_wall_s=min(walls), monte_carlo_wall_all_s=walls, monte_carlo_kernel_ms=kms,
               bytes_over_pcie=dict(simulate=item * (T * B + (T + 1) * d * B + T * nu * B + T * B + d * B),
                                    monte_carlo=item * (2 * d * B + B) + 8 * B),
               same_bits=True,
               not_slower_than_the_simulate_call=bool(min(walls) <= min(p[1] for p in parts)))
    for k in [k for k in s._cache if k[0] == 'problem']:
        s._cache.pop(k).close()
    return out, s


def rates(B, T, reps):
    rows = {}
    for label, occupancy, debug in (('occupancy off', False, None), ('occupancy on', True, None),
                                    ('occupancy on, no in-wave combine', True, {'SDP_EXTRA_DEFINES': 'SDP_MC_COMBINE=0'})):
        _, s = models.searev()
        s.debug_defines = debug
        pol = np.load(os.path.join(ROOT, 'tests', 'golden', 'g4_searev.npz'))['committed_policy']
        x0 = np.array([10 / 3., 0., 0.])
        quiet(s.monte_carlo, pol, x0, min(T, 32), seed=2, n_traj=B, occupancy=occupancy)        # warm-up
        res, walls = timed(lambda: quiet(s.monte_carlo, pol, x0, T, seed=2, n_traj=B, occupancy=occupancy), reps)
        kms = kernel_ms(s)
        rows[label] = dict(wall_s=min(walls), wall_all_s=walls, kernel_ms=kms,
                           steps_per_second_kernel=B * T / (kms * 1e-3), steps_per_second_wall=B * T / min(walls),
                           mean=res.mean, stderr=res.stderr, n_outside=int(res.n_outside.sum()),
                           launches=-(-T // s.steps_per_launch),
                           busiest_node_share=(float(res.occupancy.max()) / float(res.occupancy.sum())
                                               if occupancy else None),
                           nodes_visited=int((res.occupancy > 0).sum()) if occupancy else None)
        for k in [k for k in s._cache if k[0] == 'problem']:
            s._cache.pop(k).close()
    return dict(model='searev 31x61x61', B=B, T=T, reps=reps, steps_per_launch=s.steps_per_launch, runs=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--small', action='store_true', help='tiny sizes: a rehearsal, not a measurement')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'montecarlo_times.json'))
    a = ap.parse_args()
    nat.require_gpu()
    nat.check(nat.lib().sdp_set_device(0))
    info = nat.device_info(0)
    if a.small:
        job, s = same_job(1024, 16, 2)
        rate = rates(1 << 12, 64, 2)
    else:
        job, s = same_job(65536, 512, 3)
        rate = rates(1 << 20, 2048, 2)
    cus = int(info['compute_units'])
    notes = code_object_notes(s)
    out = dict(device=info, small=bool(a.small), same_job=job, rate=rate, kernel=dict(
        notes, threads_per_workgroup=256, waves_launched_at_2e20=min(-(-(1 << 20) // 256), cus * 8) * 4,
        grid_cap_workgroups=cus * 8, dynamic_lds_bytes_9_points=8 * 8 + 9 * np.dtype(s.dtype).itemsize))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == '__main__':
    main()
