"""What the Monte Carlo evaluation under lookahead controls (kernel sdp_montecarlo_lookahead,
csrc/sdp_lookahead_kernel.h) costs, written to profiles/mc_lookahead_times.json.  Searev's grid (31 x 61 x 61),
9 perturbation points, 8-byte reals, B = 65 536 trajectories of T = 64 steps.

  (a) kernel time: `sdp_montecarlo_lookahead` against `sdp_simulate_lookahead` fed the same draws (the HIP events
      around the launches).  The same backups; one Philox call and one table lookup per step more, T (d + nu + 2) B
      stores fewer.  Accepted at ratio <= 1.10.
  (b) wall time of one call: `monte_carlo_lookahead` against the route without it -- `monte_carlo_draws`, then
      `simulate_lookahead`, then the sums on the host.
  (c) the call of (a) with occupancy=True, against (a).

Warm chip (every path once before the timed rounds, which also checks equal bits), the paths in turn within one
process, three rounds, the median of the rounds.

    python tools/mc_lookahead_times.py [--small] [--out profiles/mc_lookahead_times.json]
"""
import argparse
import contextlib
import io
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stodynprog_amd import models, _native as nat           # noqa: E402


def quiet(f, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all='ignore'):
        return f(*a, **kw)


def registers(module):
    """{kernel: (VGPRs, SGPRs, scratch bytes, vector spills)} of the closed-loop kernels, from the code object's notes"""
    llvm = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(nat.HIPCC))), 'llvm', 'bin')
    with tempfile.TemporaryDirectory() as tmp:
        elf = os.path.join(tmp, 'unit.elf')
        subprocess.run([os.path.join(llvm, 'clang-offload-bundler'), '--unbundle', '--type=o',
                        '--targets=hipv4-amdgcn-amd-amdhsa--gfx950', '--input=' + module, '--output=' + elf],
                       check=True, capture_output=True)
        notes = subprocess.run([os.path.join(llvm, 'llvm-readelf'), '--notes', elf], check=True, capture_output=True,
                               text=True).stdout
    out = {}
    for block in notes.split('  - .agpr_count')[1:]:
        name = re.search(r'^\s+\.name:\s+(\w+)\s*$', block, re.M).group(1)
        f = {k: int(v) for k, v in re.findall(r'^\s+(\.[a-z_]+):\s+(\d+)\s*$', block, re.M)}
        if name in ('sdp_simulate_lookahead', 'sdp_montecarlo_lookahead'):
            out[name] = dict(vgprs=f['.vgpr_count'], sgprs=f['.sgpr_count'], scratch_bytes=f['.private_segment_fixed_size'],
                             vgpr_spills=f['.vgpr_spill_count'], sgpr_spills=f['.sgpr_spill_count'])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--small', action='store_true', help='a tiny problem: a rehearsal, not a measurement')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mc_lookahead_times.json'))
    a = ap.parse_args()
    nat.require_gpu()
    nat.check(nat.lib().sdp_set_device(0))
    rounds, seed = 3, 3
    B, T = (257, 4) if a.small else (65536, 64)
    s = models.searev(**(dict(n_E=9, n_S=11, n_A=10, step=0.05) if a.small else {}))[1]
    dims = s._state_grid_shape
    rng = np.random.default_rng(1)
    J_next = rng.standard_normal(dims)
    lo = np.array([g[0] for g in s.state_grid])
    hi = np.array([g[-1] for g in s.state_grid])
    x0 = lo + (hi - lo) * rng.random((B, len(dims)))

    def old_route():
        """(cost_sum, x_final), kernel ms: the draws on the host, the closed loop, the sums on the host"""
        _, w = s.monte_carlo_draws(seed, B, T)
        x, u, g, q = s.simulate_lookahead(J_next, x0, w)
        ms = s._lookahead_prob.last_kernel_ms()
        acc = np.zeros(B)
        for k in range(T):
            acc = acc + g[k]
        return (acc, x[T]), ms

    def new_route(occupancy=False):
        res = s.monte_carlo_lookahead(J_next, x0, T, seed=seed, occupancy=occupancy)
        assert res.path == 'device'
        return (res.cost_sum, res.x_final), s._lookahead_prob.last_kernel_ms()

    paths = dict(simulate_lookahead_on_host_draws=old_route, monte_carlo_lookahead=new_route,
                 monte_carlo_lookahead_occupancy=lambda: new_route(True))
    first = {k: quiet(f)[0] for k, f in paths.items()}                   # warm-up, and the bits
    for k, out in first.items():
        assert all(np.array_equal(p, q, equal_nan=True) for p, q in zip(out, first['monte_carlo_lookahead'])), k
    wall = {k: [] for k in paths}
    kern = {k: [] for k in paths}
    for _ in range(rounds):
        for k, f in paths.items():
            t = time.perf_counter()
            _, ms = quiet(f)
            wall[k].append(time.perf_counter() - t)
            kern[k].append(ms)
    med = lambda v: float(np.median(v))
    rows = {k: dict(wall_s=med(wall[k]), wall_s_all_rounds=wall[k], kernel_ms=med(kern[k]), kernel_ms_all_rounds=kern[k])
            for k in paths}
    old, new, occ = (rows[k] for k in ('simulate_lookahead_on_host_draws', 'monte_carlo_lookahead',
                                        'monte_carlo_lookahead_occupancy'))
    ratio_a = new['kernel_ms'] / old['kernel_ms']
    out = dict(device=nat.device_info(0), small=bool(a.small), grid=list(dims), law_points=len(s.perturb_grid[0]),
               real_bytes=8, lanes=int(s._lookahead_prob.info['lanes']), trajectories=B, steps=T, rounds=rounds,
               same_bits=True, paths=rows,
               a_kernel_ratio=ratio_a, a_accepted_at_most=1.10, a_met=bool(ratio_a <= 1.10),
               b_wall_ratio=new['wall_s'] / old['wall_s'], b_lower=bool(new['wall_s'] < old['wall_s']),
               c_occupancy_kernel_ratio=occ['kernel_ms'] / new['kernel_ms'],
               registers=registers(s._lookahead_prob.info['module']))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == '__main__':
    main()
