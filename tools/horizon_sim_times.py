"""What the closed loops under a time-indexed policy (csrc/sdp_horizon_kernel.h) cost, written to
profiles/horizon_sim_times.json.  Problem: the time-dependent storage of tests/horizon_cases.py at 200 x 200 nodes,
9 perturbation points, T = 512 steps, 8-byte reals, a different random policy at every step.

  (a) B = 65 536: wall time of the only device route there was -- T calls simulate(pol[k], x_k, w[k:k+1], t0=k), the
      state carried on the host -- against the one call simulate(pol, x0, w).  Accepted: the one call is not slower.
  (b) kernel time per step of sdp_simulate_h against sdp_simulate, with pol[0] used at every step (the extra work is
      a policy slice that changes per step: 320 KB here).  Target: ratio <= 1.10.
  (c) the figures of (b) for monte_carlo (sdp_montecarlo_h against sdp_montecarlo) at B = 2^20, occupancy off, and the
      wall times of the calls.

Warm chip (every path once before the timed rounds), the paths in turn within one process, three rounds, the median of
the rounds; kernel times from the HIP events around the launches (sdp_problem_last_kernel_ms), wall times from
time.perf_counter around the calls (uploads, launches, downloads, host conversions).  Every pair is checked for equal bits.

    python tools/horizon_sim_times.py [--small] [--out profiles/horizon_sim_times.json]
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
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.dont_write_bytecode = True

import horizon_sim as hs                                     # noqa: E402
from stodynprog_amd import _native as nat                    # noqa: E402


def quiet(f, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all='ignore'):
        return f(*a, **kw)


def step_by_step(s, pol, x0, w, T):
    """today's device route: one call per step, the state carried on the host"""
    x = x0
    xs, us, gs = [None] * (T + 1), [None] * T, [None] * T
    for k in range(T):
        xk, uk, gk = s.simulate(pol[k], x, w[k:k + 1], t0=k)
        xs[k], us[k], gs[k] = xk[0], uk[0], gk[0]
        x = xk[1]
    xs[T] = x
    return np.stack(xs), np.stack(us), np.stack(gs)


def same(a, b):
    return all(np.array_equal(p, q, equal_nan=True) for p, q in zip(a, b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--small', action='store_true', help='a tiny problem: a rehearsal, not a measurement')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'horizon_sim_times.json'))
    a = ap.parse_args()
    nat.require_gpu()
    nat.check(nat.lib().sdp_set_device(0))
    n, T, B, B_mc, rounds = (21, 8, 257, 1000, 3) if a.small else (200, 512, 65536, 1 << 20, 3)
    s = hs.timing_problem(n, 13 if a.small else n)
    dims = s._state_grid_shape
    rng = np.random.default_rng(1)
    pol = rng.uniform(-1.0, 1.0, (T,) + dims + (1,))
    same_pol = np.broadcast_to(pol[0], pol.shape)
    lo = np.array([g[0] for g in s.state_grid])
    hi = np.array([g[-1] for g in s.state_grid])
    x0 = lo + (hi - lo) * rng.random((B, 2))
    w = rng.normal(0.0, 0.3, (T, B))
    x0_mc = lo + (hi - lo) * rng.random((B_mc, 2))
    # the model's drift 0.15 (k - 3) is meant for 8 steps; over 512 the stock leaves the grid and is extrapolated: the
    # arithmetic per step is the same wherever the state is

    def prob():
        return s._problem(0, s._trace_now(0))

    paths = {
        'T calls of simulate (today)': lambda: step_by_step(s, pol, x0, w, T),
        'one call, time-indexed': lambda: s.simulate(pol, x0, w),
        'sdp_simulate, pol[0]': lambda: s.simulate(pol[0], x0, w),
        'sdp_simulate_h, pol[0] at every step': lambda: s.simulate(same_pol, x0, w),
        'sdp_montecarlo, pol[0]': lambda: s.monte_carlo(pol[0], x0_mc, T, seed=7),
        'sdp_montecarlo_h, pol[0] at every step': lambda: s.monte_carlo(same_pol, x0_mc, T, seed=7),
        'monte_carlo, time-indexed': lambda: s.monte_carlo(pol, x0_mc, T, seed=7),
    }
    # warm-up: code object, buffers, clocks; and the bits of every pair
    pairs = (('T calls of simulate (today)', 'one call, time-indexed'),
             ('sdp_simulate, pol[0]', 'sdp_simulate_h, pol[0] at every step'))
    for p, q in pairs:
        assert same(quiet(paths[p]), quiet(paths[q])), '{} and {} differ'.format(p, q)
    mc_a, mc_b = quiet(paths['sdp_montecarlo, pol[0]']), quiet(paths['sdp_montecarlo_h, pol[0] at every step'])
    assert same((mc_a.cost_sum, mc_a.x_final, mc_a.n_outside), (mc_b.cost_sum, mc_b.x_final, mc_b.n_outside))
    quiet(paths['monte_carlo, time-indexed'])
    wall = {k: [] for k in paths}
    kern = {k: [] for k in paths}
    for _ in range(rounds):                                      # in turn, same process, same box
        for k, f in paths.items():
            t = time.perf_counter()
            quiet(f)
            wall[k].append(time.perf_counter() - t)
            kern[k].append(prob().last_kernel_ms())              # (of the call's last launch sequence)
    rows = {}
    for k in paths:
        rows[k] = dict(wall_s=float(np.median(wall[k])), wall_s_all_rounds=wall[k])
        if k != 'T calls of simulate (today)':
            rows[k].update(kernel_ms=float(np.median(kern[k])), kernel_ms_all_rounds=kern[k],
                           kernel_us_per_step=float(np.median(kern[k])) * 1e3 / T)
    ratio_a = rows['one call, time-indexed']['wall_s'] / rows['T calls of simulate (today)']['wall_s']
    ratio_b = rows['sdp_simulate_h, pol[0] at every step']['kernel_ms'] / rows['sdp_simulate, pol[0]']['kernel_ms']
    ratio_c = rows['sdp_montecarlo_h, pol[0] at every step']['kernel_ms'] / rows['sdp_montecarlo, pol[0]']['kernel_ms']
    out = dict(device=nat.device_info(0), small=bool(a.small), grid=list(dims), law_points=9, steps=T, real_bytes=8,
               trajectories_simulate=B, trajectories_monte_carlo=B_mc, rounds=rounds,
               policy_bytes_per_step=int(np.prod(dims)) * 8, horizon_chunk_bytes=int(s.horizon_chunk_bytes),
               runs=rows, same_bits=True,
               a_one_call_over_T_calls_wall=ratio_a, a_accepted=bool(ratio_a <= 1.0),
               b_simulate_h_over_simulate_kernel=ratio_b, b_target_at_most=1.10, b_met=bool(ratio_b <= 1.10),
               c_montecarlo_h_over_montecarlo_kernel=ratio_c, c_target_at_most=1.10, c_met=bool(ratio_c <= 1.10))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == '__main__':
    main()
