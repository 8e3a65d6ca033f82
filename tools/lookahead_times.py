"""What the one-step lookahead at arbitrary states (csrc/sdp_lookahead_kernel.h) costs, written to
profiles/lookahead_times.json.  Searev's grid (31 x 61 x 61), 9 perturbation points, 8-byte reals.

  (a) against the sweep: `lookahead` with B = S states placed at the nodes -- the cells and the gathers of one sweep;
      the extra work is the box and the state reads -- against the direct sweep (kernel = 'generic') measured in the
      same process.  Kernel times from the HIP events around the launches.  Accepted at ratio <= 1.10 (the margin
      of DESIGN.md 5c: the boxes differ 2-4 % run to run).  Both lattices are timed: made on the device, made by the host.
  (b) closed loop: `simulate_lookahead` at B = 65 536, T = 64, the device path against path='host' (one sdp_lookahead
      call per step with a host-made lattice, the model's step by the callables): wall times of the calls and the
      kernel time of the device path.

Warm chip (every path once before the timed rounds, which also checks equal bits), the paths in turn within one
process, three rounds, the median of the rounds.

    python tools/lookahead_times.py [--small] [--out profiles/lookahead_times.json]
"""
import argparse
import contextlib
import io
import itertools
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


def same(a, b):
    return all(np.array_equal(p, q, equal_nan=True) for p, q in zip(a, b))


def problem(small):
    """(solver for the lookahead, solver for the direct sweep): Searev's grid and lattice"""
    kw = dict(n_E=9, n_S=11, n_A=10, step=0.05) if small else {}
    look = models.searev(**kw)[1]
    sweep = models.searev(**kw)[1]
    sweep.kernel = 'generic'
    return look, sweep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--small', action='store_true', help='a tiny problem: a rehearsal, not a measurement')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lookahead_times.json'))
    a = ap.parse_args()
    nat.require_gpu()
    nat.check(nat.lib().sdp_set_device(0))
    rounds, sweeps = 3, 10
    B_sim, T = (257, 4) if a.small else (65536, 64)
    s, v = problem(a.small)
    dims = s._state_grid_shape
    S = int(np.prod(dims))
    rng = np.random.default_rng(1)
    J_next = rng.standard_normal(dims)
    nodes = np.array(list(itertools.product(*s.state_grid)))
    plan = v._kernel_plan()
    cells = int(np.prod(plan['n'].astype(np.int64), axis=0).sum()) * plan['W']

    # ---- (a) ----
    Jv, pol = quiet(v.value_iteration, J_next, report_time=False)
    iv = v.last_policy_index
    vprob = v._problem()
    vprob.set_value(J_next)

    def sweep_ms():
        return quiet(vprob.bench_sweeps, sweeps)[1] / sweeps

    def look_ms(path):
        out = quiet(s.lookahead, J_next, nodes, path=path)
        return s._lookahead_prob.last_kernel_ms(), out

    for path in (None, 'host'):                                  # warm-up, and the bits
        _, (J, u, idx) = look_ms(path)
        assert same((J.reshape(dims), u.reshape(dims + (1,)), idx.reshape(dims)), (Jv, pol, iv)), path
    sweep_ms()
    t_sweep, t_dev, t_host = [], [], []
    for _ in range(rounds):
        t_sweep.append(sweep_ms())
        t_dev.append(look_ms(None)[0])
        t_host.append(look_ms('host')[0])
    med = lambda x: float(np.median(x))
    part_a = dict(states=S, cells=cells,
                  direct_sweep_ms=med(t_sweep), direct_sweep_ms_all_rounds=t_sweep,
                  lookahead_device_lattice_ms=med(t_dev), lookahead_device_lattice_ms_all_rounds=t_dev,
                  lookahead_host_lattice_ms=med(t_host), lookahead_host_lattice_ms_all_rounds=t_host,
                  gcells_per_s_sweep=cells / med(t_sweep) * 1e-6, gcells_per_s_lookahead=cells / med(t_dev) * 1e-6,
                  ratio_device_lattice=med(t_dev) / med(t_sweep), ratio_host_lattice=med(t_host) / med(t_sweep),
                  accepted_at_most=1.10, met=bool(med(t_dev) / med(t_sweep) <= 1.10), same_bits_as_the_sweep=True)

    # ---- (b) ----
    lo = np.array([g[0] for g in s.state_grid])
    hi = np.array([g[-1] for g in s.state_grid])
    x0 = lo + (hi - lo) * rng.random((B_sim, len(dims)))
    _, w = s.monte_carlo_draws(3, B_sim, T)
    paths = {'device': lambda: s.simulate_lookahead(J_next, x0, w), 'host': lambda: s.simulate_lookahead(J_next, x0, w, path='host')}
    assert same(quiet(paths['device']), quiet(paths['host']))
    wall = {k: [] for k in paths}
    kern = []
    for _ in range(rounds):
        for k, f in paths.items():
            t = time.perf_counter()
            quiet(f)
            wall[k].append(time.perf_counter() - t)
            if k == 'device':
                kern.append(s._lookahead_prob.last_kernel_ms())
    part_b = dict(trajectories=B_sim, steps=T,
                  device_wall_s=med(wall['device']), device_wall_s_all_rounds=wall['device'],
                  device_kernel_ms=med(kern), device_kernel_ms_all_rounds=kern,
                  host_wall_s=med(wall['host']), host_wall_s_all_rounds=wall['host'],
                  host_over_device_wall=med(wall['host']) / med(wall['device']), same_bits=True)
    out = dict(device=nat.device_info(0), small=bool(a.small), grid=list(dims), law_points=int(plan['W']), real_bytes=8,
               max_controls=int(plan['max_u']), lanes=int(s._lookahead_prob.info['lanes']), rounds=rounds,
               a_against_the_sweep=part_a, b_closed_loop=part_b)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == '__main__':
    main()
