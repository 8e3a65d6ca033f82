"""What the kernels of several perturbation variables (csrc/sdp_multiw_kernel.h) cost next to the one-variable direct
kernel, written to profiles/multiw_times.json.  Searev's grid (31 x 61 x 61), one sweep:

  one variable     Searev as it is, kernel = 'generic': the direct kernel of sdp_sweep_kernel.h, 9 points -- the YARDSTICK
  W = (9, 1)       the same model with a second perturbation variable of ONE point that the callables take and do not
                   use -- the new kernel doing the same work (9 cells per control), and the same bits
  W = (9, 9)       models.two_inflows on the same grid: 81 cells per control, 81 controls per node

Warm chip (sweeps before the timed ones), the three in turn within one process, three rounds, the median of the rounds;
per-sweep kernel time from the HIP events around the sweep kernels (sdp_problem_bench_sweeps).  Cells per second =
nodes x controls x law points / kernel time.  Accepted: W = (9, 1) at most 10 % slower than the yardstick.

    python tools/multiw_times.py [--small] [--out profiles/multiw_times.json]
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

from stodynprog_amd import SysDescription, DPSolver, models, _native as nat           # noqa: E402


def quiet(f, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return f(*a, **kw)


def searev_two(grid):
    """Searev with a second perturbation variable of one point (value 0) that the callables take and do not use"""
    wec, one = models.searev(n_E=grid[0], n_S=grid[1], n_A=grid[2])
    two = SysDescription((3, 1, 2), name='Searev + Storage, W = (9, 1)')
    two.dyn = lambda E, S, A, P, innov, idle: wec.dyn(E, S, A, P, innov)
    two.cost = lambda E, S, A, P, innov, idle: wec.cost(E, S, A, P, innov)
    two.control_box = wec.control_box
    solver = DPSolver(two)
    solver.state_grid, solver.control_steps = one.state_grid, one.control_steps
    solver._state_grid_shape, solver._state_ref_ind = one._state_grid_shape, one._state_ref_ind
    solver.perturb_grid = [one.perturb_grid[0], np.array([0.0])]
    solver.perturb_proba = [one.perturb_proba[0], np.array([1.0])]
    return one, solver


def cells(solver):
    plan = solver._kernel_plan()
    n = plan['n'].astype(np.int64)
    controls = np.prod(n, axis=0)
    S = int(np.prod(solver._shape()))
    per_node = int(controls.sum()) if plan['per_node'] else int(controls[0]) * S
    return per_node * max(plan['W'], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--small', action='store_true', help='a tiny grid: a rehearsal, not a measurement')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'multiw_times.json'))
    a = ap.parse_args()
    nat.require_gpu()
    nat.check(nat.lib().sdp_set_device(0))
    grid = (9, 11, 10) if a.small else (31, 61, 61)
    reps, rounds = (2, 3) if a.small else (10, 3)
    one, two = searev_two(grid)
    one.kernel = 'generic'
    _, both = models.two_inflows(n_a=grid[0], n_b=grid[1], n_y=grid[2], n_w=(9, 9))
    runs = {'one variable, W = 9 (direct kernel)': one, 'W = (9, 1)': two, 'W = (9, 9), two_inflows': both}
    V = {k: np.zeros(s._shape()) for k, s in runs.items()}
    out_J = {}
    probs = {}
    for k, s in runs.items():                                   # warm-up: code object, buffers, a first sweep
        out_J[k] = quiet(s.value_iteration, V[k], report_time=False)[0]
        probs[k] = s._problem(None)
        probs[k].set_value(V[k])
        probs[k].bench_sweeps(2)
    assert np.array_equal(out_J['one variable, W = 9 (direct kernel)'], out_J['W = (9, 1)']), \
        'the unused variable changed the result'
    ms = {k: [] for k in runs}
    for _ in range(rounds):                                     # alternating, same process, same box
        for k in runs:
            _, kern = probs[k].bench_sweeps(reps)
            ms[k].append(kern / reps)
    rows = {}
    for k, s in runs.items():
        med = float(np.median(ms[k]))
        rows[k] = dict(kernel_ms_per_sweep=med, kernel_ms_all_rounds=ms[k], cells_per_sweep=cells(s),
                       cells_per_second=cells(s) / (med * 1e-3), lanes_per_node=s.backend_info['lanes_per_node'],
                       perturb_vars=s.backend_info['perturb_vars'], kernel=s.backend_info['kernel'])
    base = rows['one variable, W = 9 (direct kernel)']['kernel_ms_per_sweep']
    ratio = rows['W = (9, 1)']['kernel_ms_per_sweep'] / base
    out = dict(device=nat.device_info(0), small=bool(a.small), grid=list(grid), sweeps_per_round=reps, rounds=rounds,
               runs=rows, w91_over_one_variable=ratio, accepted_at_most=1.10, accepted=bool(ratio <= 1.10),
               same_bits_w91=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == '__main__':
    main()
