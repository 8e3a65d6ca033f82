"""What running the finite-horizon policies of a family forward in one device call (SolverFamily.simulate and
SolverFamily.monte_carlo_horizon, csrc/sdp_family_horizon_kernel.h) gains over the loop of solo DPSolver.simulate and
DPSolver.monte_carlo calls with the same time-indexed policies, written to profiles/family_horizon_times.json.

  pv       models.pv_storage (deterministic, `data[k]` in the cost, 50 nodes) over 64 storage capacities, T = 48 steps
           under the policies of `fam.bellman_recursion`: `simulate` of B = 1, 256 and 4096 trajectories a member
  ar1      storage-AR1 on 41 x 61 nodes, 9 perturbation points, over 64 capacities, T = 200 steps under the time-indexed
           policies of `fam.bellman_recursion` (a receding schedule): `simulate` at B = 256, Monte Carlo at B = 256 and 4096

The yardstick is the loop of solo calls on the same inputs, kernel = 'auto' (what a user's loop runs), units compiled
and problems created beforehand.  Per path: wall time of the call (perf_counter) and the HIP-event time of its launches
(the solo loop's: the sum over the members); for the family also the host time spent on the P x T traces and the table
(`_horizon_tables`), which is part of its wall time.  Warm chip: both paths once before the timed rounds, which also
compares their bits; the paths in turn within one process; the median of three rounds.  The family runs as one chunk of
members (chunk_bytes is raised for that: `last_kernel_ms` covers one handle); its policy goes up in cuts of
horizon_chunk_bytes as it stands.

    python tools/family_horizon_times.py [--small] [--out profiles/family_horizon_times.json]
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

FIELDS = ('cost_sum', 'n_outside', 'x_final')


def quiet(f, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all='ignore'):
        return f(*a, **kw)


def pv_members(P, small):
    kw = dict(T=6, N_E=9, u_step=0.05) if small else {}
    return [models.pv_storage(E_rated=float(E), **kw)[1] for E in np.linspace(1., 4., P)]


def ar1_members(P, small):
    kw = dict(n_E=7, n_P=5, n_w=3, steps=(0.5, 0.1)) if small else dict(steps=(0.1, 0.1))
    return [models.storage_ar1(E_rated=float(E), **kw)[1] for E in np.linspace(2., 20., P)]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def measure(name, make, P, T, B, what, pol, rounds, small):
    fam, solo = SolverFamily(make(P, small)), make(P, small)
    fam.chunk_bytes = 1 << 40
    d = len(fam.dims)
    # every member starts with an empty store
    x0 = np.zeros((P, B, d))
    if what == 'simulate' and fam.W:
        _, w = fam.monte_carlo_draws(1, B, T)
    else:
        w = None
    mc_kw = dict(seed=1, n_burn=T // 10)

    def run_family():
        t = time.perf_counter()
        if what == 'simulate':
            out = fam.simulate(pol, x0, w, n_steps=T)
        else:
            out = fam.monte_carlo_horizon(pol, x0, T, **mc_kw)
        return time.perf_counter() - t, fam.last_kernel_ms(), out

    def run_solo():
        t = time.perf_counter()
        out, ms = [], 0.
        for p, s in enumerate(solo):
            if what == 'simulate':
                out.append(quiet(s.simulate, pol[p], x0[p], None if w is None else w[p], n_steps=T))
            else:
                out.append(quiet(s.monte_carlo, pol[p], x0[p], T, **mc_kw))
            assert s.backend_info['horizon_path'] == 'device'
            ms += s._problem(None if s.sys.stationnary else 0).last_kernel_ms()
        return time.perf_counter() - t, ms, out

    # warm-up, and the bits of the two paths
    _, _, a = run_family()
    _, _, each = run_solo()
    if what == 'simulate':
        same = all(np.array_equal(bits(a[i][p]), bits(each[p][i])) for p in range(P) for i in range(3))
    else:
        same = all(np.array_equal(bits(getattr(a, f)[p]), bits(getattr(each[p], f))) for p in range(P) for f in FIELDS)
    assert same, '{} {} B = {}: the family and the solo loop differ: nothing to time'.format(name, what, B)
    t = time.perf_counter()
    fam._horizon_tables(T, 0)
    tracing = time.perf_counter() - t
    times = dict(family=[], solo=[])
    for _ in range(rounds):
        for path, run in (('solo', run_solo), ('family', run_family)):
            wall, ms, _ = run()
            times[path].append((wall, ms))
    med = lambda x: float(np.median(x))
    # (backend_info['horizon']: members, n_traj, n_steps, timed, time_specialized, chunks, step_chunks, launches)
    row = dict(fam.backend_info['horizon'], case=name, call=what, rounds=rounds, same_bits=bool(same),
               family_tables_s=tracing, solo_kernel=solo[0].backend_info.get('kernel'))
    for path, got in times.items():
        row[path + '_wall_s'] = med([g[0] for g in got])
        row[path + '_wall_s_all_rounds'] = [g[0] for g in got]
        row[path + '_kernel_ms'] = med([g[1] for g in got])
    row['solo_over_family_wall'] = row['solo_wall_s'] / row['family_wall_s']
    row['family_over_solo_kernel'] = row['family_kernel_ms'] / row['solo_kernel_ms']
    row['tables_share_of_family_wall'] = tracing / row['family_wall_s']
    fam.close()
    for s in solo:
        for k in [k for k in s._cache if k[0] == 'problem']:
            s._cache.pop(k).close()
    return row


def policies(make, P, T, small):
    """(P, T) + dims + (nu,): the backward pass of the family, from a zero final cost"""
    fam = SolverFamily(make(P, small))
    _, pol = fam.bellman_recursion(T, np.zeros(fam.dims))
    fam.close()
    return pol


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--small', action='store_true', help='tiny problems: a rehearsal, not a measurement')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'family_horizon_times.json'))
    a = ap.parse_args()
    nat.require_gpu()
    nat.check(nat.lib().sdp_set_device(0))
    P = 3 if a.small else 64
    rows = []
    out = dict(device=nat.device_info(0), small=bool(a.small), real_bytes=8, members=P, rows=rows,
               accepted='at n_traj = 4096 the family\'s kernel time is at most 1.10 of the summed solo kernel times')
    plan = [('pv', pv_members, 6 if a.small else 48, [('simulate', B) for B in ((1, 70) if a.small else (1, 256, 4096))]),
            ('ar1', ar1_members, 8 if a.small else 200,
             [('simulate', 70 if a.small else 256)] + [('monte_carlo', B) for B in ((70, 300) if a.small else (256, 4096))])]
    for name, make, T, calls in plan:
        pol = policies(make, P, T, a.small)
        for what, B in calls:
            rows.append(measure(name, make, P, T, B, what, pol, 3, a.small))
            print(json.dumps(rows[-1], sort_keys=True), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'w') as f:                    # (after every row: a run cut short keeps what it has)
                json.dump(out, f, indent=1, sort_keys=True)
                f.write('\n')
    full = [r for r in rows if r['n_traj'] == 4096]
    if full:
        print('kernel time against the solo loop at n_traj = 4096:',
              ', '.join('{} {} {:.3f}'.format(r['case'], r['call'], r['family_over_solo_kernel']) for r in full))


if __name__ == '__main__':
    main()
