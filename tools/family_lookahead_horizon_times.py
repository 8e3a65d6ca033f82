"""What running a family's closed loops under lookahead controls over a horizon in one device call
(SolverFamily.simulate_lookahead and SolverFamily.monte_carlo_lookahead_horizon,
csrc/sdp_family_lookahead_horizon_kernel.h) gains over the loop of solo DPSolver.simulate_lookahead and
DPSolver.monte_carlo_lookahead calls with the same time-indexed cost-to-go, written to
profiles/family_lookahead_horizon_times.json.

  pv       models.pv_storage (deterministic, `data[k]` in the cost, 50 nodes, up to 2001 lattice points a state) over 64
           storage capacities, none coinciding with a constant of the box, T = 48 steps under the cost-to-go of
           `fam.bellman_recursion`: `simulate_lookahead` of B = 256 and 4096 trajectories a member.  The solo calls take
           the HOST path here (one device call per step and member): there is no solo kernel time to compare with.
  ar1      storage-AR1 on 41 x 61 nodes, control step 0.1, 9 perturbation points, over 64 capacities, T = 200 steps under
           the time-indexed cost-to-go of `fam.bellman_recursion`: `simulate_lookahead` at B = 256, Monte Carlo at B = 256
           and 4096.  The solo calls take the device path.

The yardstick is the loop of solo calls on the same inputs, on the same commit, units compiled beforehand.  Per path: wall
time of the call (perf_counter) and the HIP-event time of its launches (the solo loop's: the sum over the members, device
path only); for the family also the host time spent on the traces and the table (`_lookahead_horizon_tables`), which is
part of its wall time, and one member alone as a family of one.  Warm chip: both paths once before the timed rounds, which
also compares their bits; the paths in turn within one process; the median of three rounds.  The family runs as one chunk
of members (chunk_bytes is raised for that: `last_kernel_ms` covers one handle); its cost-to-go goes up in cuts of
horizon_chunk_bytes as it stands.

    python tools/family_lookahead_horizon_times.py [--small] [--compile-only] [--out profiles/family_lookahead_horizon_times.json]
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

from stodynprog_amd import SolverFamily, codegen, models, _native as nat           # noqa: E402
from stodynprog_amd.trace import TraceError                                       # noqa: E402

FIELDS = ('cost_sum', 'n_outside', 'x_final')


def quiet(f, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all='ignore'):
        return f(*a, **kw)


def pv_members(P, small):
    kw = dict(T=6, N_E=9, u_step=0.05) if small else {}
    return [models.pv_storage(E_rated=float(E), **kw)[1] for E in np.linspace(1.13, 4.28, P)]


def ar1_members(P, small):
    kw = dict(n_E=7, n_P=5, n_w=3, steps=(0.5, 0.1)) if small else dict(steps=(0.1, 0.1))
    return [models.storage_ar1(E_rated=float(E), **kw)[1] for E in np.linspace(2.5, 20.5, P)]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def registers(source):
    """{kernel: (VGPRs, SGPRs, SGPR spills)} of a unit, from the notes of its code object"""
    llvm = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(nat.HIPCC))), 'llvm', 'bin')
    with tempfile.TemporaryDirectory() as tmp:
        elf = os.path.join(tmp, 'unit.elf')
        subprocess.run([os.path.join(llvm, 'clang-offload-bundler'), '--unbundle', '--type=o',
                        '--targets=hipv4-amdgcn-amd-amdhsa--gfx950', '--input=' + nat.compile_model(source), '--output=' + elf],
                       check=True, capture_output=True)
        notes = subprocess.run([os.path.join(llvm, 'llvm-readelf'), '--notes', elf], check=True, capture_output=True, text=True).stdout
    out = {}
    for block in notes.split('  - .agpr_count')[1:]:
        name = re.search(r'^\s+\.name:\s+(\w+)\s*$', block, re.M).group(1)
        f = {k: int(v) for k, v in re.findall(r'^\s+(\.[a-z_]+):\s+(\d+)\s*$', block, re.M)}
        out[name] = dict(vgpr=f['.vgpr_count'], sgpr=f['.sgpr_count'], sgpr_spills=f['.sgpr_spill_count'],
                         scratch_bytes=f['.private_segment_fixed_size'])
    return out


def solo_unit(s, t_k):
    """the source of a member's solo lookahead unit (DPSolver._lookahead_unit's)"""
    box_t = None if s.sys.stationnary else t_k
    tb = s._trace_box_now(box_t)
    box = tb if (not isinstance(tb, TraceError) and tb.t_value is None) else None
    return codegen.lookahead_unit(s._trace_now(t_k), s.dtype, s._box_plan(box_t)['lanes'], box)


def unit_sources(make, P, T, small):
    """every unit a workload runs: the family's (all members and one alone) and the solo lookahead units of the members"""
    out = []
    for members in (make(P, small), make(P, small)[:1]):
        fam = SolverFamily(members)
        tabs, _, _, look = fam._lookahead_horizon_tables(T, 0)
        out += [tabs['source'], look['source']]
        if not fam.stationnary:
            out += [fam._tables(t)['source'] for t in range(T)]         # (bellman_recursion: a unit per step's lanes)
    for s in make(P, small):
        out += [solo_unit(s, t) for t in (range(T) if not s.sys.stationnary else [None])]
    return list(dict.fromkeys(out))


def measure(name, make, P, T, B, what, J_next, rounds, small):
    fam, solo, one = SolverFamily(make(P, small)), make(P, small), SolverFamily(make(P, small)[:1])
    fam.chunk_bytes = 1 << 40
    d = len(fam.dims)
    x0 = np.zeros((P, B, d))                                     # every member starts with an empty store
    if what == 'simulate_lookahead' and fam.W:
        _, w = fam.monte_carlo_draws(1, B, T)
    else:
        w = None
    mc_kw = dict(seed=1, n_burn=T // 10)

    def run(f, J, x, w_):
        t = time.perf_counter()
        if what == 'simulate_lookahead':
            out = f.simulate_lookahead(J, x, w_, n_steps=T)
        else:
            out = f.monte_carlo_lookahead_horizon(J, x, T, **mc_kw)
        return time.perf_counter() - t, f.last_kernel_ms(), out

    run_family = lambda: run(fam, J_next, x0, w)
    run_one = lambda: run(one, J_next[:1], x0[:1], None if w is None else w[:1])

    def run_solo():
        t = time.perf_counter()
        out, ms, paths = [], 0., set()
        for p, s in enumerate(solo):
            if what == 'simulate_lookahead':
                out.append(quiet(s.simulate_lookahead, J_next[p], x0[p], None if w is None else w[p], n_steps=T))
            else:
                out.append(quiet(s.monte_carlo_lookahead, J_next[p], x0[p], T, **mc_kw))
            paths.add(s.backend_info['lookahead_path'])
            if paths == {'device'}:
                ms += s._lookahead_prob.last_kernel_ms()
        return time.perf_counter() - t, (ms if paths == {'device'} else None), out, paths

    # warm-up, and the bits of the two paths
    _, _, a = run_family()
    _, _, each, paths = run_solo()
    run_one()
    if what == 'simulate_lookahead':
        same = all(np.array_equal(bits(a[i][p]), bits(each[p][i])) for p in range(P) for i in range(4))
    else:
        same = all(np.array_equal(bits(getattr(a, f)[p]), bits(getattr(each[p], f))) for p in range(P) for f in FIELDS)
    assert same, '{} {} B = {}: the family and the solo loop differ: nothing to time'.format(name, what, B)
    t = time.perf_counter()
    look = fam._lookahead_horizon_tables(T, 0)[3]
    tracing = time.perf_counter() - t
    times = dict(family=[], solo=[], one_member=[])
    for _ in range(rounds):
        for path, f in (('solo', run_solo), ('family', run_family), ('one_member', run_one)):
            got = f()
            times[path].append((got[0], got[1]))
    med = lambda x: None if any(v is None for v in x) else float(np.median(x))
    row = dict(fam.backend_info['horizon'], case=name, call=what, rounds=rounds, same_bits=bool(same), lanes=fam.backend_info['lanes'],
               family_tables_s=tracing, solo_path=sorted(paths), registers=registers(look['source']))
    for path, got in times.items():
        row[path + '_wall_s'] = med([g[0] for g in got])
        row[path + '_wall_s_all_rounds'] = [g[0] for g in got]
        row[path + '_kernel_ms'] = med([g[1] for g in got])
    row['solo_over_family_wall'] = row['solo_wall_s'] / row['family_wall_s']
    row['family_over_solo_kernel'] = None if row['solo_kernel_ms'] is None else row['family_kernel_ms'] / row['solo_kernel_ms']
    row['family_over_members_times_one_kernel'] = row['family_kernel_ms'] / (P * row['one_member_kernel_ms'])
    row['tables_share_of_family_wall'] = tracing / row['family_wall_s']
    fam.close()
    one.close()
    for s in solo:
        for k in [k for k in s._cache if k[0] == 'problem']:
            s._cache.pop(k).close()
    return row


def cost_to_go(make, P, T, small):
    """(P, T) + dims: the backward pass of the family from a zero final cost; step k decides with the cost-to-go of k + 1"""
    fam = SolverFamily(make(P, small))
    J_fin = np.zeros((P,) + fam.dims)
    J, _ = fam.bellman_recursion(T, J_fin)
    fam.close()
    return np.concatenate([J[:, 1:], J_fin[:, None]], axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--small', action='store_true', help='tiny problems: a rehearsal, not a measurement')
    ap.add_argument('--compile-only', action='store_true', help='compile the units of the workloads (no GPU needed) and stop')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'family_lookahead_horizon_times.json'))
    a = ap.parse_args()
    P = 3 if a.small else 64
    plan = [('pv', pv_members, 6 if a.small else 48, [('simulate_lookahead', B) for B in ((5, 70) if a.small else (256, 4096))]),
            ('ar1', ar1_members, 8 if a.small else 200,
             [('simulate_lookahead', 70 if a.small else 256)] + [('monte_carlo_lookahead', B) for B in ((70, 300) if a.small else (256, 4096))])]
    if a.compile_only:
        from concurrent.futures import ThreadPoolExecutor
        sources = [s for _, make, T, _ in plan for s in unit_sources(make, P, T, a.small)]
        with ThreadPoolExecutor(max_workers=min(6, os.cpu_count() or 1)) as pool:
            print('compiled', len(set(pool.map(nat.compile_model, sources))), 'units')
        return
    nat.require_gpu()
    nat.check(nat.lib().sdp_set_device(0))
    rows = []
    out = dict(device=nat.device_info(0), small=bool(a.small), real_bytes=8, members=P, rows=rows)
    for name, make, T, calls in plan:
        J_next = cost_to_go(make, P, T, a.small)
        for what, B in calls:
            rows.append(measure(name, make, P, T, B, what, J_next, 3, a.small))
            print(json.dumps(rows[-1], sort_keys=True), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'w') as f:                    # (after every row: a run cut short keeps what it has)
                json.dump(out, f, indent=1, sort_keys=True)
                f.write('\n')


if __name__ == '__main__':
    main()
