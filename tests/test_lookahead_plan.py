"""The lookahead units on the CPU: every case of tests/lookahead_cases.py cross-compiles for gfx950 with kernels
sdp_lookahead and sdp_simulate_lookahead free of scratch memory and vector spills; the emitted box function,
compiled as HOST C++ into a small stand-alone program, gives the bits of the scalar control_box calls; no other unit
changes its generated text; and what the two methods refuse they refuse before a device is touched.  No GPU."""
import hashlib
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import lookahead_cases as lc
from stodynprog_amd import codegen, models, lookahead as la, _native as nat
from stodynprog_amd.trace import TraceError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM_BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(nat.HIPCC))), 'llvm', 'bin')
TARGET = 'hipv4-amdgcn-amd-amdhsa--gfx950'
BOXED = [c for c in lc.TRACED if c.box == 'device']


def _kernels(source, tmp_path):
    """{kernel name: integer fields of its code-object notes} (tests/test_horizon_sim_plan.py reads them the same way)"""
    bundle, elf = nat.compile_model(source), str(tmp_path / 'unit.elf')
    subprocess.run([os.path.join(LLVM_BIN, 'clang-offload-bundler'), '--unbundle', '--type=o', '--targets=' + TARGET,
                    '--input=' + bundle, '--output=' + elf], check=True, capture_output=True)
    notes = subprocess.run([os.path.join(LLVM_BIN, 'llvm-readelf'), '--notes', elf], check=True,
                           capture_output=True, text=True).stdout
    out = {}
    for block in notes.split('  - .agpr_count')[1:]:
        name = re.search(r'^\s+\.name:\s+(\w+)\s*$', block, re.M).group(1)
        out[name] = {k: int(v) for k, v in re.findall(r'^\s+(\.[a-z_]+):\s+(\d+)\s*$', block, re.M)}
    return out


@pytest.mark.parametrize('case', lc.TRACED, ids=repr)
def test_unit_compiles_with_its_kernels_and_no_scratch(case, tmp_path):
    s = case.solver()
    source = lc.unit_source(s, case.times[0])
    assert '#define SDP_LOOKAHEAD 1' in source
    assert ('#define SDP_LOOKAHEAD_BOX 1' in source) == (case.box == 'device')
    assert '#define SDP_LANES {}\n'.format(s._box_plan(None if s.sys.stationnary else case.times[0])['lanes']) in source
    kernels = _kernels(source, tmp_path)
    wanted = ['sdp_lookahead'] + (['sdp_simulate_lookahead'] if case.box == 'device' else [])
    for k in wanted:
        assert k in kernels, (k, sorted(kernels))
        f = kernels[k]
        print(case, k, {n: f[n] for n in ('.vgpr_count', '.sgpr_count', '.private_segment_fixed_size',
                                          '.vgpr_spill_count', '.sgpr_spill_count')})
        assert f['.private_segment_fixed_size'] == 0 and f['.vgpr_spill_count'] == 0, (k, f)
        assert f['.max_flat_workgroup_size'] == 256                    # no launch bound beyond the workgroup size
    if case.box != 'device':
        assert 'sdp_simulate_lookahead' not in kernels
    print(case, 'sdp_sweep', {n: kernels['sdp_sweep'][n] for n in ('.vgpr_count', '.sgpr_count')})


def test_lane_counts_of_the_cases():
    lanes = {c.name: c.solver()._box_plan(None if c.times[0] is None else c.times[0])['lanes'] for c in lc.TRACED}
    assert lanes['lanes 1'] == 1 and lanes['lanes 8'] == 8 and lanes['lanes 64'] == 64
    assert lanes['two_reservoirs'] == 64 and lanes['two_inflows'] == 64
    for c in lc.CASES:
        want = {1: lc.B_1, 8: lc.B_8, 64: lc.B_64}.get(lanes.get(c.name))
        if want is not None:
            assert c.batches == want, (c, lanes[c.name])


# ----------------------------------------------------------------------------------------------------------------------
# the box function as host C++

def _device_helpers():
    """the one-line numpy helpers of csrc/sdp_device.h that the emitter may name, as they stand in the header"""
    with open(os.path.join(codegen.CSRC, 'sdp_device.h')) as f:
        lines = [ln for ln in f.read().splitlines()
                 if re.match(r'template <typename real> SDP_DEV \w+ sdp_(isnan|npmin|npmax|npfmin|npfmax)\(', ln)]
    assert len(lines) == 5, lines
    return '\n'.join(lines)


MAIN = r'''
int main(int argc, char **argv)
{
    if (argc != 4) return 2;
    FILE *in = fopen(argv[1], "r"), *out = fopen(argv[2], "w");
    if (!in || !out) return 3;
    const double t = strtod(argv[3], nullptr);
    int n = 0;
    if (fscanf(in, "%d", &n) != 1) return 4;
    for (int b = 0; b < n; ++b) {
        double x[BOX_D], lo[BOX_NU], hi[BOX_NU];
        for (int k = 0; k < BOX_D; ++k) {
            char word[64];
            if (fscanf(in, "%63s", word) != 1) return 5;
            x[k] = strtod(word, nullptr);
        }
        sdp_model_box(x, t, lo, hi);
        for (int c = 0; c < BOX_NU; ++c) fprintf(out, "%a %a\n", lo[c], hi[c]);
    }
    fclose(out);
    return 0;
}
'''


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize('case', BOXED + [lc.Case('nan box', lc.nan_box)], ids=repr)
def test_box_function_as_host_code_gives_the_scalar_calls_bits(case, tmp_path):
    s = case.solver()
    t_k = case.times[-1]
    tb = s._trace_box_now(None if s.sys.stationnary else t_k)
    assert not isinstance(tb, TraceError) and tb.t_value is None
    d, nu = len(s.state_grid), len(s.sys.control)
    text = codegen.box_function_source(tb)
    assert 'sdp_real' not in text and 'double *lo' in text
    program = '\n'.join(['#include <cmath>', '#include <cstdio>', '#include <cstdlib>', '#define SDP_DEV static inline',
                         '#define BOX_D {}'.format(d), '#define BOX_NU {}'.format(nu), _device_helpers(), text, MAIN])
    src, exe = tmp_path / 'box.cpp', tmp_path / 'box'
    src.write_text(program)
    cxx = shutil.which('c++') or os.path.join(LLVM_BIN, 'clang++')          # (any host C++ compiler)
    subprocess.run([cxx, '-O2', '-ffp-contract=off', '-o', str(exe), str(src)], check=True, capture_output=True)
    X = lc.states(case, s)
    if case.name == 'nan box':
        X = np.concatenate([X, [[lc.NAN_STATE]]])
    if s.dtype == np.float32:
        X = X.astype(np.float32).astype(float)                      # (the kernel widens the rounded state)
    (tmp_path / 'in.txt').write_text('{}\n'.format(len(X)) + '\n'.join(' '.join(float(v).hex() for v in row) for row in X))
    subprocess.run([str(exe), str(tmp_path / 'in.txt'), str(tmp_path / 'out.txt'), repr(float(0 if t_k is None else t_k))],
                   check=True, env={'PATH': os.environ.get('PATH', '')})
    got = np.array([[float.fromhex(w) for w in ln.split()] for ln in (tmp_path / 'out.txt').read_text().splitlines()])
    got = got.reshape(len(X), nu, 2)
    lead = () if s.sys.stationnary else (t_k,)
    with np.errstate(all='ignore'):
        want = np.array([[[float(a), float(b)] for a, b in s.sys.control_box(*(lead + tuple(x)), **s.sys.params)] for x in X])
    assert np.array_equal(_bits(got), _bits(want))
    # .. and the lattice rule on those ends is DPSolver._box_lattice's
    lo, hi, n = la.lattice_of_ends(got[:, :, 0].T, got[:, :, 1].T, s.control_steps, np.float64)
    ok = n[0] > 0
    lo2, hi2, n2 = s._box_lattice(np.array(want[:, :, 0].T), np.array(want[:, :, 1].T))
    assert ok.sum() >= len(X) - 1
    assert np.array_equal(n[:, ok], n2[:, ok]) and np.array_equal(_bits(lo[:, ok]), _bits(lo2[:, ok]))
    assert np.array_equal(_bits(hi[:, ok]), _bits(hi2[:, ok]))


# ----------------------------------------------------------------------------------------------------------------------
# no other unit changes

def _digests():
    with open(os.path.join(ROOT, 'profiles', 'plan_source_digests.txt')) as f:
        return {ln.split()[1] for ln in f if len(ln.split()) == 2 and not ln.startswith('#')}


def test_other_units_keep_their_generated_text():
    table = _digests()
    seen = set()
    specs = [('inventory', {}), ('storage_ar1', {}), ('searev', {}),
             ('two_reservoirs', dict(n_a=128, n_b=128, n_y=64, n_w=16, steps=(1. / 15, 1. / 15))), ('two_inflows', {}),
             ('inventory_fine', dict(n_x=65536, n_u=4097, n_w=16))]
    for name, kw in specs:
        for kernel in ('auto', 'staged', 'generic'):
            s = getattr(models, name)(**kw)[1]
            s.kernel = kernel
            try:
                source = s._kernel_plan()['source']
            except ValueError:
                continue                                            # (several perturbation variables take 'auto' / 'generic')
            assert 'SDP_LOOKAHEAD' not in source
            seen.add('line' if '#define SDP_LINE 1' in source else 'lead' if '#define SDP_LEAD_AXES ' in source
                     else 'column' if 'sdp_column_kernel.h' in source else 'staged' if 'sdp_staged_kernel.h' in source
                     else 'direct')
            assert hashlib.sha256(source.encode('utf-8')).hexdigest()[:16] in table, (name, kernel)
    assert seen == {'column', 'lead', 'line', 'staged', 'direct'}, seen


@pytest.mark.parametrize('case', lc.TRACED, ids=repr)
def test_a_lookahead_unit_is_the_direct_unit_plus_its_block(case):
    s = case.solver()
    t_k = case.times[0]
    look = lc.unit_source(s, t_k)
    model = s._trace_now(t_k)
    plain = codegen.translation_unit(model, s.dtype, s._box_plan(None if s.sys.stationnary else t_k)['lanes'], None)
    head, rest = look.split('#define SDP_LOOKAHEAD 1', 1)
    tail = rest.split('#include "sdp_sweep_kernel.h"', 1)[1].split('\n', 1)[1]
    assert head + '#include "sdp_sweep_kernel.h"\n' + tail == plain
    assert codegen.source_key(look) != codegen.source_key(plain)


def test_header_is_in_the_key_of_lookahead_units_only():
    assert 'sdp_lookahead_kernel.h' not in codegen._HEADERS
    with open(os.path.join(codegen.CSRC, 'sdp_sweep_kernel.h')) as f:
        text = f.read()
    assert text.count('#if defined(SDP_LOOKAHEAD)\n#include "sdp_lookahead_kernel.h"') == 2


# ----------------------------------------------------------------------------------------------------------------------
# refusals

class _Ranks(object):
    nranks = 2
    is_device = True


def test_refusals_come_before_a_device_is_touched(monkeypatch):
    monkeypatch.setattr(nat, 'require_gpu', lambda *a, **k: pytest.fail('a device was asked for'))
    monkeypatch.setattr(nat, 'lib', lambda *a, **k: pytest.fail('the library was asked for'))
    s = lc.symbolic_time()
    dims = tuple(len(g) for g in s.state_grid)
    J = np.zeros(dims)
    J_all = np.zeros((8,) + dims)
    x0 = np.zeros((3, 2))
    w = np.zeros((6, 3))
    # shapes
    for bad in (J[:-1], J[None], J[..., None]):
        with pytest.raises(ValueError) as err:
            s.lookahead(bad, x0, 0)
        assert str(dims) in str(err.value) and str(bad.shape) in str(err.value)
    with pytest.raises(ValueError):
        s.lookahead(J, np.zeros((3, 3)), 0)
    with pytest.raises(ValueError):
        s.lookahead(J, x0)                                          # a time-dependent system without its time index
    with pytest.raises(ValueError):
        s.lookahead(J, x0, 0, path='fast')
    for bad in (J[:-1], J_all[:, :-1], J_all[None]):
        with pytest.raises(ValueError) as err:
            s.simulate_lookahead(bad, x0, w, n_steps=2)
        assert 'T_J' in str(err.value) and str(bad.shape) in str(err.value)
    with pytest.raises(ValueError):
        s.simulate_lookahead(J, np.zeros((3, 3)), w)
    with pytest.raises(ValueError):
        s.simulate_lookahead(J, x0, np.zeros((6, 4)))
    with pytest.raises(ValueError):
        s.simulate_lookahead(J, x0, None, n_steps=2)
    # beyond the cost-to-go's steps, and before them
    with pytest.raises(ValueError) as err:
        s.simulate_lookahead(J_all, x0, w, n_steps=6, t0=3)
    assert all(n in str(err.value) for n in ('t0 = 3', 'n_steps = 6', 'T_J = 8')), str(err.value)
    with pytest.raises(ValueError) as err:
        s.simulate_lookahead(J_all, x0, w, n_steps=2, t0=-1)
    assert all(n in str(err.value) for n in ('t0 = -1', 'n_steps = 2', 'T_J = 8')), str(err.value)
    # a communicator of several ranks
    s.comm = _Ranks()
    with pytest.raises(NotImplementedError):
        s.lookahead(J, x0, 0)
    with pytest.raises(NotImplementedError):
        s.simulate_lookahead(J, x0, w)


def test_abi_declares_the_two_entry_points():
    with open(os.path.join(ROOT, 'include', 'sdp_hip.h')) as f:
        header = f.read()
    with open(os.path.join(codegen.CSRC, 'sdp_hip.hip')) as f:
        library = f.read()
    for name in ('sdp_problem_lookahead', 'sdp_problem_simulate_lookahead'):
        assert re.search(r'^int {}\('.format(name), header, re.M)
        assert 'extern "C" int {}('.format(name) in library
