"""Kernel sdp_transitions (csrc/sdp_trans_kernel.h) is part of every generated unit -- stochastic, deterministic,
several perturbation variables, node-order and column units -- without scratch memory or vector spills, and what
DPSolver.transition_operator refuses it refuses before it touches a device.  No GPU: the units of
tests/forward_cases.py are cross-compiled for gfx950 (the code objects the build keeps) and their notes are read."""
import os
import re
import subprocess

import numpy as np
import pytest

import forward_cases as fc
from stodynprog_amd import DPSolver, codegen, forward, models, _native as nat

LLVM_BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(nat.HIPCC))), 'llvm', 'bin')
TARGET = 'hipv4-amdgcn-amd-amdhsa--gfx950'


def _kernels(source, tmp_path):
    """{kernel name: integer fields of its code-object notes}, and the disassembly (tests/test_montecarlo_kernel.py
    reads the notes the same way)"""
    bundle, elf = nat.compile_model(source), str(tmp_path / 'unit.elf')
    subprocess.run([os.path.join(LLVM_BIN, 'clang-offload-bundler'), '--unbundle', '--type=o', '--targets=' + TARGET,
                    '--input=' + bundle, '--output=' + elf], check=True, capture_output=True)
    notes = subprocess.run([os.path.join(LLVM_BIN, 'llvm-readelf'), '--notes', elf], check=True,
                           capture_output=True, text=True).stdout
    out = {}
    for block in notes.split('  - .agpr_count')[1:]:
        name = re.search(r'^\s+\.name:\s+(\w+)\s*$', block, re.M).group(1)
        out[name] = {k: int(v) for k, v in re.findall(r'^\s+(\.[a-z_]+):\s+(\d+)\s*$', block, re.M)}
    dis = subprocess.run([os.path.join(LLVM_BIN, 'llvm-objdump'), '-d', elf], check=True,
                         capture_output=True, text=True).stdout
    return out, dis


UNITS = [(c.name, dtkey, kernel) for c in fc.DEVICE_CASES for dtkey in sorted(fc.DTYPES) for kernel in (None, 'generic')]


@pytest.mark.parametrize('name,dtkey,kernel', UNITS)
def test_kernel_is_in_the_unit_without_scratch(name, dtkey, kernel, tmp_path):
    case = fc.BY_NAME[name]
    s = case.solver(fc.DTYPES[dtkey], kernel)
    plan = fc.plan_of(s, case.times[-1])
    if kernel is None and name in ('storage_ar1', 'searev'):
        assert plan['column'], name                       # the column family carries the kernel too
    kernels, dis = _kernels(plan['source'], tmp_path)
    assert 'sdp_transitions' in kernels and 'sdp_evalpol' in kernels, sorted(kernels)
    f = kernels['sdp_transitions']
    print(name, dtkey, kernel, {k: f[k] for k in ('.vgpr_count', '.sgpr_count', '.private_segment_fixed_size')})
    assert f['.private_segment_fixed_size'] == 0 and f['.vgpr_spill_count'] == 0, f
    assert f['.group_segment_fixed_size'] == 0, f            # no LDS
    body = dis.split('<sdp_transitions>:')[1].split('>:\n')[0]
    assert 'scratch_' not in body


def test_searev_at_its_own_size_does_not_spill(tmp_path):
    """the unit the measurement runs (tools/forward_times.py): 31 x 61 x 61 x 9, 8-byte reals"""
    kernels, _ = _kernels(models.searev()[1]._kernel_plan()['source'], tmp_path)
    f = kernels['sdp_transitions']
    assert f['.private_segment_fixed_size'] == 0 and f['.vgpr_spill_count'] == 0, f


def test_header_is_part_of_the_cache_key():
    assert 'sdp_trans_kernel.h' in codegen._HEADERS


def test_the_entry_positions_have_their_own_limit():
    """beyond 2^32 - 1 entries the refusal names the 32-bit positions, not the cap a user may have raised"""
    _, s = models.synthetic3d(N=256)
    s.TRANSITION_MAX_BYTES = 1 << 60
    pol = np.broadcast_to(np.zeros(1), (256, 256, 256, len(s.sys.control)))
    with pytest.raises(ValueError) as err:
        s.transition_operator(pol)
    assert '32-bit' in str(err.value) and 'TRANSITION_MAX_BYTES' not in str(err.value)


def test_the_cap_raises_before_anything_is_allocated():
    _, s = models.synthetic3d(N=256)                        # 256^3 nodes, 32 points, 8 vertices: 4.3e9 entries
    pol = np.broadcast_to(np.zeros(1), (256, 256, 256, len(s.sys.control)))
    S, nnz, nbytes = s._transition_size()
    assert nnz == 256 ** 3 * 32 * 8 and nbytes == forward.operator_bytes(nnz, S, 8) == nnz * 12 + 8 * (S + 1)
    with pytest.raises(ValueError) as err:
        s.transition_operator(pol)
    assert str(nnz) in str(err.value) and str(nbytes) in str(err.value) and 'TRANSITION_MAX_BYTES' in str(err.value)
    assert DPSolver.TRANSITION_MAX_BYTES == 2 << 30
    # the cap is the attribute: a small problem is refused under a small cap, with its bytes in the text
    case = fc.BY_NAME['inventory']
    small = case.solver()
    small.TRANSITION_MAX_BYTES = 1000
    with pytest.raises(ValueError) as err:
        small.transition_operator(case.policy(small))
    assert '{} bytes'.format(10 * 4 * 2 * 12 + 8 * 11) in str(err.value)


def test_a_communicator_is_refused():
    case = fc.BY_NAME['inventory']
    s = case.solver()
    s.comm = object()                                       # (never touched: refused by its presence)
    with pytest.raises(NotImplementedError):
        s.transition_operator(case.policy(s))
    with pytest.raises(NotImplementedError):
        s.stationary_distribution(case.policy(s))


def test_a_policy_of_the_wrong_shape_is_refused():
    case = fc.BY_NAME['storage_ar1']
    s = case.solver()
    pol = case.policy(s)
    for bad in (pol[..., :1], pol[:-1], pol.reshape(-1, 2), pol[..., 0]):
        with pytest.raises(ValueError):
            s.transition_operator(bad)
        with pytest.raises(ValueError):
            forward.entries(s, bad)


@pytest.mark.parametrize('dtkey', sorted(fc.DTYPES))
def test_long_line_is_past_the_launch_caps_of_256_compute_units(dtkey):
    """what tests/test_gpu_forward.py asserts with the chip's own count, on the MI355X's: every launch of the build and
    of a push makes a second trip, push_until's statistics with 8-byte reals; and the unit travels with the build"""
    dt = np.dtype(fc.DTYPES[dtkey])
    case = fc.long_line(256)
    s = case.solver(dt.type)
    plan = fc.plan_of(s)
    assert plan['source'] in fc.unit_sources()
    assert plan['source'] == fc.plan_of(fc.long_line(64).solver(dt.type))['source']      # (whatever the chip)
    e = forward.entries(s, case.policy(s))
    assert (e.S, e.W, e.V) == (524417, 2, 2) and len(e.val) == 4 * e.S
    indptr, _, _ = forward.csr(e.S, e.tgt, e.src, e.val)
    lengths = np.diff(indptr)
    assert 3 <= lengths.min() and lengths.max() < 256 and (lengths < 8).sum() > e.S - 8
    caps = fc.long_line_caps(e.S, len(e.val), lengths, 256, dt.itemsize)
    assert caps['sdp_transitions'] == (4098, 2048) and caps['k_iota, k_trans_gather, k_trans_count'] == (8195, 2048)
    assert caps['k_push'] == (2049, 2048) and caps['k_push_group<16>'] == (32777, 16384)
    assert caps['k_diff_stats'] == ((1025, 1024) if dt.itemsize == 8 else (513, 1024))
    assert forward.operator_bytes(len(e.val), e.S, dt.itemsize) < 64 << 20
