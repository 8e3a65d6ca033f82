"""Kernel sdp_montecarlo (csrc/sdp_mc_kernel.h) is part of every unit of a stochastic system, uses no scratch memory
and spills nothing, and its header is part of the units' cache key.  No GPU: units are cross-compiled for gfx950 and
their code-object notes are read."""
import os
import re
import subprocess

import numpy as np
import pytest

from stodynprog_amd import SysDescription, DPSolver, codegen, models, _native as nat

LLVM_BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(nat.HIPCC))), 'llvm', 'bin')
TARGET = 'hipv4-amdgcn-amd-amdhsa--gfx950'


def _kernels(source, tmp_path):
    """{kernel name: integer fields of its code-object notes}, and the disassembly"""
    src, bundle, elf = (str(tmp_path / f) for f in ('unit.hip', 'unit.co', 'unit.elf'))
    with open(src, 'w') as f:
        f.write(source)
    subprocess.run([nat.HIPCC] + codegen.HIPCC_FLAGS + ['-o', bundle, src], check=True, capture_output=True)
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


def _as32(s):
    t = DPSolver(s.sys, dtype=np.float32)
    t.state_grid, t.perturb_grid = s.state_grid, s.perturb_grid
    t.perturb_proba, t.control_steps = s.perturb_proba, s.control_steps
    return t


# unit: (solver maker, most vector registers sdp_montecarlo may take).  A SIMD holds 512 per lane, handed out in blocks
# of 8: 64 is eight waves per SIMD, 72 seven, 80 six, 96 five.  The kernel is meant for eight; the one- and two-
# dimensional 8-byte units and the 4-byte unit get there on vector registers, the three-dimensional 8-byte ones do not
# without scratch memory (asking the allocator for eight made Searev spill 28 bytes per lane), so their counts of today
# are pinned instead: a change that costs any unit a wave shows here.
UNITS = {
    'inventory': (lambda: models.inventory()[1], 64),
    'storage_ar1': (lambda: models.storage_ar1()[1], 64),
    'synthetic3d fp32': (lambda: _as32(models.synthetic3d(N=20)[1]), 64),
    'searev (column unit)': (lambda: models.searev()[1], 80),
    'two reservoirs': (lambda: models.two_reservoirs(n_a=12, n_b=10, n_y=8)[1], 96),
}


@pytest.mark.parametrize('unit', sorted(UNITS))
def test_kernel_is_in_the_unit_without_scratch(unit, tmp_path):
    make, most_vgprs = UNITS[unit]
    kernels, dis = _kernels(make()._kernel_plan()['source'], tmp_path)
    assert 'sdp_montecarlo' in kernels and 'sdp_simulate' in kernels, sorted(kernels)
    f = kernels['sdp_montecarlo']
    print(unit, {k: f[k] for k in ('.vgpr_count', '.sgpr_count', '.private_segment_fixed_size')})
    # (scalar registers may overflow into lanes of a vector register: no memory is involved)
    assert f['.private_segment_fixed_size'] == 0 and f['.vgpr_spill_count'] == 0, f
    assert f['.vgpr_count'] <= most_vgprs, f
    assert f['.group_segment_fixed_size'] == 0, f        # the draw table is dynamic LDS, sized by the law
    body = dis.split('<sdp_montecarlo>:')[1].split('>:\n')[0]
    assert 'scratch_' not in body
    assert 'v_mul_hi_u32' in body                        # Philox: 32-bit integer multiplies
    assert 'global_atomic_add_x2' in body                # the occupancy: vector atomics on 64-bit counts
    # nothing is stored per step: the state, the sum and the counter once per launch, and the atomic
    assert len(re.findall(r'\bglobal_store', body)) <= 3 + len(make().state_grid), re.findall(r'\bglobal_store\S*', body)


def test_deterministic_unit_has_no_monte_carlo_kernel(tmp_path):
    s = SysDescription((1, 1, 0), name='deterministic')
    s.dyn = lambda x, u: (x + u,)
    s.cost = lambda x, u: x * x
    s.control_box = lambda x: ((-1., 1.),)
    solver = DPSolver(s)
    solver.discretize_state(-1, 1, 5)
    solver.control_steps = (0.5,)
    kernels, _ = _kernels(solver._kernel_plan()['source'], tmp_path)
    assert 'sdp_simulate' in kernels and 'sdp_montecarlo' not in kernels


def test_header_is_part_of_the_cache_key():
    assert 'sdp_mc_kernel.h' in codegen._HEADERS
    assert '#include "sdp_mc_kernel.h"' in open(os.path.join(nat.CSRC, 'sdp_sweep_kernel.h')).read()
