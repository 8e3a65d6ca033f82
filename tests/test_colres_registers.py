"""The benchmark's unit -- the held-tail form of the resident-chunk column kernel (csrc/sdp_colres_kernel.h) -- fits four
waves per SIMD without spilling, and carries the direct exchange's peer stores only when a unit is planned for it.
No GPU: the unit is cross-compiled for gfx950 and its code-object notes and disassembly are read."""
import os
import re
import subprocess

import pytest

from stodynprog_amd import codegen, models, _native as nat

LLVM_BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(nat.HIPCC))), 'llvm', 'bin')
TARGET = 'hipv4-amdgcn-amd-amdhsa--gfx950'


class _DeviceComm:
    """What the planner asks of a communicator: a device communicator of two ranks (nothing is launched)."""
    is_device = True
    nranks = 2
    rank = 0


def _bench_solver(exchange=None):
    _, s = models.synthetic3d(N=256)          # bench.py's flagship problem (synth256, fp64)
    if exchange is not None:
        s.comm, s.comm_exchange = _DeviceComm(), exchange
    return s


def _kernel(source, tmp_path, name='sdp_sweep_col'):
    """(code-object notes of kernel `name` as a dict of its integer fields, its disassembly) for a generated unit"""
    src, bundle, elf = (str(tmp_path / f) for f in ('unit.hip', 'unit.co', 'unit.elf'))
    with open(src, 'w') as f:
        f.write(source)
    subprocess.run([nat.HIPCC] + codegen.HIPCC_FLAGS + ['-o', bundle, src], check=True, capture_output=True)
    subprocess.run([os.path.join(LLVM_BIN, 'clang-offload-bundler'), '--unbundle', '--type=o', '--targets=' + TARGET,
                    '--input=' + bundle, '--output=' + elf], check=True, capture_output=True)
    notes = subprocess.run([os.path.join(LLVM_BIN, 'llvm-readelf'), '--notes', elf], check=True,
                           capture_output=True, text=True).stdout
    fields = None
    for block in notes.split('  - .agpr_count')[1:]:
        if re.search(r'^\s+\.name:\s+{}\s*$'.format(name), block, re.M):
            fields = {k: int(v) for k, v in re.findall(r'^\s+(\.[a-z_]+):\s+(\d+)\s*$', block, re.M)}
    assert fields is not None, 'no kernel {} in the code object'.format(name)
    dis = subprocess.run([os.path.join(LLVM_BIN, 'llvm-objdump'), '-d', elf], check=True,
                         capture_output=True, text=True).stdout
    body = dis.split('<{}>:'.format(name))[1].split('>:\n')[0]
    return fields, body


def _peer_flag(source):
    return '#define SDP_PEER_STORES 1' in source


@pytest.fixture(scope='module')
def single(tmp_path_factory):
    source = _bench_solver()._kernel_plan()['source']
    return source, _kernel(source, tmp_path_factory.mktemp('single'))


def test_benchmark_unit_is_the_held_tail_at_four_waves(single):
    source, _ = single
    assert '#define SDP_COL_TAIL_HOLD 1' in source
    assert re.search(r'^#define SDP_COL_MIN_WAVES 4\b', source, re.M)


def test_benchmark_unit_does_not_spill(single):
    _, (fields, body) = single
    assert fields['.vgpr_count'] <= 128, fields          # four waves per SIMD
    assert fields['.vgpr_spill_count'] == 0, fields
    assert fields['.private_segment_fixed_size'] == 0, fields
    assert 'scratch_' not in body
    assert fields['.sgpr_spill_count'] <= 96, fields       # (158 before the peer stores were planned out)


def test_single_gpu_unit_has_no_peer_stores(single):
    source, (_, body) = single
    assert '#define SDP_PEER_STORES 0' in source
    # J, policy value and policy index: one store each, nothing stores into another rank's J
    assert len(re.findall(r'\bglobal_store', body)) == 3, re.findall(r'\bglobal_store\S*', body)
    for exchange in ('rccl', 'peer', 'sendrecv'):
        assert not _peer_flag(_bench_solver(exchange)._kernel_plan()['source']), exchange


def test_direct_exchange_unit_keeps_the_peer_stores(single, tmp_path):
    source = _bench_solver('direct')._kernel_plan()['source']
    assert _peer_flag(source)
    _, body = _kernel(source, tmp_path)
    assert len(re.findall(r'\bglobal_store', body)) > 3
    # the code object claims the peer stores only then (sdp_problem_set_direct_exchange checks the claim)
    assert source.replace('#define SDP_PEER_STORES 1', '#define SDP_PEER_STORES 0') == single[0]
