"""SDP_BNB_LEAN (the bookkeeping of the branch and bound, csrc/sdp_colfilter_kernel.h) as a switch and in registers.
No GPU: the units of the benchmark, of the shifted lattice (noisy256) and of 4-byte reals (synth512f32) are
cross-compiled for gfx950 with and without the switch, and their code-object notes and disassemblies are read.

Nothing plans the switch: a unit carries the macro only when a caller sets it, so every planned text -- and the table
of digests under profiles/ -- is what it was.  The default build of the benchmark unit meets the pins of
tests/test_colres_registers.py; the other two units have no pins of their own (the shifted lattice's unit spills three
registers once per workgroup, outside the unit loop), so the default is held to the budget of the SAME unit with the
earlier bookkeeping: no more vector registers and no more scratch traffic."""
import hashlib
import os
import re

import numpy as np
import pytest

from stodynprog_amd import codegen, models
from test_colres_registers import _kernel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFF = {'SDP_BNB_LEAN': '0'}


def _solver(which, debug=None):
    if which == 'synth256':
        _, s = models.synthetic3d(N=256)
    elif which == 'noisy256':
        _, s = models.synthetic3d(N=256, stock_noise=0.07)
    else:
        _, s = models.synthetic3d(N=512)
        s.dtype = np.dtype('float32')
    s.debug_defines = debug
    return s


def _source(which, debug=None):
    return _solver(which, debug)._kernel_plan()['source']


UNITS = ('synth256', 'noisy256', 'synth512f32')


@pytest.fixture(scope='module')
def built(tmp_path_factory):
    out = {}
    for which in UNITS:
        for key, debug in (('lean', None), ('off', OFF)):
            out[which, key] = _kernel(_source(which, debug), tmp_path_factory.mktemp('{}_{}'.format(which, key)))
    return out


def test_the_switch_is_registered_and_nothing_plans_it():
    assert 'SDP_BNB_LEAN' in codegen.DEBUG_NAMES
    with open(os.path.join(ROOT, 'profiles', 'plan_source_digests.txt')) as f:
        table = {ln.split()[1] for ln in f if len(ln.split()) == 2 and not ln.startswith('#')}
    for which in UNITS:
        plain, off = _source(which), _source(which, OFF)
        assert 'SDP_BNB_LEAN' not in plain and '#define SDP_COL_BNB 1' in plain
        # the unit's text without the switch is the committed digest's text
        assert hashlib.sha256(plain.encode('utf-8')).hexdigest()[:16] in table, which
        # the switch adds its own line and changes nothing else
        assert [ln for ln in off.splitlines() if 'SDP_BNB_LEAN' not in ln] == plain.splitlines()
        assert off.count('#define SDP_BNB_LEAN 0') == 1


def test_the_benchmark_unit_keeps_its_pins(built):
    fields, body = built['synth256', 'lean']
    assert fields['.vgpr_count'] <= 128, fields          # four waves per SIMD
    assert fields['.vgpr_spill_count'] == 0, fields
    assert fields['.private_segment_fixed_size'] == 0, fields
    assert 'scratch_' not in body
    assert fields['.sgpr_spill_count'] <= 96, fields
    assert fields['.group_segment_fixed_size'] == built['synth256', 'off'][0]['.group_segment_fixed_size'] <= 40960


@pytest.mark.parametrize('which', UNITS)
def test_no_unit_needs_more_registers_than_with_the_earlier_bookkeeping(built, which):
    (lean, body), (off, body_off) = built[which, 'lean'], built[which, 'off']
    print(which, {k: (lean[k], off[k]) for k in ('.vgpr_count', '.vgpr_spill_count', '.sgpr_spill_count',
                                                 '.private_segment_fixed_size', '.group_segment_fixed_size')})
    assert lean['.vgpr_count'] <= off['.vgpr_count']
    assert lean['.group_segment_fixed_size'] == off['.group_segment_fixed_size']
    # (spill code that a unit does have is scanned when the unit is built: _native.compile_model, codegen.spill_hazards)
    assert len(re.findall(r'\bscratch_', body)) <= len(re.findall(r'\bscratch_', body_off))


def test_the_lean_form_has_the_shorter_vector_stream(built):
    """static: the whole kernel's vector instructions do not grow (the evaluation trip and the bound stage's chunk are
    shorter by more than the one-by-one path of a partial last block adds)"""
    def valu(body):
        return len(re.findall(r'^\s+v_', body, re.M))
    assert valu(built['synth256', 'lean'][1]) < valu(built['synth256', 'off'][1])
