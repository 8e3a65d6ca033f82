"""The plan of the lean reductions (codegen.table_phase_plan: SDP_COL_REDUCE_FUSED and SDP_COL_DMAX_HI of
csrc/sdp_colres_kernel.h), without a GPU.

- both items are planned on the benchmark unit and on every resident-chunk case of tests/column_forms.py that is not on the
  shifted lattice; an item's debug define at 0 takes exactly its line out of the text, and both at 0 give the text -- hence
  the code object -- the unit had before;
- shifted, 4-byte and full-table units carry neither macro and keep the digests of profiles/plan_source_digests.txt;
- the benchmark unit keeps its LDS image and its register pins, read from the code object as
  tests/test_colres_registers.py does, and shows the instructions the items are about."""
import hashlib
import os
import re

import numpy as np
import pytest

import column_forms as cf
from stodynprog_amd import DPSolver, codegen, models
from test_colres_registers import _kernel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITEMS = codegen.TABLE_PHASE_MACROS
ALL_OFF = {m: '0' for m in ITEMS}
BEFORE = '3d2815a5444aeecc'          # the benchmark unit's digest in the table before the items were planned
HELD = [c for c in cf.CASES if c.hold and not c.noise]
SHIFTED = [c for c in cf.CASES if c.noise]
OTHER = [c for c in cf.CASES if c.name.startswith(('full_', 'f32_'))]


def _bench(debug=None):
    _, s = models.synthetic3d(N=256)
    s.debug_defines = debug
    return s._kernel_plan()


def _digest(src):
    return hashlib.sha256(src.encode('utf-8')).hexdigest()[:16]


def _table():
    with open(os.path.join(ROOT, 'profiles', 'plan_source_digests.txt')) as f:
        return {ln.split()[-1] for ln in f if ln.split() and not ln.startswith('#')}


def _items(src):
    return tuple(m for m in ITEMS if cf.macro(src, m) == '1')


def test_the_switches_are_registered():
    assert set(ITEMS) <= codegen.DEBUG_NAMES and ITEMS == ('SDP_COL_REDUCE_FUSED', 'SDP_COL_DMAX_HI')


def test_the_benchmark_unit_plans_every_item_and_each_switch_takes_out_its_line():
    plan = _bench()
    src, unit = plan['source'], plan['unit']
    assert _items(src) == ITEMS
    assert (unit.reduce_fused, unit.dmax_hi) == (1, 1)
    assert _digest(src) in _table()
    for m in ITEMS:
        off = _bench({m: '0'})['source']
        assert _items(off) == tuple(k for k in ITEMS if k != m)
        assert off.splitlines() == [ln for ln in src.splitlines() if not ln.startswith('#define {} '.format(m))]
    # both off: the text of before, to the byte
    none = _bench(dict(ALL_OFF))['source']
    assert _items(none) == () and not any(m in none for m in ITEMS)
    assert _digest(none) == BEFORE


@pytest.mark.parametrize('case', HELD, ids=[c.name for c in HELD])
def test_the_held_tail_cases_plan_every_item(case, debug_defines):
    if case.debug:
        debug_defines.set(**case.debug)
    for geometry in case.geometries:
        plan = case.solver(geometry)._kernel_plan()
        assert cf.macro(plan['source'], 'SDP_COL_TAIL_HOLD') == '1' and cf.macro(plan['source'], 'SDP_COL_SHIFT') is None
        assert _items(plan['source']) == ITEMS, (case, geometry)
        assert _digest(plan['source']) in _table(), (case, geometry)


def test_resident_chunks_without_the_held_tail_plan_them_too():
    for case in (c for c in cf.CASES if c.name.startswith('res_n')):
        src = case.solver('many')._kernel_plan()['source']
        assert cf.macro(src, 'SDP_COL_TAIL_HOLD') is None and _items(src) == ITEMS, case


@pytest.mark.parametrize('case', SHIFTED + OTHER, ids=[c.name for c in SHIFTED + OTHER])
def test_shifted_4_byte_and_full_table_units_carry_none_and_keep_their_digests(case, debug_defines):
    if case.debug:
        debug_defines.set(**case.debug)
    table = _table()
    for geometry in case.geometries:
        src = case.solver(geometry)._kernel_plan()['source']
        assert not any(m in src for m in ITEMS), (case, geometry)
        assert _digest(src) in table, (case, geometry)


def test_the_other_benchmark_configurations_keep_their_digests():
    table = _table()
    for kw, dt in ((dict(N=256, stock_noise=0.07), np.float64), (dict(N=256, stock_noise=0.07, nested=True), np.float64),
                   (dict(N=512), np.float32), (dict(N=256), np.float32)):
        _, s = models.synthetic3d(**kw)
        s.dtype = np.dtype(dt)
        src = s._kernel_plan()['source']
        assert not any(m in src for m in ITEMS), kw
        assert _digest(src) in table, kw


def test_units_outside_the_form_are_left_as_they_are():
    unit = _bench()['unit']._replace(reduce_fused=None, dmax_hi=None)
    for other in (unit._replace(shift=True), unit._replace(wres=0, form='full table'), unit._replace(wpair=True)):
        assert codegen.table_phase_plan(other, np.float64) == other
    assert codegen.table_phase_plan(unit, np.float32) == unit
    assert codegen.table_phase_plan(unit, np.float64) == unit._replace(reduce_fused=1, dmax_hi=1)
    assert codegen.table_phase_plan(unit, np.float64, {'SDP_COL_DMAX_HI': '0'}) == unit._replace(reduce_fused=1)


# ---------------------------------------------------------------------------
# the benchmark unit's code object

@pytest.fixture(scope='module')
def built(tmp_path_factory):
    return {key: _kernel(_bench(dbg)['source'], tmp_path_factory.mktemp(key))
            for key, dbg in (('on', None), ('off', dict(ALL_OFF)))}


def test_the_benchmark_unit_keeps_its_image_and_its_pins(built):
    fields, body = built['on']
    assert fields['.vgpr_count'] <= 128, fields          # four waves per SIMD
    assert fields['.vgpr_spill_count'] == 0, fields
    assert fields['.private_segment_fixed_size'] == 0, fields
    assert 'scratch_' not in body
    assert fields['.sgpr_spill_count'] <= 96, fields
    assert fields['.group_segment_fixed_size'] == built['off'][0]['.group_segment_fixed_size'] == 39104
    assert _bench()['unit'].lds_bytes == 39104


def test_the_code_object_shows_the_items(built):
    on, off = built['on'][1], built['off'][1]
    count = lambda pat, body: len(re.findall(pat, body, re.M))
    # the reductions: a fused multiply-add per point of either reduction
    fused = lambda body: count(r'^\s+v_fma(c)?_f64', body)
    assert fused(on) >= fused(off) + 32
    # the column bound: six integer maxima on the lanes' high words, none of the 8-byte maximum's row shifts
    assert count(r'^\s+v_max_u32_dpp', on) == 6 and count(r'^\s+v_max_u32_dpp', off) == 0
    # the whole vector stream is shorter
    assert count(r'^\s+v_', on) < count(r'^\s+v_', off) - 60
    # .. and the weights' scalar loads stay in the unit loop: no more spill traffic than before
    lanes = lambda body: count(r'^\s+v_(read|write)lane_b32', body)
    assert lanes(on) <= lanes(off)
