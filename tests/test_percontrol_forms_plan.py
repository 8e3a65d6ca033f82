"""The table of the table-per-control unit (tests/percontrol_forms.py) still means what it says, without a GPU: every
case plans the form and the macros it claims at every geometry, the split rule restated from column_grid gives the units
it claims for 256 compute units, the table as a whole reaches every form it is for, and its units compile for gfx950.
When a planner change moves a shape to another form, these tests name the case that lost its coverage."""
import os

import numpy as np
import pytest

import percontrol_forms as pf

_IDS = ['{}-{}'.format(c.name, g) for c, g in pf.PAIRS]


def _cols(shape):
    return int(np.prod(shape[1:]))


@pytest.mark.parametrize('case,geometry', pf.PAIRS, ids=_IDS)
def test_every_case_plans_the_form_and_the_units_it_claims(case, geometry):
    s = case.solver(geometry)
    plan = s._kernel_plan()
    assert plan['unit'].form == 'table per control' and plan['per_control'], (case, plan['unit'])
    assert '#include "sdp_column_kernel.h"' in plan['source']
    missing = pf.missing_claims(case.claims, plan['source'])
    assert not missing, '{} at {}: (macro, claimed, planned) {}'.format(case, geometry, missing)
    assert s._shape()[0] == case.n0 and plan['W'] == case.W and s.dtype == case.dtype
    # the direct kernel it is compared with
    assert '#include "sdp_column_kernel.h"' not in case.solver(geometry, 'generic')._kernel_plan()['source']
    # the geometry is what its name says, and the split rule cuts the columns into the units claimed
    cols = _cols(s._shape())
    assert cols >= 4 * pf.CUS if geometry == 'many' else 7 <= cols <= 9, (case, geometry, cols)
    bounds = pf.sweep_bounds(s, pf.CUS, plan['col_seg_nodes'])
    rows = {hi - lo for lo, hi in bounds}
    assert rows == case.units[geometry], (case, geometry, rows)
    assert plan['col_seg_nodes'] == int(case.claims['SDP_COL_THREADS']) and max(rows) <= plan['col_seg_nodes']
    if geometry == 'many':
        launches = pf.launch_columns(s._shape(), case.rs, s.host_overlap)
        assert launches == [cols] and bounds == pf.unit_bounds(case.n0, cols, pf.CUS, plan['col_seg_nodes'])
        assert pf.walk_branch(s._shape(), len(bounds), len(launches)) == case.walk, case
        # (a live product path: what 'auto' runs at this size)
        assert case.solver(geometry, 'auto')._kernel_plan()['per_control'], case


def test_the_split_rule_is_that_of_column_grid():
    # 600 rows on 7 columns: 4 * 256 / 7 -> 147 splits wanted, 600 // 64 = 9 allowed
    assert pf.splits(600, 7, 256) == 9 and pf.unit_rows(600, 7, 256) == {66, 67}
    assert pf.unit_bounds(600, 7, 256)[:2] == [(0, 66), (66, 133)] and pf.unit_bounds(600, 7, 256)[-1] == (533, 600)
    # enough columns: one unit, unless the unit has a segment length
    assert pf.splits(600, 1025, 256) == 1 and pf.splits(600, 1025, 256, 512) == 2 and pf.splits(2050, 1025, 256, 512) == 5
    assert pf.splits(63, 7, 256) == 1 and pf.splits(1024, 120, 256, 192) == 9 and pf.splits(1024, 1024, 256, 192) == 6
    # the phased downloads: 1500 x 1025 x 8 bytes in four launches of 256 or 257 columns, each split four times
    assert pf.launch_columns((1500, 1025), 8) == [256, 256, 256, 257] and pf.launch_columns((1500, 1025), 8, False) == [1025]
    assert pf.launch_columns((600, 1025), 8) == [1025] and pf.launch_columns((2052, 1025), 4) == [256, 256, 256, 257]
    assert pf.unit_rows(1500, 256, 256, 512) == {375} and pf.unit_rows(1500, 1025, 256, 512) == {500}
    nodes = pf.sample_nodes((600, 7), pf.unit_bounds(600, 7, 256))
    assert list(nodes) == sorted(set(nodes)) and nodes.max() == 600 * 7 - 1
    assert {65 * 7, 66 * 7, 599 * 7, 0} <= set(nodes) and set(range(6, 4200, 7)) <= set(nodes)


def test_the_inputs_are_what_they_are_for():
    for rs in (8, 4):
        V = pf.inputs((40, 9), rs)
        assert tuple(V) == pf.INPUTS and all(v.shape == (40, 9) and v.dtype == np.float64 for v in V.values())
        assert not V['zeros'].any() and np.isfinite(V['random']).all()
        assert np.isnan(V['special']).any() and (V['special'] == np.inf).any() and (V['special'] == -np.inf).any()
        real = np.float64 if rs == 8 else np.float32
        flat = V['flat'].astype(real)
        # a cost of the size the models have is lost in the rounding of the lower half, and coarsened in the upper
        assert (flat[:20] + real(7.3) == flat[:20]).all() and (flat[20:] + real(0.0005) == flat[20:]).all()
        assert (flat[20:] + real(0.01) != flat[20:]).all()


def test_the_table_covers_the_forms_it_is_for():
    reached = set()
    for c in pf.CASES:
        wide = 'wide' if c.claims['SDP_COLU_WIDE_LOADS'] == '1' else 'narrow'
        reached.add('{} loads, {} bytes'.format(wide, c.rs))
        wc, chunks = c.wchunk()
        Wn = max(c.W, 1)
        if Wn > 1:
            reached.add('wchunk = W' if wc == Wn else 'wchunk = 1' if wc == 1 else
                        'wchunk between 1 and W, ragged' if chunks[-1] < wc else 'wchunk between 1 and W')
            reached.add('lead_w {}, cost_w {}, wchunk < W: {}'.format(c.claims['SDP_LEAD_HAS_W'], c.claims['SDP_COST_HAS_W'], wc < Wn))
            if wc < Wn:
                reached.add('wchunk < W, {} loads, {} bytes'.format(wide, c.rs))
        else:
            reached.add('deterministic')
        reached.add('SDP_D ' + c.claims['SDP_D'])
        reached.add('walk ' + c.walk)
        if max(max(u) for u in c.units.values()) > 256:
            reached.add('units above 256 rows')
        rpl = 16 // c.rs
        threads = int(c.claims['SDP_COL_THREADS'])
        if wide == 'wide' and c.n0 // rpl > threads:
            reached.add('more row groups than threads')
        if wide == 'wide' and threads // min(threads, c.n0 // rpl) > 1:
            reached.add('thread groups along w')
        if wide == 'narrow' and c.n0 > 2 * threads:
            reached.add('three trips of the narrow row loop')
        reached.add('{} threads'.format(threads))
    wanted = {'wide loads, 8 bytes', 'narrow loads, 8 bytes', 'wide loads, 4 bytes', 'narrow loads, 4 bytes',
              'wchunk = W', 'wchunk between 1 and W, ragged', 'wchunk = 1',
              'wchunk < W, wide loads, 8 bytes', 'wchunk < W, narrow loads, 8 bytes',
              'wchunk < W, wide loads, 4 bytes', 'wchunk < W, narrow loads, 4 bytes',
              'lead_w 0, cost_w 1, wchunk < W: True', 'lead_w 1, cost_w 1, wchunk < W: True',
              'lead_w 1, cost_w 0, wchunk < W: True', 'lead_w 0, cost_w 0, wchunk < W: True',
              'deterministic', 'SDP_D 2', 'SDP_D 3', 'SDP_D 4', 'walk xcd', 'walk tiles', 'walk identity',
              'units above 256 rows', 'more row groups than threads', 'thread groups along w',
              'three trips of the narrow row loop', '64 threads', '128 threads', '512 threads'}
    assert not wanted - reached, 'the table no longer reaches: {}'.format(sorted(wanted - reached))
    assert any(c.solver('many')._kernel_plan()['per_node'] for c in pf.CASES), 'no box that depends on the trailing state'
    assert len(pf.BY_NAME) == len(pf.CASES)
    assert all('many' in c.geometries for c in pf.CASES) and any('few' in c.geometries for c in pf.CASES)


@pytest.mark.timeout(1200)
def test_the_units_compile_for_gfx950():
    """(hipcc cross-compiles; `build()` compiles the same units ahead -- __graft_entry__._prebuild_models --, so on a
    built tree this finds them in the cache)"""
    from stodynprog_amd import _native as nat
    sources = {}
    for c in pf.CASES:
        for what, src in pf.unit_sources(c).items():
            sources.setdefault(src, (c, what))
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=min(6, os.cpu_count() or 1)) as pool:
        mods = list(pool.map(nat.compile_model, list(sources)))
    for (src, what), mod in zip(sources.items(), mods):
        assert mod and os.path.exists(mod), what
