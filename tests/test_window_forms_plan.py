"""The table of the row-window unit (tests/window_forms.py) still means what it says, without a GPU: every case plans
the form, the macros and the segment length it claims at every geometry, the split rule restated from column_grid gives
units with the groups, chunks and trips it claims for 256 compute units, the table as a whole reaches every shape of
phase B it is for, and its units compile for gfx950."""
import os

import numpy as np
import pytest

import window_forms as wf

_IDS = ['{}-{}'.format(c.name, g) for c, g in wf.PAIRS]


@pytest.mark.parametrize('case,geometry', wf.PAIRS, ids=_IDS)
def test_every_case_plans_the_form_and_the_units_it_claims(case, geometry):
    s = case.solver(geometry)
    plan = s._kernel_plan()
    unit = plan['unit']
    assert unit.form == 'row window' and plan['window'], (case, unit)
    missing = wf.missing_claims(case.claims, plan['source'])
    assert not missing, '{} at {}: (macro, claimed, planned) {}'.format(case, geometry, missing)
    assert plan['col_seg_nodes'] == case.seg_nodes and s._shape()[0] == case.n0 and s.dtype == case.dtype
    assert (unit.a_lw is not None) == (case.order == 'order 2'), (case, unit.a_lw)
    assert '#include "sdp_column_kernel.h"' not in case.solver(geometry, 'generic')._kernel_plan()['source']
    cols = int(np.prod(s._shape()[1:]))
    if geometry != 'some':
        assert cols >= 4 * wf.CUS if geometry == 'many' else 7 <= cols <= 9, (case, geometry, cols)
    shapes = {hi - lo: wf.phase_b(hi - lo) for lo, hi in wf.sweep_bounds(s, wf.CUS, case.seg_nodes)}
    assert shapes == case.units[geometry], (case, geometry, shapes)
    assert max(shapes) <= case.seg_nodes


def test_phase_b_is_that_of_the_kernel():
    assert wf.phase_b(64) == (1, 8, False) and wf.phase_b(65) == (2, 4, False) and wf.phase_b(171) == (3, 2, False)
    assert wf.phase_b(227) == (4, 2, False) and wf.phase_b(320) == (5, 1, False) and wf.phase_b(512) == (8, 1, False)
    assert wf.phase_b(513) == (9, 1, True)
    assert [wf.chunk_range(3, k, 8) for k in range(8)] == [(0, 0), (0, 0), (0, 1), (1, 1), (1, 1), (1, 2), (2, 2), (2, 3)]


def test_the_table_covers_the_forms_it_is_for():
    reached = set()
    for c, g in wf.PAIRS:
        reached.add('{}, {} bytes'.format(c.order, c.rs))
        reached.add(c.order)
        reached.add('{} bytes'.format(c.rs))
        for rows, (groups, chunks, again) in c.units[g].items():
            reached.add('chunks {}'.format(chunks))
            if again:
                reached.add('groups > waves')
            if rows == c.seg_nodes or rows > 512:
                reached.add('a unit of the planned segment length, or of more rows than threads')
            if groups * chunks < wf.WAVES:
                reached.add('idle waves')
            if rows % 64:
                reached.add('a ragged last group')
        if c.reach is not None and g == 'many':
            reached.add('a window narrower than the controls need, at many')
    wanted = {'chunks 8', 'chunks 4', 'chunks 2', 'chunks 1', 'groups > waves', 'order 2', 'round robin', '8 bytes',
              '4 bytes', 'a unit of the planned segment length, or of more rows than threads', 'idle waves',
              'a ragged last group', 'a window narrower than the controls need, at many'}
    assert not wanted - reached, 'the table no longer reaches: {}'.format(sorted(wanted - reached))
    assert len(wf.BY_NAME) == len(wf.CASES)


def test_the_coarse_controls_leave_chunks_empty_and_pairs_incomplete():
    """from the box table and the restated chunk rule: at 'few' (8 chunks) the narrowest box of every unit has fewer
    controls than the unit has chunks, the first chunk of such a node is empty, and box sizes are no multiple of
    SDP_COL_UNROLL_U -- at 'many' (one chunk) the remainder loop then runs for them"""
    case = wf.BY_NAME['storage_2048_coarse_controls']
    s = case.solver('few')
    total = wf.box_sizes(s)
    unroll = 2                      # SDP_COL_UNROLL_U of csrc/sdp_column_kernel.h without the pair layout
    src = s._kernel_plan()['source']
    assert wf.macro(src, 'SDP_COL_UNROLL_U') is None and wf.macro(src, 'SDP_COL_WPAIR') == '0'
    assert (total % unroll != 0).any() and total.min() >= 1
    for lo, hi in wf.sweep_bounds(s, wf.CUS, case.seg_nodes):
        _, chunks, _ = wf.phase_b(hi - lo)
        assert chunks == 8 and total[lo:hi].min() < chunks
    assert wf.chunk_range(int(total.min()), 0, 8) == (0, 0)
    assert wf.empty_chunks(case, 'few') > 0 and wf.empty_chunks(case, 'many') == 0
    assert (wf.box_sizes(case.solver('many')) % unroll != 0).any()


def test_the_narrow_window_is_narrower_than_the_controls_need():
    case = wf.BY_NAME['storage_2048_narrow_window']
    s = case.solver('many')
    rows = int(case.claims['SDP_COL_ROWS'])
    honest = type(s)._lead_reach_rows(s, s._traced(), s._box_plan(None))
    assert s._kernel_plan()['unit'].window_rows == rows and max(case.units['many']) + honest > rows, honest


def test_the_sample_holds_the_first_and_the_last_unit_of_a_column_and_their_boundaries():
    for c, g in wf.PAIRS:
        s = c.solver(g)
        shape = s._shape()
        cols = int(np.prod(shape[1:]))
        bounds = wf.sweep_bounds(s, wf.CUS, c.seg_nodes)
        rows = set((wf.sample_nodes(shape, bounds) // cols).tolist())
        assert {0, c.n0 - 1} <= rows and all({lo, hi - 1} <= rows for lo, hi in bounds), (c, g)


@pytest.mark.timeout(1200)
def test_the_units_compile_for_gfx950():
    """(hipcc cross-compiles; `build()` compiles the same units ahead -- __graft_entry__._prebuild_models --, so on a
    built tree this finds them in the cache)"""
    from stodynprog_amd import _native as nat
    sources = {}
    for c in wf.CASES:
        for what, src in wf.unit_sources(c).items():
            sources.setdefault(src, (c, what))
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=min(6, os.cpu_count() or 1)) as pool:
        mods = list(pool.map(nat.compile_model, list(sources)))
    for (src, what), mod in zip(sources.items(), mods):
        assert mod and os.path.exists(mod), what
