"""The table of column-kernel forms (tests/column_forms.py) still means what it says, without a GPU: every case
plans the macros it claims at every geometry it runs at, the held tail is covered at its four geometries, and the
units of the held tail and of 1024-thread workgroups compile for gfx950.  When a planner change moves a shape to
another form, these tests name the case that lost its coverage instead of letting it test something else."""
import os

import pytest

import column_forms as cf


def _source(case, geometry, debug_defines, **kw):
    if case.debug:
        debug_defines.set(**case.debug)
    else:
        debug_defines.unset('SDP_COL_WRES')
    return case.solver(geometry, **kw)._kernel_plan()['source']


@pytest.mark.parametrize('case,geometry', cf.PAIRS, ids=['{}-{}'.format(c.name, g) for c, g in cf.PAIRS])
def test_every_case_plans_the_form_it_claims(case, geometry, debug_defines):
    src = _source(case, geometry, debug_defines)
    assert '#include "sdp_column_kernel.h"' in src, case
    missing = cf.missing_claims(case, geometry, src)
    assert not missing, '{} at {}: (macro, claimed, planned) {}'.format(case, geometry, missing)
    assert cf.hold_geometry(src) == case.hold, (case, geometry, cf.hold_geometry(src))
    # the kernels it is compared with: the same family without the filter, and the direct kernel
    assert cf.macro(_source(case, geometry, debug_defines, certified_filter=False), 'SDP_COL_FILTER') is None
    assert '#include "sdp_column_kernel.h"' not in _source(case, geometry, debug_defines, kernel='generic')


def test_the_table_covers_the_forms_it_is_for():
    holds = {c.hold for c in cf.CASES if c.hold}
    assert {(8, 2, 4), (4, 4, 2), (16, 1, 4), (8, 1, 4)} <= holds, holds
    # each of them also with noise in the stock (the planner keeps the hold on the shifted lattice)
    noisy = {c.hold for c in cf.CASES if c.hold and c.noise}
    assert {(8, 2, 4), (4, 4, 2), (16, 1, 4), (8, 1, 4)} <= noisy, noisy
    for c in cf.CASES:
        if c.hold and c.n_u == 64:
            assert 'split' in c.geometries and 'many' in c.geometries, c
    # 1024 threads: in 8-byte reals at both geometries somewhere, and in 4-byte reals
    wide = [(c, g) for c, g in cf.PAIRS if cf.claims(c, g).get('SDP_COL_THREADS') == '1024']
    assert {g for c, g in wide if c.dtype.itemsize == 8} == {'many', 'split'}
    assert any(c.dtype.itemsize == 4 for c, g in wide)
    # the branch and bound's partial last block of 8 controls: 1, 1 and 7 controls in it
    assert {c.n_u % 8 for c in cf.CASES if cf.claims(c, 'many').get('SDP_COL_BNB') == '1'} >= {1, 7}
    assert len({c.name for c in cf.CASES}) == len(cf.CASES)


def test_split_rows_are_the_boundaries_of_column_grid():
    # n0 = 256: at most 4 row ranges of >= 64 rows -- boundaries 128 (2), 85 / 170 (3), 64 / 128 / 192 (4)
    assert cf.split_rows(256) == [63, 64, 84, 85, 127, 128, 169, 170, 191, 192]
    assert cf.split_rows(128) == [63, 64]
    nodes = cf.sample_nodes((256, 8, 8))
    assert len(nodes) >= 500 and nodes.max() == 256 * 64 - 1 and (sorted(set(nodes)) == list(nodes))


def _compiled_units():
    out = []
    for c, g in cf.PAIRS:
        if c.hold or cf.claims(c, g).get('SDP_COL_THREADS') == '1024':
            out.append((c, g))
    return out


@pytest.mark.timeout(1200)
def test_held_tail_and_1024_thread_units_compile_for_gfx950(debug_defines):
    """(hipcc cross-compiles; `build()` compiles the same units ahead -- __graft_entry__._prebuild_models --, so on a
    built tree this finds them in the cache)"""
    from stodynprog_amd import _native as nat
    sources = {}
    for c, g in _compiled_units():
        sources.setdefault(_source(c, g, debug_defines), c)
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=min(6, os.cpu_count() or 1)) as pool:
        mods = list(pool.map(nat.compile_model, list(sources)))
    for (src, case), mod in zip(sources.items(), mods):
        assert mod and os.path.exists(mod), case
