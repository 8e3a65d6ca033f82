"""The table of line-kernel cases (tests/line_forms.py) still means what it says, without a GPU: every case plans the
line kernel with the lane count, SDP_LINE_W and SDP_LINE_CHAIN it claims, by the branch of the lane formula it claims;
the table covers every lane count, both branches, the ends of W, both chain forms, both span kinds, a launch of fewer
than 8 tiles and a ragged tile of 64; the counters it claims cover every decision path; and its units compile for
gfx950.  When a planner change moves a shape to another lane count, these tests name the case that lost its coverage."""
import os

import numpy as np
import pytest

import line_forms as lf

_IDS = [c.name for c in lf.CASES]


@pytest.mark.parametrize('case', lf.CASES, ids=_IDS)
def test_every_case_plans_the_line_kernel_it_claims(case):
    s = case.solver()
    plan = s._kernel_plan()
    src = plan['source']
    assert lf.planned(src) == (case.lanes, case.n_w, case.chain), (case, lf.planned(src))
    assert plan['lanes'] == case.lanes and plan['line'] and plan['max_u'] == case.controls, (case, plan['lanes'], plan['max_u'])
    # the branch of the lane formula that decided
    need, want = lf.lane_formula(case.n_x, plan['max_u'], case.n_w)
    assert min(64, max(need, want)) == case.lanes, (case, need, want)
    by = 'floor' if need == want == 1 else ('both' if need == want else ('need' if need > want else 'want'))
    assert by == case.by, (case, need, want)
    # the span, the lattice, the boxes that collapse
    g = np.asarray(s.state_grid[0], dtype=float)
    span = g[-1] - g[0]
    assert (np.frexp(span)[0] == 0.5) == case.pow2, (case, span)
    assert lf.lattice_usable(s) == case.usable, case
    counts = lf.control_counts(s)
    assert int((counts == 1).sum()) == case.collapsed and counts.max() == case.controls, (case, counts.min(), counts.max())
    assert (lf.macro(src, 'SDP_NU') == '2') == (case.model == 'two orders')
    # the diagnostic builds are the same plan with their switches, the twin is not the line kernel
    for debug in (lf.DIAG, lf.DIAG_WIDE):
        d = case.solver(debug=debug)._kernel_plan()['source']
        assert lf.planned(d) == lf.planned(src) and lf.macro(d, 'SDP_LINE_DIAG') == '1', case
    assert lf.macro(d, 'SDP_LINE_FILTER_SCALE') == '1e+18' and lf.macro(src, 'SDP_LINE_DIAG') is None
    twin = case.solver('generic')._kernel_plan()['source']
    assert lf.planned(twin) is None and 'sdp_line_kernel.h' not in twin, case


def test_the_header_is_included_only_through_the_line_switch():
    """(what `planned` keys on: sdp_sweep_kernel.h includes the line header where the unit defines SDP_LINE)"""
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(here, 'stodynprog_amd', 'csrc', 'sdp_sweep_kernel.h')) as f:
        text = f.read()
    assert '#if defined(SDP_LINE)\n#include "sdp_line_kernel.h"' in text and text.count('#include "sdp_line_kernel.h"') == 1


def test_the_table_covers_the_shapes_it_is_for():
    cases = lf.CASES
    assert len({c.name for c in cases}) == len(cases)
    assert {c.lanes for c in cases} == {1, 2, 4, 8, 16, 32, 64}
    assert {'need', 'want'} <= {c.by for c in cases}
    assert {1, 64, 65, 1024} <= {c.n_w for c in cases}
    assert 0 in {c.chain for c in cases} and any(c.chain > 0 for c in cases)
    assert {c.pow2 for c in cases} == {True, False}
    assert any(c.tiles < 8 for c in cases)
    assert any(c.lanes == 1 and c.n_x > 64 and c.n_x % 64 for c in cases)
    # every form of the header at lanes 1, 32 and 64
    forms = {'chain': lambda c: c.chain > 0, 'two perturbation terms': lambda c: c.name.startswith('two terms'),
             'a span that is no power of two': lambda c: not c.pow2, 'a span that is one': lambda c: c.pow2,
             'a box that collapses': lambda c: c.collapsed > 0,
             'a box that collapses, span no power of two': lambda c: c.collapsed > 0 and not c.pow2,
             'two controls': lambda c: c.model == 'two orders', 'a stock that leaves the grid': lambda c: c.name.startswith('leaves'),
             'an unusable lattice': lambda c: not c.usable, 'three rows': lambda c: c.n_x == 3,
             'a flat objective': lambda c: c.name.startswith('flat cost')}
    for what, has in forms.items():
        assert {1, 32, 64} <= {c.lanes for c in cases if has(c)}, what
    # every case has every input, with the special values where they are meant to be
    for c in (lf.BY_NAME['three rows@1'], lf.BY_NAME['40x17x1'], lf.BY_NAME['flat cost@64']):
        V = c.inputs()
        assert tuple(V) == c.input_names == lf.INPUTS and all(v.shape == (c.n_x,) for v in V.values())
        sp = V['special']
        assert np.isnan(sp).any() and np.isposinf(sp).any() and np.isneginf(sp).any()
        assert all(np.isfinite(V[k]).all() for k in lf.INPUTS if k != 'special')


def test_the_sampled_nodes_straddle_the_tiles():
    c = lf.BY_NAME['4000x1025x9']                  # NPW = 2, 2000 tiles, shares of 250 tiles
    nodes = set(c.sample_nodes().tolist())
    assert {0, 1, 2, 3997, 3998, 3999, 499, 500, 3499, 3500} <= nodes and len(nodes) <= 40
    c = lf.BY_NAME['3000x513x32']                  # NPW = 4, 750 tiles
    assert {0, 3, 4, 2995, 2996, 2999} <= set(c.sample_nodes().tolist())
    c = lf.BY_NAME['5000x33x5']                    # up to 2e6 cells: every node
    assert np.array_equal(c.sample_nodes(), np.arange(5000))


def test_the_claimed_paths_cover_every_decision():
    """each of the nine counters is claimed somewhere; the ones every shape must reach, at lanes 1, 32 and 64"""
    by_counter = {k: set() for k in lf.COUNTERS}
    for name, per_input in lf.PATHS.items():
        assert name in lf.BY_NAME, name
        for vname in per_input:
            counters = lf.claimed(lf.BY_NAME[name], vname)
            assert vname in lf.BY_NAME[name].input_names and counters and set(counters) <= set(lf.COUNTERS), (name, vname)
            for k in counters:
                by_counter[k].add(lf.BY_NAME[name].lanes)
    for k in lf.COUNTERS:
        assert by_counter[k], 'no case claims ' + k
    for k in ('single1', 'undecided1', 'evals2', 'long way', 'bad'):
        assert {1, 32, 64} <= by_counter[k], (k, sorted(by_counter[k]))
    # (what could not be reached at a lane count says so, with the reason)
    for k, lanes in lf.UNREACHED.items():
        assert k in lf.COUNTERS and not (set(lanes) & by_counter[k]), (k, lanes, sorted(by_counter[k]))


def test_more_than_1024_perturbation_points_are_refused():
    s = lf.shop(70, 33, 1025)
    s.kernel = 'line'
    with pytest.raises(ValueError, match="kernel = 'line' needs"):
        s._kernel_plan()
    s = lf.shop(70, 33, 1025)                      # (and 'auto' leaves such a problem to the direct kernel)
    assert lf.planned(s._kernel_plan()['source']) is None


@pytest.mark.timeout(1200)
def test_the_units_of_the_table_compile_for_gfx950():
    """plain and diagnostic (hipcc cross-compiles; `build()` compiles the same units ahead --
    __graft_entry__._prebuild_models --, so on a built tree this finds them in the cache)"""
    from stodynprog_amd import _native as nat
    sources = {}
    for c in lf.CASES:
        for what, src in lf.unit_sources(c).items():
            if what != 'generic':
                sources.setdefault(src, (c, what))
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=min(6, os.cpu_count() or 1)) as pool:
        mods = list(pool.map(nat.compile_model, list(sources)))
    for (src, case), mod in zip(sources.items(), mods):
        assert mod and os.path.exists(mod), case
