"""The record of a column unit (codegen.ColumnUnit, plan['unit']) against the text generated from it, without a GPU:
`solver.plan_info` -- what backend_info says about a plan -- reads the record, so the record must say what the source
defines.  Every pair of tests/column_forms.py, every run of tests/fp32_cases.py and every family of tests/policies.py:
a column plan's fields equal the macros of its source, any other plan has no record, and the filter form and the
regrouped sums of plan_info are the rule on the macros that backend_info used to apply to the text."""
import pytest

import column_forms as cf
import fp32_cases as fc
import policies as P
from stodynprog_amd import DPSolver, codegen, models
from stodynprog_amd.solver import plan_info

_FP32 = [(c, r) for c in fc.CASES + [fc.CONFIG5] for r in c.runs]
_SEEN = set()           # forms of plan_info that check_plan has met (the last test: none of its equalities is vacuous)


def _one(value):
    return '1' if value else None


def _num(value):
    return str(value) if value else None


def check_plan(plan):
    """the record of `plan` against plan['source']; returns plan_info(plan)"""
    src, unit = plan['source'], plan['unit']
    macro = lambda name: cf.macro(src, name)
    assert (unit is not None) == bool(plan['column']) == ('#include "sdp_column_kernel.h"' in src)
    if unit is not None:
        assert isinstance(unit, codegen.ColumnUnit)
        with pytest.raises(AttributeError):
            unit.threads = 64
        assert macro('SDP_COL_N0') == str(unit.n0) and macro('SDP_COL_W') == str(max(unit.w, 1))
        assert macro('SDP_COL_THREADS') == str(unit.threads)
        assert macro('SDP_COL_WRES') == _num(unit.wres)
        assert macro('SDP_COL_SHIFT') == _one(unit.shift)
        assert macro('SDP_COL_SHIFT_ROWS') == (str(unit.shift_rows) if unit.shift else None) and (unit.shift or not unit.shift_rows)
        assert macro('SDP_COL_WPAIR') == ('1' if unit.wpair else '0')
        assert macro('SDP_COL_FILTER') == _one(unit.filtered)
        table = unit.frontier is not None
        assert macro('SDP_COL_UTAB') == (str(len(unit.frontier)) if table else None)
        assert macro('SDP_COL_UTAB_N') == (str(unit.utab_n) if table else None) and (table or not unit.utab_n)
        assert (macro('SDP_COL_LEAN2'), macro('SDP_COL_WIDE2')) == {
            'none': (None, None), 'lean2': ('1', None), 'wide2': (None, '1')}[unit.short]
        assert macro('SDP_COL_BNB') == _one(unit.bnb)
        assert macro('SDP_BNB_PAD_ROWS') == _num(unit.bnb_pad)
        assert macro('SDP_BNB_UNIFORM') == _one(unit.uniform)
        assert macro('SDP_COL_TAIL_HOLD') == _one(unit.tail_hold)
        assert macro('SDP_COL_ROWS') == _num(unit.window_rows)
        assert macro('SDP_COL_WCHUNK') == _num(unit.wchunk)
        # the tuning macros the planner defines (no case here hands one over in a debug dict)
        assert macro('SDP_COL_UNROLL_W') == _num(unit.unroll_w) and macro('SDP_COL_MIN_WAVES') == _num(unit.min_waves)
        assert macro('SDP_COL_A_ORDER') == ('2' if unit.a_lw else None) and macro('SDP_COL_A_LW') == _num(unit.a_lw)
        assert macro('SDP_COL_A_GROUP') == _num(unit.a_group) and macro('SDP_COL_A_WIDE_LOADS') == _num(unit.wide_loads)
        assert macro('SDP_BNB_CHUNK') == _num(unit.bnb_chunk) and macro('SDP_COLU_WIDE_LOADS') == _num(unit.colu_wide_loads)
        # the form, and the plan's keys that say it again
        assert unit.form == ('row window' if unit.window_rows else 'table per control' if unit.wchunk else
                             'resident chunks' if unit.wres else 'full table')
        assert P.family_of(plan) == {'row window': 'row window', 'table per control': 'table per control'}.get(unit.form, 'column')
        assert plan['window'] == ((unit.threads, unit.lds_bytes, unit.window_rows, unit.seg_nodes) if unit.window_rows else None)
        assert plan['col_seg_nodes'] == unit.seg_nodes and unit.lds_bytes <= codegen.COLUMN_LDS_MAX
    info = plan_info(plan)
    filtered = bool(plan['filtered'])
    assert info['certified_filter'] == filtered and (filtered or info['filter_form'] is None)
    assert (info['filter_form'] == 'shifted lattice') == (macro('SDP_COL_SHIFT') == '1' or bool(plan['line']))
    assert info['regrouped_sums'] == (filtered and macro('SDP_COL_SHIFT') == '1' and macro('SDP_COL_SHIFT_CHAIN') != '0')
    assert info['kernel'] == {'row window': 'column', 'table per control': 'column'}.get(P.family_of(plan), P.family_of(plan))
    _SEEN.update(k for k, v in (('shifted lattice', info['filter_form'] == 'shifted lattice' and plan['column']),
                                ('regrouped', info['regrouped_sums']), ('line', plan['line']),
                                ('reduced array', info['filter_form'] == 'reduced array'),
                                ('reduced table', info['filter_form'] == 'reduced table'),
                                ('no record', unit is None)) if v)
    return info


@pytest.mark.parametrize('case,geometry', cf.PAIRS, ids=['{}-{}'.format(c.name, g) for c, g in cf.PAIRS])
def test_the_record_of_every_column_form_is_its_source(case, geometry, debug_defines):
    if case.debug:
        debug_defines.set(**case.debug)
    else:
        debug_defines.unset('SDP_COL_WRES')
    plan = case.solver(geometry)._kernel_plan()
    assert plan['unit'] is not None and check_plan(plan)['kernel'] == 'column'
    assert check_plan(case.solver(geometry, kernel='generic')._kernel_plan())['kernel'] == 'generic'


@pytest.mark.parametrize('case,run', _FP32, ids=['{}-{}'.format(c.name, r).replace(' ', '_') for c, r in _FP32])
def test_the_record_of_every_4_byte_run_is_its_source(case, run):
    check_plan(fc.plan_of(case.solver(run)))


@pytest.mark.parametrize('family', P.FAMILIES, ids=[f.name for f in P.FAMILIES])
def test_the_record_of_every_family_is_its_source(family):
    plan = family.solver()._kernel_plan()
    assert (plan['unit'] is not None) == (family.plans in ('column', 'row window', 'table per control'))
    check_plan(plan)


def test_the_uniform_stage_pads_the_image_the_record_counts(debug_defines):
    import test_gpu_uniform_bound as ub
    debug_defines.set(**ub.FORCED)
    plan = ub.solver(64, 'auto', 8.0)._kernel_plan()
    unit = plan['unit']
    check_plan(plan)
    assert unit.uniform and unit.bnb_pad == codegen.BNB_PAD and unit.wres == ub.WRES and unit.short == 'lean2' and unit.bnb
    args = (ub.WRES, ub.N_W, ub.N0, 3, 8, unit.threads)
    kw = dict(reduced=True, utab_values=codegen.utab_reals(len(unit.frontier), unit.utab_n))
    assert unit.lds_bytes == codegen._column_lds(*args, bnb_pad=True, **kw)
    assert unit.lds_bytes == codegen._column_lds(*args, **kw) + 2 * codegen.BNB_PAD * 8
    # the A/B switch keeps the padding and leaves the stage out
    debug_defines.set(SDP_BNB_UNIFORM=0)
    off = ub.solver(64, 'auto', 8.0)._kernel_plan()
    check_plan(off)
    assert off['unit']._replace(frontier=None) == unit._replace(uniform=False, frontier=None)        # (each trace has its own nodes)


def test_no_equality_above_is_vacuous(debug_defines):
    """the plans of this file have every form that plan_info tells apart -- with one model more for a chain of sums in
    another nesting, which no table plans in the column family"""
    debug_defines.unset('SDP_COL_WRES')
    sysd, ref = models.synthetic3d(N=256, stock_noise=0.07, nested=True)
    s = DPSolver(sysd)
    s.state_grid, s.perturb_grid = ref.state_grid, ref.perturb_grid
    s.perturb_proba, s.control_steps = ref.perturb_proba, ref.control_steps
    info = check_plan(s._kernel_plan())
    assert info['regrouped_sums'] and info['filter_form'] == 'shifted lattice'
    _SEEN.clear()
    for family in P.FAMILIES:
        check_plan(family.solver()._kernel_plan())
    for case, geometry in cf.PAIRS:
        if not case.debug:
            check_plan(case.solver(geometry)._kernel_plan())
    assert {'shifted lattice', 'line', 'reduced array', 'reduced table', 'no record'} <= _SEEN, _SEEN
