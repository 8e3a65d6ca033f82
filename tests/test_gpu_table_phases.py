"""The lean reductions of the plain resident-chunk column kernel (csrc/sdp_colres_kernel.h, codegen.table_phase_plan) on the
device: the fused sums into A[r] (SDP_COL_REDUCE_FUSED) and the column bound's maximum over the high words (SDP_COL_DMAX_HI).

Both touch only what the certified filter reads -- A[r], the column's bound D: J, policy and index are the reference's bits
whatever they do.  So per shape and input the unit with both items planned equals, bit for bit on all nodes, the same unit
with each item switched off in turn (its debug define at 0: the instruction stream of before for that item) and the direct
kernel (kernel='generic', which shares none of this code), and the numpy oracle on >= 500 sampled nodes that include rows 0
and n0 - 1 and the rows around every split boundary.

Shapes (tests/column_forms.py): the benchmark's geometry -- 256 rows, 16 of 32 points resident -- on 8 x 8 columns, where
every column is split into row ranges, and on 128 x 128, where a workgroup carries its state from unit to unit; 33 points
(an odd head of 17); 128 rows with 24 of 40 points resident.  These are the smallest that run both builds, both reductions,
the write-back and the hand-over from unit to unit.
Inputs: sweep 3 of the benchmark's chain, a seeded standard-normal cost-to-go (several survivors), NaN blocks and +inf rows
(D = +inf: the capped high word).  A diagnostic build shows on every shape that the first pass RAN on the smooth input: no
node took every control the long way, which would give the right bits without any of this."""
import numpy as np
import pytest

import column_forms as cf
from stodynprog_amd import DPSolver, codegen, models

ITEMS = codegen.TABLE_PHASE_MACROS
PAIRS = [('hold_8x2x4', 'split'), ('hold_8x2x4', 'many'), ('hold_4x4x2_w33', 'split'),
         ('hold_4x4x2_n128_w40_wres24', 'split')]
_CASES = {c.name: c for c in cf.CASES}
COUNT = dict(SDP_EXTRA_DEFINES='SDP_DIAG_BNB_COUNT=1')      # diagnostic build: J := blocks asked for (+ ..), -1: every control the long way


def _runs(case):
    """(name, debug dict, kernel) of every unit a shape is run with"""
    base = dict(case.debug)
    return ([('all', base, 'auto')] + [('no ' + m, dict(base, **{m: '0'}), 'auto') for m in ITEMS] +
            [('generic', base, 'generic')])


def units():
    """the generated sources of this file's runs (__graft_entry__.build compiles them ahead of the run)"""
    out = []
    saved = DPSolver.debug_defines
    try:
        for name, geometry in PAIRS:
            case = _CASES[name]
            for _, dbg, kernel in _runs(case) + [('count', dict(case.debug, **COUNT), 'auto')]:
                DPSolver.debug_defines = dbg or None
                out.append(case.solver(geometry, kernel=kernel)._kernel_plan()['source'])
    finally:
        DPSolver.debug_defines = saved
    return out


pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def inputs():
    """per (case, geometry): the three cost-to-go arrays and the direct kernel's sweep of each -- computed once, shared, never
    written to"""
    import test_gpu_column_forms as tcf
    made = {}

    def get(name, geometry):
        if (name, geometry) not in made:
            case = _CASES[name]
            saved = DPSolver.debug_defines
            DPSolver.debug_defines = dict(case.debug) or None
            gen = case.solver(geometry, kernel='generic')
            try:
                shape = gen._state_grid_shape
                J2, _ = tcf._quiet(gen.value_iterations, models.synthetic3d_V0(gen.state_grid, case.dtype), 2, report_time=False)
                Vb = np.random.default_rng(1000 + case.n0 + case.n_u).standard_normal(shape).astype(case.dtype)
                Vs = {'sweep 3': np.asarray(J2), 'normal V': Vb, 'NaN / inf': tcf._special_values(Vb)}
                ref = {}
                for key, V in Vs.items():
                    V.setflags(write=False)
                    ref[key] = tuple(np.array(v) for v in tcf._sweep(gen, V))
                assert gen.backend_info['kernel'] == 'generic'
            finally:
                DPSolver.debug_defines = saved
                for k in [k for k in gen._cache if k[0] == 'problem']:
                    gen._cache.pop(k).close()
            made[name, geometry] = (Vs, ref)
        return made[name, geometry]
    return get


@pytest.mark.timeout(300)
@pytest.mark.parametrize('name,geometry', PAIRS, ids=['{}-{}'.format(*p) for p in PAIRS])
def test_every_item_on_equals_each_item_off_the_direct_kernel_and_the_oracle(gpu, debug_defines, inputs, name, geometry):
    import test_gpu_column_forms as tcf
    case = _CASES[name]
    Vs, ref = inputs(name, geometry)
    nodes = None
    got = {}
    for run, dbg, kernel in _runs(case)[:-1]:
        debug_defines.unset(*(ITEMS + ('SDP_COL_WRES', 'SDP_EXTRA_DEFINES')))
        if dbg:
            debug_defines.set(**dbg)
        s = case.solver(geometry, kernel=kernel)
        try:
            src = s._kernel_plan()['source']
            for m in ITEMS:
                assert (cf.macro(src, m) == '1') == (dbg.get(m) != '0'), (run, m)
            assert cf.hold_geometry(src) == case.hold and not cf.missing_claims(case, geometry, src)
            if nodes is None:
                nodes = cf.sample_nodes(s._state_grid_shape, seed=len(name))
                assert len(nodes) >= 500
            for key, V in Vs.items():
                got[run, key] = tuple(np.array(v) for v in tcf._sweep(s, V))
            assert s.backend_info['kernel'] == 'column' and s.backend_info['certified_filter']
            assert tcf._ran_source(s) == src
        finally:
            for k in [k for k in s._cache if k[0] == 'problem']:
                s._cache.pop(k).close()
    for key, V in Vs.items():
        what = '{} {} {}'.format(name, geometry, key)
        tcf._same(got['all', key], ref[key], what + ': all items vs the direct kernel')
        for m in ITEMS:
            tcf._same(got['all', key], got['no ' + m, key], what + ': all items vs {} = 0'.format(m))
        tcf._against_oracle(case, geometry, V, got['all', key], nodes, what, key != 'NaN / inf', key == 'sweep 3')
    assert np.isnan(got['all', 'NaN / inf'][0]).any() and np.isfinite(got['all', 'NaN / inf'][0]).any()


@pytest.mark.timeout(120)
@pytest.mark.parametrize('name,geometry', PAIRS, ids=['{}-{}'.format(*p) for p in PAIRS])
def test_the_first_pass_ran_on_the_smooth_input(gpu, debug_defines, inputs, name, geometry):
    """the diagnostic build stores the blocks each node asked for, or -1 where its wave took every control the long way"""
    import test_gpu_column_forms as tcf
    case = _CASES[name]
    debug_defines.set(**dict(case.debug, **COUNT))
    s = case.solver(geometry)
    try:
        src = s._kernel_plan()['source']
        assert all(cf.macro(src, m) == '1' for m in ITEMS) and '#define SDP_DIAG_BNB_COUNT 1' in src
        J, _, _ = tcf._sweep(s, inputs(name, geometry)[0]['sweep 3'])
        cnt = np.round(J).astype(int)
        assert (cnt >= 0).all(), 'a wave took every control the long way'
        assert (cnt < 10000).all(), 'the first pass left more than its survivor at a node of the smooth input'
    finally:
        for k in [k for k in s._cache if k[0] == 'problem']:
            s._cache.pop(k).close()
