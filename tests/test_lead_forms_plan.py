"""The table of lead-kernel forms (tests/lead_forms.py) still means what it says, without a GPU: every case plans the
reduced-array sweep (csrc/sdp_lead_kernel.h) with the number of stocks, the permutation and the cost switch it claims;
what is not this family is refused; the index maps the table restates from SdpLeadGeom are consistent with each other
(they are what a mismatch on the device is read against); the grids are the kind the table says they are; and the
numpy oracle alone shows that the models exercise the controls the GPU tests compare.  When a planner change moves a
form to another family, these tests name the case that lost its coverage."""
import functools

import numpy as np
import pytest

import lead_forms as lf
from oracle import vi_numpy
from stodynprog_amd import codegen, models

_IDS = [c.name for c in lf.CASES]


@pytest.mark.parametrize('case', lf.CASES, ids=_IDS)
def test_every_case_plans_the_lead_form_it_claims(case):
    s = case.solver()
    plan = s._kernel_plan()
    assert plan['lead_axes'] == case.lead_axes, (case, plan['lead_axes'])
    assert (None if plan['lead_perm'] is None else tuple(plan['lead_perm'])) == case.lead_perm, (case, plan['lead_perm'])
    assert plan['filtered'] and plan['lanes'] == 1 and not plan['column'] and not plan['line'] and plan['staged'] is None
    src = plan['source']
    assert '#define SDP_LEAD_AXES {}\n'.format(case.lead_axes) in src
    assert 'sdp_model_leads' in src and ('sdp_model_trails' in src) == (case.lead_axes < len(s._shape()))
    if case.permuted:
        assert src.count('#define SDP_LEAD_PERM') == 1 and case.perm_define() in src, (case, lf.macro(src, 'SDP_LEAD_PERM'))
    else:
        assert '#define SDP_LEAD_PERM' not in src
    assert lf.macro(src, 'SDP_LEAD_COST_HAS_W') == ('1' if case.cost_w else '0') and src.count('#define SDP_LEAD_COST_HAS_W') == 1
    assert s.dtype == np.float64 and len(s.perturb_grid) == 1
    # the direct kernel it is compared with shares none of this
    twin = case.solver('generic')._kernel_plan()
    assert not twin['lead_axes'] and 'SDP_LEAD_AXES' not in twin['source']
    # the radius runs are the same plan with the switch
    for what, debug in lf.RADIUS_RUNS.get(case.name, {}).items():
        d = case.solver()
        d.debug_defines = dict(debug)
        dsrc = d._kernel_plan()['source']
        assert float(lf.macro(dsrc, 'SDP_LEAD_FILTER_SCALE')) == float(debug['SDP_LEAD_FILTER_SCALE']), (case, what)
        assert lf.macro(dsrc, 'SDP_LEAD_AXES') == str(case.lead_axes) and (case.perm_define() is None or case.perm_define() in dsrc)
    assert lf.macro(src, 'SDP_LEAD_FILTER_SCALE') is None


def test_the_three_control_box_has_a_digit_with_one_point():
    """`three_controls`: 84 controls at most, and ONE lattice point of the second control at the nodes where b = 0"""
    s = lf.BY_NAME['three_controls'].solver()
    plan = s._kernel_plan()
    n = np.asarray(plan['n']).reshape(3, -1)
    assert plan['max_u'] == 84 and plan['per_node'] and n.shape[1] == int(np.prod(s._shape()))
    b = np.broadcast_to(np.asarray(s.state_grid[2])[None, None, :], s._shape()).ravel()
    assert np.array_equal(n[1] == 1, b == 0.) and (n[1] == 1).sum() == 24
    assert len(np.unique(n[1])) > 2 and len(np.unique(n[2])) > 1 and (n[0] == 3).all()


@pytest.mark.parametrize('case', lf.CASES, ids=_IDS)
def test_four_byte_reals_are_not_this_family(case):
    s = case.solver(dtype=np.float32)
    plan = s._kernel_plan()
    assert not plan['lead_axes'] and plan['lead_perm'] is None and 'SDP_LEAD_AXES' not in plan['source']
    s = case.solver('lead', dtype=np.float32)
    with pytest.raises(ValueError, match="kernel = 'lead' needs"):
        s._kernel_plan()


def test_no_perturbation_at_all_is_not_this_family():
    """`all_stocks` with w also taken out of the cost: W = 0, nothing to reduce over"""
    _, s = lf.all_stocks_deterministic()
    assert s._traced().controlled_axes() == 2 and not s.perturb_grid
    plan = s._kernel_plan()
    assert not plan['lead_axes'] and 'SDP_LEAD_AXES' not in plan['source']
    _, s = lf.all_stocks_deterministic()
    s.kernel = 'lead'
    with pytest.raises(ValueError, match="kernel = 'lead' needs"):
        s._kernel_plan()
    # (and with w in the cost alone it is: TracedModel.controlled_axes gives m = d)
    assert lf.BY_NAME['all_stocks'].solver()._traced().controlled_axes() == 2


def test_the_baseline_rows_are_the_units_of_the_older_tests():
    """the generated text does not depend on the grid or on the law: the baseline rows compile the sources that
    tests/test_gpu_lead.py runs, so they are the forms covered before this table (codegen.source_key: the cache key
    of a unit hashes this text with the headers and the flags)"""
    import test_gpu_lead as old
    pairs = [('listed_first', old._small()()[1]), ('stock_last', old._stock_not_first(False)[1]),
             ('stock_middle', old._stock_not_first(True)[1]), ('listed_first', models.two_reservoirs()[1])]
    for name, theirs in pairs:
        mine = lf.BY_NAME[name].solver()._kernel_plan()['source']
        assert codegen.source_key(mine) == codegen.source_key(theirs._kernel_plan()['source']), name
    # .. while every new form is a unit of its own
    keys = {c.name: codegen.source_key(c.solver()._kernel_plan()['source']) for c in lf.CASES}
    for name in lf.NEW_FORMS:
        assert [k for k in keys.values()].count(keys[name]) == 1, name


def test_the_table_covers_the_forms_it_is_for():
    cases = lf.CASES
    assert len({c.name for c in cases}) == len(cases) and set(lf.NEW_FORMS) <= set(lf.BY_NAME)
    dims = {c.name: len(c.solver()._shape()) for c in cases}
    assert any(c.lead_axes == dims[c.name] for c in cases), 'no case without an exogenous axis'
    assert {c.lead_axes for c in cases} == {1, 2, 3}
    assert any(c.lead_axes == 2 and c.permuted and dims[c.name] == 4 for c in cases), 'two trailing axes, permuted'
    assert any(c.cost_w and c.permuted for c in cases) and any(c.cost_w and not c.permuted for c in cases)
    perms = {c.lead_perm for c in cases}
    assert {None, (1, 2, 0), (0, 2, 1), (1, 3, 0, 2), (1, 0), (1, 0, 2)} <= perms
    assert [c.name for c in cases if c.sampled] == ['phased_permuted'] and set(lf.RADIUS_RUNS) <= set(lf.BY_NAME)
    three = set()
    for c in cases:
        s = c.solver()
        shape = s._shape()
        g = lf.geom_of(c, shape)
        assert s.dtype == np.float64 and len(s.perturb_grid[0]) in (3, 5, 7), c
        law = models.NormalLaw(0, 0.2)
        assert s.perturb_grid[0][0] == -0.5 and s.perturb_grid[0][-1] == 0.5 and repr(s.sys.perturb_laws[0]) == repr(law), c
        if c.sampled:
            continue
        assert len(set(shape)) == len(shape), (c, shape)               # swapped strides change the results
        assert g.ls % 64 and int(np.prod(shape)) <= 600, (c, g.ls)      # a wave straddles planes
        if 3 in shape:
            three.add(c.name)
        if c.lead_axes >= 2 and c.name != 'flat_permuted':              # the pow2 bit of SdpLeadGeom is mixed (the flat
            # objective keeps the axes of the test it comes from: both stocks on [0, 3])
            spans = [s.state_grid[p][-1] - s.state_grid[p][0] for p in (c.lead_perm or range(len(shape)))[:c.lead_axes]]
            pow2 = [np.frexp(v)[0] == 0.5 for v in spans]
            assert any(pow2) and not all(pow2), (c, spans)
    assert three and len(three) < len(lf.SMALL)


def test_the_inputs_keep_the_reference_node_finite():
    for c in lf.SMALL:
        shape = c.solver()._shape()
        V = lf.inputs(shape)
        assert tuple(V) == lf.INPUTS and all(v.shape == shape and v.dtype == np.float64 for v in V.values())
        assert lf.ref_index(shape) == c.solver()._state_ref_ind
        bad = V['non-finite']
        assert np.isnan(bad).sum() == 1 and np.isposinf(bad).sum() == 1 and np.isneginf(bad).sum() == 1
        assert np.isfinite(bad[lf.ref_index(shape)])
        assert all(np.isfinite(V[k]).all() for k in lf.INPUTS if k != 'non-finite') and not V['zeros'].any()
        again = lf.inputs(shape)
        assert all(np.array_equal(V[k], again[k], equal_nan=True) for k in lf.INPUTS)


# ---------------------------------------------------------------------------------------------------------------------
# the index maps

@pytest.mark.parametrize('case', lf.CASES, ids=_IDS)
def test_the_index_maps_are_consistent(case):
    shape = case.solver()._shape()
    g = lf.geom_of(case, shape)
    S = int(np.prod(shape))
    assert g.S == S and g.ts * g.ls == S
    nodes = np.arange(S) if case.sampled is None else case.sample_nodes(shape)
    lead, trail = g.split(nodes)
    assert lead.min() >= 0 and lead.max() < g.ls and trail.min() >= 0 and trail.max() < g.ts
    assert np.array_equal(g.join(lead, trail), nodes)                   # join after split: the node
    pos = g.position(nodes)
    if case.sampled is None:
        # inverse bijections of range(S), and the positions a permutation of it
        assert len(set(zip(lead.tolist(), trail.tolist()))) == S
        assert np.array_equal(np.sort(pos), np.arange(S))
        ll, tt = np.divmod(np.arange(S), g.ts)                          # every (lead, trail) pair, joined and split again
        back = g.split(g.join(ll, tt))
        assert np.array_equal(back[0], ll) and np.array_equal(back[1], tt)
        assert len(np.unique(g.join(ll, tt))) == S
    else:
        assert len(np.unique(pos)) == len(nodes) and pos.min() >= 0 and pos.max() < S
    every_lead = np.arange(g.ls)
    assert np.array_equal(g.base(every_lead), g.join(every_lead, np.zeros_like(every_lead)))
    if not case.permuted:
        assert np.array_equal(lead, nodes // g.ts) and np.array_equal(trail, nodes % g.ts)
        assert np.array_equal(g.base(every_lead), every_lead * g.ts)
        assert g.nstr == g.phys
    else:
        assert not np.array_equal(lead, nodes // g.ts)
    # the `outside` test of sdp_sweep on one GPU (lmax >= aux_end = ls): the highest lattice corner is inside
    assert g.highest_corner() == g.ls - 1
    # a plane-major array read with the second pass's strides (per STATE VARIABLE) is the node-order array
    V = np.random.default_rng(S % 1000).standard_normal(S)
    Vt = np.zeros(S)
    if case.sampled is None:
        Vt[pos] = V
        ind = np.unravel_index(nodes, shape)
    else:
        allpos = g.position(np.arange(S))
        Vt[allpos] = V
        assert np.array_equal(np.sort(allpos), np.arange(S))
        ind = np.unravel_index(nodes, shape)
    at = sum(i.astype(np.int64) * g.M[p] for p, i in enumerate(ind))
    assert np.array_equal(Vt[at], V[nodes])
    assert sorted(g.M) == sorted(list(g.pm) + [g.ls * t for t in g.tm])


def test_the_index_maps_on_a_worked_example():
    """`interleaved`, (y, a, z, b) on 3 x 5 x 4 x 6 nodes with perm (1, 3, 0, 2), by hand: logical axes (a, b, y, z) of
    5, 6, 3, 4 points; node-order strides 120, 24, 6, 1 of (y, a, z, b)"""
    g = lf.Geom((3, 5, 4, 6), 2, (1, 3, 0, 2))
    assert g.ord == (5, 6, 3, 4) and g.nstr == (24, 1, 120, 6)
    assert g.pm == (6, 1) and g.ls == 30 and g.tm == (4, 1) and g.ts == 12
    assert g.M == (30 * 4, 6, 30, 1)                                    # strides of (y, a, z, b) in the plane-major copy
    node = 2 * 120 + 3 * 24 + 1 * 6 + 5                                 # y = 2, a = 3, z = 1, b = 5
    lead, trail = g.split(node)
    assert (int(lead), int(trail)) == (3 * 6 + 5, 2 * 4 + 1) and int(g.join(lead, trail)) == node
    assert int(g.base(lead)) == 3 * 24 + 5 and int(g.position(node)) == 9 * 30 + 23
    g = lf.Geom((9, 7), 2)                                              # no trailing axis: one plane
    assert g.ts == 1 and g.tm == () and g.ls == 63 and g.pm == (7, 1) and g.M == (7, 1)
    assert np.array_equal(g.position(np.arange(63)), np.arange(63))


# ---------------------------------------------------------------------------------------------------------------------
# the oracle alone

@functools.lru_cache(maxsize=None)
def _oracle_indices(name, which):
    case = lf.BY_NAME[name]
    s = case.solver()
    shape = s._shape()
    nodes = case.sample_nodes(shape)
    with np.errstate(all='ignore'):
        _, _, idx, _ = vi_numpy.value_iteration(vi_numpy.Spec.from_solver(s), lf.inputs(shape)[which], nodes=nodes)
    return idx


@pytest.mark.parametrize('which', ['smooth', 'random'])
@pytest.mark.parametrize('case', lf.CASES, ids=_IDS)
def test_the_oracle_uses_the_control_lattice(case, which):
    """the policies the GPU tests compare are not all one corner of the box: at least 5 distinct policy indices, at
    most half of the nodes at index 0 (the large case: on its sampled nodes)"""
    idx = _oracle_indices(case.name, which)
    assert len(idx) == (case.sampled or int(np.prod(case.solver()._shape())))
    assert len(np.unique(idx)) >= 5, (case, which, np.unique(idx))
    assert (idx == 0).sum() * 2 <= len(idx), (case, which, int((idx == 0).sum()), len(idx))


def test_the_flat_objective_has_near_ties():
    """`flat_permuted` on its own input: the argmin spreads over the lattice (what the radius far too small gets wrong)"""
    s = lf.BY_NAME['flat_permuted'].solver()
    with np.errstate(all='ignore'):
        _, _, idx, mar = vi_numpy.value_iteration(vi_numpy.Spec.from_solver(s), lf.flat_input(s))
    assert len(np.unique(idx)) > 5 and np.median(mar) < 1e-12


def test_the_large_case_takes_the_phased_host_path():
    """the conditions of sdp_problem_backup_host's phased branch (csrc/sdp_hip.hip), restated: 8 MiB of values or
    more, and at least 64 nodes for each of its four phases"""
    case = lf.BY_NAME['phased_permuted']
    s = case.solver()
    S = int(np.prod(s._shape()))
    assert S * s.dtype.itemsize >= 8 << 20 and S >= 256
    assert S * s.dtype.itemsize == 8 << 20                          # (exactly at the threshold)
    assert s.host_overlap and s.comm is None
    nodes = case.sample_nodes(s._shape())
    assert len(nodes) == case.sampled == len(set(nodes.tolist()))
    for ph in (1, 2, 3):
        assert {S * ph // 4 - 1, S * ph // 4} <= set(nodes.tolist())
    # every phase holds nodes of every plane: a phase is no range of lead indices
    g = lf.geom_of(case, s._shape())
    lead, trail = g.split(np.arange(S // 4))
    assert len(np.unique(lead)) == g.ls and len(np.unique(trail)) == g.ts // 4
    # the other cases stay below the threshold
    assert all(int(np.prod(c.solver()._shape())) * 8 < 8 << 20 for c in lf.SMALL)
