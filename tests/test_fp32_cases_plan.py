"""The table of 4-byte cases (tests/fp32_cases.py) still means what it says, without a GPU: every run of every case
plans a unit of 4-byte reals of the family it claims, with the macros it claims; a kernel the case says is 8-byte
only refuses it; every model is one whose trace repeats numpy bit for bit.  A planner change that moves a case to
another family names it here instead of letting tests/test_gpu_fp32_oracle.py test something else."""
import numpy as np
import pytest

import fp32_cases as fc

_ALL = fc.CASES + [fc.CONFIG5]


@pytest.mark.parametrize('case', _ALL, ids=[c.name for c in _ALL])
def test_every_case_plans_the_family_and_dtype_it_claims(case):
    for run in case.runs:
        s = case.solver(run)
        assert s.dtype == np.float32
        model = s._trace_now(None if s.sys.stationnary else 0)
        assert model.bit_exact and not model.inexact_ops(), (case, model.inexact_ops())
        missing = fc.unmet(case, run, fc.plan_of(s))
        assert not missing, '{} in {}: {}'.format(case, run, missing)
    for kernel in case.refused:
        s = case.solver(fc.Run(kernel, kernel))
        with pytest.raises(ValueError, match='8-byte reals'):
            fc.plan_of(s)
        # ... which the same problem in 8-byte reals does plan
        ref = case.reference()
        ref.kernel = kernel
        assert fc.policies.family_of(fc.plan_of(ref)) == kernel


def test_the_table_covers_what_it_is_for():
    names = [c.name for c in _ALL]
    assert len(set(names)) == len(names)
    runs = [(c, r) for c in _ALL for r in c.runs]
    # the direct kernel -- the yardstick of the other 4-byte tests -- runs in every case
    for c in _ALL:
        assert any(r.family == 'generic' for r in c.runs), c
    families = {r.family for _, r in runs}
    assert {'generic', 'column', 'table per control', 'staged'} <= families, families
    # the pair table with an even W, an odd W and W = 1; the wide short first pass; 1024 threads
    W = {fc.plan_of(c.solver(r))['W'] for c, r in runs if r.macros.get('SDP_COL_WPAIR') == '1'}
    assert 1 in W and any(w % 2 for w in W if w > 1) and any(w % 2 == 0 for w in W), W
    assert any(r.macros.get('SDP_COL_WIDE2') == '1' for _, r in runs)
    assert any(r.macros.get('SDP_COL_THREADS') == '1024' for _, r in runs)
    # every 4-byte row of tests/column_forms.py at every geometry it has there
    assert {'{}-{}'.format(c.name, g) for c, g in fc.cf.PAIRS if c.dtype.itemsize == 4} <= set(names)
    # shapes: four axes without a perturbation and two controls; an axis of two points; both kinds of span
    shapes = {c.name: c.reference()._state_grid_shape for c in fc.CASES}
    assert len(shapes['four_axes_deterministic']) == 4 and 2 in shapes['edges']
    det = fc.plan_of(fc.CASES[names.index('four_axes_deterministic')].solver(fc.GENERIC))
    assert det['W'] == 0 and len(fc.CASES[names.index('four_axes_deterministic')].reference().control_steps) == 2


def test_sampled_nodes_include_the_boundaries():
    assert fc.nodes_of((24, 24, 24)) is None
    nodes = fc.nodes_of((600, 8, 8))
    assert nodes[0] == 0 and nodes[-1] == 600 * 64 - 1 and len(nodes) >= 2500 and (np.diff(nodes) > 0).all()
    assert set(fc.cf.sample_nodes((600, 8, 8))) <= set(nodes)
