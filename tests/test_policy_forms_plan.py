"""The tables of tests/policies.py still mean what they say, without a GPU: every family plans the family or form it
claims, the units of tests/test_gpu_simulate_forms.py are the forms they are named after, and the generated policies
have the properties their names promise."""
import numpy as np
import pytest

import column_forms as cf
import policies as P


@pytest.mark.parametrize('family', P.FAMILIES, ids=[f.name for f in P.FAMILIES])
def test_every_family_plans_what_it_claims(family):
    s = family.solver()
    assert s.dtype == family.dtype
    assert P.family_of(s._kernel_plan()) == family.plans, (family, P.family_of(s._kernel_plan()))
    assert P.family_of(family.solver(kernel='generic')._kernel_plan()) == 'generic'


def test_the_simulated_units_are_the_forms_they_are_named_after(debug_defines):
    import test_gpu_simulate_forms as sf
    debug_defines.unset('SDP_COL_WRES')
    forms = {}
    for name, (make, info) in sf.UNITS.items():
        s = make()
        plan = s._kernel_plan()
        src = plan['source']
        expect = ('row window' if name == 'row window' else
                  'table per control' if name.startswith('table per control') else info['kernel'])
        assert P.family_of(plan) == expect, (name, P.family_of(plan))
        assert ('fp32' in name) == (s.dtype == np.float32), name
        if name.startswith(('full table', 'resident chunks', 'held tail')):
            forms[name] = (cf.macro(src, 'SDP_COL_WRES'), cf.hold_geometry(src))
    assert forms['full table'][0] is None and forms['full table fp32'][0] is None
    assert forms['resident chunks'][0] is not None and forms['resident chunks'][1] is None
    assert forms['held tail'][1] is not None


def test_generated_policies_are_what_their_names_say():
    case = [c for c in cf.CASES if c.name == 'hold_8x2x4'][0]
    s = case.solver('split')
    dims = s._state_grid_shape
    lo, hi = -1.0, 1.0                       # the box of the benchmark model
    step = s.control_steps[0]
    lattice = lo + step * np.arange(int(np.ceil((hi - lo) / step)) + 1)
    smooth = P.policy(s, 'smooth', seed=1)
    assert smooth.shape == dims + (1,) and (smooth >= lo).all() and (smooth <= hi).all()
    assert not np.isin(smooth, lattice).any()
    assert np.abs(np.diff(smooth[..., 0], axis=0)).max() < 0.2 * (hi - lo)            # continuous along axis 0
    out = P.policy(s, 'outside', seed=1)
    assert out.min() < lo - 2.5 * (hi - lo) and out.max() > hi + 2.5 * (hi - lo)
    rnd = P.policy(s, 'random', seed=1)
    assert (rnd >= lo).all() and (rnd <= hi).all()
    # neighbouring nodes of one column reach far apart: a jump of more than half the box
    assert (np.abs(np.diff(rnd[..., 0], axis=0)) > 0.5 * (hi - lo)).mean() > 0.1
    sp = P.policy(s, 'special', seed=1)
    bad = ~np.isfinite(sp[..., 0])
    assert np.isnan(sp).any() and np.isposinf(sp).any() and np.isneginf(sp).any()
    assert bad[0].any() and bad[-1].any() and bad[:, -1, -1].sum() >= 5
    assert all(bad[r].any() for r in cf.split_rows(dims[0]))
    assert np.array_equal(sp[~bad], smooth[~bad])
    # two controls: their components are generated independently
    two = P.FAMILIES[[f.name for f in P.FAMILIES].index('lead')].solver()
    p2 = P.policy(two, 'smooth', seed=1)
    assert p2.shape[-1] == 2
    z = [(p2[..., c] - p2[..., c].min()) / np.ptp(p2[..., c]) for c in range(2)]
    assert not np.allclose(z[0], z[1])
