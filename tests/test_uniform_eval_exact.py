"""The UNIFORM EVALUATION stage of the branch and bound (SDP_BNB_UNIFORM_EVAL: sdp_short_bnb of
csrc/sdp_colfilter_kernel.h, the per-control records of sdp_col_phase_u, the radius of csrc/sdp_colres_kernel.h), checked in
EXACT arithmetic (no GPU), in the style of tests/test_uniform_bound_exact.py and tests/test_filter_bound_exact.py, whose
helpers it uses.

Control c of lane r is evaluated at row r + k_c + phi_c of the padded reduced table, k_c = floor(pa_c) and
phi_c = pa_c - k_c of the record the control table's wave makes from pa_c = fl(+-a_c k), instead of at the cell the
reference's own chain of roundings gives fl(X_r +- a_c).  Here
  (a) the planner's delta (codegen.uniform_eval_delta) is compared with the true distance between the two positions, pair
      by pair, each formed with Python floats operation by operation as the kernel rounds and subtracted in rationals;
  (b) |E - K P* - F'| <= radius is checked exactly with F' as the stage forms it and the radius as the kernel forms it;
  (c) the records satisfy k_c + phi_c = pa_c;
  (d) the units that must not plan the stage keep the text they had."""
import math
from fractions import Fraction

import numpy as np
import pytest

from test_filter_bound_exact import U, filter_constants, fma, pack_index, random_problem, reduced_table, reference_value
from test_uniform_bound_exact import AXES, PAD, _resident, _source, kernel_cell, lattice

from stodynprog_amd import DPSolver, codegen, models, solver as solver_mod

import test_gpu_uniform_eval as ue

EPS = 2.0 ** -52


def record(av, k_rows, lead):
    """the record of one control as the control table's wave makes it (sdp_col_phase_u): (k_c, phi_c, pa_c)"""
    pa = (-av if lead == 'sub' else av) * k_rows
    kf = math.floor(pa)
    return int(kf), pa - float(kf), pa


def reference_position(X, av, axis, lead):
    """where the reference evaluates the control of a node at X: cell and fraction of sdp_lean2_cell, as a rational"""
    n0 = len(axis)
    smin, span = float(axis[0]), float(axis[-1] - axis[0])
    q0, lam0 = kernel_cell(X - av if lead == 'sub' else X + av, smin, span, float(n0 - 1), n0)
    return Fraction(q0) + Fraction(lam0)


# ---------------------------------------------------------------------------
# (a) the planner's delta
STOCK_AXES = {
    'flagship': (0.0, 1.0, 256),
    'rows12': (0.0, 1.0, 12),
    'division': (0.5, 3.5, 12),          # smin != 0, a span that is not a power of two: the division of pyx:75
    'reciprocal': (-3.0, 5.0, 12),       # a power-of-two span: the product with the reciprocal
}


@pytest.mark.parametrize('axis', sorted(STOCK_AXES))
def test_the_planners_delta_covers_the_distance_of_every_pair(axis):
    lo, hi, n0 = STOCK_AXES[axis]
    x = np.linspace(lo, hi, n0)
    delta, dx, unit_axis = codegen.uniform_eval_delta(x, n0)
    assert unit_axis == (axis in ('flagship', 'rows12')) and 0 < dx < delta <= codegen.EVAL_DELTA_CAP
    k_rows = float(n0 - 1) / float(x[-1] - x[0])
    worst, clamped_lo, clamped_hi = Fraction(0), 0, 0
    for n_u, reach, _, _ in ue.CASES.values():
        # the lattice as the kernels form it: n points from lo to hi, a = b u in one rounding
        b = reach * (hi - lo) / (n0 - 1.0)
        for lead in ('add', 'sub'):
            for uc in np.linspace(-1.0, 1.0, n_u):
                av = float(b * uc)
                kc, phi, pa = record(av, k_rows, lead)
                assert abs(kc) + 2 <= PAD
                for r in range(n0):
                    X = float(x[r])
                    assert abs((X - float(x[0])) * k_rows - float(r)) <= dx        # (the kernel's check of the node)
                    ref = reference_position(X, av, x, lead)
                    worst = max(worst, abs(ref - (r + kc + Fraction(phi))))
                    clamped_lo += r + kc < 0
                    clamped_hi += r + kc > n0 - 2
    assert clamped_lo > 100 and clamped_hi > 100               # (controls whose cell is clamped at either end)
    assert worst <= Fraction(delta), (float(worst) / U, delta / U)
    assert worst > 0 and float(worst) > delta / 64             # (a bound, not a guess far above what happens)


def test_the_units_of_the_gpu_cases_carry_that_delta(debug_defines):
    debug_defines.set(**ue.FORCED)
    for n_u, reach, lo, hi in ue.CASES.values():
        plan = ue.solver(n_u, 'auto', reach, lo=lo, hi=hi)._kernel_plan()
        unit = plan['unit']
        delta, dx, unit_axis = codegen.uniform_eval_delta(np.linspace(lo, hi, ue.N0), ue.N0)
        assert (unit.eval_delta, unit.eval_dx, unit.eval_unit_axis) == (delta, dx, unit_axis)
        assert '#define SDP_BNB_UNIFORM_EVAL_DELTA {} '.format(float(delta).hex()) in plan['source']
        assert '#define SDP_BNB_UNIFORM_EVAL_DX {} '.format(float(dx).hex()) in plan['source']
        assert solver_mod.plan_info(plan)['uniform_eval'] == dict(delta_rows=delta, node_rows=dx, unit_axis=unit_axis)


# ---------------------------------------------------------------------------
# (b) the radius
def uniform_eval_check(T, p, axis, r, K, a, h, chunked, sign, lead):
    """Returns (the largest |E - K P* - F'| / radius over the controls, the radius, how many controls lie beyond the axis on
    either side), or None where the kernel would not run the stage (a reach beyond the padding, a node off its row)."""
    W, N0 = T.shape
    fc = filter_constants(p)
    A = reduced_table(T, p, chunked)
    delta, dx, _ = codegen.uniform_eval_delta(axis, N0)
    smin, span, nm1 = float(axis[0]), float(axis[-1] - axis[0]), float(N0 - 1)
    k_rows = nm1 / span
    X = float(axis[r])
    if not abs((X - smin) * k_rows - float(r)) <= dx:              # the caller of sdp_short_bnb, lane by lane
        return None
    recs = [record(v, k_rows, lead) for v in a]
    if max(abs(kc) for kc, _, _ in recs) + 2 > PAD:
        return None
    dcol = max(fc['pcap'] * max(abs(T[w][q]) for w in range(W)) + fc['floor'] for q in range(N0))
    n = len(a)
    bits = max((n - 1).bit_length(), 1)
    mask = (1 << bits) - 1
    where = {'add': lambda v: X + v, 'sub': lambda v: X - v}[lead]
    cell = lambda v: kernel_cell(where(v), smin, span, nm1, N0)
    L = max(1.0, abs(cell(min(a))[1]), abs(cell(max(a))[1]))
    s_node = fma(fc['pcap'], abs(K) + max(abs(v) for v in h), (1.0 + 2.0 * L) * dcol)
    # the radius of before, then the position term and the padded rows' 8 u S_node (csrc/sdp_colres_kernel.h)
    radius = fma(1.0, fma(2.0 * delta, dcol, (4.0 * EPS) * s_node), (fc['cu'] + 2.0 ** (bits + 1 - 52)) * s_node)
    # the padded table (sdp_sweep_col of csrc/sdp_colres_kernel.h)
    Ap = {q: float(A[q]) for q in range(N0)}
    for j in range(1, PAD + 1):
        Ap[-j] = fma(-float(j), A[1] - A[0], A[0])
        Ap[N0 - 1 + j] = fma(float(j), A[N0 - 1] - A[N0 - 2], A[N0 - 1])
    p_exact = sum(Fraction(v) for v in p)
    worst, below, above = Fraction(0), 0, 0
    for ci in range(n):
        kc, phi, _ = recs[ci]
        a0, a1 = Ap[r + kc], Ap[r + kc + 1]
        F = fma(sign * h[ci], fc['psum'], fma(phi, a1 - a0, a0))
        Fp = pack_index(F, ci, mask)
        q0, lam0 = cell(a[ci])                                     # what the reference computes
        E = reference_value(T, p, K + sign * h[ci], q0, lam0)
        worst = max(worst, abs(Fraction(E) - Fraction(K) * p_exact - Fraction(Fp)))
        below += r + kc < 0
        above += r + kc > N0 - 2
    return float(worst / Fraction(radius)), radius, below, above


REGIMES = ['ordinary', 'large', 'small', 'mixed', 'cancel', 'weights']


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('axis', sorted(AXES))
def test_the_radius_covers_the_uniform_evaluation_exactly(regime, axis):
    rng = np.random.default_rng(900 + REGIMES.index(regime) * 4 + sorted(AXES).index(axis))
    worst, checked, below, above, on_rows = 0.0, 0, 0, 0, 0
    for trial in range(60):
        T, p, _ = random_problem(rng, regime)
        if regime == 'cancel' and trial % 2:
            T = T * np.linspace(1.0, 40.0, T.shape[1])             # a steep table: the slope is most of D
        W, N0 = T.shape
        x = AXES[axis](N0)
        k_rows = float(N0 - 1) / float(x[-1] - x[0])
        scale = float(np.abs(T).max())
        n = int(rng.integers(1, 70))
        lead = 'sub' if trial % 2 else 'add'
        reach = float(rng.uniform(min(N0, 12), 13.5)) if trial % 2 == 0 else float(10.0 ** rng.uniform(-1, 1.1))
        a = lattice(rng, n, k_rows, reach, lead)
        if trial % 3 == 0:
            # phi at 0 and just below 1: positions on a row, and one unit in the last place below it
            j = float(rng.integers(-3, 4))
            a[0] = j / k_rows
            if n > 1:
                a[-1] = math.nextafter(j + 1.0, -math.inf) / k_rows
            on_rows += 1
        K = float(rng.standard_normal()) * scale * 10.0 ** rng.uniform(-3, 3)
        h = [float(v) * scale * 10.0 ** rng.uniform(-3, 3) for v in rng.standard_normal(n)]
        sign = -1.0 if trial % 3 == 0 else 1.0
        for r in sorted({0, N0 - 1, int(rng.integers(0, N0))}):
            out = uniform_eval_check(T, p, x, r, K, a, h, bool(trial % 4 == 1), sign, lead)
            if out is None:
                continue
            checked += 1
            below += out[2]
            above += out[3]
            assert np.isfinite(out[1]) and out[1] > 0.0
            assert out[0] <= 1.0, (regime, axis, trial, r, out)
            worst = max(worst, out[0])
    assert checked >= 100 and below >= 100 and above >= 100 and on_rows >= 15, (checked, below, above, on_rows)
    assert worst < 0.8, worst


# ---------------------------------------------------------------------------
# (c) the records
def test_whole_part_and_fraction_of_a_record_add_up_to_its_position():
    rng = np.random.default_rng(41)
    rounds_to_one = 0
    values = [float(v) for v in rng.uniform(-14.0, 14.0, size=4000)] + [float(j) for j in range(-14, 15)]
    values += [-(2.0 ** -e) for e in range(1, 80)] + [2.0 ** -e for e in range(1, 80)]
    values += [math.nextafter(float(j), -math.inf) for j in range(-13, 14)]
    for pa in values:
        kc, phi, got = record(pa, 1.0, 'add')
        assert got == pa and 0.0 <= phi <= 1.0 and kc == math.floor(pa)
        err = abs(Fraction(kc) + Fraction(phi) - Fraction(pa))
        if phi == 1.0:
            rounds_to_one += 1
            assert err <= Fraction(1, 2 ** 53)                     # (a tiny negative position: the difference rounds to 1)
        else:
            assert err == 0
    assert rounds_to_one >= 20


# ---------------------------------------------------------------------------
# (d) the planner
def _plans_it(source):
    return '#define SDP_BNB_UNIFORM_EVAL 1' in source


def test_the_benchmark_unit_plans_the_stage_and_the_switch_takes_it_out():
    _, s = models.synthetic3d(N=256)
    on = _source(s)
    off = _source(s, {'SDP_BNB_UNIFORM_EVAL': '0'})
    assert _plans_it(on) and '#define SDP_BNB_UNIFORM 1' in on and '#define SDP_LEAN2_A_FIXED 1' in on
    assert 'SDP_BNB_UNIFORM_EVAL' not in off and '#define SDP_BNB_UNIFORM 1' in off
    # the switch changes nothing else: the lines that define the stage's macros are the whole difference
    assert [ln for ln in on.splitlines() if 'SDP_BNB_UNIFORM_EVAL' not in ln] == off.splitlines()
    assert len(on.splitlines()) - len(off.splitlines()) == 4
    # the bound stage's own switch leaves both stages out
    assert 'SDP_BNB_UNIFORM_EVAL' not in _source(s, {'SDP_BNB_UNIFORM': '0'})
    # .. while the bookkeeping of before round 9 keeps the stage: its switch still changes nothing but its own line
    assert _plans_it(_source(s, {'SDP_BNB_LEAN': '0'}))


@pytest.mark.parametrize('what', ['axis', 'box', 'reals', 'shift'])
def test_units_that_must_not_plan_the_stage_keep_their_text(what):
    if what == 'axis':
        s = _resident(axis=np.geomspace(0.01, 1.0, 256))                # a geometric stock axis
    elif what == 'box':
        s = _resident(box=lambda x0, x1, x2: ((-1., 1. - 0.5 * x0),))   # a box per node: no control table
    elif what == 'reals':
        s = _resident(dtype=np.float32)
    else:
        s = _resident(noise=0.07)                                       # the shifted lattice
    src = _source(s)
    assert 'SDP_BNB_UNIFORM_EVAL' not in src
    assert src == _source(s, {'SDP_BNB_UNIFORM_EVAL': '0'})
    plan = s._kernel_plan()
    assert plan['unit'].eval_delta == 0.0 and solver_mod.plan_info(plan)['uniform_eval'] is None


def test_a_control_part_that_depends_on_the_column_does_not_plan_the_stage():
    """one copy of the records serves every column of a workgroup: a of x0' = x0 + a has to follow from the control alone"""
    sysd, ref = models.synthetic3d(N=8)
    sysd.dyn = lambda x0, x1, x2, u, w: (x0 + (0.02 + 0.01 * x1) * u, 0.1 + 0.6 * x1 + 0.2 * x2 + w, 0.2 + 0.1 * x1 + 0.5 * x2 + 0.5 * w)
    s = DPSolver(sysd)
    s.discretize_state(0, 1, 256, 0, 1, 128, 0, 1, 128)
    s.perturb_grid, s.perturb_proba = ref.perturb_grid, ref.perturb_proba
    s.control_steps = (2. / 62.5,)
    src = _source(s)
    if '#define SDP_BNB_UNIFORM 1' in src:
        assert '#define SDP_LEAN2_A_FIXED 0' in src
    assert 'SDP_BNB_UNIFORM_EVAL' not in src


def test_the_stage_costs_no_lds_and_the_record_does_not_depend_on_the_bound_stages_switch():
    """the records lie in the slots a had in the control tables: the planned image is the one without the stage, and the
    record's fields are the same whether or not SDP_BNB_UNIFORM = 0 leaves both uniform stages out of the text"""
    units = {}
    saved = DPSolver.debug_defines
    try:
        for key, dbg in (('on', None), ('off', {'SDP_BNB_UNIFORM_EVAL': '0'}), ('no_uniform', {'SDP_BNB_UNIFORM': '0'})):
            DPSolver.debug_defines = dbg
            units[key] = models.synthetic3d(N=256)[1]._kernel_plan()['unit']
    finally:
        DPSolver.debug_defines = saved
    unit, off = units['on'], units['off']
    assert unit.eval_delta > 0 and unit.lds_bytes == off.lds_bytes and unit.min_waves == off.min_waves == 4
    assert off._replace(frontier=None) == unit._replace(frontier=None, eval_delta=0.0, eval_dx=0.0, eval_unit_axis=False)
    assert units['no_uniform']._replace(frontier=None) == unit._replace(frontier=None, uniform=False)
