"""The UNIFORM bound stage of the branch and bound (SDP_BNB_UNIFORM: sdp_short_bnb of csrc/sdp_colfilter_kernel.h, the
records of sdp_col_phase_u, the padding of the reduced table in csrc/sdp_colres_kernel.h), checked in EXACT arithmetic
(no GPU), in the style of tests/test_filter_bound_exact.py, whose helpers it uses.

Where node r of a column sits at row r of the stock axis, the block ends of lane r are taken at  r + k_b + phi_b,
k_b = floor(start_b), phi_b = start_b - k_b  of the block records, instead of  pX + start_b  located per node; the
reduced table is padded with the linear continuation of its first and last cell instead of clamped cells.  Here the
records, the padding and the bound are computed with Python floats, operation by operation as the kernel rounds, and
the bound is compared -- exactly -- with the F' of every control of the block AS THE EVALUATION STAGE FORMS IT (the
reference's cell of fl(X +- a), fused operations on the unpadded table): it must lie below it up to the 24 u S_node
the skip test allows (16 u as before, 8 u for the padded rows).  Finite inputs only.

The second half checks what the planner refuses: a stock axis that is not uniform, a box per node, 4-byte reals, the
shifted lattice -- each keeps the unit it had."""
import math
from fractions import Fraction

import numpy as np
import pytest

from test_filter_bound_exact import BNB_DELTA, U, filter_constants, fma, random_problem, reduced_table

from stodynprog_amd import DPSolver, codegen, models

PAD = codegen.BNB_PAD


def kernel_cell(xn0, smin, span, nm1, n0):
    """sdp_lean2_cell: the reference's cell of a position, in the axis mode the kernel picks (sdp_col_axis_mode)"""
    pow2 = span > 0 and math.frexp(span)[0] == 0.5
    if pow2 and smin == 0.0 and span == 1.0:
        sn = xn0
    elif pow2:
        sn = (xn0 - smin) * (1.0 / span)
    else:
        sn = (xn0 - smin) / span
    p = sn * nm1
    q0 = max(min(int(p), n0 - 2), 0)
    return q0, p - float(q0)


def uniform_bound_check(T, p, axis, r, K, a, h, chunked, sign, block, lead='add'):
    """Returns (the largest (LB - F') / (24 u S_node) over the controls of every block, whether the lattice's ends lie
    beyond BOTH ends of the axis, so that padded rows are read on either side), or None where
    the kernel would not run the stage (blocks out of order, a reach beyond the padding, a node off its row)."""
    W, N0 = T.shape
    fc = filter_constants(p)
    A = reduced_table(T, p, chunked)
    smin, span, nm1 = float(axis[0]), float(axis[-1] - axis[0]), float(N0 - 1)
    k_rows = nm1 / span
    X = float(axis[r])
    if not abs((X - smin) * k_rows - float(r)) <= 2.0 ** -22:      # the caller of sdp_short_bnb, lane by lane
        return None
    dcol = max(fc['pcap'] * max(abs(T[w][q]) for w in range(W)) + fc['floor'] for q in range(N0))
    n = len(a)
    where = {'add': lambda v: X + v, 'sub': lambda v: X - v}[lead]
    cell = lambda v: kernel_cell(where(v), smin, span, nm1, N0)
    L = max(1.0, abs(cell(min(a))[1]), abs(cell(max(a))[1]))
    s_node = fma(fc['pcap'], abs(K) + max(abs(v) for v in h), (1.0 + 2.0 * L) * dcol)
    # the records of the table's wave (sdp_col_phase_u)
    blocks = [range(b0, min(b0 + block, n)) for b0 in range(0, n, block)]
    pa = [(-v if lead == 'sub' else v) * k_rows for v in a]
    lo = [min(pa[c] for c in m) for m in blocks]
    hi = [max(pa[c] for c in m) for m in blocks]
    if any(hi[b] + 2 * BNB_DELTA > lo[b + 1] for b in range(len(blocks) - 1)):
        return None
    assert abs(X) < 2.0 ** 30 / k_rows - abs(smin) - max(abs(v) for v in a)       # (st[3])
    starts = [v - BNB_DELTA for v in lo] + [hi[-1] + BNB_DELTA]
    between = max([lo[b + 1] - lo[b] for b in range(len(blocks) - 1)] + [hi[-1] - lo[-1]])
    extra = max(int(between + 4 * BNB_DELTA) - 1, 0)
    kb = [math.floor(v) for v in starts]
    phi = [v - float(k) for v, k in zip(starts, kb)]          # (one subtraction, as the wave does it)
    assert all(0.0 <= f <= 1.0 and abs(Fraction(f) + k - Fraction(v)) <= Fraction(1, 2 ** 53) for f, k, v in zip(phi, kb, starts))
    if max(abs(k) for k in kb) + 2 > PAD:
        return None
    # (the rows strictly between two ends: the two that the ends' cells bring along and at most `extra` more)
    assert max(kb[b + 1] - kb[b] for b in range(len(blocks))) - 2 <= extra
    hp = [min((sign * h[c]) * fc['psum'] for c in m) for m in blocks]
    # the padded table (sdp_sweep_col of csrc/sdp_colres_kernel.h)
    Ap = {q: float(A[q]) for q in range(N0)}
    for j in range(1, PAD + 1):
        Ap[-j] = fma(-float(j), A[1] - A[0], A[0])
        Ap[N0 - 1 + j] = fma(float(j), A[N0 - 1] - A[N0 - 2], A[N0 - 1])
    ends = [fma(f, Ap[r + k + 1] - Ap[r + k], Ap[r + k]) for f, k in zip(phi, kb)]
    worst = Fraction(-10 ** 9)
    for b, members in enumerate(blocks):
        m = min(ends[b], ends[b + 1], Ap[r + kb[b] + 1], Ap[r + kb[b + 1]])
        for kk in range(extra):
            m = min(m, Ap[r + min(kb[b] + 2 + kk, kb[b + 1] - 1)])
        lbv = hp[b] + m
        for ci in members:
            q0, lam0 = cell(a[ci])
            # the kernel's own position of the control lies between the block's ends (or in a clamped cell beyond them)
            assert float(r) + starts[b] <= float(q0) + lam0 <= float(r) + starts[b + 1]
            F = fma(sign * h[ci], fc['psum'], fma(lam0, A[q0 + 1] - A[q0], A[q0]))
            worst = max(worst, (Fraction(lbv) - Fraction(F)) / (24 * Fraction(U) * Fraction(s_node)))
    return float(worst), bool(r + kb[0] < 0 and r + kb[-1] >= N0 - 1)


def lattice(rng, n, k_rows, reach_rows, lead):
    """a monotone in the control, steps of at least 4 DELTA rows, about +-reach_rows rows"""
    spread = reach_rows / k_rows
    a = -spread + np.cumsum(rng.uniform(0.1, 1.0, size=n)) * (2 * spread / n) + np.arange(n) * 4 * BNB_DELTA / k_rows
    a = [float(v) for v in a]
    return a[::-1] if lead == 'sub' else a


AXES = {
    'unit': lambda n: np.linspace(0.0, 1.0, n),                   # (axis mode 2)
    'pow2': lambda n: np.linspace(-3.0, 5.0, n),                  # (a power-of-two span: mode 1)
    'span': lambda n: np.linspace(0.3, 7.1, n),                   # (span != 1, a true division: mode 0)
    'rounded': lambda n: np.linspace(-0.7, 0.9, n),               # (stored values off their rows: delta > 0)
}


@pytest.mark.parametrize('regime', ['ordinary', 'large', 'small', 'mixed', 'cancel', 'weights'])
@pytest.mark.parametrize('axis', sorted(AXES))
def test_the_uniform_bound_lies_below_every_control_of_its_block(regime, axis):
    rng = np.random.default_rng(700 + ['ordinary', 'large', 'small', 'mixed', 'cancel', 'weights'].index(regime) * 4
                                + sorted(AXES).index(axis))
    worst, checked, beyond, short_last = -1e9, 0, 0, 0
    for trial in range(60):
        T, p, _ = random_problem(rng, regime)
        W, N0 = T.shape
        x = AXES[axis](N0)
        assert codegen.uniform_rows_axis(x, np.float64, N0)
        k_rows = float(N0 - 1) / float(x[-1] - x[0])
        scale = float(np.abs(T).max())
        n = int(rng.integers(1, 90))
        lead = 'sub' if trial % 2 else 'add'
        # (reach in rows: within a cell ... the padding's 14; every other trial past both ends of the axis of 3 - 13 rows)
        reach = float(rng.uniform(min(N0, 12), 13.5)) if trial % 2 == 0 else float(10.0 ** rng.uniform(-1, 1.1))
        a = lattice(rng, n, k_rows, reach, lead)
        K = float(rng.standard_normal()) * scale * 10.0 ** rng.uniform(-3, 3)
        h = [float(v) * scale * 10.0 ** rng.uniform(-3, 3) for v in rng.standard_normal(n)]
        sign = -1.0 if trial % 3 == 0 else 1.0
        block = 8 if trial % 5 else 16
        for r in sorted({0, N0 - 1, int(rng.integers(0, N0))}):
            out = uniform_bound_check(T, p, x, r, K, a, h, bool(trial % 4 == 1), sign, block, lead)
            if out is None:
                continue
            checked += 1
            beyond += out[1]
            short_last += n % block != 0
            assert out[0] <= 1.0, (regime, axis, trial, r, out)
            worst = max(worst, out[0])
    assert checked >= 100 and beyond >= 10 and short_last >= 50, (checked, beyond, short_last)
    assert worst < 0.5, worst                                  # (a handful of roundings against twenty-four)


def test_a_block_end_exactly_on_a_row():
    """phi_b = 0: the end IS the row; the row is an end, not a row between"""
    rng = np.random.default_rng(77)
    hits = 0
    for trial in range(40):
        T, p, _ = random_problem(rng, 'ordinary')
        W, N0 = T.shape
        N0 = 9                                                 # (k = 8 rows per unit: a = (j + DELTA) / 8 is exact)
        T = rng.standard_normal((W, N0))
        x = np.linspace(0.0, 1.0, N0)
        n = 24
        a = [(float(j // 2) + BNB_DELTA + (j % 2) * 0.37) / 8.0 - 0.75 for j in range(n)]      # blocks of 8 start on rows -6, -2, 2
        h = [float(v) for v in rng.standard_normal(n)]
        for r in range(N0):
            out = uniform_bound_check(T, p, x, r, 0.3, a, h, False, 1.0, 8)
            assert out is not None and out[0] <= 1.0, (trial, r, out)
            hits += 1
    starts = [min(a[b0:b0 + 8]) * 8.0 - BNB_DELTA for b0 in (0, 8, 16)]
    assert starts == [-6.0, -2.0, 2.0] and hits == 360


def test_the_rounded_axis_is_off_its_rows_and_still_planned():
    x = AXES['rounded'](11)
    k = 10.0 / float(x[-1] - x[0])
    off = max(abs(Fraction(float(v)) - Fraction(float(x[0]))) * Fraction(k) - r for r, v in enumerate(x))
    assert 0 < off < Fraction(1, 2 ** 40)
    assert codegen.uniform_rows_axis(x, np.float64, 11)


def test_the_axis_check_refuses_what_is_not_a_uniform_grid():
    x = np.linspace(0.0, 1.0, 33)
    assert codegen.uniform_rows_axis(x, np.float64, 33)
    assert not codegen.uniform_rows_axis(x, np.float32, 33)                          # 4-byte reals
    assert not codegen.uniform_rows_axis(x, np.float64, 32)                          # not the column's axis
    assert not codegen.uniform_rows_axis(x ** 2, np.float64, 33)                     # not uniform
    y = x.copy()
    y[7] += 2.0 ** -20 / 32                                                          # one node 2^-20 rows off its row
    assert not codegen.uniform_rows_axis(y, np.float64, 33)
    y[7] = x[7] + 2.0 ** -30 / 32                                                    # .. 2^-30 rows: within the bound
    assert codegen.uniform_rows_axis(y, np.float64, 33)
    assert not codegen.uniform_rows_axis(x[::-1], np.float64, 33)
    assert not codegen.uniform_rows_axis(np.array([0.0]), np.float64, 1)
    y = x.copy()
    y[3] = np.nan
    assert not codegen.uniform_rows_axis(y, np.float64, 33)


# ---------------------------------------------------------------------------
# the planner
def _resident(noise=0.0, dtype=np.float64, box=None, axis=None):
    """the benchmark model at a shape that plans the resident-chunk form with the branch and bound (tests/column_forms.py)"""
    sysd, ref = models.synthetic3d(N=8, stock_noise=noise)
    if box is not None:
        sysd.control_box = box
    s = DPSolver(sysd, dtype=dtype)
    s.discretize_state(0, 1, 256, 0, 1, 128, 0, 1, 128)
    if axis is not None:
        s.state_grid = [np.asarray(axis)] + list(s.state_grid[1:])
    s.perturb_grid, s.perturb_proba = ref.perturb_grid, ref.perturb_proba
    s.control_steps = (2. / 62.5,)
    return s


def _source(s, debug=None):
    saved = DPSolver.debug_defines
    DPSolver.debug_defines = debug
    try:
        return s._kernel_plan()['source']
    finally:
        DPSolver.debug_defines = saved


def _plans_it(source):
    return '#define SDP_BNB_UNIFORM 1' in source


def test_the_benchmark_shape_plans_the_uniform_stage_and_the_switch_takes_it_out():
    on = _source(_resident())
    off = _source(_resident(), {'SDP_BNB_UNIFORM': '0'})
    assert _plans_it(on) and '#define SDP_COL_BNB 1' in on and '#define SDP_COL_WRES 16' in on
    assert not _plans_it(off)
    # the switch changes nothing else: the line that defines the macro is the whole difference
    assert [ln for ln in on.splitlines() if 'SDP_BNB_UNIFORM' not in ln] == off.splitlines()


@pytest.mark.parametrize('what', ['axis', 'box', 'reals', 'shift'])
def test_the_planner_refuses_the_uniform_stage_and_keeps_the_unit_it_had(what):
    if what == 'axis':
        s = _resident(axis=np.linspace(0.0, 1.0, 256) ** 1.5)          # a stock axis that is not uniform
    elif what == 'box':
        s = _resident(box=lambda x0, x1, x2: ((-1., 1. - 0.5 * x0),))   # a box per node: no control table
    elif what == 'reals':
        s = _resident(dtype=np.float32)
    else:
        s = _resident(noise=0.07)                                       # the shifted lattice
    src = _source(s)
    assert not _plans_it(src)
    # today's plan: what the unit was with the stage switched off altogether
    assert src == _source(s, {'SDP_BNB_UNIFORM': '0'})
    if what == 'axis':
        assert '#define SDP_COL_BNB 1' in src and '#define SDP_COL_LEAN2 1' in src
    if what == 'shift':
        assert '#define SDP_COL_SHIFT 1' in src and '#define SDP_COL_BNB 1' in src
    if what == 'box':
        assert 'SDP_COL_LEAN2' not in src


def _lds_of(source):
    """the LDS image the plan counted against what the generated unit's struct holds: (planned padding rows or 0)"""
    import re
    m = re.search(r'^#define SDP_BNB_PAD_ROWS (\d+)', source, re.M)
    return int(m.group(1)) if m else 0


def test_the_planned_image_counts_the_padding():
    """codegen._column_lds mirrors struct SdpColLds: 2 x BNB_PAD reals more where a unit pads its reduced table; the plan's
    LDS bytes and the unit's define come from ONE decision (codegen.uniform_stage_pad)"""
    base = codegen._column_lds(16, 32, 256, 3, 8, 256, reduced=True, utab_values=codegen.utab_reals(2, 64))
    padded = codegen._column_lds(16, 32, 256, 3, 8, 256, reduced=True, utab_values=codegen.utab_reals(2, 64), bnb_pad=True)
    assert padded - base == 2 * PAD * 8 and 4 * padded <= codegen.COLUMN_LDS_MAX
    for debug in (None, {'SDP_BNB_UNIFORM': '0'}):             # (the A/B switch keeps the padding)
        assert _lds_of(_source(_resident(), debug)) == PAD
    for debug in ({'SDP_COL_BNB': '0'}, {'SDP_COL_LEAN2': '0'}):
        src = _source(_resident(), debug)
        assert _lds_of(src) == 0 and not _plans_it(src)


def test_the_padding_is_not_granted_where_it_costs_the_cu_a_workgroup():
    """33 perturbation points, 17 resident (tests/column_forms.py hold_4x4x2_w33): 256 bytes more would leave three
    workgroups per CU where four fit"""
    s = _resident()
    s.discretize_perturb(-0.3, 0.3, 33)
    src = _source(s)
    assert '#define SDP_COL_WRES 17' in src and '#define SDP_COL_MIN_WAVES 4' in src
    assert not _plans_it(src) and _lds_of(src) == 0


@pytest.mark.parametrize('n0', [65, 129, 193])
def test_the_planner_refuses_an_axis_whose_last_two_rows_sit_in_two_waves(n0, debug_defines):
    debug_defines.set(SDP_COL_WRES=16)
    s = _resident()
    s.discretize_state(0, 1, n0, 0, 1, 128, 0, 1, 128)
    src = _source(s, DPSolver.debug_defines)
    assert '#define SDP_COL_BNB 1' in src and '#define SDP_COL_WRES 16' in src
    assert not _plans_it(src) and _lds_of(src) == 0
    s.discretize_state(0, 1, n0 + 1, 0, 1, 128, 0, 1, 128)
    assert _plans_it(_source(s, DPSolver.debug_defines))


def test_the_planner_refuses_a_lattice_that_reaches_past_the_padding():
    """the reach is proved on the host (codegen.uniform_stage_reach): max |a| k + 3 rows within the padding, else the unit
    keeps the bound stage that locates every end per node -- and with it its branch and bound"""
    def gain(rows):
        sysd, ref = models.synthetic3d(N=8)
        b = rows / 255.0
        sysd.dyn = lambda x0, x1, x2, u, w: (x0 + b * u, 0.1 + 0.6 * x1 + 0.2 * x2 + w, 0.2 + 0.1 * x1 + 0.5 * x2 + 0.5 * w)
        s = DPSolver(sysd)
        s.discretize_state(0, 1, 256, 0, 1, 128, 0, 1, 128)
        s.perturb_grid, s.perturb_proba = ref.perturb_grid, ref.perturb_proba
        s.control_steps = (2. / 62.5,)
        return _source(s)
    for rows, planned in ((8.2, True), (12.9, True), (13.1, False), (40.0, False)):
        src = gain(rows)
        assert '#define SDP_COL_BNB 1' in src and '#define SDP_COL_LEAN2 1' in src, rows
        assert _plans_it(src) == planned and (_lds_of(src) == PAD) == planned, rows
