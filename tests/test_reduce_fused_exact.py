"""The fused reduction and the rounded-up column bound of the plain resident-chunk kernel (SDP_COL_REDUCE_FUSED and
SDP_COL_DMAX_HI of csrc/sdp_colres_kernel.h), checked in EXACT arithmetic (no GPU).

(a) The reduction.  The kernel forms  A[r] = fl(head + tail),  tail = fma(p_w, T[w][r], ..) over w = C .. W-1 from 0,
head the same over w = 0 .. C-1: the exact product, ONE rounding per point, head plus tail last.  `fused_table` restates
that, and takes the place of `reduced_table` -- the separately rounded product and sum -- in the modules whose checks read it:
the short pass' radius |E - K P* - F'| <= radius (tests/test_filter_bound_exact.py), the block bound of the uniform bound stage
(tests/test_uniform_bound_exact.py) and the radius of the uniform evaluation stage (tests/test_uniform_eval_exact.py) are then
run as they stand -- the same cases, seeds, regimes and assertions, on the table the kernel now makes.  (Those checks take
D as the exact maximum; the kernel's D' >= D only widens every radius and slack, each a chain of sums and products with
non-negative factors, monotone in D.)

(b) The bound.  D' = (high word of D + 1, low word 0), capped at +inf's pattern.  D' >= D for every D >= 0 and +inf; for
every NORMAL D below the last 2^-20 of the last binade D' <= D (1 + 2^-20), exactly.  Two ends where the relative bound
cannot hold, and what holds there instead:
  * zero and subnormals have no implicit leading bit: the high word's step is 2^-1042 whatever the value, so
    D' <= D + 2^-1042.  The kernel's D is never there: D >= floor = 2 tiny / cu > tiny (sdp_col_filter_setup).
  * high word 0x7fefffff: D' = +inf.  Such a D is far past the 2^1000 the filter admits (SDP_COL_FILTER_LIMIT): the node
    takes every control the long way with D itself, too."""
import math
import struct
from fractions import Fraction

import numpy as np
import pytest

import test_filter_bound_exact as fb
import test_uniform_bound_exact as ub
import test_uniform_eval_exact as ue

REGIMES = ['ordinary', 'large', 'small', 'mixed', 'cancel', 'weights']


def fused_table(T, p, chunked=True):   # (`chunked`: the signature of reduced_table; the order below whatever it says)
    """A[r] as SDP_COL_REDUCE_FUSED accumulates it (the two reductions of sdp_sweep_col): always the resident-chunk order, the form's only one"""
    W, N0 = T.shape
    C = (W + 1) // 2
    A = np.zeros(N0)
    for r in range(N0):
        tail = 0.0
        for w in range(C, W):
            tail = fb.fma(p[w], T[w][r], tail)
        head = 0.0
        for w in range(C):
            head = fb.fma(p[w], T[w][r], head)
        A[r] = head + tail
    return A


@pytest.fixture
def fused(monkeypatch):
    for mod in (fb, ub, ue):
        monkeypatch.setattr(mod, 'reduced_table', fused_table)


def test_the_fused_sums_are_other_numbers_and_closer_to_the_exact_sum_than_one_rounding_per_point_allows():
    """(the checks below are not the earlier ones run again: the table differs; and what the radius' derivation uses of the
    form -- every partial sum within u of the exact fused step, so A within (W + 1) u sum |p_w T_w| (1 + ..) of the exact sum)"""
    rng = np.random.default_rng(11)
    differs = 0
    for _ in range(50):
        T, p, _ = fb.random_problem(rng, 'ordinary')
        W, N0 = T.shape
        A = fused_table(T, p)
        differs += int((A != fb.reduced_table(T, p, True)).any())
        for r in range(N0):
            exact = sum(Fraction(p[w]) * Fraction(T[w][r]) for w in range(W))
            mass = sum(abs(Fraction(p[w]) * Fraction(T[w][r])) for w in range(W))
            assert abs(Fraction(A[r]) - exact) <= (W + 1) * Fraction(fb.U) * mass * (1 + Fraction(W + 1, 2 ** 52))
    assert differs > 10, differs


@pytest.mark.parametrize('regime', REGIMES)
def test_the_short_pass_radius_covers_the_fused_table(fused, regime):
    # (the resident-chunk order is the fused form's only one: the cases of chunked = True)
    fb.test_the_short_pass_radius_covers_the_difference_exactly(regime, True)


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('axis', sorted(ub.AXES))
def test_the_uniform_block_bound_holds_on_the_fused_table(fused, regime, axis):
    ub.test_the_uniform_bound_lies_below_every_control_of_its_block(regime, axis)


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('axis', sorted(ue.AXES))
def test_the_uniform_evaluation_radius_covers_the_fused_table(fused, regime, axis):
    ue.test_the_radius_covers_the_uniform_evaluation_exactly(regime, axis)


# ---------------------------------------------------------------------------
# (b) D' of SDP_COL_DMAX_HI (sdp_wave_bound_hi)

def bits_of(d):
    return struct.unpack('<Q', struct.pack('<d', d))[0]


def from_words(hi, lo):
    return struct.unpack('<d', struct.pack('<Q', (hi << 32) | lo))[0]


def bound_hi(d):
    """what the kernel forms from one lane's D (the wave's maximum of the high words is one lane's high word)"""
    return from_words(min((bits_of(d) >> 32) + 1, 0x7ff00000), 0)


STEP = Fraction(1, 2 ** 20)
TOP = from_words(0x7fefffff, 0)                            # first value whose bound is +inf


def check(d):
    dp = bound_hi(d)
    assert dp >= d and not math.isnan(dp), (d, dp)
    if math.isinf(d) or d >= TOP:
        assert dp == math.inf, (d, dp)
    elif d >= fb.TINY:
        assert Fraction(dp) <= Fraction(d) * (1 + STEP), (d, dp)
    else:
        assert Fraction(dp) <= Fraction(d) + Fraction(2) ** -1042, (d, dp)


def test_the_bound_on_zero_subnormals_and_every_binade_boundary():
    check(0.0)
    for d in (5e-324, 1e-320, from_words(0, 0xffffffff), from_words(1, 0), from_words(0x000fffff, 0xffffffff)):
        assert d < fb.TINY
        check(d)
    for e in range(-1022, 1024):
        b = math.ldexp(1.0, e)
        for d in (math.nextafter(b, 0.0), b, math.nextafter(b, math.inf)):
            check(d)
        # the last value of a high word and the first of the next, in the middle of the binade
        hi = bits_of(b) >> 32
        check(from_words(hi + 0x7ffff, 0xffffffff))
        check(from_words(hi + 0x80000, 0))


def test_the_bound_at_the_top_of_the_range():
    for lo in (0, 1, 0xffffffff):
        d = from_words(0x7fefffff, lo)
        assert math.isfinite(d) and bound_hi(d) == math.inf
        check(d)
    assert from_words(0x7ff00000, 0) == math.inf and bound_hi(math.inf) == math.inf
    check(math.inf)
    # the last high word whose bound is finite: the largest finite pattern with low word 0
    d = from_words(0x7feffffe, 0xffffffff)
    assert bound_hi(d) == TOP and math.isfinite(TOP)
    check(d)
    # .. and all of this lies past what the filter admits for D
    assert TOP > 2.0 ** 1000


def test_the_bound_on_random_values_and_on_the_floor_of_the_kernel():
    rng = np.random.default_rng(3)
    for hi, lo in zip(rng.integers(0x00100000, 0x7fefffff, size=4000), rng.integers(0, 2 ** 32, size=4000)):
        check(from_words(int(hi), int(lo)))
    # the smallest D a kernel forms: floor = 2 tiny / cu, a normal number
    for W in (1, 8, 32, 1024):
        fc = fb.filter_constants(np.full(W, 1.0 / W))
        assert fc['floor'] > fb.TINY
        check(fc['floor'])


def test_the_unsigned_order_of_the_high_words_is_the_numeric_order():
    """what lets the wave's maximum be taken on the high words alone, as unsigned integers"""
    rng = np.random.default_rng(4)
    vals = [0.0, 5e-324, fb.TINY, 1.0, math.inf] + [from_words(int(h), int(l)) for h, l in
                                                     zip(rng.integers(0, 0x7ff00000, size=2000), rng.integers(0, 2 ** 32, size=2000))]
    vals.sort()
    his = [bits_of(v) >> 32 for v in vals]
    assert his == sorted(his)
    assert bound_hi(max(vals[:-1])) == from_words(min(max(his[:-1]) + 1, 0x7ff00000), 0)
