"""The convergence rule of the sweep loops with `tol` (stodynprog_amd/convergence.py), on the CPU: the statistics
every layer must reproduce bit for bit, the stopping rule, the check schedule, argument validation before any
device call, and the exported C entry points."""
import ctypes as C
import math

import numpy as np
import pytest

from stodynprog_amd import convergence as conv, DPSolver, _native as nat
from stodynprog_amd import models

INF, NAN = np.inf, np.nan


def test_equal_infinities_give_zero():
    a = np.array([INF, -INF, 1.0, 2.0])
    b = np.array([INF, -INF, 1.0, 1.5])
    assert conv.diff_stats(a, b) == (0.0, 0.5)
    # unequal infinities are differences like any other
    assert conv.diff_stats(np.array([INF, 0.0]), np.array([-INF, 0.0])) == (0.0, INF)
    assert conv.diff_stats(np.array([-INF, 1.0]), np.array([3.0, 1.0])) == (-INF, 0.0)


@pytest.mark.parametrize('where', [0, 3, 6])
def test_nan_propagates_to_both(where):
    a = np.linspace(0, 1, 7)
    b = a * 0.5
    for x, y in ((a.copy(), b), (a, b.copy())):
        (x if x is not a else y)[where] = NAN
        dmin, dmax = conv.diff_stats(x, y)
        assert math.isnan(dmin) and math.isnan(dmax)
    # a NaN span never converges, whatever the tolerance
    assert not conv.converged(NAN, NAN, 1e300) and not conv.converged(0.0, NAN, INF)


def test_difference_is_rounded_in_the_problem_type():
    a = np.array([1.0 + 2.0 ** -20, 3.0], dtype=np.float32)
    b = np.array([1.0, 3.0 - 2.0 ** -22], dtype=np.float32)
    dmin, dmax = conv.diff_stats(a, b)
    d = a - b                                                    # float32 arithmetic
    assert dmin == float(d.min()) and dmax == float(d.max())
    # a 4-byte difference that a float64 subtraction would keep exactly rounds here
    x, y = np.float32(16777216.0), np.float32(0.75)
    assert conv.diff_stats(np.array([x]), np.array([y]))[0] == float(np.float32(x - y)) != 16777216.0 - 0.75
    # the caller's starting array (float64) is taken in the problem type, as the device takes it
    assert conv.diff_stats(np.array([x]), np.array([0.75]), np.float32) == conv.diff_stats(
        np.array([x]), np.array([y]))


def test_no_signed_zero():
    a = np.array([0.0, -0.0, 5.0])
    b = np.array([-0.0, 0.0, 5.0])
    dmin, dmax = conv.diff_stats(a, b)
    assert dmin == 0.0 and dmax == 0.0
    assert math.copysign(1.0, dmin) == 1.0 and math.copysign(1.0, dmax) == 1.0
    for dt in (np.float32, np.float64):
        r = np.random.default_rng(1).standard_normal(100).astype(dt)
        dmin, dmax = conv.diff_stats(r, r.copy())
        assert math.copysign(1.0, dmin) == 1.0 and math.copysign(1.0, dmax) == 1.0


def test_min_and_max_do_not_depend_on_the_order():
    rng = np.random.default_rng(7)
    a, b = rng.standard_normal(1000), rng.standard_normal(1000)
    p = rng.permutation(1000)
    assert conv.diff_stats(a, b) == conv.diff_stats(a[p], b[p]) == conv.diff_stats(a.reshape(10, 100),
                                                                                   b.reshape(10, 100))


def test_span_rule():
    assert conv.converged(-1.0, 1.0, 2.0) and not conv.converged(-1.0, 1.0, np.nextafter(2.0, 0.0))
    assert conv.converged(3.0, 3.0, 0.0)
    assert not conv.converged(-INF, 1.0, 1e308)
    # the span without rel_dp: J grows by the average cost every sweep, the span goes to zero all the same
    J1 = np.array([1.0, 2.0, 4.0])
    assert conv.converged(*conv.diff_stats(J1 + 7.5, J1), 0.0)


@pytest.mark.parametrize('n_iter,check_every,expected', [
    (10, 3, [3, 6, 9, 10]), (10, 1, list(range(1, 11))), (10, 10, [10]), (10, 20, [10]), (1, 1, [1]),
    (1, 5, [1]), (12, 4, [4, 8, 12]), (7, 2, [2, 4, 6, 7])])
def test_check_schedule(n_iter, check_every, expected):
    assert conv.check_schedule(n_iter, check_every) == expected
    assert [k for k in range(1, n_iter + 1) if conv.is_check(k, n_iter, check_every)] == expected
    # the library's stats buffer holds ceil(n_iter / check_every) checks: exactly enough
    assert len(expected) == -(-n_iter // check_every)


def test_record_bounds():
    r = conv.SweepConvergence(0.1, 2, 4, [2, 4], [-1.0, 0.5], [1.0, 0.55], refs=[10.0, 20.0])
    assert r.converged and r.n_iter == 4 and r.checked == [2, 4]
    assert np.array_equal(r.span, [2.0, 0.55 - 0.5])
    assert np.array_equal(r.lower, [9.0, 20.5]) and np.array_equal(r.upper, [11.0, 20.55])
    r = conv.SweepConvergence(0.1, 1, 3, [1, 2, 3], [0.0] * 3, [1.0] * 3)
    assert not r.converged and np.array_equal(r.lower, r.dmin) and np.array_equal(r.upper, r.dmax)
    r = conv.SweepConvergence(0.0, 1, 2, [1, 2], [NAN, NAN], [NAN, NAN])
    assert not r.converged


@pytest.mark.parametrize('tol,check_every', [(-1e-9, 1), (NAN, 1), (-INF, 1), (1e-3, 0), (1e-3, -2), (1e-3, 1.5),
                                             ('abc', 1), (1e-3, True)])
def test_bad_arguments_raise_before_any_device_call(monkeypatch, tol, check_every):
    _, solver = models.inventory()

    def no_device(*a, **k):
        raise AssertionError('the device was touched before the arguments were checked')

    monkeypatch.setattr(nat, 'lib', no_device)
    monkeypatch.setattr(solver, '_trace_now', no_device)
    monkeypatch.setattr(solver, '_problem', no_device)
    shape = solver._state_grid_shape
    pol = np.zeros(shape + (len(solver.sys.control),))
    with pytest.raises(ValueError):
        solver.value_iterations(np.zeros(shape), 5, tol=tol, check_every=check_every, report_time=False)
    with pytest.raises(ValueError):
        solver.eval_policy(pol, 5, tol=tol, check_every=check_every, report_time=False)
    with pytest.raises(ValueError):
        solver.policy_iteration(pol, 5, 2, tol=tol, check_every=check_every)


def test_validate_accepts_good_arguments():
    assert conv.validate(0, 1) == (0.0, 1)
    assert conv.validate(np.float32(1e-3), np.int64(10)) == (float(np.float32(1e-3)), 10)
    assert conv.validate(INF, 3) == (INF, 3)


def test_new_abi_symbols_are_exported():
    lib = nat.lib()
    for name in ('sdp_problem_vi_until', 'sdp_problem_eval_policy_until'):
        assert hasattr(lib, name) and name in nat.EXPORTS
    stats = np.zeros(4)
    n = C.c_int32(0)
    # argument errors through the status-code convention, no GPU needed
    assert lib.sdp_problem_vi_until(None, 3, 0, 0, 1, 0.0, C.byref(n), nat.ptr(stats), None) == -1
    assert lib.sdp_problem_eval_policy_until(None, 3, 0, 0, 1, 0.0, C.byref(n), nat.ptr(stats), None) == -1
    assert b'NULL' in lib.sdp_last_error()


def test_a_call_without_tol_leaves_no_record(monkeypatch):
    _, solver = models.inventory()
    assert solver.last_convergence is None
    solver.last_convergence = 'stale'

    def stop(*a, **k):
        raise RuntimeError('stop here')

    monkeypatch.setattr(solver, '_trace_now', stop)
    with pytest.raises(RuntimeError):
        solver.value_iterations(np.zeros(solver._state_grid_shape), 2, report_time=False)
    assert solver.last_convergence is None
