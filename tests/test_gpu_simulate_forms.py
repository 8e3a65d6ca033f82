"""DPSolver.simulate (kernel sdp_simulate, compiled into every unit) in a unit of every family and column form, in
both reals where the family plans them, against the numpy closed loop (oracle/vi_numpy.simulate): states, controls
and costs bit for bit, NaN where the oracle has NaN.

Every batch gives each trajectory its own start state and its own perturbation column; some start off the grid and
some perturbations push the state out of it.  The policies are those of tests/policies.py (on the lattice, smooth,
beyond the box, with NaN and infinities)."""
import contextlib
import io

import numpy as np
import pytest

import column_forms as cf
import policies as P
from oracle import vi_numpy
from stodynprog_amd import SysDescription, DPSolver, models, _native as nat
from test_gpu_call_to_call import storage, VALUES

pytestmark = pytest.mark.gpu


def _quiet(f, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all='ignore'):
        return f(*a, **kw)


def _case(name, geometry='split'):
    return lambda: [c for c in cf.CASES if c.name == name][0].solver(geometry)


def _family(name):
    return lambda: [f for f in P.FAMILIES if f.name == name][0].solver()


# unit: (solver maker, what backend_info must say after a run)
UNITS = {
    'full table': (_case('full_n500'), dict(kernel='column')),
    'full table fp32': (_case('f32_n512_u129'), dict(kernel='column')),
    'resident chunks': (_case('res1024_u301'), dict(kernel='column')),
    'held tail': (_case('hold_8x2x4'), dict(kernel='column')),
    'row window': (_family('row window'), dict(kernel='column', table_per_control=False)),
    'table per control': (_family('table per control'), dict(kernel='column', table_per_control=True)),
    'table per control fp32': (_family('table per control fp32'), dict(kernel='column', table_per_control=True)),
    'shifted lattice': (_family('shifted lattice'), dict(kernel='column', filter_form='shifted lattice')),
    'shifted lattice fp32': (_family('shifted lattice fp32'), dict(kernel='column')),
    'column': (_family('column'), dict(kernel='column', filter_form='reduced table')),
    'column fp32': (_family('column fp32'), dict(kernel='column')),
    'line': (_family('line'), dict(kernel='line')),
    'lead': (_family('lead'), dict(kernel='lead')),
    'staged': (_family('staged'), dict(kernel='staged')),
    'staged fp32': (_family('staged fp32'), dict(kernel='staged')),
    'generic': (_family('generic'), dict(kernel='generic')),
    'generic fp32': (_family('generic fp32'), dict(kernel='generic')),
}


def _starts(s, B, rng):
    """B start states, about a quarter of them off the grid"""
    lo = np.array([g[0] for g in s.state_grid])
    hi = np.array([g[-1] for g in s.state_grid])
    return lo + (hi - lo) * rng.uniform(-0.25, 1.25, (B, len(lo)))


def _noise(s, T, B, rng):
    """(T, B) perturbations, one column per trajectory; every 7th trajectory gets five times the spread"""
    w = s.perturb_grid[0]
    sd = (w[-1] - w[0]) / 6.0
    out = rng.normal(0.0, sd, (T, B))
    out[:, ::7] *= 5.0
    return out


def _same(got, ref, what):
    for a, b, name in zip(got, ref, ('x', 'u', 'g')):
        assert a.shape == b.shape and a.dtype == b.dtype, (what, name, a.shape, b.shape, a.dtype, b.dtype)
        bad = ~((a == b) | (np.isnan(a) & np.isnan(b)))
        if bad.any():
            k, b_ = np.argwhere(bad.reshape(bad.shape[0], bad.shape[1], -1).any(-1))[0]
            raise AssertionError('{}: {} differs at {} entries, first at step {} trajectory {}: {!r} vs {!r}'.format(
                what, name, int(bad.sum()), k, b_, a[k, b_], b[k, b_]))


def _close(s):
    for k in [k for k in s._cache if k[0] == 'problem']:
        s._cache.pop(k).close()


@pytest.mark.timeout(600)
@pytest.mark.parametrize('unit', sorted(UNITS))
def test_simulate_in_every_unit(gpu, unit):
    make, info = UNITS[unit]
    s = make()
    try:
        spec = vi_numpy.Spec.from_solver(s)
        rng = np.random.default_rng(len(unit))
        T = 24
        for kind in ('lattice', 'smooth', 'outside', 'special'):
            pol = P.policy(s, kind, seed=3)
            for B in (1, 63, 64, 65, 1000):
                x0 = _starts(s, B, rng)
                # (n_steps shorter than the perturbation sequences for half of the batches)
                w = _noise(s, T + 5 * (B % 2), B, rng)
                got = _quiet(s.simulate, pol, x0, w, n_steps=T if B % 2 else None)
                with np.errstate(all='ignore'):
                    ref = vi_numpy.simulate(spec, pol, x0, w, T, dtype=s.dtype)
                _same(got, ref, '{} {} B={}'.format(unit, kind, B))
            for k, v in info.items():
                assert s.backend_info[k] == v, (unit, kind, k, s.backend_info)
            assert s.backend_info['mode'] == 'traced', s.backend_info
        if s.dtype == np.float32:
            # no step at all: the start states, in 4-byte reals
            x0 = _starts(s, 5, rng)
            x, u, g = _quiet(s.simulate, pol, x0, _noise(s, 0, 5, rng))
            assert x.shape == (1, 5, x0.shape[1]) and u.shape[0] == 0 and g.shape == (0, 5)
            assert np.array_equal(x[0], x0.astype(np.float32))
    finally:
        _close(s)


def _deterministic(dtype):
    s = SysDescription((2, 1, 0), name='deterministic stock')
    s.dyn = lambda e, p, u: (e + 0.7 * u, 0.9 * p + 0.1 * e)
    s.cost = lambda e, p, u: (p - u) * (p - u) + 0.2 * e
    s.control_box = lambda e, p: ((-1., 1.),)
    solver = DPSolver(s, dtype=dtype)
    solver.discretize_state(0, 4, 17, -2, 2, 9)
    solver.control_steps = (0.25,)
    return solver


@pytest.mark.timeout(300)
@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['fp64', 'fp32'])
def test_simulate_deterministic_and_time_indexed_models(gpu, dtype):
    rng = np.random.default_rng(4)
    s = _deterministic(dtype)
    spec = vi_numpy.Spec.from_solver(s)
    for kind in ('smooth', 'outside', 'special'):
        pol = P.policy(s, kind, seed=1)
        x0 = _starts(s, 65, rng)
        got = _quiet(s.simulate, pol, x0, n_steps=17)
        with np.errstate(all='ignore'):
            _same(got, vi_numpy.simulate(spec, pol, x0, None, 17, dtype=dtype), 'deterministic {}'.format(kind))
    _close(s)
    # a non-stationary model whose dynamics and cost read the time index: t0 + k reaches them
    _, fh = models.finite_horizon()
    fh = P.as_dtype(fh, dtype)
    spec = vi_numpy.Spec.from_solver(fh)
    for t0 in (3, 11):
        pol = P.policy(fh, 'smooth', seed=t0)
        x0 = _starts(fh, 70, rng)
        w = _noise(fh, 15, 70, rng)
        got = _quiet(fh.simulate, pol, x0, w, t0=t0)
        assert fh.backend_info['mode'] == 'traced' and not fh.backend_info['time_specialized'], fh.backend_info
        with np.errstate(all='ignore'):
            _same(got, vi_numpy.simulate(spec, pol, x0, w, 15, t0=t0, dtype=dtype), 'finite horizon t0={}'.format(t0))
    _close(fh)


@pytest.mark.timeout(600)
def test_simulate_past_the_launch_cap(gpu):
    """more trajectories than the launch's blocks x 64 lanes (sdp_problem_simulate caps the grid at cus * 32 blocks):
    the grid-stride loop must reach every one of them"""
    cus = int(nat.device_info(0)['compute_units'])
    B = cus * 32 * 64 + 129
    s = P.FAMILIES[[f.name for f in P.FAMILIES].index('column')].solver()
    rng = np.random.default_rng(9)
    pol = P.policy(s, 'smooth', seed=2)
    x0 = _starts(s, B, rng)
    w = _noise(s, 2, B, rng)
    try:
        got = _quiet(s.simulate, pol, x0, w)
        with np.errstate(all='ignore'):
            ref = vi_numpy.simulate(vi_numpy.Spec.from_solver(s), pol, x0, w, 2)
        _same(got, ref, 'B = {}'.format(B))
    finally:
        _close(s)


@pytest.mark.timeout(300)
def test_simulate_follows_a_lifted_constant(gpu):
    """the parameter study of test_gpu_call_to_call, simulated: from the second value on the constants are kernel
    parameters, and every call must follow the value of the moment"""
    coef = dict(zip(('g', 'rho', 'k', 'cap'), VALUES[0]))
    s = storage(coef)
    s.kernel = 'column'
    rng = np.random.default_rng(12)
    pol = P.policy(s, 'smooth', seed=4)
    x0 = _starts(s, 65, rng)
    w = _noise(s, 20, 65, rng)
    runs, lifted = [], []
    try:
        for values in VALUES:
            coef.update(zip(('g', 'rho', 'k', 'cap'), values))
            got = _quiet(s.simulate, pol, x0, w)
            lifted.append(s.backend_info['lifted_constants'])
            with np.errstate(all='ignore'):
                ref = vi_numpy.simulate(vi_numpy.Spec.from_solver(s), pol, x0, w, 20)
            _same(got, ref, 'values {}'.format(values))
            runs.append(got)
    finally:
        _close(s)
    assert lifted[0] == 0 and all(n > 0 for n in lifted[1:]), lifted
    assert not np.array_equal(runs[1][0], runs[2][0])           # the new exogenous coefficient moved the states
    for a, b in zip(runs[0], runs[-1]):
        assert np.array_equal(a, b)
