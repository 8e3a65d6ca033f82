"""Closed loops of families over a horizon on the device (tests/family_horizon_cases.py): member p of everything
`SolverFamily.simulate` and `SolverFamily.monte_carlo_horizon` return equals, bit for bit, what `solvers[p].simulate` and
`solvers[p].monte_carlo` return on their device path (kernels sdp_simulate_h and sdp_montecarlo_h of the member's own unit)
-- every member, trajectory and step -- for every model kind and policy shape, for every way the kernels map members to
XCDs, past the bound of either grid, however the run is cut into member chunks, policy uploads and launches, with one
seed or one per member, with the members' own laws or the caller's, and with grid ends that differ from member to
member.  The `data[k]` families are also compared with the pinned oracle chained step by step (tests/horizon_sim.py)."""
import contextlib
import functools
import io

import numpy as np
import pytest

import family_cases as fc
import family_horizon_cases as fh
import family_mc_cases as mcc
import horizon_sim as hs
from stodynprog_amd import SolverFamily, _native as nat

pytestmark = pytest.mark.gpu

FIELDS = ('cost_sum', 'n_outside', 'x_final', 'occupancy')


def _quiet(f, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all='ignore'):
        return f(*a, **kw)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == 'f' else a


def _equal(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    assert np.array_equal(_bits(a), _bits(b)), (what, int((_bits(a) != _bits(b)).sum()))


def _family(hz):
    return SolverFamily(hz.solvers())


def _close(solvers):
    for s in solvers:
        for k in [k for k in s._cache if k[0] == 'problem']:
            s._cache.pop(k).close()


@functools.lru_cache(maxsize=None)
def _policy(name):
    pol = fh.policies({h.name: h for h in fh.FAMILIES}[name])
    pol.setflags(write=False)
    return pol


def _simulate_against_solo(fam, solvers, hz, pol, x0, w, what):
    """every member of fam.simulate against the solo call; the family's result"""
    got = fam.simulate(pol, x0, w, n_steps=hz.n_steps, t0=hz.t0)
    for p, s in enumerate(solvers):
        ref = _quiet(s.simulate, pol[p] if np.ndim(pol) > len(fam.dims) + 1 else pol, x0[p] if np.ndim(x0) == 3 else x0,
                     None if w is None else (w[p] if np.ndim(w) == 3 else w), n_steps=hz.n_steps, t0=hz.t0)
        assert s.backend_info['horizon_path'] == 'device', (what, p, s.backend_info)
        for name, a, b in zip('xug', got, ref):
            _equal(a[p], b, '{} member {} {}'.format(what, p, name))
    return got


def _same_mc(one, ref, what):
    assert one.path == ref.path == 'device', what
    for name in FIELDS:
        a, b = getattr(one, name), getattr(ref, name)
        if b is None:
            assert a is None, (what, name)
            continue
        _equal(a, b, (what, name))
    assert (one.n_steps, one.n_burn, one.seed, one.traj_offset, one.n_traj) == \
        (ref.n_steps, ref.n_burn, ref.seed, ref.traj_offset, ref.n_traj), what


def _mc_against_solo(res, solvers, hz, pol, x0, seeds, what, laws=None, **kw):
    assert len(res) == len(solvers) and res.path == 'device'
    for p, s in enumerate(solvers):
        ref = _quiet(s.monte_carlo, pol[p] if np.ndim(pol) > len(s._shape()) + 1 else pol, x0[p] if np.ndim(x0) == 3 else x0,
                     hz.n_steps, seed=seeds[p] if np.ndim(seeds) else seeds, law=None if laws is None else laws[p],
                     t0=hz.t0, **kw)
        assert s.backend_info['horizon_path'] == 'device', (what, p, s.backend_info)
        _same_mc(res[p], ref, '{} member {}'.format(what, p))


@pytest.mark.parametrize('hz', fh.PARITY, ids=repr)
def test_parity_with_the_solo_call(gpu, hz):
    fam, pol, solvers = _family(hz), _policy(hz.name), fh.solo(hz.solvers())
    try:
        for B in fh.BATCHES:
            x0, w = fh.starts(hz, B), fh.noise(hz, B)
            x, u, g = _simulate_against_solo(fam, solvers, hz, pol, x0, w, '{} B={}'.format(hz, B))
            assert x.shape == (fam.P, hz.n_steps + 1, B, len(fam.dims)) and u.shape == (fam.P, hz.n_steps, B, fam.nu)
            assert g.shape == (fam.P, hz.n_steps, B) and x.dtype == u.dtype == g.dtype == fam.dtype
            info = fam.backend_info['horizon']
            assert info == dict(members=fam.P, n_traj=B, n_steps=hz.n_steps, timed=True, time_specialized=hz.int_time,
                                chunks=1, step_chunks=1, launches=1), info
            assert fam.last_kernel_ms() > 0
            if fam.W:
                kw = dict(n_burn=2, occupancy=True, traj_offset=1000)
                res = fam.monte_carlo_horizon(pol, x0, hz.n_steps, seed=3, t0=hz.t0, **kw)
                assert res.occupancy.shape == (fam.P,) + fam.dims
                assert np.all(res.occupancy.reshape(fam.P, -1).sum(axis=1) == B * (hz.n_steps - 2))
                _mc_against_solo(res, solvers, hz, pol, x0, 3, '{} B={}'.format(hz, B), **kw)
        # a single start state drops the B axis, shared starts and sequences are every member's
        x0, w = fh.starts(hz, 1), fh.noise(hz, 1)
        one = fam.simulate(pol, x0[0, 0], None if w is None else w[0, :, 0], n_steps=hz.n_steps, t0=hz.t0)
        many = fam.simulate(pol, np.broadcast_to(x0[:1], x0.shape), None if w is None else np.broadcast_to(w[:1], w.shape),
                            n_steps=hz.n_steps, t0=hz.t0)
        for a, b in zip(one, many):
            _equal(a, b[:, :, 0], 'single start')
    finally:
        fam.close()
        _close(solvers)


def test_the_policies_of_the_backward_pass_run_forward(gpu):
    """pv_sized end to end: fam.bellman_recursion, then fam.simulate with what it returned, against the solo calls"""
    hz = fh.PV_SIZED
    fam, solvers = _family(hz), fh.solo(hz.solvers())
    try:
        J, pol = fam.bellman_recursion(hz.n_steps, np.zeros(fam.dims))
        assert pol.shape == (fam.P, hz.n_steps) + fam.dims + (fam.nu,)
        assert any(not np.array_equal(pol[0, k], pol[0, k + 1]) for k in range(hz.n_steps - 1))
        x0 = np.array([[0.], [0.4], [0.9]])                              # (B, d) shared: inside every member's grid
        _simulate_against_solo(fam, solvers, hz, pol, x0, None, 'bellman_recursion')
    finally:
        fam.close()
        _close(solvers)


@pytest.mark.parametrize('hz', (fh.PV_SIZED, fh.LOOKUP), ids=repr)
def test_against_the_chained_oracle(gpu, hz):
    fam, pol = _family(hz), _policy(hz.name)
    B = 65
    x0, w = fh.starts(hz, B), fh.noise(hz, B)
    try:
        got = fam.simulate(pol, x0, w, n_steps=hz.n_steps, t0=hz.t0)
        for p, s in enumerate(hz.solvers()):
            ref = hs.simulate_indexed(hs.spec_of(s, True), pol[p], x0[p], None if w is None else w[p], hz.n_steps, hz.t0, s.dtype)
            for name, a, b in zip('xug', got, ref):
                _equal(a[p], np.asarray(b, dtype=s.dtype), '{} member {} {}'.format(hz, p, name))
        if fam.W:
            # Monte Carlo: the family's draws in numpy fed to that chain, summed on the host
            n_burn = 2
            res = fam.monte_carlo_horizon(pol, x0, hz.n_steps, seed=(11, 12), n_burn=n_burn, t0=hz.t0)
            _, draws = fam.monte_carlo_draws((11, 12), B, hz.n_steps)
            for p, s in enumerate(hz.solvers()):
                x, _, g = hs.simulate_indexed(hs.spec_of(s, True), pol[p], x0[p], draws[p], hz.n_steps, hz.t0, s.dtype)
                acc = np.zeros(B, dtype=s.dtype)
                for k in range(n_burn, hz.n_steps):
                    acc = acc + np.asarray(g[k], dtype=s.dtype)
                _equal(res.cost_sum[p], acc, 'cost_sum member {}'.format(p))
                _equal(res.x_final[p], np.asarray(x[-1], dtype=s.dtype), 'x_final member {}'.format(p))
                smin, smax = s.state_grid[0][0], s.state_grid[0][-1]
                xs = np.asarray(x[n_burn:hz.n_steps], dtype=float)
                outside = ~np.all((xs >= smin) & (xs <= smax), axis=2)
                assert np.array_equal(res.n_outside[p], outside.sum(axis=0))
    finally:
        fam.close()


def test_lookup_under_a_stationary_policy(gpu):
    """a data[k] model under one stationary policy per member, and under one for all: policy stride 0, table stride n"""
    hz = fh.LOOKUP
    fam, solvers = _family(hz), fh.solo(hz.solvers())
    B = 65
    x0, w = fh.starts(hz, B), fh.noise(hz, B)
    try:
        for pol in (_policy(hz.name)[:, 3], _policy(hz.name)[1, 5]):
            _simulate_against_solo(fam, solvers, hz, pol, x0, w, 'stationary policy')
            info = fam.backend_info['horizon']
            assert not info['timed'] and info['time_specialized'] and info['step_chunks'] == 1
            res = fam.monte_carlo_horizon(pol, x0, hz.n_steps, seed=5, occupancy=True)
            _mc_against_solo(res, solvers, hz, pol, x0, 5, 'stationary policy', occupancy=True)
    finally:
        fam.close()
        _close(solvers)


@functools.lru_cache(maxsize=None)
def _line_policies(n_steps):
    """member p of a line family is the same problem whatever P: the policies of the largest family serve them all"""
    return _policy(fh.MAPPING[max(fh.MAPPING_P)].name)[:, :n_steps]


@functools.lru_cache(maxsize=None)
def _line_w(B, n_steps):
    return np.random.default_rng(B + n_steps).normal(0., 0.1, (n_steps, B))


@functools.lru_cache(maxsize=None)
def _line_solo(p, B, n_steps):
    """line member p alone: its solo results"""
    pol = _line_policies(n_steps)[p]
    s = fh.solo([fc.line_members(p + 1, fc.LINE_NX)[p]()])[0]
    sim = _quiet(s.simulate, pol, fh.line_starts(B), _line_w(B, n_steps))
    assert s.backend_info['horizon_path'] == 'device'
    res = _quiet(s.monte_carlo, pol, fh.line_starts(B), n_steps, seed=5, occupancy=True)
    assert s.backend_info['horizon_path'] == 'device'
    _close([s])
    return sim, res


def _line_family(P, B, n_steps):
    fam = SolverFamily(fh.MAPPING[P].solvers())
    pol = np.ascontiguousarray(_line_policies(n_steps)[:P])
    try:
        got = fam.simulate(pol, fh.line_starts(B), _line_w(B, n_steps))
        res = fam.monte_carlo_horizon(pol, fh.line_starts(B), n_steps, seed=5, occupancy=True)
        for p in range(P):
            sim, ref = _line_solo(p, B, n_steps)
            for name, a, b in zip('xug', got, sim):
                _equal(a[p], b, 'line P={} member {} {}'.format(P, p, name))
            _same_mc(res[p], ref, 'line P={} member {}'.format(P, p))
    finally:
        fam.close()


@pytest.mark.parametrize('P', fh.MAPPING_P)
def test_every_mapping_of_members_to_xcds(gpu, P):
    assert -(-fh.B_MAPPING // fh.SIM_TILE) == 5 and -(-fh.B_MAPPING // fh.MC_TILE) == 2       # the last tiles are ragged
    _line_family(P, fh.B_MAPPING, fh.T)


def test_past_both_launch_caps(gpu):
    cus = nat.device_info(0)['compute_units']
    B = max(fh.sim_cap_batch(cus), mcc.cap_batch(cus))
    plan = fh.launch(B, 9, cus * 32 // 8, fh.SIM_TILE)
    assert max(trip for _, _, trip in plan['visits'][0]) >= 1            # XCD 0 walks again
    for per_cu in range(1, 9):
        plan = fh.launch(B, 9, cus * per_cu // 8, fh.MC_TILE)
        assert max(trip for xcd in plan['visits'] for _, _, trip in xcd) >= 1
    _line_family(9, B, fh.STEPS_CAP)


def test_cuts_change_no_bit(gpu):
    hz = fh.CUTS                                                         # storage_ar1, five members, T = 8
    fam, pol = _family(hz), _policy(hz.name)
    B = 70
    x0, w = fh.starts(hz, B), fh.noise(hz, B)
    kw = dict(seed=9, n_burn=2, occupancy=True, traj_offset=12)
    try:
        whole = fam.simulate(pol, x0, w)
        whole_mc = fam.monte_carlo_horizon(pol, x0, hz.n_steps, **kw)
        assert fam.backend_info['horizon'] == dict(members=5, n_traj=B, n_steps=8, timed=True, time_specialized=False,
                                                   chunks=1, step_chunks=1, launches=1)
        solvers = fh.solo(hz.solvers())
        _mc_against_solo(whole_mc, solvers, hz, pol, x0, 9, 'cuts', n_burn=2, occupancy=True, traj_offset=12)
        _close(solvers)
        # two member chunks, one-step policy uploads, launches of at most three steps
        S, rs = int(np.prod(fam.dims)), fam.dtype.itemsize
        fam.horizon_chunk_bytes = 1
        fam.steps_per_launch = 3
        pol_d, _ = fam._horizon_policy(pol, hz.n_steps, 0)
        table = fam._horizon_tables(hz.n_steps, 0)[1]
        extra_sim = fam._horizon_bytes(pol_d, table) + (2 * B + 8 * B + 9 * 2 * B + 8 * 2 * B + 8 * B) * rs
        fam.chunk_bytes = fh.member_chunk_bytes(fam, extra_sim, 3)
        cut = fam.simulate(pol, x0, w)
        assert fam.backend_info['horizon'] == dict(members=5, n_traj=B, n_steps=8, timed=True, time_specialized=False,
                                                   chunks=2, step_chunks=16, launches=16)
        for name, a, b in zip('xug', cut, whole):
            _equal(a, b, 'cut ' + name)
        extra_mc = fam._mc_member_bytes(B, 3, True) + fam._horizon_bytes(pol_d, table) - fam.nu * S * rs
        fam.chunk_bytes = fh.member_chunk_bytes(fam, extra_mc, 3)
        cut_mc = fam.monte_carlo_horizon(pol, x0, hz.n_steps, **kw)
        assert fam.backend_info['horizon']['chunks'] == 2 and fam.backend_info['horizon']['launches'] == 16
        for name in FIELDS:
            _equal(getattr(cut_mc, name), getattr(whole_mc, name), 'cut ' + name)
        # whole uploads, launches of three steps: 3 + 3 + 2
        del fam.horizon_chunk_bytes, fam.chunk_bytes
        again = fam.monte_carlo_horizon(pol, x0, hz.n_steps, **kw)
        assert fam.backend_info['horizon']['chunks'] == 1 and fam.backend_info['horizon']['launches'] == 3
        for name in FIELDS:
            _equal(getattr(again, name), getattr(whole_mc, name), 'launches ' + name)
    finally:
        fam.close()


def test_seeds_laws_and_outside_counts(gpu):
    hz = fh.AR1_64
    fam, pol, solvers = _family(hz), _policy(hz.name), fh.solo(hz.solvers())
    x0 = fh.starts(hz, 65)
    kw = dict(n_burn=2, occupancy=True)
    try:
        # one seed, then one per member
        one = fam.monte_carlo_horizon(pol, x0, hz.n_steps, seed=4, **kw)
        assert one.seeds == (4, 4, 4)
        _mc_against_solo(one, solvers, hz, pol, x0, 4, 'one seed', **kw)
        each = fam.monte_carlo_horizon(pol, x0, hz.n_steps, seed=(4, 5, 6), **kw)
        assert each.seeds == (4, 5, 6)
        _equal(each.cost_sum[0], one.cost_sum[0], 'member 0 keeps its seed')
        _mc_against_solo(each, solvers, hz, pol, x0, (4, 5, 6), 'a seed per member', **kw)
        # a law per member, then one law of 70 points (the binary search of the index)
        laws = mcc.member_laws()
        res = fam.monte_carlo_horizon(pol, x0, hz.n_steps, seed=11, law=laws, **kw)
        _mc_against_solo(res, solvers, hz, pol, x0, 11, 'law per member', laws=laws, **kw)
        assert not np.array_equal(res.cost_sum, fam.monte_carlo_horizon(pol, x0, hz.n_steps, seed=11, **kw).cost_sum)
        long_ = mcc.long_law()
        res = fam.monte_carlo_horizon(pol, x0, hz.n_steps, seed=11, law=long_, **kw)
        _mc_against_solo(res, solvers, hz, pol, x0, 11, 'long law', laws=[long_] * 3, **kw)
    finally:
        fam.close()
        _close(solvers)
    # grid ends per member: the outside counts
    hz = fh.OUTSIDE
    fam, pol, solvers = _family(hz), _policy(hz.name), fh.solo(hz.solvers())
    x0 = mcc.outside_starts()
    try:
        res = fam.monte_carlo_horizon(pol, x0, hz.n_steps, seed=3, n_burn=2)
        assert res.n_outside[0].sum() == 0 and res.n_outside[1].sum() > 0
        _mc_against_solo(res, solvers, hz, pol, x0, 3, 'outside', n_burn=2)
    finally:
        fam.close()
        _close(solvers)


def test_a_stationary_policy_on_a_symbolic_model_gives_monte_carlo(gpu):
    hz = fh.AR1_64
    fam = _family(hz)
    pol = _policy(hz.name)[:, 2]
    x0 = fh.starts(hz, 65)
    kw = dict(seed=7, n_burn=3, occupancy=True, traj_offset=5)
    try:
        ref = fam.monte_carlo(pol, x0, 24, **kw)
        res = fam.monte_carlo_horizon(pol, x0, 24, **kw)
        info = fam.backend_info['horizon']
        assert not info['timed'] and not info['time_specialized'] and info['step_chunks'] == 1 and info['launches'] == 1
        for name in FIELDS:
            _equal(getattr(res, name), getattr(ref, name), name)
        # .. and the same slice at every step of a time-indexed policy
        tiled = np.ascontiguousarray(np.broadcast_to(pol[:, None], (fam.P, 24) + pol.shape[1:]))
        res = fam.monte_carlo_horizon(tiled, x0, 24, **kw)
        for name in FIELDS:
            _equal(getattr(res, name), getattr(ref, name), 'tiled ' + name)
    finally:
        fam.close()


def test_the_other_methods_return_what_they_returned_before(gpu):
    hz = fh.AR1_64
    fam, pol = _family(hz), _policy(hz.name)
    J0 = fc.start(hz.case)
    x0, w = fh.starts(hz, 65), fh.noise(hz, 65)
    try:
        before = fam.value_iterations(J0, 3), fam.monte_carlo(pol[:, 0], x0, 12, seed=2, occupancy=True)
        handle = fam._handle[1]
        first = fam.simulate(pol, x0, w), fam.monte_carlo_horizon(pol, x0, hz.n_steps, seed=2, occupancy=True)
        assert fam._handle[1] is handle                                 # the handle is reused
        after = fam.value_iterations(J0, 3), fam.monte_carlo(pol[:, 0], x0, 12, seed=2, occupancy=True)
        again = fam.simulate(pol, x0, w), fam.monte_carlo_horizon(pol, x0, hz.n_steps, seed=2, occupancy=True)
        for a, b in zip(before[0], after[0]):
            _equal(a, b, 'value_iterations')
        for name in FIELDS:
            _equal(getattr(before[1], name), getattr(after[1], name), 'monte_carlo ' + name)
            _equal(getattr(first[1], name), getattr(again[1], name), 'monte_carlo_horizon ' + name)
        for a, b in zip(first[0], again[0]):
            _equal(a, b, 'simulate')
    finally:
        fam.close()
