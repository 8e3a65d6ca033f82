"""Test infrastructure of the Monte Carlo evaluation under lookahead controls (DPSolver.monte_carlo_lookahead,
stodynprog_amd/lookahead.py:monte_carlo_lookahead, kernel sdp_montecarlo_lookahead): the yardstick and its reductions.

The yardstick is never the code under test: it is `lookahead_cases.oracle_closed_loop` -- the pinned oracle chained
step by step -- fed with `solver.monte_carlo_draws`, and the reductions formed here in numpy exactly as the definition
states them: over the steps k >= n_burn, acc = acc + g_k in the problem's reals (k ascending), n_outside the x_k
outside the grid or NaN, occupancy the `montecarlo.nearest_nodes(x_k)`; x_final = x_T.  A closed loop is computed
once for the largest batch of a case: trajectory b is a function of (seed, traj_offset + b, x0[b]) alone, so every
smaller batch and every n_burn is a slice or another reduction of the same arrays.
"""
import numpy as np

import lookahead_cases as lc
from stodynprog_amd import montecarlo as mc

SEED = 0x9E3779B97F4A7C15            # a 64-bit seed
OFFSET = (1 << 32) + 12345           # a trajectory id above 2^32
N_BURNS = (0, 2)

STOCHASTIC = [c for c in lc.CASES if c.name != 'deterministic']
NAN_CASES = [lc.Case('nan box', lc.nan_box), lc.Case('nan box f32', lambda: lc.nan_box(np.float32))]
BOXED = [c for c in STOCHASTIC if c.box == 'device']


def past_a_workgroup(case):
    """one batch just past the trajectories of a workgroup of 256: 4 waves of 64 / lanes trajectories"""
    return {lc.B_64: 5, lc.B_8: 33, lc.B_1: 257}[case.batches]


def horizon(case):
    """(t0, T) of a case: the first time index it is checked at"""
    return (0 if case.times[0] is None else case.times[0]), lc.T_SIM


def bits(a):
    a = np.ascontiguousarray(a)
    if a.dtype.kind == 'f':
        return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)
    return a


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def oracle_inputs(solver, seed, B, T, law=None, traj_offset=0):
    """what `oracle_closed_loop` takes as w for the draws of (seed, ids, steps 0..T-1): the values of one variable, or
    the indices into the flat law of several (the default law only)"""
    idx, w = solver.monte_carlo_draws(seed, B, T, law=law, traj_offset=traj_offset)
    if len(solver.perturb_grid) >= 2:
        assert law is None
        return idx.astype(float)
    return w


def closed_loop(case, solver, J_next, x0, T, seed=SEED, traj_offset=OFFSET, law=None, t0=0, nan_rows=()):
    """(x (T+1, B, d), g (T, B)) in the problem's reals: the oracle chained step by step on the draws.  `nan_rows`:
    trajectories that START at a state without a valid lattice.  The oracle raises there (asserted), as the reference
    does; the definition gives u = NaN, so the row is written down by its rule: the state goes NaN and stays, every
    cost is NaN."""
    spec = lc.spec_of(case, solver)
    x0 = np.atleast_2d(np.asarray(x0, dtype=float))
    B = x0.shape[0]
    w = oracle_inputs(solver, seed, B, T, law, traj_offset)
    keep = np.array([b for b in range(B) if b not in nan_rows], dtype=int)
    xo, _, go, _ = lc.oracle_closed_loop(solver, spec, J_next, x0[keep], w[:, keep], T, t0)
    x = np.full((T + 1, B, x0.shape[1]), np.nan, dtype=solver.dtype)
    g = np.full((T, B), np.nan, dtype=solver.dtype)
    x[:, keep], g[:, keep] = xo, go
    for b in nan_rows:
        try:
            lc.oracle_lookahead(solver, spec, J_next if np.ndim(J_next) == x0.shape[1] else J_next[t0], x0[b:b + 1],
                                None if spec.stationnary else t0)
        except ValueError:
            pass
        else:
            raise AssertionError('the oracle found a lattice at row {}'.format(b))
        x[0, b] = x0[b].astype(solver.dtype)
    return x, g


def reduce(solver, x, g, n_burn, rows=None, occupancy=True):
    """(cost_sum, n_outside, x_final, occupancy) of the trajectories `rows` (default: all) of a closed loop"""
    dt = np.dtype(solver.dtype)
    if rows is not None:
        x, g = x[:, rows], g[:, rows]
    T, B = g.shape
    dims = tuple(len(a) for a in solver.state_grid)
    smin = np.array([a[0] for a in solver.state_grid]).astype(dt)
    smax = np.array([a[-1] for a in solver.state_grid]).astype(dt)
    acc = np.zeros(B, dtype=dt)
    n_out = np.zeros(B, dtype=np.int64)
    occ = np.zeros(dims, dtype=np.int64) if occupancy else None
    with np.errstate(all='ignore'):
        for k in range(n_burn, T):
            acc = acc + g[k]
            n_out += ~np.all((x[k] >= smin) & (x[k] <= smax), axis=1)
            if occupancy:
                np.add.at(occ, tuple(mc.nearest_nodes(x[k], solver.state_grid, dt).T), 1)
    return acc, n_out, np.ascontiguousarray(x[T]), occ


def check(res, want, what, occupancy=True):
    """a MonteCarloResult against the yardstick's (cost_sum, n_outside, x_final, occupancy), on bits"""
    acc, n_out, x_final, occ = want
    assert same(res.cost_sum, acc), (what, 'cost_sum', np.flatnonzero(bits(res.cost_sum) != bits(acc))[:8])
    assert same(res.n_outside, n_out), (what, 'n_outside')
    assert same(res.x_final, x_final), (what, 'x_final')
    if occupancy:
        assert same(res.occupancy, occ), (what, 'occupancy')
        assert int(res.occupancy.sum()) == len(acc) * (res.n_steps - res.n_burn), (what, 'occupancy total')
    else:
        assert res.occupancy is None, what


def unit_sources():
    """the lookahead units of the test cases outside `lookahead_cases.unit_sources` (the build compiles them ahead):
    the 4-byte twin of the NaN-box model"""
    return [lc.unit_source(lc.nan_box(np.float32))]
