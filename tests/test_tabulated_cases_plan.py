"""The table of tabulated mode (tests/tabulated_cases.py) still means what it says, without a GPU: every model is one the
tracer refuses, has the state, control and perturbation counts, the range of lattice sizes and the lane trips it claims;
the tied runs, the NaN and the infinities lie on the lanes and trips they are there for (from the oracle's per-control
vector, `==` not close); the wild next states are restated by the oracle as the kernels' rule has them; and the chunked
sweeps cut their nodes into the batches they are there for (from the flush rule of DPSolver._backup_tabulated,
restated).  When a change of a model empties a case, these tests name it."""
import numpy as np
import pytest

import tabulated_cases as tc
from oracle import vi_numpy
from stodynprog_amd.trace import TraceError

_IDS = [c.name for c in tc.CASES]
# the multiple of 64 a case's tied run reaches across (None: the run lies on one trip of the lanes)
STRADDLES = {'line ragged': 64, 'line ties 0.75': None, 'line ties 0.99': 128, 'line last': None,
             'U = 63': None, 'U = 64': None, 'U = 65': 64}


def _times(case):
    return list(range(case.t_fin)) if case.t_fin else [None]


def _full_vectors(solver, V, t_k=None):
    """[(U, winner, per-control vector)] of the oracle at every node"""
    spec = vi_numpy.Spec.from_solver(solver)
    interp = vi_numpy.Interp(*spec.state_grid)
    interp.set_values(np.asarray(V, dtype=float))
    out = []
    with np.errstate(all='ignore'):
        for x in tc.nodes_of(solver):
            _, _, flat, _, full = vi_numpy.backup_node(spec, x, interp, t_k, full=True)
            out.append((np.size(full), flat, np.ravel(full)))
    return out


@pytest.mark.parametrize('case', tc.CASES, ids=_IDS)
def test_every_case_is_untraceable_and_has_the_lattices_it_claims(case):
    s = case.solver()
    assert isinstance(s._traced(), TraceError), case
    assert (len(s.sys.state), len(s.sys.control), s._law_points()) == (case.d, case.nu, case.W), case
    assert s.sys.stationnary == (case.t_fin == 0)
    if case.W:          # no two weights equal: a sum over the perturbation points in another order gives other bits
        p = s.perturb_proba[0]
        assert len(set(p.tolist())) == case.W == len(s.perturb_grid[0]) and abs(p.sum() - 1.0) < 1e-15
    shape = s._shape()
    assert len(shape) == case.d and int(np.prod(shape)) <= 2000
    U = np.concatenate([tc.lattice_sizes(s, t) for t in _times(case)])
    assert (int(U.min()), int(U.max())) == case.U, (case, U.min(), U.max())
    assert case.trips == tc.trips(U.max()) == -(-case.U[1] // 64)
    assert int(U.sum()) * max(case.W, 1) <= 300_000
    if case.mirrored is not None:
        m = case.mirrored()
        Um = tc.lattice_sizes(m)
        assert isinstance(m._traced(), TraceError) and sorted(Um) == sorted(U) and m._shape() == shape
        # the lattices grow along the sweep and shrink along the mirrored one
        half = len(U) // 2
        assert U[:half].sum() < U[half:].sum() and Um[:half].sum() > Um[half:].sum()


def test_the_table_reaches_what_it_is_for():
    by = tc.BY_NAME
    assert len(by) == len(tc.CASES)
    assert {c.d for c in tc.CASES} == {1, 2, 3, 4} and {c.trips for c in tc.CASES} >= {1, 2, 3, 4}
    assert by['four states'].W == 0 and by['four states'].d == 4 and by['four states'].nu == 2
    assert by['time index'].t_fin >= 2 and by['time index'].d >= 3
    U = tc.lattice_sizes(by['line ragged'].solver())
    assert list(U[:4]) == [1, 5, 9, 14] and list(U[-2:]) == [125, 129]
    assert any(u < 64 for u in U) and any(64 < u < 128 for u in U) and any(u > 128 for u in U)
    assert U[-1] > 100 * U[0]
    assert [by['U = {}'.format(n)].U for n in (63, 64, 65)] == [(63, 63), (64, 64), (65, 65)]
    # two controls: 1 x 1, 1 x n, n x 1 and 9 x 17, a flat index past 128
    dims = {tc.two_controls()().control_grids(x)[1] for x in tc.nodes_of(by['two controls'].solver())}
    assert {(1, 1), (1, 17), (9, 1), (9, 17)} <= dims and len({a for a, _ in dims}) >= 5 and len({b for _, b in dims}) >= 5
    # four states: the optimum lies past the first trip of the lanes at most nodes, and past the second at some
    s = by['four states'].solver()
    _, _, idx = tc.oracle_sweep(s, tc.inputs(s._shape())['smooth'])
    assert (idx >= 64).sum() >= 160 and (idx >= 128).sum() >= 20 and idx.max() > 192
    for name in ('three states', 'time index'):
        s = by[name].solver()
        _, _, idx = tc.oracle_sweep(s, tc.inputs(s._shape())['random'], 1 if by[name].t_fin else None)
        assert (idx >= 64).any() and (idx < 64).any(), name
    assert set(tc.CHUNKS) == {'line ragged', 'two controls', 'four states'} and all(1 in k for k in tc.CHUNKS.values())
    assert all(by[n].mirrored is not None for n in tc.CHUNKS)


@pytest.mark.parametrize('case', [c for c in tc.CASES if c.ties], ids=lambda c: c.name)
def test_the_tied_runs_lie_where_the_table_says(case):
    s = case.solver()
    V = tc.inputs(s._shape())
    first, last, winner = case.ties
    for vname in ('zeros', 'smooth', 'random', 'kinked'):
        vectors = _full_vectors(s, V[vname])
        U, flat, full = max(vectors, key=lambda v: v[0])
        assert U == case.U[1]
        tied = np.flatnonzero(full == full.min())                       # exactly equal, not close
        assert list(tied) == list(range(first, last + 1)) and flat == winner == first, (case, vname, tied, flat)
        m = STRADDLES[case.name]
        across = [k for k in range(64, U, 64) if first < k <= last]
        assert across == ([m] if m else []), (case, across)
        if m:       # the winner sits on a HIGHER lane than its rivals of the next trip
            assert winner % 64 > last % 64 and winner // 64 + 1 == last // 64
    # the last control alone on the third trip; a run wholly on the second
    if case.name == 'line last':
        assert winner == 128 == case.U[1] - 1 and all(f == u - 1 for u, f, _ in _full_vectors(s, V['random']))
    if case.name == 'line ties 0.75':
        assert 64 <= first and last < 128


@pytest.mark.parametrize('name', ['line ragged', 'line ties 0.75', 'U = 63', 'U = 64', 'U = 65', 'two controls', 'four states'])
def test_on_the_flat_input_index_0_wins_against_every_lane_and_trip(name):
    """whatever the control costs is lost in the rounding of 2^60: at every node (but one, at most, of the small ones)
    index 0 wins, tied with others (where
    the next state leaves the grid the weights' rounding tells some apart) -- with ALL of them at the node that has the
    most, and on most nodes with controls of every lane trip"""
    s = tc.BY_NAME[name].solver()
    vectors = _full_vectors(s, tc.inputs(s._shape())['flat'])
    assert sum(f == 0 for _, f, _ in vectors) >= len(vectors) - 1 and all(f == 0 for U, f, _ in vectors if U > 64)
    assert all((full == full[0]).sum() > 1 for U, _, full in vectors if U > 1)
    many = [np.flatnonzero(full == full[0]) for U, _, full in vectors if U > 64]
    assert not many or sum(t.max() >= 64 for t in many) > len(many) // 2
    U, _, full = max(vectors, key=lambda v: v[0])
    assert U == tc.BY_NAME[name].U[1] and (full == full[0]).all()


@pytest.mark.parametrize('case,mark', tc.MARK_RUNS, ids=['{}-{}'.format(c.name, m) for c, m in tc.MARK_RUNS])
def test_the_cost_variants_put_their_values_where_the_table_says(case, mark):
    s = tc.with_cost_marks(case.solver(), mark)
    assert isinstance(s._traced(), TraceError)
    vectors = _full_vectors(s, tc.inputs(s._shape())['random'])
    if mark == 'inf nodes':
        n0 = s._shape()[0]
        rows = np.repeat(np.arange(n0), len(vectors) // n0)
        every = tc.MARKS[mark][1]
        hit = [v for r, v in zip(rows, vectors) if r % every == 0]
        rest = [v for r, v in zip(rows, vectors) if r % every]
        assert hit and all(f == 0 and (full == np.inf).all() for _, f, full in hit)
        assert any(U > 128 for U, _, _ in hit) and any(U == 1 for U, _, _ in hit)
        assert all(np.isfinite(full).all() for _, _, full in rest)
    elif mark == 'nan 37 and 100':
        hit = [v for v in vectors if v[0] > 100]
        assert hit and all(f == 37 and list(np.flatnonzero(np.isnan(full))) == [37, 100] for _, f, full in hit)
        assert all(f == 37 for U, f, _ in vectors if 37 < U <= 100) and all(np.isfinite(full).all() for U, _, full in vectors if U <= 37)
    elif mark == 'nan past 64':
        hit = [v for v in vectors if v[0] > 70]
        assert hit and all(f == 70 and list(np.flatnonzero(np.isnan(full))) == [70] for _, f, full in hit)
        assert any(v[0] <= 70 for v in vectors)
    elif mark == 'finite at 70 alone':
        hit = [v for v in vectors if v[0] > 70]
        assert hit and all(f == 70 and list(np.flatnonzero(np.isfinite(full))) == [70] and (np.delete(full, 70) == np.inf).all()
                           for _, f, full in hit)
        assert all(f == 0 and (full == np.inf).all() for U, f, full in vectors if U <= 70) and len(hit) < len(vectors)
    else:
        hit = [v for v in vectors if v[0] > 69]
        assert hit and all(f == 5 and list(np.flatnonzero(full == -np.inf)) == [5, 69] for _, f, full in hit)


def test_the_wild_next_states_are_what_the_oracle_restates():
    """the rule of sdp_interp_point (pinned on the reference's golden vectors and by
    test_gpu_interp::test_extrapolation_and_cast_edge_cases): cell = clamp(trunc(p), 0, n - 2) with a NaN and a number
    beyond int giving cell 0, lam = p - cell unclamped"""
    s = tc.BY_NAME['wild next state'].solver()
    grid = s.state_grid
    u = s.control_grids((0., 0.))[0][0]
    assert list(u) == list(np.arange(17) * 0.125 - 1.0)                    # the controls are exact: u == 0, -0.5, -0.25
    seen = dict(nan=0, far=0, last=0, huge=0, inf=0)
    for a, b in tc.nodes_of(s):
        x0, x1 = s.sys.dyn(a, b, u.reshape(-1, 1), np.asarray(s.perturb_grid[0]))
        x0, x1 = np.broadcast_to(x0, (17, 3)), np.broadcast_to(x1, (17, 3))
        p0 = (x0 - grid[0][0]) / (grid[0][-1] - grid[0][0]) * (len(grid[0]) - 1)
        seen['nan'] += int(np.isnan(x0).sum())
        seen['far'] += int((np.abs(p0) > 40).sum())
        seen['last'] += int((x1 == grid[1][-1]).sum())
        seen['huge'] += int((x1 == 1e300).sum())
        seen['inf'] += int(np.isinf(x1).sum())
    assert all(seen.values()), seen
    # the oracle's interpolation at such points, against the rule written out for the 6 x 5 grid
    V = tc.inputs(s._shape())['random']
    interp = vi_numpy.Interp(*grid)
    interp.set_values(V)

    def rule(x0, x1):
        cell, lam = [], []
        for x, n in ((x0, 6), (x1, 5)):
            p = (x - 0.0) / (1.0 - 0.0) * (n - 1)
            q = int(p) if abs(p) < 2.0 ** 31 else -2 ** 31                 # (a NaN compares false: cell 0 after the clamp)
            q = max(min(q, n - 2), 0)
            cell.append(q)
            lam.append(p - q)
        (i, j), (l0, l1) = cell, lam
        lo = (1.0 - l1) * V[i, j] + l1 * V[i, j + 1]
        hi = (1.0 - l1) * V[i + 1, j] + l1 * V[i + 1, j + 1]
        return (1.0 - l0) * lo + l0 * hi
    with np.errstate(all='ignore'):
        for x0, x1 in ((10.2, 0.3), (-9.8, 0.7), (0.4, 1.0), (1.0, 1.0), (0.4, 1e300), (0.4, -1e300), (np.nan, 0.5),
                       (0.2, np.inf), (5e9, 0.5)):
            got, want = float(interp(np.float64(x0), np.float64(x1))), rule(x0, x1)
            assert got == want or (np.isnan(got) and np.isnan(want)), (x0, x1, got, want)
        assert np.isnan(rule(np.nan, 0.5)) and np.isfinite(rule(0.4, 1e300)) and abs(rule(0.4, 1e300)) > 1e299
        # the sweep has finite nodes and NaN nodes, and more than one winner
        J, _, idx = tc.oracle_sweep(s, V)
    assert np.isnan(J).any() and np.isfinite(J).any() and len(np.unique(idx)) > 3


@pytest.mark.parametrize('name', sorted(tc.CHUNKS))
def test_the_chunked_sweeps_cut_the_batches_they_are_there_for(name):
    case = tc.BY_NAME[name]
    grows = shrinks = ragged = single = False
    for k, mirrored, make in tc.chunked_runs(case):
        cells = tc.lattice_sizes(make()) * max(case.W, 1)
        plan = tc.batches(cells, k)
        assert sum(n for n, _ in plan) == len(cells) and sum(c for _, c in plan) == cells.sum()
        assert all(c >= k for _, c in plan[:-1]) and len(plan) >= 6
        if k == 1:      # one node per call: the buffers grow from the smallest lattice, or start at the largest
            assert [c for _, c in plan] == list(cells) and len(plan) == len(cells)
            single = True
            assert plan[0][1] == (cells.max() if mirrored else cells.min())
        sizes = [c for _, c in plan]
        # a batch larger than the capacity the handle kept (bytes + bytes / 4 of the largest so far): a reallocation
        grows |= any(c > 1.25 * max(sizes[:i]) for i, c in enumerate(sizes) if i)
        # a smaller batch after a larger one: what is left of the larger lies behind it
        shrinks |= any(c < max(sizes[:i]) for i, c in enumerate(sizes) if i)
        ragged |= k > 1 and plan[-1][0] < plan[-2][0] and plan[-1][1] < k
    assert grows and shrinks and ragged and single, (name, grows, shrinks, ragged, single)


def test_the_flush_rule_restated():
    assert tc.batches([3, 3, 3, 3], 1) == [(1, 3)] * 4
    assert tc.batches([3, 3, 3, 3], 6) == [(2, 6), (2, 6)] and tc.batches([3, 3, 3, 3], 7) == [(3, 9), (1, 3)]
    assert tc.batches([5, 1, 1], 100) == [(3, 7)] and tc.batches([], 5) == []
    assert tc.alternating([5, 1, 9, 3]) == [1, 2, 3, 0] and tc.alternating([2, 2, 7]) == [0, 2, 1]


def test_the_lookahead_batches_mix_what_they_are_there_for():
    for name in ('two controls', 'three states', 'four states'):
        s = tc.BY_NAME[name].solver()
        nodes = {tuple(x) for x in tc.nodes_of(s)}
        for B in (1, 7, 65):
            x = tc.lookahead_states(s, B)
            assert x.shape == (B, len(s._shape()))
            _, _, n = tc.la.lattice(s.sys.control_box, s.sys.params, s.control_steps, x, None, np.float64)
            assert tuple(x[0]) in nodes
            if B >= 7:
                dead = n[0] == 0
                assert dead.sum() == B // 7 and (n[:, dead] == 0).all() and (n[:, ~dead] > 0).all()
                lo = np.array([g[0] for g in s.state_grid])
                hi = np.array([g[-1] for g in s.state_grid])
                assert ((x < lo) | (x > hi)).any() and sum(tuple(r) in nodes for r in x) >= 3 * (B // 7)
            if B == 65:
                assert {tc.NAN_A, tc.INF_A, tc.BIG_A} <= set(x[:, 0])
