"""The table of staged-kernel forms (tests/staged_forms.py) still means what it says, without a GPU: every case plans,
per real type, the (cu, cw) pair, the tile and the budget it claims, and its generated source holds them; the chunks
are ragged where the case says so; the kernel's box prediction and cut, restated in numpy (`Reach`), take every staging
path a case claims on at least 16 (tile, chunk) pairs and miss early on at least 64 (control, node) pairs -- conditions
on the inputs, large enough that a one-cell disagreement between numpy and the device cannot empty a path; the oracle
alone shows that the models use their control lattice; and the sample the oracle runs on holds nodes of every path.
When a planner change moves a case to another pair, these tests name the case that lost its coverage.

The whole file takes 11 s on the CPU (measured: `Reach` of all 29 runs about 6 s, the oracle on 400 nodes of each from
two inputs about 4 s)."""
import numpy as np
import pytest

import staged_forms as sf
from stodynprog_amd import codegen


def _plan(case, rs, monkeypatch, kernel='staged'):
    if case.budget is not None:
        monkeypatch.setattr(codegen, 'STAGED_LDS_BYTES', case.budget)
    s = case.solver(rs, kernel)
    return s, s._kernel_plan()


def test_the_table_restates_the_planners_constants():
    assert sf.TILES == codegen.STAGED_TILES and sf.BUDGET == codegen.STAGED_LDS_BYTES
    assert sf.BUDGET // 8 == 9728


@pytest.mark.parametrize('case,rs', sf.RUNS, ids=sf.RUN_IDS)
def test_every_case_plans_the_chunk_it_claims(case, rs, monkeypatch):
    s, plan = _plan(case, rs, monkeypatch)
    d = len(s._shape())
    want = case.plan(rs, d)
    assert plan['staged'] == want, (case, rs, plan['staged'], want)
    assert s.dtype.itemsize == rs and not plan['column'] and not plan['lead_axes'] and not plan['line'] and not plan['filtered']
    # (every operator of the model is one correctly rounded operation on both sides: the oracle is compared bit for bit)
    assert plan['model'].bit_exact and not plan['model'].inexact_ops(), (case, plan['model'].inexact_ops())
    src = plan['source']
    tile = want['tile'] + (1,) * (4 - d)
    for name, value in [('SDP_STG_THREADS', 512), ('SDP_STG_CU', want['cu']), ('SDP_STG_CW', want['cw']),
                        ('SDP_STG_CAP', want['cap'])] + [('SDP_STG_T%d' % k, tile[k]) for k in range(4)]:
        assert sf.macro(src, name) == str(value) and src.count('#define {} '.format(name)) == 1, (case, rs, name)
    assert int(np.prod(tile)) == 512 and '#include "sdp_staged_kernel.h"' in src
    assert sf.macro(src, 'SDP_D') == str(d) and sf.macro(src, 'SDP_NU') == str(len(s.sys.control))
    assert sf.macro(src, 'SDP_HAS_W') == ('1' if s.perturb_grid else '0')
    # the direct kernel it is compared with shares none of this
    twin = _plan(case, rs, monkeypatch, 'generic')[1]
    assert twin['staged'] is None and 'SDP_STG_' not in twin['source']
    # the unit build() compiles is this one
    units = sf.unit_sources(case)
    assert units['staged, {} bytes'.format(rs)] == src and units['generic, {} bytes'.format(rs)] == twin['source']
    assert len(units) == 2 * len(case.sizes)


@pytest.mark.parametrize('case,rs', sf.RUNS, ids=sf.RUN_IDS)
def test_the_chunks_are_what_the_case_says(case, rs):
    r = sf.reach(case.name, rs)
    cu, cw = case.plans[rs]
    assert (r.staged['cu'], r.staged['cw']) == (cu, cw)
    claims = case.claimed(rs)
    n_ctrl = int(r.n_ctrl.max())
    assert (r.n_ctrl > 0).all()
    if 'ragged_u' in claims:
        assert n_ctrl % cu != 0 and n_ctrl > cu, (case, rs, n_ctrl, cu)
    if 'ragged_w' in claims:
        assert r.W % cw != 0 and r.W > cw, (case, rs, r.W, cw)
    if 'boxes' in claims:
        assert r.W > cw, (case, rs, r.W, cw)
    else:
        assert r.Wn <= cw or r.W == 0
    if 'uneven' in claims:
        assert r.uneven_tiles * 2 > r.n_tiles and len(np.unique(r.totals[r.totals > 0])) >= 4, (case, rs, r.uneven_tiles)
    else:
        assert r.uneven_tiles == 0
    if r.W == 0:
        assert r.Wn == 1 and cw == 1
    # the planner's copy of the row stride is the kernel's rule on every row length met (and on every length at all)
    tl, d = r.staged['tile'][-1], r.d
    for length in set(r.ext_last) | set(range(2, 200)):
        assert codegen.staged_row_stride(length, tl, d, rs) == sf.kernel_row_stride(length, tl, d, rs) >= length
    if d == 1 or tl >= 32 or rs == 4:
        assert all(sf.kernel_row_stride(length, tl, d, rs) == length | 1 for length in r.ext_last)
    else:
        assert all(sf.kernel_row_stride(length, tl, d, rs) % (2 * tl) == tl for length in r.ext_last)


@pytest.mark.parametrize('case,rs', sf.RUNS, ids=sf.RUN_IDS)
def test_reach_takes_the_paths_the_case_claims(case, rs):
    r = sf.reach(case.name, rs)
    assert sum(r.counts.values()) > 0 and case.paths[rs]
    for path in case.paths[rs]:
        assert r.counts[path] >= 16, (case, rs, path, r.counts)
        assert len(r.nodes[path]) >= 50, (case, rs, path)
        assert (r.read_vertices[path] if path != 'none' else r.missed_vertices[path]), (case, rs, path)
    if 'early' in case.claimed(rs):
        assert r.early_pairs >= r.early_only_pairs >= 64 and len(r.early_nodes) >= 50, (case, rs, r.early_only_pairs)
        assert r.W > case.plans[rs][1]
    assert r.missed_cells <= r.cells and r.missed_pairs >= r.early_pairs
    if 'none' in case.paths[rs]:
        assert r.counts['none'] == sum(r.counts.values()) and r.missed_cells == r.cells    # everything from global memory
    if set(case.paths[rs]) & {'cut0', 'cutlast'}:
        assert r.missed_cells > 0 and any(r.missed_vertices[p] for p in ('cut0', 'cutlast')), (case, rs)
    if 'cutlast' in case.paths[rs]:
        assert r.d - 1 in r.cut_axes
    # a run whose every control misses somewhere keeps no sum of the gather: it checks the fall-back alone
    assert (r.missed_pairs * r.Wn == r.cells) == (case.name == 'budget_32'), (case, rs, r.missed_pairs)
    if r.W > case.plans[rs][1] and case.name != 'budget_32':
        assert (r.cells // r.Wn - r.missed_pairs) >= 1000, (case, rs, 'too few sums carried from box to box')


def test_the_table_covers_the_forms_it_is_for():
    assert len(sf.BY_NAME) == len(sf.CASES)
    runs = [(c, rs, sf.reach(c.name, rs)) for c, rs in sf.RUNS]
    assert {c.plans[rs][0] for c, rs, _ in runs} == {4, 2, 1}
    assert any(c.plans[rs][1] == r.W > 0 for c, rs, r in runs), 'cw = W'
    assert any(c.plans[rs][1] < r.W and r.W % c.plans[rs][1] == 0 for c, rs, r in runs), 'cw < W dividing W'
    assert any('ragged_w' in c.claimed(rs) for c, rs, r in runs), 'cw < W ragged'
    for rs in (8, 4):
        assert any(c.plans[rs_][1] < r.W for c, rs_, r in runs if rs_ == rs), rs
        assert {c.plans[rs_][0] for c, rs_, _ in runs if rs_ == rs} >= {4, 2}, rs
    assert {r.d for _, _, r in runs} == {1, 2, 3, 4} and {rs for _, rs, _ in runs} == {8, 4}
    assert {r.staged['tile'] for _, _, r in runs} == set(sf.TILES.values())
    # every path and every kind of chunk is claimed; all four paths at the natural budget or through the hook
    assert {p for c, rs, _ in runs for p in c.paths[rs]} == set(sf.PATHS)
    assert {k for c, rs, _ in runs for k in c.claimed(rs)} == set(sf.CLAIMS)
    natural = {p for c, rs, _ in runs for p in c.paths[rs] if c.budget is None}
    assert natural == {'fit', 'cut0', 'cutlast'}
    # one state variable: more nodes than the budget, cw < W, the row cut with more than 64 vertices left, len | 1
    one = [(c, rs, r) for c, rs, r in runs if r.d == 1]
    assert any(r.S > r.staged['cap'] and c.plans[rs][1] < r.W and 'cutlast' in c.paths[rs] and c.budget is None
               and r.staged['cap'] > 64 and max(r.ext_last) > r.staged['cap'] for c, rs, r in one)
    # four state variables: above 9728 nodes, a plan other than (4, W)
    assert any(r.d == 4 and r.S > 9728 and c.plans[rs] != (4, r.W) for c, rs, r in runs)
    # len | 1 in 8 bytes by the tile (d = 2) and in 4 bytes by the type (d = 3)
    assert any(r.d == 2 and rs == 8 for _, rs, r in runs) and any(r.d == 3 and rs == 4 for _, rs, r in runs)
    assert any(r.d >= 3 and rs == 8 for _, rs, r in runs), 'the padded stride of 8-byte rows'
    # no perturbation with cu < 4; two controls whose lattice is no multiple of cu
    assert any(r.W == 0 and c.plans[rs][0] < 4 for c, rs, r in runs)
    two = [(c, rs, r) for c, rs, r in runs if len(c.solver(rs).sys.control) == 2]
    assert two and all(int(r.n_ctrl.max()) % c.plans[rs][0] != 0 for c, rs, r in two)
    # folded dynamics with cw < W
    assert 'early' in sf.BY_NAME['folded'].claimed(8) and sf.reach('folded', 8).counts['cut0'] == 0
    # the axes: different lengths; no axis a multiple of its tile edge in at least half of the cases; one case with
    # an axis shorter than its tile edge
    ragged = short = 0
    for c in sf.CASES:
        shape = c.solver()._shape()
        tile = sf.TILES[len(shape)]
        assert len(set(shape)) == len(shape), (c, shape)
        ragged += all(n % t for n, t in zip(shape, tile))
        short += any(n < t for n, t in zip(shape, tile))
        assert int(np.prod(shape)) <= 10 ** 5 and c.sampled >= 400
        law = c.solver().sys.perturb_laws or []
        assert len(law) == (1 if c.solver().perturb_grid else 0) and all(repr(l) == repr(sf.NormalLaw(0, 0.5)) for l in law)
    assert 2 * ragged >= len(sf.CASES) and short >= 1, (ragged, short)
    # the hook is used only where stated, and the natural budget is the planner's
    assert [c.name for c in sf.CASES if c.budget is not None] == ['budget_512', 'budget_32']


# ---------------------------------------------------------------------------------------------------------------------
# the sample and the oracle alone

@pytest.mark.parametrize('case,rs', sf.RUNS, ids=sf.RUN_IDS)
def test_the_sample_holds_nodes_of_every_claimed_path(case, rs):
    r = sf.reach(case.name, rs)
    nodes = sf.sample_nodes(case, rs)
    assert len(nodes) == len(set(nodes.tolist())) == case.sampled >= 400
    assert nodes[0] == 0 and nodes[-1] == r.S - 1
    for path in case.paths[rs]:
        assert np.isin(nodes, r.nodes[path]).sum() >= min(50, len(r.nodes[path])), (case, rs, path)
    if 'early' in case.claimed(rs):
        assert np.isin(nodes, r.early_nodes).sum() >= 50, (case, rs)
    assert np.array_equal(nodes, sf.sample_nodes(case, rs))


@pytest.mark.parametrize('which', sf.INPUTS)
@pytest.mark.parametrize('case,rs', sf.RUNS, ids=sf.RUN_IDS)
def test_the_oracle_uses_the_control_lattice(case, rs, which):
    """the policies the GPU tests compare are not all one corner of the box: at least 5 distinct policy indices (every
    index of the lattice where it has fewer), at most half of the sampled nodes at index 0"""
    nodes, J, pol, idx = sf.oracle(case.name, rs, which)
    lattice = int(sf.reach(case.name, rs).n_ctrl.max())
    assert len(idx) == case.sampled and J.dtype == sf.REALS[rs] and pol.dtype == sf.REALS[rs]
    assert np.isfinite(J).all()
    assert len(np.unique(idx)) >= min(5, lattice), (case, rs, which, np.unique(idx))
    assert (idx == 0).sum() * 2 <= len(idx), (case, rs, which, int((idx == 0).sum()), len(idx))


def test_the_horizon_table_reaches_no_plan_with_several_boxes():
    """the staged rows of tests/horizon_cases.py plan cw = W at every step: the finite-horizon recursion with cw < W is
    run by tests/test_gpu_staged_forms.py on a case of this table"""
    import horizon_cases as hc
    rows = [f for f in hc.FAMILIES if f.kernel == 'staged']
    assert len(rows) == 2
    for f in rows:
        s = f.solver()
        for t in (0, 3):
            plan = s._kernel_plan(t, s._trace_now(t))
            assert plan['staged']['cw'] == plan['W'] and plan['staged']['cu'] == 4, (f, t, plan['staged'])
