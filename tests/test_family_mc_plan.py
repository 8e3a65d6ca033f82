"""Monte Carlo evaluation of families on the CPU (tests/family_mc_cases.py): the Monte Carlo unit cross-compiles for
gfx950 with exactly its one kernel, free of scratch memory, vector spills and static LDS; the sweep and evaluation
units keep their text; the tile-to-XCD mapping and the grid bound, restated; what `SolverFamily.monte_carlo` refuses
before a device is touched; the result class in numpy alone; and the inputs of the GPU tests have the properties
those tests rely on, by the definition of the draws and the host loop.  No GPU."""
import hashlib
import os
import re

import numpy as np
import pytest

import family_mc_cases as mcc
from test_family_plan import _kernels, _digests, ROOT
from stodynprog_amd import SolverFamily, DPSolver, codegen, montecarlo as mc, _native as nat

UNITS = mcc.PARITY + [mcc.MAPPING[2]]


@pytest.mark.parametrize('case', UNITS, ids=repr)
def test_the_unit_compiles_with_its_one_kernel(case, tmp_path):
    fam = SolverFamily(case.solvers())
    tabs = fam._tables()
    source = codegen.family_mc_unit(tabs['model'], fam.dtype)
    assert '#define SDP_FAMILY 1' in source and '#define SDP_FAMILY_MC 1' in source and '#define SDP_LANES 1\n' in source
    assert '#include "sdp_family_mc_kernel.h"' in source and 'sdp_model_cell_at(' in source
    assert '#include "sdp_family_kernel.h"' not in source and '#include "sdp_sweep_kernel.h"' not in source
    assert 'SDP_FAMILY_POLICY' not in source
    kernels = _kernels(source, tmp_path)
    assert sorted(kernels) == ['sdp_family_montecarlo'], sorted(kernels)
    f = kernels['sdp_family_montecarlo']
    print(case, {n: f[n] for n in ('.vgpr_count', '.sgpr_count', '.private_segment_fixed_size', '.vgpr_spill_count',
                                   '.sgpr_spill_count', '.group_segment_fixed_size', '.max_flat_workgroup_size')})
    assert f['.private_segment_fixed_size'] == 0 and f['.vgpr_spill_count'] == 0, f
    assert f['.group_segment_fixed_size'] == 0, f                       # (the draw table is dynamic LDS)
    assert f['.max_flat_workgroup_size'] == mcc.TILE == 256
    # the sweep and the evaluation unit of the same family keep the text on record; the new unit's is on record too
    policy = codegen.family_policy_unit(tabs['model'], fam.dtype)
    digest = lambda text: hashlib.sha256(text.encode('utf-8')).hexdigest()[:16]
    assert digest(tabs['source']) in _digests() and digest(policy) in _digests() and digest(source) in _digests(), case
    assert len({codegen.source_key(source), codegen.source_key(policy), codegen.source_key(tabs['source'])}) == 3


def test_the_unit_does_not_depend_on_the_lane_count_and_its_key_covers_its_header(monkeypatch, tmp_path):
    fam = _ar1()
    tabs = fam._tables()
    one = SolverFamily(mcc.LAWS.solvers()[:1])
    assert one._tables()['source'] != tabs['source']
    source = codegen.family_mc_unit(tabs['model'], fam.dtype)
    assert codegen.family_mc_unit(one._tables()['model'], one.dtype) == source
    assert 'sdp_family_mc_kernel.h' not in codegen._HEADERS
    policy = codegen.family_policy_unit(tabs['model'], fam.dtype)
    keys = codegen.source_key(source), codegen.source_key(tabs['source']), codegen.source_key(policy)
    csrc = tmp_path / 'csrc'
    csrc.mkdir()
    for fn in os.listdir(codegen.CSRC):
        if fn.endswith('.h'):
            (csrc / fn).write_bytes(open(os.path.join(codegen.CSRC, fn), 'rb').read())
    monkeypatch.setattr(codegen, 'CSRC', str(csrc))
    codegen._digest_cache.clear()
    now = lambda: (codegen.source_key(source), codegen.source_key(tabs['source']), codegen.source_key(policy))
    assert now() == keys
    # an edit of the new header changes the key of the Monte Carlo unit alone
    with open(str(csrc / 'sdp_family_mc_kernel.h'), 'a') as f:
        f.write('// edited\n')
    assert now()[0] != keys[0] and now()[1:] == keys[1:]
    # .. and it includes the family header and the draw helpers: an edit of either changes its key as well
    mine = now()[0]
    with open(str(csrc / 'sdp_family_kernel.h'), 'a') as f:
        f.write('// edited\n')
    assert now()[0] != mine
    mine = now()[0]
    with open(str(csrc / 'sdp_mc_kernel.h'), 'a') as f:
        f.write('// edited\n')
    codegen._digest_cache.clear()
    assert now()[0] != mine
    codegen._digest_cache.clear()


def test_the_unit_says_what_it_is_and_the_library_checks_it():
    read = lambda *path: open(os.path.join(*path)).read()
    header = read(codegen.CSRC, 'sdp_family_mc_kernel.h')
    args = read(codegen.CSRC, 'sdp_kernel_args.h')
    library = read(codegen.CSRC, 'sdp_hip.hip')
    draws = read(codegen.CSRC, 'sdp_mc_kernel.h')
    assert 'SDP_META_F_FAMILY_MC = 4096' in args
    assert 'SDP_META_F_FAMILY | SDP_META_F_FAMILY_MC, 0, 0, SDP_FMC_TILE' in header
    assert '#define SDP_FMC_TILE SDP_MC_THREADS' in header and '#define SDP_MC_THREADS {}'.format(mcc.TILE) in draws
    assert '!(m[SDP_META_FLAGS] & SDP_META_F_FAMILY_MC)' in library and 'm[SDP_META_THREADS] != 256' in library
    # the draw helpers are included, not restated; the solo entry point is what the macro leaves out
    assert '#define SDP_MC_HELPERS_ONLY 1' in header and '#include "sdp_mc_kernel.h"' in header
    assert '#if !defined(SDP_MC_HELPERS_ONLY)\n' in draws
    assert 'SDP_DEV' not in header                                      # (no device function of its own)
    for helper in ('sdp_philox4x32_10(', 'sdp_mc_uniform(', 'sdp_mc_index(', 'sdp_mc_visit('):
        assert helper in header and re.search(r'^SDP_DEV \w+ ' + re.escape(helper), draws, re.M), helper
    # the ABI: header, library and binding move together
    abi = read(ROOT, 'include', 'sdp_hip.h')
    real_lib = nat.lib()
    for name in ('sdp_family_load_mc_unit', 'sdp_family_montecarlo'):
        assert re.search(r'^int {}\('.format(name), abi, re.M) and 'extern "C" int {}('.format(name) in library
        assert name in nat.EXPORTS and hasattr(real_lib, name)
    assert real_lib.sdp_family_load_mc_unit(None, None) == -1
    assert real_lib.sdp_family_montecarlo(None, None, 1, 1, 0, None, 0, None, None, 1, None, 0., 1, None, None, None, None) == -1
    # the grid bound and the walk the restatement restates
    for line in ('const int64_t tiles = (B + threads - 1) / threads;', 'const int64_t cap = (int64_t)f->cus * per_cu / 8;',
                 'if (per_cu > 8) per_cu = 8;'):
        assert line in library, line
    for line in ('const int64_t tile = (int64_t)part * per_part + unit % per_part;',
                 'const int64_t p = first + 8 * (int)(unit / per_part);', 'if (p != loaded) {'):
        assert line in header, line


@pytest.mark.parametrize('n_active', (1, 2, 7, 8, 9, 17))
def test_the_launch_plan_on_256_compute_units(n_active):
    for B, per_cu in ((mcc.B_PARITY, 8), (mcc.B_MAPPING, 8), (4096, 7), (mcc.cap_batch(256), 8), (mcc.cap_batch(256), 5)):
        plan = mcc.launch(B, n_active, 256, per_cu)
        tiles = -(-B // 256)
        assert plan['tiles'] == tiles
        # every tile of every member exactly once
        seen = sorted((p, t) for xcd in plan['visits'] for p, t, _ in xcd)
        assert seen == [(p, t) for p in range(n_active) for t in range(tiles)]
        # a member's tiles stay on its XCDs: one XCD with 8 members or more, 8 // n_active contiguous parts with fewer
        homes = {}
        for xcd, visits in enumerate(plan['visits']):
            for p, t, _ in visits:
                homes.setdefault(p, set()).add(xcd)
        for p, xcds in homes.items():
            if n_active >= 8:
                assert xcds == {p % 8}
            else:
                assert xcds <= set(range(p * plan['parts'], (p + 1) * plan['parts']))
        for xcd, visits in enumerate(plan['visits']):
            if n_active < 8 and visits:
                ts = [t for _, t, _ in visits]
                assert ts == list(range(ts[0], ts[0] + len(ts)))         # a contiguous part
        # the grid: a multiple of 8, at most the resident workgroups
        assert plan['blocks'] % 8 == 0 and 8 <= plan['blocks'] <= max(8, 256 * min(per_cu, 8))
        assert plan['per_xcd'] == max(1, min(plan['wanted'], 256 * min(per_cu, 8) // 8))
    # 64 members of 4096 trajectories fill the chip: 1024 tiles, one workgroup each
    full = mcc.launch(4096, 64, 256, 8)
    assert full['blocks'] == 1024 and all(trip == 0 for xcd in full['visits'] for _, _, trip in xcd)
    # the cap case of the GPU test walks again whatever the occupancy query answers
    if n_active == 9:
        for per_cu in range(1, 9):
            plan = mcc.launch(mcc.cap_batch(256), 9, 256, per_cu)
            assert mcc.cap_batch(256) % 256 == 1 and 9 * plan['tiles'] > 8 * 256
            assert max(trip for xcd in plan['visits'] for _, _, trip in xcd) >= 1


def _ar1():
    return SolverFamily(mcc.LAWS.solvers())


def test_argument_checks_come_before_a_device_is_touched(monkeypatch):
    monkeypatch.setattr(nat, 'require_gpu', lambda *a, **k: pytest.fail('a device was asked for'))
    monkeypatch.setattr(nat, 'lib', lambda *a, **k: pytest.fail('the library was asked for'))
    monkeypatch.setattr(nat, 'compile_model', lambda *a, **k: pytest.fail('the compiler was asked for'))
    fam = _ar1()
    pol, x0 = np.zeros((3, 7, 5, 2)), np.zeros((3, 4, 2))
    # a time-indexed policy, or any extra leading axis
    for shape in ((6, 3, 7, 5, 2), (3, 6, 7, 5, 2), (1, 1, 3, 7, 5, 2)):
        with pytest.raises(NotImplementedError) as err:
            fam.monte_carlo(np.zeros(shape), x0, 5)
        assert 'time-indexed' in str(err.value)
    # wrong shapes
    for bad in (np.zeros((7, 5)), np.zeros((2, 7, 5, 2)), np.zeros((3, 7, 5, 1)), np.zeros((3, 7, 4, 2))):
        with pytest.raises(ValueError) as err:
            fam.monte_carlo(bad, x0, 5)
        assert str(bad.shape) in str(err.value)
    for bad in (np.zeros(3), np.zeros((4, 3)), np.zeros((2, 4, 2)), np.zeros((3, 4, 2, 1)), np.zeros(())):
        with pytest.raises(ValueError) as err:
            fam.monte_carlo(pol, bad, 5, n_traj=4)
        assert 'x0' in str(err.value)
    with pytest.raises(ValueError) as err:
        fam.monte_carlo(pol, np.zeros(2), 5)
    assert 'n_traj' in str(err.value)
    with pytest.raises(ValueError) as err:
        fam.monte_carlo(pol, x0, 5, n_traj=5)
    assert 'n_traj = 5' in str(err.value)
    # steps, burn-in, cuts, seeds, trajectory ids
    for kw in (dict(n_steps=0), dict(n_steps=5, n_burn=5), dict(n_steps=5, n_burn=-1)):
        with pytest.raises(ValueError) as err:
            fam.monte_carlo(pol, x0, **kw)
        assert 'n_burn' in str(err.value)
    fam.steps_per_launch = 0
    with pytest.raises(ValueError) as err:
        fam.monte_carlo(pol, x0, 5)
    assert 'steps_per_launch' in str(err.value)
    del fam.steps_per_launch
    assert fam.steps_per_launch == SolverFamily.steps_per_launch == DPSolver.steps_per_launch
    for seed in (-1, 1 << 64, (1, 2), (1, 2, -3), (1, 2, 3, 4)):
        with pytest.raises(ValueError) as err:
            fam.monte_carlo(pol, x0, 5, seed=seed)
        assert 'seed' in str(err.value)
    for offset in (-1, (1 << 64) - 3):
        with pytest.raises(ValueError) as err:
            fam.monte_carlo(pol, x0, 5, traj_offset=offset)
        assert 'trajectory ids' in str(err.value)
    # laws: the solo limits, and one number of points for all members
    grid, proba = np.linspace(-1., 1., 5), np.full(5, 0.2)
    with pytest.raises(ValueError) as err:
        fam.monte_carlo(pol, x0, 5, law=[(grid, proba), (grid[:4], np.full(4, 0.25)), (grid, proba)])
    assert 'member 1' in str(err.value) and '4 points' in str(err.value)
    with pytest.raises(ValueError) as err:
        fam.monte_carlo(pol, x0, 5, law=[(grid, proba)] * 2)
    assert 'sequence of 3' in str(err.value)
    with pytest.raises(ValueError):
        fam.monte_carlo(pol, x0, 5, law=(grid, proba * 2))
    with pytest.raises(ValueError) as err:
        fam.monte_carlo(pol, x0, 5, law=(np.zeros(4097), np.full(4097, 1. / 4097)))
    assert '4097' in str(err.value)
    # members whose model looks data up as data[k]; deterministic members (the solo message)
    pv = SolverFamily(mcc.BY_NAME['pv_sized'].solvers())
    with pytest.raises(NotImplementedError) as err:
        pv.monte_carlo(np.zeros((3, 9, 1)), np.zeros((3, 4, 1)), 5)
    assert 'deterministic system has nothing to draw' in str(err.value)
    # (a stochastic member with data[k]: models.finite_horizon takes t symbolically and runs; a model with a table does not)
    lookup = SolverFamily([_data_member(0.9), _data_member(0.8)])
    with pytest.raises(NotImplementedError) as err:
        lookup.monte_carlo(np.zeros((2, 9, 1)), np.zeros((2, 4, 1)), 5)
    assert 'data[k]' in str(err.value)
    symbolic = SolverFamily(mcc.BY_NAME['finite_horizon'].solvers())
    assert not symbolic._tables(0)['time_specialized']
    # the chunks of a Monte Carlo run count its arrays beside the handle's
    tabs = fam._tables()
    per = fam._member_bytes(tabs)
    extra = fam._mc_member_bytes(65, 3, True)
    assert extra == (2 * 35 + 3 * 65) * 8 + 8 * 65 + 8 * 35 + 3 * 16 + 8
    assert fam._mc_member_bytes(65, 3, False) == extra - 8 * 35
    fam.chunk_bytes = mcc.chunk_bytes_for(fam, 2, 65, 3, True)
    assert fam._chunks(tabs, extra) == [(0, 2), (2, 3)] and per + extra > 0


def _data_member(decay):
    from stodynprog_amd import SysDescription
    from stodynprog_amd.models import NormalLaw
    data = np.linspace(0., 1., 16)
    sysd = SysDescription((1, 1, 1), stationnary=False, name='lookup')
    sysd.dyn = lambda k, x, u, w: (decay * x + u + w + data[k],)
    sysd.cost = lambda k, x, u, w: x * x + 0.25 * u * u
    sysd.control_box = lambda k, x: ((-1., 1.),)
    sysd.perturb_laws = [NormalLaw(0, 0.1)]
    s = DPSolver(sysd)
    s.discretize_state(-2, 2, 9)
    s.discretize_perturb(-0.3, 0.3, 3)
    s.control_steps = (0.125,)
    return s


def test_the_result_class_in_numpy_alone():
    rng = np.random.default_rng(3)
    P, B, d = 3, 7, 2
    cost_sum = rng.uniform(0., 5., size=(P, B)).astype(np.float32)
    n_out = rng.integers(0, 4, size=(P, B))
    x_final = rng.uniform(size=(P, B, d)).astype(np.float32)
    occ = rng.integers(0, 9, size=(P, 4, 5))
    res = mc.FamilyMonteCarloResult(cost_sum, n_out, x_final, occ, 12, 2, (5, 5, 9), 3, 0, 'device')
    assert len(res) == P and res.path == 'device' and res.seeds == (5, 5, 9)
    assert res.cost_mean.dtype == np.float64 and np.array_equal(res.cost_mean, cost_sum.astype(np.float64) / 10.)
    for p in range(P):
        ref = mc.MonteCarloResult(cost_sum[p], n_out[p], x_final[p], occ[p], 12, 2, res.seeds[p], 3, 0, 'device')
        one = res[p]
        assert isinstance(one, mc.MonteCarloResult) and one.seed == ref.seed and one.n_traj == B
        for name in ('cost_sum', 'cost_mean', 'n_outside', 'x_final', 'occupancy'):
            assert np.array_equal(getattr(one, name), getattr(ref, name)), name
        assert one.mean == ref.mean == res.mean[p] and one.stderr == ref.stderr == res.stderr[p]
        assert (one.n_steps, one.n_burn, one.traj_offset, one.t0) == (12, 2, 3, 0)
    diff = res.cost_mean[0] - res.cost_mean[1]
    assert res.paired(0, 1) == (float(diff.mean()), float(diff.std(ddof=1) / np.sqrt(B)))
    assert res.paired(1, 0)[0] == -res.paired(0, 1)[0]
    with pytest.raises(ValueError) as err:
        res.paired(0, 2)
    assert 'different seeds' in str(err.value)
    single = mc.FamilyMonteCarloResult(cost_sum[:, :1], n_out[:, :1], x_final[:, :1], None, 12, 2, (1, 1, 1), 0, 0, 'device')
    assert single[0].occupancy is None and np.isnan(single.paired(0, 1)[1]) and np.all(np.isnan(single.stderr))
    with pytest.raises(ValueError):
        mc.FamilyMonteCarloResult(cost_sum, n_out, x_final, None, 12, 2, (1, 2), 0, 0, 'device')


def test_family_draws_are_the_stacked_solo_draws():
    fam = _ar1()
    for seed, law in ((4, None), ((4, 5, 6), mcc.member_laws()), (7, mcc.shared_law())):
        idx, w = fam.monte_carlo_draws(seed, 11, 6, law=law, traj_offset=40)
        assert idx.shape == w.shape == (3, 6, 11) and w.dtype == fam.dtype
        for p, s in enumerate(fam.solvers):
            seed_p = seed if np.ndim(seed) == 0 else seed[p]
            law_p = law[p] if isinstance(law, list) else law
            i1, w1 = s.monte_carlo_draws(seed_p, 11, 6, law=law_p, traj_offset=40)
            assert np.array_equal(idx[p], i1) and np.array_equal(w[p], w1)
    # one seed: the same indices for members with the same law weights (common random numbers)
    idx, _ = fam.monte_carlo_draws(9, 11, 6, law=mcc.shared_law())
    assert np.array_equal(idx[0], idx[1]) and np.array_equal(idx[0], idx[2])


# ----------------------------------------------------------------------------------------------------------------------
# the inputs of the GPU tests, by the definition of the draws and the host loop

def test_the_outside_case_has_a_member_inside_and_a_member_outside():
    pol, x0 = mcc.policies(mcc.OUTSIDE), mcc.outside_starts()
    counts = [mcc.host_run(s, pol[p], x0, mcc.STEPS_OUTSIDE, 0, 3)[1] for p, s in enumerate(mcc.OUTSIDE.solvers())]
    print('n_outside per member:', [int(c.sum()) for c in counts])
    assert counts[0].sum() == 0 and counts[1].sum() > 0
    grids = [s.state_grid for s in mcc.OUTSIDE.solvers()]
    assert grids[0][0][-1] == 10. and grids[1][0][-1] == 2. and np.all((x0[:, 0] > 2.) & (x0[:, 0] < 10.))


def test_the_occupancy_cases_visit_a_node_from_two_trajectories_at_one_step():
    # fewer nodes than trajectories: at every step two trajectories share their nearest node
    for case in mcc.PARITY:
        assert int(np.prod(case.solvers()[0]._shape())) < mcc.B_PARITY, case
    # .. and by the host loop: inventory's trajectories sit at the empty stock
    case = mcc.PARITY[0]
    pol, x0 = mcc.policies(case), mcc.starts(case, mcc.B_PARITY)
    _, _, _, occ = mcc.host_run(case.solvers()[0], pol[0], x0[0], mcc.N_STEPS, mcc.N_BURN, 3, occupancy=True)
    assert occ.sum() == mcc.B_PARITY * (mcc.N_STEPS - mcc.N_BURN) and occ.max() > (mcc.N_STEPS - mcc.N_BURN)


def test_the_laws_reach_every_branch_of_the_index():
    fam = _ar1()
    idx, _ = fam.monte_carlo_draws(11, mcc.B_PARITY, mcc.N_STEPS, law=mcc.member_laws())
    assert all(len(np.unique(i)) >= 5 for i in idx), [len(np.unique(i)) for i in idx]
    for p, (grid, proba) in enumerate(mcc.member_laws()):
        s = fam.solvers[p]
        assert len(grid) == 9 != len(s.perturb_grid[0]) and not np.array_equal(grid[:3], s.perturb_grid[0])
    idx, _ = fam.monte_carlo_draws(11, mcc.B_PARITY, mcc.N_STEPS, law=mcc.long_law())
    assert len(mcc.long_law()[0]) == 70 and (idx < 64).any() and (idx > 64).any()
    with open(os.path.join(codegen.CSRC, 'sdp_mc_kernel.h')) as f:
        assert '#define SDP_MC_COUNT_MAX 64' in f.read()


def test_the_build_compiles_the_units_of_the_gpu_tests():
    units = mcc.unit_sources()
    for case in mcc.FAMILIES:
        fam = SolverFamily(case.solvers())
        tabs = fam._tables()
        assert tabs['source'] in units and codegen.family_mc_unit(tabs['model'], fam.dtype) in units, case
    with open(os.path.join(ROOT, '__graft_entry__.py')) as f:
        assert 'family_mc_cases.unit_sources()' in f.read()
