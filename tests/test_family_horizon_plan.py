"""Closed loops of families over a horizon on the CPU (tests/family_horizon_cases.py): the horizon unit cross-compiles
for gfx950 with exactly its kernels, free of scratch memory, vector spills and static LDS; its key covers its header and
leaves the other units' alone; the unit says what it is and the library checks it; the table of constants is the solo
one, stacked; what `SolverFamily.simulate` and `SolverFamily.monte_carlo_horizon` refuse before a device is touched; the
tile-to-XCD mapping and the two grid bounds, restated; and the inputs of the GPU tests have the properties those tests
rely on.  No GPU."""
import hashlib
import os
import re

import numpy as np
import pytest

import family_horizon_cases as fh
import family_mc_cases as mcc
from test_family_plan import _kernels, _digests, ROOT
from stodynprog_amd import SolverFamily, codegen, _native as nat

NOTES = ('.vgpr_count', '.sgpr_count', '.private_segment_fixed_size', '.vgpr_spill_count', '.sgpr_spill_count',
         '.group_segment_fixed_size', '.max_flat_workgroup_size')


def _unit(hz):
    fam = SolverFamily(hz.solvers())
    tabs = fam._tables(None if fam.stationnary else hz.t0)
    return fam, tabs, codegen.family_horizon_unit(tabs['model'], fam.dtype)


@pytest.mark.parametrize('hz', fh.PARITY + [fh.MAPPING[2]], ids=repr)
def test_the_unit_compiles_with_its_kernels(hz, tmp_path):
    fam, tabs, source = _unit(hz)
    assert '#define SDP_FAMILY 1' in source and '#define SDP_FAMILY_HORIZON 1' in source and '#define SDP_LANES 1\n' in source
    assert '#include "sdp_family_horizon_kernel.h"' in source and 'sdp_model_cell_at(' in source
    assert '#include "sdp_family_kernel.h"' not in source and '#include "sdp_sweep_kernel.h"' not in source
    assert 'SDP_FAMILY_MC' not in source and 'SDP_FAMILY_POLICY' not in source
    kernels = _kernels(source, tmp_path)
    wanted = ['sdp_family_montecarlo_h', 'sdp_family_simulate'] if fam.W else ['sdp_family_simulate']
    assert sorted(kernels) == wanted, sorted(kernels)
    for name, threads in (('sdp_family_simulate', fh.SIM_TILE), ('sdp_family_montecarlo_h', fh.MC_TILE)):
        if name not in kernels:
            continue
        f = kernels[name]
        print(hz, name, {n: f[n] for n in NOTES})
        assert f['.private_segment_fixed_size'] == 0 and f['.vgpr_spill_count'] == 0, f
        assert f['.group_segment_fixed_size'] == 0, f                   # (the draw table is dynamic LDS)
        assert f['.max_flat_workgroup_size'] == threads
    # the family's other units keep the text on record; the new unit's is on record too
    digest = lambda text: hashlib.sha256(text.encode('utf-8')).hexdigest()[:16]
    assert digest(tabs['source']) in _digests() and digest(source) in _digests(), hz
    if fam.stationnary:
        assert digest(codegen.family_mc_unit(tabs['model'], fam.dtype)) in _digests()
        assert digest(codegen.family_policy_unit(tabs['model'], fam.dtype)) in _digests()


def test_one_unit_per_structure_and_its_key_covers_its_header(monkeypatch, tmp_path):
    fam, tabs, source = _unit(fh.AR1_64)
    # the lane count does not enter, nor does the step of a model traced per step
    one = SolverFamily(fh.AR1_64.solvers()[:1])
    assert one._tables()['source'] != tabs['source']
    assert codegen.family_horizon_unit(one._tables()['model'], one.dtype) == source
    pv = SolverFamily(fh.PV_SIZED.solvers())
    assert len({codegen.family_horizon_unit(pv._tables(t)['model'], pv.dtype) for t in range(6)}) == 1
    assert 'sdp_family_horizon_kernel.h' not in codegen._HEADERS
    units = [source, tabs['source'], codegen.family_policy_unit(tabs['model'], fam.dtype),
             codegen.family_mc_unit(tabs['model'], fam.dtype)]
    assert len({codegen.source_key(u) for u in units}) == 4
    csrc = tmp_path / 'csrc'
    csrc.mkdir()
    for fn in os.listdir(codegen.CSRC):
        if fn.endswith('.h'):
            (csrc / fn).write_bytes(open(os.path.join(codegen.CSRC, fn), 'rb').read())
    monkeypatch.setattr(codegen, 'CSRC', str(csrc))
    codegen._digest_cache.clear()
    now = lambda: [codegen.source_key(u) for u in units]
    keys = now()
    # an edit of the new header changes the key of the horizon unit alone
    with open(str(csrc / 'sdp_family_horizon_kernel.h'), 'a') as f:
        f.write('// edited\n')
    assert now()[0] != keys[0] and now()[1:] == keys[1:]
    # .. and it includes the family header and the draw helpers: an edit of either changes its key as well; one of the
    # Monte Carlo unit's header does not
    mine = now()[0]
    with open(str(csrc / 'sdp_family_mc_kernel.h'), 'a') as f:
        f.write('// edited\n')
    assert now()[0] == mine
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
    header = read(codegen.CSRC, 'sdp_family_horizon_kernel.h')
    args = read(codegen.CSRC, 'sdp_kernel_args.h')
    library = read(codegen.CSRC, 'sdp_hip.hip')
    draws = read(codegen.CSRC, 'sdp_mc_kernel.h')
    sweep = read(codegen.CSRC, 'sdp_family_kernel.h')
    assert 'SDP_META_F_FAMILY_HORIZON = 16384' in args
    assert 'SDP_META_F_FAMILY | SDP_META_F_FAMILY_HORIZON, 0, 0, SDP_FH_MC_THREADS, SDP_FH_SIM_TILE' in header
    assert '#define SDP_FH_SIM_TILE {} '.format(fh.SIM_TILE) in header and '#define SDP_FH_MC_TILE SDP_MC_THREADS' in header
    assert '#define SDP_MC_THREADS {}'.format(fh.MC_TILE) in draws
    assert '__launch_bounds__(SDP_FH_SIM_TILE) sdp_family_simulate(' in header
    assert '__launch_bounds__(SDP_FH_MC_TILE) sdp_family_montecarlo_h(' in header
    assert '!(m[SDP_META_FLAGS] & SDP_META_F_FAMILY_HORIZON)' in library and 'm[SDP_META_COL_ROWS] != 64' in library
    assert '!defined(SDP_FAMILY_HORIZON)' in sweep                      # (the unit does not carry sdp_family_sweep)
    # the draw helpers are included, not restated; the model's time is the solo kernels'
    assert '#define SDP_MC_HELPERS_ONLY 1' in header and '#include "sdp_mc_kernel.h"' in header
    for helper in ('sdp_philox4x32_10(', 'sdp_mc_uniform(', 'sdp_mc_index(', 'sdp_mc_visit('):
        assert helper in header and not re.search(r'^SDP_DEV \w+ ' + re.escape(helper), header, re.M), helper
    assert header.count('(sdp_real)(a.t0 + (double)step)') == 2 and header.count('if (counted) acc = acc + g;') == 1
    assert 'sdp_interp_point<sdp_real, SDP_D, double>(pk + c * a.S, grid, x)' in header
    assert 'SdpLerp<sdp_real, SDP_D, double, 0, false>::eval(pk + c * a.S, grid, cell, 0)' in header
    # the simulate kernel has neither LDS nor a barrier: both are below its end
    sim = header[header.index('sdp_family_simulate(SdpFamilySimHArgs a)'):header.index('#if SDP_HAS_W')]
    assert '__syncthreads' not in sim and '__shared__' not in sim
    # the ABI: header, library and binding move together
    abi = read(ROOT, 'include', 'sdp_hip.h')
    integration = read(ROOT, 'INTEGRATION.md')
    real_lib = nat.lib()
    for name in ('sdp_family_load_horizon_unit', 'sdp_family_simulate', 'sdp_family_montecarlo_h'):
        assert re.search(r'^int {}\('.format(name), abi, re.M) and 'extern "C" int {}('.format(name) in library
        assert name in nat.EXPORTS and hasattr(real_lib, name) and '`{}`'.format(name) in integration
    assert real_lib.sdp_family_load_horizon_unit(None, None) == -1
    assert real_lib.sdp_family_simulate(None, None, 1, 1, None, 0, 0, 1, 1, 1, None, None, 0., None, None, None) == -1
    assert real_lib.sdp_family_montecarlo_h(None, None, 1, 1, None, 0, 0, 1, 1, 1, 0, None, 0, None, None, 1, None, 0., 1,
                                            None, None, None, None) == -1
    # the grid bounds and the walk the restatement restates
    for line in ('family_horizon_per_xcd(f, (B + 63) / 64, (int64_t)f->cus * 32 / 8)',
                 'family_horizon_per_xcd(f, (B + threads - 1) / threads, (int64_t)f->cus * per_cu / 8)',
                 'if (per_cu > 8) per_cu = 8;', 'if (per_xcd > cap) per_xcd = cap;'):
        assert line in library, line
    for line in ('const int64_t tile = (int64_t)k.part * k.per_part + unit % k.per_part;',
                 'const int64_t p = k.first + 8 * (int)(unit / k.per_part);', 'if (p != loaded) {'):
        assert line in header, line


@pytest.mark.parametrize('hz', (fh.PV_SIZED, fh.LOOKUP, fh.FINITE, fh.AR1_64, fh.AR1_32), ids=repr)
def test_the_table_is_the_solo_tables_stacked(hz):
    fam = SolverFamily(hz.solvers())
    tabs, table, timed = fam._horizon_tables(hz.n_steps, hz.t0)
    assert timed == hz.int_time and table.dtype == fam.dtype and table.flags.c_contiguous
    bits = lambda a: np.ascontiguousarray(a).view(np.uint8)
    if timed:
        # a row per member and step: row (p, k) is row k of the member's own table
        assert table.shape == (fam.P, hz.n_steps, tabs['prm'].shape[1])
        for dt in (np.float64, np.float32):
            for p, s in enumerate(hz.solvers()):
                s.dtype = np.dtype(dt)
                solo = s._horizon_table(s._trace_now(hz.t0), True, hz.n_steps, hz.t0)
                assert solo is not None and solo.shape == table[p].shape
                assert np.array_equal(bits(solo), bits(table[p].astype(dt) if dt != fam.dtype else table[p])), (hz, p, dt)
        assert any(not np.array_equal(table[0, k], table[0, k + 1]) for k in range(hz.n_steps - 1))
        # a later start reads the later rows
        late = fam._horizon_tables(hz.n_steps - 2, hz.t0 + 2)[1]
        assert np.array_equal(bits(late), bits(table[:, 2:]))
    else:
        # symbolic in time: one row per member, passed once (the solo call tiles its row n_steps times)
        assert table.shape == (fam.P, 1, tabs['prm'].shape[1]) and np.array_equal(bits(table[:, 0]), bits(tabs['prm']))
        for p, s in enumerate(hz.solvers()):
            model = s._trace_now(None if s.sys.stationnary else hz.t0)
            model.lift_constants()
            solo = s._horizon_table(model, True, hz.n_steps, hz.t0)
            assert solo.shape == (hz.n_steps, table.shape[2])
            assert np.array_equal(bits(solo), bits(np.broadcast_to(table[p], solo.shape))), (hz, p)
    # the policy: control axis first, the steps of the call alone; a stationary one is one slice
    pol = fh.policies(hz)
    pol_d, pol_timed = fam._horizon_policy(pol, hz.n_steps, hz.t0)
    S = int(np.prod(fam.dims))
    assert pol_timed and pol_d.shape == (fam.P, hz.n_steps, fam.nu, S) and pol_d.dtype == fam.dtype
    for p, s in enumerate(fam.solvers):
        solo = s._horizon_policy(pol[p], True, hz.n_steps, hz.t0)
        assert np.array_equal(bits(solo.reshape(hz.n_steps, fam.nu, S)), bits(pol_d[p]))
    for given in (pol[:, 0], pol[0, 0]):
        pol_d, pol_timed = fam._horizon_policy(given, hz.n_steps, hz.t0)
        assert not pol_timed and pol_d.shape == (fam.P, 1, fam.nu, S)
        for p, s in enumerate(fam.solvers):
            solo = s._horizon_policy(given[p] if given.ndim == pol.ndim - 1 else given, False, 1, 0)
            assert np.array_equal(bits(solo.reshape(1, fam.nu, S)), bits(pol_d[p]))


def _no_device(monkeypatch):
    monkeypatch.setattr(nat, 'require_gpu', lambda *a, **k: pytest.fail('a device was asked for'))
    monkeypatch.setattr(nat, 'lib', lambda *a, **k: pytest.fail('the library was asked for'))
    monkeypatch.setattr(nat, 'compile_model', lambda *a, **k: pytest.fail('the compiler was asked for'))


def test_argument_checks_come_before_a_device_is_touched(monkeypatch):
    _no_device(monkeypatch)
    fam = SolverFamily(fh.AR1_64.solvers())                             # dims (7, 5), nu = 2, P = 3
    pol, x0, w = np.zeros((3, 8, 7, 5, 2)), np.zeros((3, 4, 2)), np.zeros((3, 8, 4))
    both = (lambda p, x, **kw: fam.simulate(p, x, kw.pop('w', w), **kw),
            lambda p, x, **kw: fam.monte_carlo_horizon(p, x, kw.pop('n_steps', 8), **kw))
    # the shapes of pol: no (T_pol,) + ... form, the members' axis comes first
    for call in both:
        for bad in (np.zeros((7, 5)), np.zeros((2, 7, 5, 2)), np.zeros((8, 7, 5, 2)), np.zeros((2, 8, 7, 5, 2)),
                    np.zeros((3, 8, 7, 5, 1)), np.zeros((1, 3, 8, 7, 5, 2))):
            with pytest.raises(ValueError) as err:
                call(bad, x0)
            assert str(bad.shape) in str(err.value) and 'pol' in str(err.value)
        for bad in (np.zeros(3), np.zeros((4, 3)), np.zeros((2, 4, 2)), np.zeros((3, 4, 2, 1)), np.zeros(())):
            with pytest.raises(ValueError) as err:
                call(pol, bad, n_traj=4) if call is both[1] else call(pol, bad)
            assert 'x0' in str(err.value)
        # the steps of the policy
        for kw, text in ((dict(t0=0.5), 'integer'), (dict(t0=-1), 'T_pol = 8'), (dict(t0=1), 'T_pol = 8')):
            with pytest.raises(ValueError) as err:
                call(pol, x0, **kw)
            assert text in str(err.value)
    # w and n_steps of simulate
    for bad in (np.zeros((8, 3)), np.zeros((2, 8, 4)), np.zeros((3, 8, 4, 1))):
        with pytest.raises(ValueError) as err:
            fam.simulate(pol, x0, bad)
        assert 'w must have shape' in str(err.value)
    with pytest.raises(ValueError) as err:
        fam.simulate(pol, x0)
    assert 'stochastic members need' in str(err.value)
    with pytest.raises(ValueError) as err:
        fam.simulate(pol, x0, w, n_steps=9)
    assert 'w holds 8 steps' in str(err.value)
    with pytest.raises(ValueError) as err:
        fam.simulate(pol, x0, w, n_steps=0)
    assert 'n_steps >= 1' in str(err.value)
    # Monte Carlo: steps, burn-in, cuts, seeds, trajectory ids, laws -- as fam.monte_carlo checks them
    with pytest.raises(ValueError) as err:
        fam.monte_carlo_horizon(pol, np.zeros(2), 8)
    assert 'n_traj' in str(err.value)
    for kw in (dict(n_steps=0), dict(n_steps=5, n_burn=5), dict(n_steps=5, n_burn=-1)):
        with pytest.raises(ValueError) as err:
            fam.monte_carlo_horizon(pol, x0, **kw)
        assert 'n_burn' in str(err.value)
    fam.steps_per_launch = 0
    with pytest.raises(ValueError) as err:
        fam.monte_carlo_horizon(pol, x0, 5)
    assert 'steps_per_launch' in str(err.value)
    del fam.steps_per_launch
    for seed in (-1, 1 << 64, (1, 2), (1, 2, -3)):
        with pytest.raises(ValueError) as err:
            fam.monte_carlo_horizon(pol, x0, 5, seed=seed)
        assert 'seed' in str(err.value)
    with pytest.raises(ValueError) as err:
        fam.monte_carlo_horizon(pol, x0, 5, traj_offset=-1)
    assert 'trajectory ids' in str(err.value)
    grid, proba = np.linspace(-1., 1., 5), np.full(5, 0.2)
    with pytest.raises(ValueError) as err:
        fam.monte_carlo_horizon(pol, x0, 5, law=[(grid, proba), (grid[:4], np.full(4, 0.25)), (grid, proba)])
    assert 'member 1' in str(err.value) and '4 points' in str(err.value)
    # deterministic members: Monte Carlo has nothing to draw (the existing message); simulate needs n_steps
    pv = SolverFamily(fh.PV_SIZED.solvers())
    with pytest.raises(NotImplementedError) as err:
        pv.monte_carlo_horizon(np.zeros((3, 6, 9, 1)), np.zeros((3, 4, 1)), 5)
    assert 'deterministic system has nothing to draw' in str(err.value)
    with pytest.raises(ValueError) as err:
        pv.simulate(np.zeros((3, 6, 9, 1)), np.zeros((3, 4, 1)))
    assert 'give n_steps' in str(err.value)
    # data[k] members: an integer time index, also under a stationary policy; a step past the data does not trace
    with pytest.raises(ValueError) as err:
        pv.simulate(np.zeros((3, 9, 1)), np.zeros((3, 4, 1)), n_steps=2, t0=0.5)
    assert 'integer' in str(err.value) and 'data[k]' in str(err.value)
    lookup = SolverFamily(fh.LOOKUP.solvers())                          # (16 entries of data)
    for call in (lambda: lookup.simulate(np.zeros((2, 9, 1)), np.zeros((2, 4, 1)), np.zeros((7, 4)), t0=12),
                 lambda: lookup.monte_carlo_horizon(np.zeros((2, 9, 1)), np.zeros((2, 4, 1)), 7, t0=12)):
        with pytest.raises(NotImplementedError) as err:
            call()
        assert 'member 0 at step 16' in str(err.value) and 'no host path' in str(err.value)
    # fam.monte_carlo still refuses both, and says where to go
    with pytest.raises(NotImplementedError) as err:
        fam.monte_carlo(pol, x0, 5)
    assert 'time-indexed' in str(err.value) and 'monte_carlo_horizon' in str(err.value)
    with pytest.raises(NotImplementedError) as err:
        lookup.monte_carlo(np.zeros((2, 9, 1)), np.zeros((2, 4, 1)), 5)
    assert 'data[k]' in str(err.value) and 'monte_carlo_horizon' in str(err.value)
    assert 'monte_carlo_horizon' in SolverFamily.monte_carlo.__doc__


def test_steps_and_members_of_another_structure_are_named(monkeypatch):
    _no_device(monkeypatch)
    from stodynprog_amd import DPSolver, SysDescription
    from stodynprog_amd.models import NormalLaw

    def switching(sign_at):
        """lookup, but a Python `if` on data[k] picks the expression: the structure changes at step `sign_at`"""
        data = np.where(np.arange(16) < sign_at, 0.5, -0.5) * (1. + 0.01 * np.arange(16))
        sysd = SysDescription((1, 1, 1), stationnary=False, name='switching')
        sysd.dyn = lambda k, x, u, w: ((0.9 * x + u + w + data[k]) if data[k] > 0 else (0.9 * x + (u - abs(x)) + w + data[k]),)
        sysd.cost = lambda k, x, u, w: x * x + 0.25 * u * u
        sysd.control_box = lambda k, x: ((-1., 1.),)
        sysd.perturb_laws = [NormalLaw(0, 0.1)]
        s = DPSolver(sysd)
        s.discretize_state(-2, 2, 9)
        s.discretize_perturb(-0.3, 0.3, 3)
        s.control_steps = (0.125,)
        return s
    fam = SolverFamily([switching(20), switching(5)])                    # (the same structure at step 0)
    pol, x0 = np.zeros((2, 9, 1)), np.zeros((2, 4, 1))
    for call in (lambda: fam.simulate(pol, x0, np.zeros((8, 4))), lambda: fam.monte_carlo_horizon(pol, x0, 8)):
        with pytest.raises(ValueError) as err:
            call()
        assert 'member 1 at step 5' in str(err.value) and 'structure' in str(err.value)
    assert fam._horizon_tables(5, 0)[2]                                 # the steps 0 .. 4 share a structure


@pytest.mark.parametrize('P', (1,) + fh.MAPPING_P)
def test_the_launch_plan_on_256_compute_units(P):
    cus = 256
    for tile, caps, batches in ((fh.SIM_TILE, (cus * 32 // 8,), fh.BATCHES + (fh.B_MAPPING, 4096, fh.sim_cap_batch(cus))),
                                (fh.MC_TILE, tuple(cus * k // 8 for k in range(1, 9)),
                                 fh.BATCHES + (fh.B_MAPPING, 4096, mcc.cap_batch(cus)))):
        for cap in caps:
            for B in batches:
                plan = fh.launch(B, P, cap, tile)
                tiles = -(-B // tile)
                assert plan['tiles'] == tiles
                # every tile of every member exactly once
                seen = sorted((p, t) for xcd in plan['visits'] for p, t, _ in xcd)
                assert seen == [(p, t) for p in range(P) for t in range(tiles)]
                # a member's tiles stay on its XCDs: one XCD with 8 members or more, 8 // P contiguous parts with fewer
                for xcd, visits in enumerate(plan['visits']):
                    for p, t, _ in visits:
                        assert (p % 8 == xcd) if P >= 8 else (p * plan['parts'] <= xcd < (p + 1) * plan['parts'])
                    if P < 8 and visits:
                        ts = [t for _, t, _ in visits]
                        assert ts == list(range(ts[0], ts[0] + len(ts)))
                # the grid: a multiple of 8, at most the cap an XCD
                assert plan['blocks'] % 8 == 0 and 8 <= plan['blocks'] <= 8 * max(1, cap)
                assert plan['per_xcd'] == max(1, min(plan['wanted'], cap))
    if P == 9:
        # the batches of the GPU test are past both caps: a second trip of the stride loop
        B = max(fh.sim_cap_batch(cus), mcc.cap_batch(cus))
        assert fh.sim_cap_batch(cus) % 64 == 1 and 2 * (-(-fh.sim_cap_batch(cus) // 64)) > cus * 32 // 8
        assert max(trip for _, _, trip in fh.launch(B, 9, cus * 32 // 8, fh.SIM_TILE)['visits'][0]) >= 1
        for per_cu in range(1, 9):
            plan = fh.launch(B, 9, cus * per_cu // 8, fh.MC_TILE)
            assert 9 * plan['tiles'] > 8 * cus and max(trip for xcd in plan['visits'] for _, _, trip in xcd) >= 1


# ----------------------------------------------------------------------------------------------------------------------
# the inputs of the GPU tests, by the definition of the draws and the host loop

def test_the_step_policies_are_pairwise_different():
    for hz in fh.FAMILIES:
        pol = fh.policies(hz)
        assert pol.shape[:2] == (len(hz.case.members), hz.T_pol) and hz.t0 + hz.n_steps <= hz.T_pol
        flat = pol.reshape(pol.shape[0] * pol.shape[1], -1)
        assert len({row.tobytes() for row in flat}) == flat.shape[0], hz   # (every member, every step)


def test_the_outside_case_has_a_member_inside_and_a_member_outside():
    hz = fh.OUTSIDE
    pol, x0 = fh.policies(hz), mcc.outside_starts()
    counts = [mcc.host_run(s, pol[p], x0, hz.n_steps, 2, 3)[1] for p, s in enumerate(hz.solvers())]
    print('n_outside per member:', [int(c.sum()) for c in counts])
    assert counts[0].sum() == 0 and counts[1].sum() > 0


def test_the_laws_reach_every_branch_of_the_index():
    fam = SolverFamily(fh.AR1_64.solvers())
    idx, _ = fam.monte_carlo_draws(11, 65, fh.T, law=mcc.long_law())
    assert len(mcc.long_law()[0]) == 70 and (idx < 64).any() and (idx > 64).any()
    idx, _ = fam.monte_carlo_draws(11, 65, fh.T, law=mcc.member_laws())
    assert all(len(np.unique(i)) >= 5 for i in idx)


def test_the_cuts_of_the_gpu_test():
    hz = fh.CUTS
    fam = SolverFamily(hz.solvers())
    pol_d, _ = fam._horizon_policy(fh.policies(hz), hz.n_steps, 0)
    tabs, table, _ = fam._horizon_tables(hz.n_steps, 0)
    assert fam.horizon_chunk_bytes == SolverFamily.horizon_chunk_bytes == type(fam.solvers[0]).horizon_chunk_bytes
    assert fam._horizon_bytes(pol_d, table) == (8 * 2 * 35 + 5) * 8
    extra = fam._mc_member_bytes(70, 3, True) + fam._horizon_bytes(pol_d, table) - 2 * 35 * 8
    fam.chunk_bytes = fh.member_chunk_bytes(fam, extra, 3)
    assert fam._chunks(tabs, extra) == [(0, 3), (3, 5)]


def test_the_build_compiles_the_units_of_the_gpu_tests():
    units = fh.unit_sources()
    for hz in fh.FAMILIES:
        fam, tabs, source = _unit(hz)
        assert tabs['source'] in units and source in units, hz
    with open(os.path.join(ROOT, '__graft_entry__.py')) as f:
        assert 'family_horizon_cases.unit_sources()' in f.read()


def test_the_timing_tool_and_the_example_run_units_the_build_compiles():
    """tools/family_horizon_times.py and examples/sizing_pv_storage.py (64 capacities of models.pv_storage and of
    storage-AR1) need no unit of their own: every source they run is on record as one the build compiles"""
    from stodynprog_amd import models
    digest = lambda text: hashlib.sha256(text.encode('utf-8')).hexdigest()[:16]
    table = _digests()
    for solvers, steps in (([models.pv_storage(E_rated=float(E))[1] for E in np.linspace(1., 4., 64)], (0, 23, 47)),
                           ([models.storage_ar1(E_rated=float(E), steps=(0.1, 0.1))[1] for E in np.linspace(2., 20., 64)], (None,))):
        fam = SolverFamily(solvers)
        sources = {fam._tables(t)['source'] for t in steps}
        sources.add(codegen.family_horizon_unit(fam._tables(steps[0])['model'], fam.dtype))
        sources |= {s._kernel_plan(steps[0], s._trace_now(steps[0]))['source'] for s in solvers}
        assert all(digest(src) in table for src in sources), sorted(digest(src) for src in sources if digest(src) not in table)
