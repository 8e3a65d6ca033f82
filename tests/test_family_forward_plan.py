"""Transition operators of families on the CPU (tests/family_forward_cases.py): what `SolverFamily.transition_operator`,
`stationary_distribution` and the operator refuse, before a device is touched; the chunk arithmetic; the recorded stop
counts against forward.stationary; `forward.FamilyStationary` in numpy alone; the generated transition unit (lifted
constants, its marks and header, one kernel, no scratch memory, no spilled vector register, no LDS); the launch geometry
restated in the case file against the constants of the header and the library; and the properties of the cases the GPU
tests rely on, by the definition.  No GPU."""
import os
import re

import numpy as np
import pytest

import family_cases as fc
import family_forward_cases as ffc
from test_family_plan import _kernels, ROOT
from stodynprog_amd import SolverFamily, DPSolver, FamilyTransitionOperator, codegen, forward, models, _native as nat
from stodynprog_amd.family import _trace_member


def _ar1():
    return SolverFamily([make() for make in ffc.BY_NAME['storage_ar1 f64'].members])


def _no_device(monkeypatch):
    monkeypatch.setattr(nat, 'require_gpu', lambda *a, **k: pytest.fail('a device was asked for'))
    monkeypatch.setattr(nat, 'lib', lambda *a, **k: pytest.fail('the library was asked for'))
    monkeypatch.setattr(nat, 'compile_model', lambda *a, **k: pytest.fail('the compiler was asked for'))


def test_refusals_come_before_a_device_is_touched(monkeypatch):
    _no_device(monkeypatch)
    fam = _ar1()
    pol = np.zeros((3, 7, 5, 2))
    # a wrong policy shape: both accepted shapes and the number of members are named
    for bad in (np.zeros((7, 5)), np.zeros((2, 7, 5, 2)), np.zeros((3, 7, 5, 1)), np.zeros((3, 7, 4, 2)), np.zeros((1, 3, 7, 5, 2))):
        for call in (fam.transition_operator, fam.stationary_distribution):
            with pytest.raises(ValueError) as err:
                call(bad)
            assert str(bad.shape) in str(err.value) and '(3, 7, 5, 2)' in str(err.value) and 'all 3 members' in str(err.value)
    # a member whose operator is past the cap, with the solo wording
    S, nnz, nbytes = fam._transition_size()
    assert (S, nnz, nbytes) == (35, 35 * 3 * 4, 35 * 3 * 4 * 12 + 8 * 36) == fam.solvers[1]._transition_size()
    fam.solvers[1].TRANSITION_MAX_BYTES = nbytes - 1
    with pytest.raises(ValueError) as err:
        fam.transition_operator(pol)
    assert str(err.value) == ('member 1: the transition operator of this grid has nnz = {} entries and takes {} bytes: more than '
                              'DPSolver.TRANSITION_MAX_BYTES = {} bytes'.format(nnz, nbytes, nbytes - 1))
    solo = fam.solvers[1]
    monkeypatch.setattr(solo, '_check_supported', lambda: None)
    with pytest.raises(ValueError) as one:
        solo.transition_operator(pol[1])
    assert str(err.value) == 'member 1: ' + str(one.value)
    del fam.solvers[1].TRANSITION_MAX_BYTES
    # .. or past 2**32 - 1 entries whatever the cap
    big = fam.solvers[2]
    monkeypatch.setattr(big, '_transition_size', lambda: (1 << 28, 1 << 32, 5 << 30))
    big.TRANSITION_MAX_BYTES = 6 << 30
    with pytest.raises(ValueError) as err:
        fam.transition_operator(pol)
    assert str(err.value).startswith('member 2: the transition operator of this grid has nnz = 4294967296 entries')
    assert '32-bit words, at most 2**32 - 1 entries whatever the cap' in str(err.value)
    # what the solo `stationary` refuses
    fam = _ar1()
    for kw, text in ((dict(tol=-1.), 'tol'), (dict(tol=float('nan')), 'tol'), (dict(check_every=0), 'check_every'),
                     (dict(n_max=0), 'n_max must be at least 1')):
        with pytest.raises(ValueError) as err:
            fam.stationary_distribution(pol, **kw)
        assert text in str(err.value), kw
        with pytest.raises(ValueError) as one:
            forward.stationary((np.zeros(2, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0)), **kw)
        assert str(err.value) == str(one.value), kw
    # a wrong start vector, and an argument `stationary` does not have
    for bad in (np.zeros((7,)), np.zeros((2, 7, 5)), np.zeros((3, 5, 7))):
        with pytest.raises(ValueError) as err:
            fam.stationary_distribution(pol, mu0=bad)
        assert str(bad.shape) in str(err.value) and 'all 3 members' in str(err.value)
    with pytest.raises(TypeError):
        fam.stationary_distribution(pol, n_iter=3)


def test_the_operator_refuses_before_it_calls_the_library(monkeypatch):
    """an operator object on handles that are never used: shapes, counts and tolerances are checked in Python"""
    calls = []

    class Lib(object):
        def __getattr__(self, name):
            def call(*args):
                calls.append(name)
                return 0
            return call
    monkeypatch.setattr(nat, 'lib', lambda: Lib())
    op = FamilyTransitionOperator([(0, 2, None), (2, 3, None)], (7, 5), np.float64, 35 * 12)
    assert op.P == 3 and op.nnz == 3 * 35 * 12 and op.info['chunks'] == 2 and op.info['members'] == 3
    assert op.nbytes == op.info['bytes'] == forward.operator_bytes(2 * 420, 70, 8) + forward.operator_bytes(420, 35, 8)
    del calls[:]
    for bad in (np.zeros(35), np.zeros((2, 7, 5)), np.zeros((3, 35))):
        for call in (op.push, lambda mu: op.stationary(mu0=mu)):
            with pytest.raises(ValueError) as err:
                call(bad)
            assert str(bad.shape) in str(err.value) and '(3, 7, 5)' in str(err.value)
    with pytest.raises(ValueError):
        op.push(np.zeros((7, 5)), -1)
    for kw in (dict(tol=-1.), dict(check_every=0), dict(n_max=0)):
        with pytest.raises(ValueError):
            op.stationary(**kw)
    with pytest.raises(IndexError):
        op.tocsr(3)
    assert calls == []
    op.close()
    assert calls == ['sdp_transop_destroy'] * 2
    with pytest.raises(ValueError, match='closed'):
        op.push(np.zeros((7, 5)))


def test_the_chunk_arithmetic():
    fam = SolverFamily([make() for make in ffc.CHUNKS.members])
    tabs = fam._tables()
    S, nnz, nbytes = fam._transition_size()
    rs = 8
    # the operator, the entries in emission order, the sort's temporaries, the histogram, policy + mean cost + two vectors
    extra = fam._transition_bytes()
    assert extra == nbytes + nnz * (4 + rs) + nnz * 24 + 8 * (S + 1) + S * rs * (2 + 3) + 32
    assert fam._chunks(tabs, extra, fam._transition_most()) == [(0, 5)]
    fam.chunk_bytes = ffc.chunk_bytes_for(fam, 2)
    assert fam._chunks(tabs, extra, fam._transition_most()) == [(0, 2), (2, 4), (4, 5)]
    assert fam._chunks(tabs, extra, 1) == [(p, p + 1) for p in range(5)]
    assert fam._chunks(tabs) == fam._chunks(tabs, 0, None)                 # (the other calls' chunks are what they were)
    # a chunk stays below 2**32 entries, 2**31 rows and 65535 members
    assert fam._transition_most() == min((2 ** 32 - 1) // nnz, (2 ** 31 - 1) // S, 65535) == 65535
    for dims, W, most in (((1 << 20,), 1023, (2 ** 32 - 1) // ((1 << 20) * 1023 * 2)), ((70000,), 1, (2 ** 31 - 1) // 70000),
                          ((1 << 15, 1 << 15), 1, 1)):
        fam.dims, fam.W = dims, W
        assert fam._transition_most() == most, dims
        assert most * int(np.prod(dims)) < 2 ** 31 and most * int(np.prod(dims)) * W * (1 << len(dims)) < 2 ** 32 or most == 1


def test_the_recorded_stop_counts_are_the_definitions():
    solvers, pol, ref = ffc.reference('shrink', None)
    assert len(ref) == 16 and pol.shape == (16, 10, 1)
    pushes, capped = [], []
    for e, csr in ref:
        r = forward.stationary(csr, e.mean_cost, tol=ffc.SHRINK['tol'], check_every=ffc.SHRINK['check_every'], n_max=ffc.SHRINK['n_max'])
        # (no push renormalises: a push moves the total by a rounding of it at most, so by eps a push; the largest is 6 ulp)
        assert r.converged and abs(float(r.mass) - 1.) <= r.n_done * np.finfo(float).eps
        pushes.append(r.n_done)
        capped.append(forward.stationary(csr, e.mean_cost, **ffc.SHRINK_CAPPED))
    assert pushes == ffc.SHRINK_PUSHES
    assert sorted((n, pushes.count(n)) for n in set(pushes)) == [(18, 6), (20, 5), (21, 5)]
    assert fc.list_sizes(pushes, ffc.SHRINK['n_max']) == ffc.SHRINK_SIZES == [16, 10, 5, 0]
    # capped below the slowest member's count, a check every third push: the members of 18 stop converged at the check of
    # push 18, the others at the cap with the delta of that last check
    n_max = ffc.SHRINK_CAPPED['n_max']
    assert max(pushes) > n_max and n_max % ffc.SHRINK_CAPPED['check_every'] != 0
    for n, r in zip(pushes, capped):
        assert r.n_done == min(n, n_max) and r.converged == (n < n_max)
        assert (r.delta <= ffc.SHRINK_CAPPED['tol']) == (n < n_max) and r.delta == r.delta


def test_family_stationary_in_numpy_alone():
    rng = np.random.default_rng(5)
    mu = rng.uniform(size=(3, 4, 5)).astype(np.float32)
    gbar = rng.uniform(size=(3, 4, 5)).astype(np.float32)
    n_done, delta = np.array([7, 9, 12], dtype=np.int32), np.array([1e-9, 1e-7, np.nan])
    res = forward.FamilyStationary(mu, n_done, delta, 1e-8, gbar)
    assert len(res) == 3 and res.mu is mu and res.n_done.tolist() == [7, 9, 12] and res.converged.tolist() == [True, False, False]
    assert res.mass.dtype == np.float32 and res.average_cost.dtype == np.float64 and res.delta.dtype == np.float64
    for p in range(3):
        one, ref = res[p], forward.finish(mu[p], n_done[p], delta[p], 1e-8, gbar[p])
        assert isinstance(one, forward.Stationary) and one.mu.shape == (4, 5) and np.array_equal(one.mu, ref.mu)
        assert (one.n_done, one.converged, one.average_cost, one.mass) == (ref.n_done, ref.converged, ref.average_cost, ref.mass)
        assert one.average_cost == res.average_cost[p] and one.mass == res.mass[p] and one.converged == res.converged[p]
        assert (one.delta == res.delta[p]) or (one.delta != one.delta and np.isnan(res.delta[p]))
    bare = forward.FamilyStationary(mu, n_done, delta, 1e-8)
    assert bare[1].average_cost is None and np.all(np.isnan(bare.average_cost))
    assert 'FamilyStationary(3 members' in repr(res)


UNITS = [(ffc.BY_NAME[name], t_k) for name, t_k in (('inventory P=3', None), ('storage_ar1 f64', None), ('storage_ar1 f32', None),
                                                    ('three_d', None), ('four_d', None), ('finite_horizon', 3),
                                                    ('pv_sized', 1), ('nan', None))]


@pytest.mark.parametrize('case,t_k', UNITS, ids=[c.name for c, _ in UNITS])
def test_the_unit_compiles_with_its_one_kernel(case, t_k, tmp_path):
    fam = SolverFamily(case.solvers())
    tabs = fam._tables(t_k)
    source = codegen.family_trans_unit(tabs['model'], fam.dtype)
    assert '#define SDP_FAMILY 1' in source and '#define SDP_FAMILY_TRANS 1' in source and '#define SDP_LANES 1\n' in source
    assert '#include "sdp_family_trans_kernel.h"' in source and 'sdp_model_cell_at(' in source          # lifted constants
    assert '#define SDP_NPARAMS {}\n'.format(tabs['prm'].shape[1]) in source and tabs['prm'].shape[1] >= 1
    assert '#include "sdp_family_kernel.h"' not in source and '#include "sdp_sweep_kernel.h"' not in source
    for other in ('SDP_FAMILY_POLICY', 'SDP_FAMILY_MC', 'SDP_FAMILY_HORIZON', 'SDP_FAMILY_LOOKAHEAD'):
        assert other not in source
    kernels = _kernels(source, tmp_path)
    assert sorted(kernels) == ['sdp_family_transitions'], sorted(kernels)
    f = kernels['sdp_family_transitions']
    print(case, {n: f[n] for n in ('.vgpr_count', '.sgpr_count', '.private_segment_fixed_size', '.vgpr_spill_count',
                                   '.sgpr_spill_count', '.group_segment_fixed_size', '.max_flat_workgroup_size')})
    assert f['.private_segment_fixed_size'] == 0 and f['.vgpr_spill_count'] == 0, f
    assert f['.group_segment_fixed_size'] == 0, f                        # no LDS
    assert f['.max_flat_workgroup_size'] == ffc.THREADS == codegen.FAMILY_TRANS_THREADS == 256
    assert f['.vgpr_count'] <= 128, f                                    # four waves a SIMD or more (the 4-D unit: 74 registers)
    # one unit per model structure and real type: the other units of the family have other keys
    others = [tabs['source'], codegen.family_policy_unit(tabs['model'], fam.dtype)]
    assert len({codegen.source_key(s) for s in others + [source]}) == 3


def test_the_unit_is_one_per_structure_and_its_key_covers_its_header(monkeypatch, tmp_path):
    fam = _ar1()
    tabs = fam._tables()
    source = codegen.family_trans_unit(tabs['model'], fam.dtype)
    one = SolverFamily([ffc.BY_NAME['storage_ar1 f64'].members[1]()])
    assert codegen.family_trans_unit(one._tables()['model'], one.dtype) == source
    assert codegen.family_trans_unit(tabs['model'], np.float32) != source
    assert 'sdp_family_trans_kernel.h' not in codegen._HEADERS
    keys = codegen.source_key(source), codegen.source_key(tabs['source'])
    csrc = tmp_path / 'csrc'
    csrc.mkdir()
    for fn in os.listdir(codegen.CSRC):
        if fn.endswith('.h'):
            (csrc / fn).write_bytes(open(os.path.join(codegen.CSRC, fn), 'rb').read())
    monkeypatch.setattr(codegen, 'CSRC', str(csrc))
    codegen._digest_cache.clear()
    now = lambda: (codegen.source_key(source), codegen.source_key(tabs['source']))
    assert now() == keys
    with open(str(csrc / 'sdp_family_trans_kernel.h'), 'a') as f:
        f.write('// edited\n')
    assert now()[0] != keys[0] and now()[1] == keys[1]
    mine = now()[0]
    with open(str(csrc / 'sdp_family_kernel.h'), 'a') as f:
        f.write('// edited\n')
    assert now()[0] != mine
    codegen._digest_cache.clear()
    # a model that was not lifted, and models with several perturbation variables
    plain = _trace_member(fam.solvers[0])
    plain.param_index = None
    with pytest.raises(ValueError, match='lifted constants'):
        codegen.family_trans_unit(plain, np.float64)
    two = models.two_inflows(n_a=4, n_b=3, n_y=3, n_w=(3, 2))[1]
    model = two._trace_now(None)
    model.lift_constants()
    assert model.n_perturb == 2
    with pytest.raises(NotImplementedError, match='one perturbation variable at most'):
        codegen.family_trans_unit(model, np.float64)
    with pytest.raises(NotImplementedError, match='perturbation variables'):
        SolverFamily([two])


def test_the_launch_geometry_restated():
    read = lambda *path: open(os.path.join(*path)).read()
    header = read(codegen.CSRC, 'sdp_family_trans_kernel.h')
    args = read(codegen.CSRC, 'sdp_kernel_args.h')
    library = read(codegen.CSRC, 'sdp_hip.hip')
    sweep = read(codegen.CSRC, 'sdp_family_kernel.h')
    assert '#define SDP_FTRANS_THREADS {}\n'.format(ffc.THREADS) in header
    assert '#define SDP_FTRANS_TILE (SDP_FTRANS_THREADS >> SDP_D)' in header and '#define SDP_FTRANS_V (1 << SDP_D)' in header
    assert [ffc.tile(d) for d in (1, 2, 3, 4)] == [128, 64, 32, 16] == [codegen.family_trans_tile(d) for d in (1, 2, 3, 4)]
    assert 'SDP_META_F_FAMILY_TRANS = 32768' in args and 'struct SdpFamilyTransArgs {' in args
    assert 'SDP_META_F_FAMILY | SDP_META_F_FAMILY_TRANS, 0, 0, SDP_FTRANS_THREADS, SDP_FTRANS_TILE' in header
    assert '!defined(SDP_FAMILY_TRANS)' in sweep                           # (the unit does not carry sdp_family_sweep)
    assert '__shared__' not in header and '__shfl' not in header and '__syncthreads' not in header
    # the flat walk: unit = p tiles + tile, a workgroup strides over the units; the host's grid
    for line in ('const int64_t units = (int64_t)a.n_active * tiles;', 'const int64_t p = unit / tiles;',
                 'for (int64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {'):
        assert line in header, line
    for line in ('int64_t blocks = P * tiles;', 'if (blocks > (int64_t)f->cus * 8) blocks = (int64_t)f->cus * 8;',
                 'const int64_t tiles = (S + f->trans_tile - 1) / f->trans_tile;',
                 '!(m[SDP_META_FLAGS] & SDP_META_F_FAMILY_TRANS)', 'm[SDP_META_COL_ROWS] != (256 >> f->d)',
                 '#define SDP_PUSH_LONG {}\n'.format(ffc.PUSH_LONG), '#define SDP_PUSH_WIDE {}\n'.format(ffc.PUSH_WIDE),
                 'if (bx > {}) bx = {};'.format(ffc.REDUCTION_BLOCKS, ffc.REDUCTION_BLOCKS),
                 'if (MEMBERS && !flags[(int32_t)t / Sm]) continue;', 'if (MEMBERS && live) live = flags[t / Sm] != 0;'):
        assert line in library, line
    # the case past the caps, on the 256 compute units it is sized for
    for name, (wanted, cap) in ffc.caps(2, ffc.LONG_NX, 1, 256).items():
        assert wanted > cap, (name, wanted, cap)
    # the ABI: header, library and binding move together
    abi = read(ROOT, 'include', 'sdp_hip.h')
    real_lib = nat.lib()
    for name in ('sdp_family_load_trans_unit', 'sdp_family_transop_create', 'sdp_transop_push_until_members'):
        assert re.search(r'^int {}\('.format(name), abi, re.M) and 'extern "C" int {}('.format(name) in library
        assert name in nat.EXPORTS and hasattr(real_lib, name)
    assert real_lib.sdp_family_load_trans_unit(None, None) == -1
    assert real_lib.sdp_family_transop_create(None, None, 0., None) == -1
    assert real_lib.sdp_transop_push_until_members(None, 1, 1, 0., None, None) == -1


def test_the_cases_have_the_properties_the_gpu_tests_rely_on():
    rows = lambda ref: [np.diff(csr[0]) for _, csr in ref]
    # inventory: empty rows, lane rows and rows of k_push_group<16>; two identical members under different policies
    solvers, pol, ref = ffc.reference('inventory P=3', None)
    lengths = np.concatenate(rows(ref))
    assert lengths.min() == 0 and (lengths[lengths > 0] < ffc.PUSH_LONG).any()
    assert ((lengths >= ffc.PUSH_LONG) & (lengths < ffc.PUSH_WIDE)).any() and lengths.max() < ffc.PUSH_WIDE
    assert not np.array_equal(pol[0], pol[2]) and not np.array_equal(ref[0][0].val, ref[2][0].val)
    # policies differ per member and lie off every lattice
    for case in ffc.CASES:
        pol = ffc.reference(case.name, case.times[0])[1]
        assert pol.dtype == case.dtype and all(not np.array_equal(pol[0], pol[p]) for p in range(1, len(pol))), case
    # storage_ar1: the AR(1) axis leaves the grid, weights go negative
    assert any((e.val < 0).any() for e, _ in ffc.reference('storage_ar1 f64', None)[2])
    # the deterministic data[k] case: W = 1, another row of constants per member and per step
    fam = SolverFamily(ffc.BY_NAME['pv_sized'].solvers())
    assert fam.W == 0 and ffc.reference('pv_sized', 1)[2][0][0].W == 1
    t1, t3 = fam._tables(1), fam._tables(3)
    assert t1['time_specialized'] and not np.array_equal(t1['prm'], t3['prm']) and not np.array_equal(t1['prm'][0], t1['prm'][1])
    assert not SolverFamily(ffc.BY_NAME['finite_horizon'].solvers())._tables(3)['time_specialized']
    # nan: NaN next states in member 0 alone; they propagate there
    ref = ffc.reference('nan', None)[2]
    assert np.isnan(ref[0][0].val).any() and np.isnan(ref[0][0].mean_cost).sum() == 2 and not np.isnan(ref[1][0].val).any()
    assert np.isnan(forward.push(ref[0][1], np.full(7, 1. / 7))).any()
    # wide: rows of k_push_group<64> in member 0, which stops first; every row of member 1 on the lane path
    ref = ffc.reference('wide', None)[2]
    wide, short = rows(ref)
    assert wide.max() >= ffc.PUSH_WIDE and (wide >= ffc.PUSH_WIDE).sum() >= 1 and short.max() < ffc.PUSH_LONG
    stat = ffc.BY_NAME['wide'].stat
    first, second = (forward.stationary(csr, e.mean_cost, **stat) for e, csr in ref)
    assert first.converged and first.n_done < second.n_done == stat['n_max'] and not second.converged
    # tiles: one ragged tile, two tiles with the second ragged, seven tiles
    tiles = lambda name: -(-int(np.prod(ffc.BY_NAME[name].solvers()[0]._shape())) // ffc.tile(len(ffc.BY_NAME[name].solvers()[0]._shape())))
    assert [tiles(n) for n in ('inventory P=3', 'storage_ar1 f64', 'three_d', 'four_d')] == [1, 1, 2, 7]
    assert ffc.BY_NAME['three_d'].solvers()[0]._shape() == (5, 4, 3) and ffc.BY_NAME['four_d'].solvers()[0]._shape() == (4, 3, 3, 3)


def test_the_build_compiles_the_units_of_the_gpu_tests():
    units = ffc.unit_sources()
    for case in ffc.CASES + [ffc.CHUNKS, ffc.SHRINK_CASE]:
        fam = SolverFamily(case.solvers())
        for t_k in case.times:
            tabs = fam._tables(t_k)
            assert tabs['source'] in units and codegen.family_trans_unit(tabs['model'], fam.dtype) in units, case
    with open(os.path.join(ROOT, '__graft_entry__.py')) as f:
        assert 'family_forward_cases.unit_sources()' in f.read()
