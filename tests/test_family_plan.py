"""Families of same-shaped problems on the CPU (tests/family_cases.py): every case's unit cross-compiles for gfx950
with kernel sdp_family_sweep free of scratch memory, vector spills and LDS; row p of every table the device gets is
member p's own; what a family refuses it refuses before a device is touched; no other unit changes its generated
text; and the members of the `tol` case need different numbers of sweeps.  No GPU."""
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

import family_cases as fc
from oracle import vi_numpy
from stodynprog_amd import SolverFamily, DPSolver, SysDescription, codegen, models, convergence as conv, _native as nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM_BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(nat.HIPCC))), 'llvm', 'bin')
TARGET = 'hipv4-amdgcn-amd-amdhsa--gfx950'


def _kernels(source, tmp_path):
    """{kernel name: integer fields of its code-object notes} (tests/test_lookahead_plan.py reads them the same way)"""
    bundle, elf = nat.compile_model(source), str(tmp_path / 'unit.elf')
    subprocess.run([os.path.join(LLVM_BIN, 'clang-offload-bundler'), '--unbundle', '--type=o', '--targets=' + TARGET,
                    '--input=' + bundle, '--output=' + elf], check=True, capture_output=True)
    notes = subprocess.run([os.path.join(LLVM_BIN, 'llvm-readelf'), '--notes', elf], check=True,
                           capture_output=True, text=True).stdout
    out = {}
    for block in notes.split('  - .agpr_count')[1:]:
        name = re.search(r'^\s+\.name:\s+(\w+)\s*$', block, re.M).group(1)
        out[name] = {k: int(v) for k, v in re.findall(r'^\s+(\.[a-z_]+):\s+(\d+)\s*$', block, re.M)}
    return out


def _steps(case):
    return [None] if case.horizon is None else list(range(case.horizon))


@pytest.mark.parametrize('case', fc.CASES, ids=repr)
def test_unit_compiles_without_scratch_spills_or_lds(case, tmp_path):
    fam = SolverFamily(case.solvers())
    seen = set()
    for t_k in _steps(case):
        tabs = fam._tables(t_k)
        source = tabs['source']
        if source in seen:
            continue
        seen.add(source)
        assert '#define SDP_FAMILY 1' in source and '#include "sdp_family_kernel.h"' in source
        assert 'sdp_model_cell_at(' in source and '#include "sdp_sweep_kernel.h"' not in source
        box_t = None if fam.stationnary else t_k
        assert '#define SDP_LANES {}\n'.format(max(s._box_plan(box_t)['lanes'] for s in fam.solvers)) in source
        kernels = _kernels(source, tmp_path)
        assert sorted(kernels) == ['sdp_family_sweep'], sorted(kernels)
        f = kernels['sdp_family_sweep']
        print(case, t_k, {n: f[n] for n in ('.vgpr_count', '.sgpr_count', '.private_segment_fixed_size',
                                            '.vgpr_spill_count', '.sgpr_spill_count', '.group_segment_fixed_size')})
        assert f['.private_segment_fixed_size'] == 0 and f['.vgpr_spill_count'] == 0, f
        assert f['.group_segment_fixed_size'] == 0, f
        assert f['.max_flat_workgroup_size'] == 256


def _bits(a, dt):
    a = np.ascontiguousarray(a, dtype=dt)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


@pytest.mark.parametrize('case', fc.CASES, ids=repr)
def test_row_p_of_every_table_is_member_p(case):
    fam = SolverFamily(case.solvers())
    twins = case.solvers()
    dt = case.dtype
    for t_k in _steps(case):
        tabs = fam._tables(t_k)
        S = int(np.prod(fam.dims))
        tables = [s._box_table(None if s.sys.stationnary else t_k) for s in twins]
        per_node = any(not (np.all(lo == lo[:, :1]) and np.all(hi == hi[:, :1]) and np.all(n == n[:, :1]))
                       for lo, hi, n in tables)
        assert tabs['per_node'] == per_node
        assert tabs['prm'].dtype == dt and tabs['axes'].dtype == dt and tabs['n'].dtype == np.int32
        for p, s in enumerate(twins):
            model = s._trace_now(t_k)
            assert np.array_equal(_bits(tabs['prm'][p], dt), _bits(model.param_values(), dt))
            assert np.array_equal(_bits(tabs['axes'][p], dt), _bits(np.concatenate(s.state_grid), dt))
            if fam.W:
                assert np.array_equal(_bits(tabs['wgrid'][p], dt), _bits(s.perturb_grid[0], dt))
                assert np.array_equal(_bits(tabs['proba'][p], dt), _bits(s.perturb_proba[0], dt))
            else:
                assert tabs['wgrid'] is None and tabs['proba'] is None
            lo, hi, n = tables[p]
            cols = S if per_node else 1
            assert tabs['lo'][p].shape == (fam.nu, cols)
            assert np.array_equal(_bits(tabs['lo'][p], dt), _bits(np.broadcast_to(lo[:, :cols] if lo.shape[1] >= cols else lo, (fam.nu, cols)), dt))
            assert np.array_equal(_bits(tabs['hi'][p], dt), _bits(np.broadcast_to(hi[:, :cols] if hi.shape[1] >= cols else hi, (fam.nu, cols)), dt))
            assert np.array_equal(tabs['n'][p], np.broadcast_to(n[:, :cols] if n.shape[1] >= cols else n, (fam.nu, cols)))


def test_shapes_the_cases_are_for():
    lanes = {}
    for case in fc.CASES:
        fam = SolverFamily(case.solvers())
        lanes[case.name] = [[s._box_plan(None if fam.stationnary else t)['lanes'] for s in fam.solvers] for t in _steps(case)]
    assert lanes['storage_ar1 f64'] == [[8, 8, 16]]                     # lattice sizes differ by member
    assert lanes['three_d'] == [[64, 64]]
    assert len({max(row) for row in lanes['finite_horizon']}) > 1        # the unit changes along the horizon
    ar1 = SolverFamily(fc.STATIONARY[2].solvers())
    assert ar1.dims == (7, 5) and all(35 % (64 // L) for L in (1, 2, 4, 8, 16, 32))
    assert ar1._tables()['per_node']
    n = ar1._tables()['n']
    assert len(np.unique(n[:, 0].prod(axis=0))) > 1 or len(np.unique(n[0, 0])) > 1
    three = SolverFamily(fc.STATIONARY[4].solvers())
    assert three.dims == (5, 4, 3) and int(three._tables()['n'][0].prod()) == 81
    fam = SolverFamily(fc.CHUNKS.solvers())
    fam.chunk_bytes = fc.chunk_bytes_for(fam, 2)
    assert fam._chunks(fam._tables()) == [(0, 2), (2, 4), (4, 5)]
    assert SolverFamily.chunk_bytes == DPSolver.horizon_chunk_bytes == 256 << 20
    fam.chunk_bytes = 1
    assert fam._chunks(fam._tables()) == [(p, p + 1) for p in range(5)]     # a member larger than the chunk runs alone


# ----------------------------------------------------------------------------------------------------------------------
# refusals

class _Ranks(object):
    nranks = 2
    is_device = True


def _five_states():
    sysd = SysDescription((5, 1, 0), name='five')
    sysd.dyn = lambda a, b, c, d, e, u: (a + u, b, c, d, e)
    sysd.cost = lambda a, b, c, d, e, u: u * u + a
    sysd.control_box = lambda a, b, c, d, e: ((0., 1.),)
    s = DPSolver(sysd)
    s.discretize_state(*([0., 1., 2] * 5))
    return s


def _untraceable():
    _, s = models.inventory()
    s.sys.dyn = lambda x, u, w: (np.sort(np.atleast_1d(x + u - w))[0],)         # (no traced counterpart)
    return s


def test_refusals_come_before_a_device_is_touched(monkeypatch):
    monkeypatch.setattr(nat, 'require_gpu', lambda *a, **k: pytest.fail('a device was asked for'))
    monkeypatch.setattr(nat, 'lib', lambda *a, **k: pytest.fail('the library was asked for'))
    inv = lambda: fc.INVENTORY[0]()
    with pytest.raises(ValueError):
        SolverFamily([])
    # members that do not agree: the first one that differs, and what differs
    other_dims = inv()
    other_dims.discretize_state(-3, 6, 12)
    for bad, what in ((other_dims, 'dims'), (fc.as_dtype(inv(), np.float32), 'dtype'),
                      (fc.storage_ar1(2, 4, 0.8)(), 'dims'), (fc.finite_horizon(0.9, 0.05, 0.1, 0.2, 0.5)(), 'dims')):
        with pytest.raises(ValueError) as err:
            SolverFamily([inv(), inv(), bad, bad])
        assert 'member 2' in str(err.value) and what in str(err.value), str(err.value)
    other_w = inv()
    other_w.perturb_grid, other_w.perturb_proba = [np.arange(3.)], [np.array([0.2, 0.5, 0.3])]
    with pytest.raises(ValueError) as err:
        SolverFamily([inv(), other_w])
    assert 'member 1' in str(err.value) and 'perturbation points' in str(err.value)
    fh9 = fc.finite_horizon(0.9, 0.05, 0.1, 0.2, 0.5)()
    st9 = fc.inventory(0.5, 3, 1)()
    st9.discretize_state(-2, 2, 9)
    with pytest.raises(ValueError) as err:
        SolverFamily([fh9, st9])
    assert 'stationnary' in str(err.value)
    two_controls = fc.storage_ar1(2, 4, 0.8)()
    one_control = models.nas_demo(n_E=7, n_P=5, n_w=3)[1]
    with pytest.raises(ValueError) as err:
        SolverFamily([two_controls, one_control])
    assert 'number of controls' in str(err.value)
    # another structure: a different model, and constants that coincide in one member
    with pytest.raises(ValueError) as err:
        SolverFamily([fc.INVENTORY[0](), fc.INVENTORY[1](), fc.COINCIDING()])
    assert 'constants that coincide in member 2' in str(err.value), str(err.value)
    with pytest.raises(ValueError) as err:
        SolverFamily([fc.COINCIDING(), fc.INVENTORY[1]()])
    assert 'member 1' in str(err.value) and 'constants that coincide in member 0' in str(err.value)
    with pytest.raises(ValueError) as err:
        other = inv()
        other.sys.cost = lambda x, u, w: np.where(x > 0, x * 0.5, -x * 3.) + u * 1. + 0.25 * u * u
        SolverFamily([inv(), other])
    assert 'member 1' in str(err.value) and 'structure' in str(err.value)
    assert SolverFamily([fc.COINCIDING()]).P == 1                      # (alone it is a family like any other)
    # what no family runs
    with pytest.raises(NotImplementedError) as err:
        SolverFamily([inv(), _untraceable()])
    assert 'member 1' in str(err.value) and 'trace' in str(err.value)
    with pytest.raises(NotImplementedError) as err:
        SolverFamily([models.two_inflows(n_a=4, n_b=4, n_y=3, n_w=(2, 2))[1]])
    assert 'perturbation variables' in str(err.value)
    ranked = inv()
    ranked.comm = _Ranks()
    with pytest.raises(NotImplementedError) as err:
        SolverFamily([inv(), ranked])
    assert 'member 1' in str(err.value) and 'communicator' in str(err.value)
    with pytest.raises(NotImplementedError) as err:
        SolverFamily([_five_states()])
    assert 'state variables' in str(err.value)
    # shapes of the start, and the assertion on the reference node
    fam = SolverFamily([f() for f in fc.INVENTORY])
    for bad in (np.zeros(9), np.zeros((2, 10)), np.zeros((3, 10, 1))):
        with pytest.raises(ValueError) as err:
            fam.value_iteration(bad)
        assert str(bad.shape) in str(err.value) and '(3, 10)' in str(err.value)
    off = np.zeros((3, 10))
    off[1, 5] = 1.
    with pytest.raises(AssertionError):
        fam.value_iterations((off, 0.), 3, rel_dp=True)
    with pytest.raises(ValueError):
        fam.value_iterations(np.zeros(10), 3, tol=-1.)


def test_a_step_whose_structures_differ_raises(monkeypatch):
    monkeypatch.setattr(nat, 'require_gpu', lambda *a, **k: pytest.fail('a device was asked for'))

    def member(zero_at):
        data = np.array([0.5, 0.25, 0.75])

        def make():
            s = fc.pv_sized(2.0, 1.0, T=3)()
            cost = s.sys.cost
            s.sys.cost = lambda k, E, P: cost(k, E, P) + (P * data[k] if k != zero_at else P)
            return s
        return make
    fam = SolverFamily([member(None)(), member(1)()])
    fam._tables(0)
    with pytest.raises(ValueError) as err:
        fam.bellman_recursion(2, np.zeros(9))
    assert 'member 1 at step 1' in str(err.value), str(err.value)


# ----------------------------------------------------------------------------------------------------------------------
# no other unit changes

def _digests():
    with open(os.path.join(ROOT, 'profiles', 'plan_source_digests.txt')) as f:
        return {ln.split()[1] for ln in f if len(ln.split()) == 2 and not ln.startswith('#')}


def test_other_units_keep_their_generated_text():
    table = _digests()
    seen = set()
    specs = [('inventory', {}), ('storage_ar1', {}), ('searev', {}),
             ('two_reservoirs', dict(n_a=128, n_b=128, n_y=64, n_w=16, steps=(1. / 15, 1. / 15))), ('two_inflows', {}),
             ('inventory_fine', dict(n_x=65536, n_u=4097, n_w=16))]
    for name, kw in specs:
        for kernel in ('auto', 'staged', 'generic'):
            s = getattr(models, name)(**kw)[1]
            s.kernel = kernel
            try:
                source = s._kernel_plan()['source']
            except ValueError:
                continue                                            # (several perturbation variables take 'auto' / 'generic')
            assert 'SDP_FAMILY' not in source
            seen.add('line' if '#define SDP_LINE 1' in source else 'lead' if '#define SDP_LEAD_AXES ' in source
                     else 'column' if 'sdp_column_kernel.h' in source else 'staged' if 'sdp_staged_kernel.h' in source
                     else 'direct')
            assert hashlib.sha256(source.encode('utf-8')).hexdigest()[:16] in table, (name, kernel)
    assert seen == {'column', 'lead', 'line', 'staged', 'direct'}, seen
    # a lifted direct unit, too: the horizon's
    _, pv = models.pv_storage()
    source = pv._kernel_plan(0, pv._trace_now(0))['source']
    assert hashlib.sha256(source.encode('utf-8')).hexdigest()[:16] in table


def test_a_family_unit_is_the_lifted_direct_unit_with_another_header():
    s = fc.INVENTORY[0]()
    fam = SolverFamily([s])
    tabs = fam._tables()
    plain = codegen.translation_unit(tabs['model'], s.dtype, tabs['lanes'], None)
    unit = tabs['source']
    assert unit.replace('#define SDP_FAMILY 1          // the unit carries sdp_family_sweep alone (csrc/sdp_family_kernel.h)\n', '') \
        .replace('#include "sdp_family_kernel.h"    // brings in the helpers of sdp_sweep_kernel.h', '#include "sdp_sweep_kernel.h"') == plain
    assert codegen.source_key(unit) != codegen.source_key(plain)
    assert 'sdp_family_kernel.h' not in codegen._HEADERS               # (in the key of family units only)


def test_abi_declares_the_family_entry_points():
    with open(os.path.join(ROOT, 'include', 'sdp_hip.h')) as f:
        header = f.read()
    with open(os.path.join(codegen.CSRC, 'sdp_hip.hip')) as f:
        library = f.read()
    names = ['sdp_family_' + n for n in ('create', 'destroy', 'set_value', 'set_params', 'vi_sweep', 'vi_sweeps', 'vi_until',
                                         'get_value', 'get_policy', 'last_kernel_ms')]
    real_lib = nat.lib()
    for name in names:
        assert re.search(r'^int {}\('.format(name), header, re.M)
        assert 'extern "C" int {}('.format(name) in library
        assert name in nat.EXPORTS and hasattr(real_lib, name)
    h = __import__('ctypes').c_void_p()
    assert real_lib.sdp_family_create(None, __import__('ctypes').byref(h)) == -1


# ----------------------------------------------------------------------------------------------------------------------
# the `tol` case

def _oracle_sweeps(s, tol, check_every, n_iter):
    spec = vi_numpy.Spec.from_solver(s)
    J = np.zeros(spec.shape)
    for k in range(1, n_iter + 1):
        (J_k, _), _, _, _ = vi_numpy.value_iteration(spec, (J, 0.), rel_dp=True, dtype=np.float64)
        if conv.is_check(k, n_iter, check_every) and conv.converged(*conv.diff_stats(J_k, J, np.float64), tol):
            return k
        J = J_k
    return n_iter


def test_members_of_the_tol_case_need_different_numbers_of_sweeps():
    t = fc.TOL
    counts = [_oracle_sweeps(make(), t['tol'], t['check_every'], t['n_iter']) for make in t['members']]
    print('sweeps to tol by the oracle:', counts)
    assert len(set(counts)) > 1 and max(counts) < t['n_iter'], counts
    assert counts[0] == counts[2]                                     # (two identical members)


# ----------------------------------------------------------------------------------------------------------------------
# the cases compared with the oracle (family_cases.ORACLE_CASES): what their table claims

PLANNED = [fc.MAPPING[0], fc.MAPPING[-1], fc.MANY] + fc.STRIDED + [fc.SHRINK_CASE]


@pytest.mark.parametrize('case', PLANNED, ids=repr)
def test_oracle_cases_compile_and_carry_their_members_rows(case, tmp_path):
    test_unit_compiles_without_scratch_spills_or_lds(case, tmp_path)
    test_row_p_of_every_table_is_member_p(case)


def test_shapes_the_oracle_cases_are_for():
    units = fc.unit_sources()
    line_units = {}
    for case in fc.ORACLE_CASES:
        fam = SolverFamily(case.solvers())
        tabs = fam._tables()
        assert tabs['source'] in units, case                          # the build compiles it ahead
        if case is fc.SHRINK_CASE:
            continue
        S = int(np.prod(fam.dims))
        # 41 controls: 64 lanes, a tile of 4 nodes; three lifted constants, no two of a member the same
        assert [int(s._box_table(None)[2].prod()) for s in fam.solvers] == [41] * fam.P
        assert tabs['lanes'] == 64 and not tabs['per_node'] and tabs['prm'].shape == (fam.P, 3)
        assert all(len(set(row)) == 3 for row in tabs['prm'].tolist())
        grid = fc.launch(S, 64, fam.P, 256)
        assert S % 4 and grid['tiles'] == {fc.LINE_NX: 3, fc.STRIDED_NX: 129, fc.LONG_NX: 4129}[S]      # the last tile is ragged
        line_units.setdefault(case.dtype, set()).add(tabs['source'])
    assert {dt: len(u) for dt, u in line_units.items()} == {np.dtype(np.float64): 1, np.dtype(np.float32): 1}
    # no solo unit for them: every unit of the line model is a family unit
    for s in (fc.MAPPING[0].solvers()[0], fc.STRIDED[1].solvers()[0]):
        s.kernel = 'generic'
        assert s._kernel_plan()['source'] not in units
    # the mappings: members per XCD at P >= 8, idle XCDs at 5..7, parts of a member's tiles below 5
    units_of = {P: fc.launch(fc.LINE_NX, 64, P, 256) for P in fc.MAPPING_P + (65,)}
    assert [units_of[P]['parts'] for P in fc.MAPPING_P] == [4, 2, 1, 1, 1, 1, 1, 1]
    assert units_of[2]['units'] == [1] * 8 and units_of[4]['units'] == [2] * 8
    assert units_of[6]['units'] == [3] * 6 + [0] * 2 and units_of[7]['units'] == [3] * 7 + [0]
    assert units_of[8]['units'] == [3] * 8 and units_of[9]['units'] == [6] + [3] * 7
    assert units_of[16]['units'] == [6] * 8 and units_of[17]['units'] == [9] + [6] * 7
    assert units_of[65]['units'] == [27] + [24] * 7
    assert all(g['per_xcd'] == max(g['units']) for g in units_of.values())       # one trip each
    # the strided case on 256 CUs: 258 units on the XCDs with two members, 387 on XCD 0, 256 workgroups an XCD
    grid = fc.launch(fc.STRIDED_NX, 64, 17, 256)
    assert grid == dict(tiles=129, parts=1, per_xcd=256, units=[387] + [258] * 7)
    # the long case: four XCDs a member, 1033 tiles each behind 256 workgroups; 65 workgroups of 256 nodes against 64
    grid = fc.launch(fc.LONG_NX, 64, 2, 256)
    assert grid == dict(tiles=4129, parts=4, per_xcd=256, units=[1033] * 8) and -(-fc.LONG_NX // 256) == 65
    # chunks at P >= 8
    fam = SolverFamily(fc.CHUNKS_17.solvers())
    fam.chunk_bytes = fc.chunk_bytes_for(fam, 9)
    assert fam._chunks(fam._tables()) == [(0, 9), (9, 17)]


def test_the_host_grid_formula_is_the_one_restated():
    """family_cases.launch restates family_backup (csrc/sdp_hip.hip); the lines it restates are still there"""
    with open(os.path.join(codegen.CSRC, 'sdp_hip.hip')) as f:
        library = f.read()
    for line in ('const int64_t tile = (64 / f->lanes) * 4;', 'const int parts = n >= 8 ? 1 : 8 / n;',
                 'int64_t per_xcd = n >= 8 ? (int64_t)((n + 7) / 8) * tiles : (tiles + parts - 1) / parts;',
                 'if (per_xcd > f->cus) per_xcd = f->cus;'):
        assert line in library, line


def test_the_list_of_the_shrink_case_runs_through_every_mapping():
    t = fc.SHRINK
    counts = [len(fc.oracle_sweeps(make, np.zeros(10), t['n_iter'], True, t['tol'], t['check_every'])[0])
              for make in t['members']]
    print('sweeps to tol by the oracle:', counts)
    assert counts == fc.SHRINK_SWEEPS and max(counts) < t['n_iter']
    sizes = fc.list_sizes(counts, t['n_iter'])
    assert sizes == fc.SHRINK_SIZES == [16, 13, 6, 4, 0]               # >= 8, >= 8, 5..7, < 5
    # non-contiguous from the first drop on
    for k in sorted(set(counts))[:-1]:
        left = [p for p, n in enumerate(counts) if n > k]
        assert left != list(range(left[0], left[0] + len(left))), (k, left)


def _walk(S, lanes, n_active, cus, stride_factor=1):
    """the (position in the list, tile) pairs kernel sdp_family_sweep visits, from its index arithmetic restated
    (csrc/sdp_family_kernel.h) on the grid `fc.launch` gives; stride_factor = 2 is a walk with a wrong stride"""
    grid = fc.launch(S, lanes, n_active, cus)
    tiles, parts = grid['tiles'], grid['parts']
    per_part = -(-tiles // parts)
    seen = []
    for block in range(grid['per_xcd'] * 8):
        xcd = block & 7
        first, part = xcd // parts, xcd % parts
        mine = (n_active - first + 7) // 8 if first < n_active else 0
        for unit in range(block >> 3, mine * per_part, grid['per_xcd'] * stride_factor):
            tile = part * per_part + unit % per_part
            if tile < tiles:
                seen.append((first + 8 * (unit // per_part), tile))
    return seen


def test_the_restated_walk_visits_every_tile_of_every_listed_member_once():
    """for every list length and grid of the oracle cases -- so the arithmetic the GPU tests restate is the kernel's
    as long as the kernel's is right -- and a doubled stride misses tiles only where a case is past the cap: the cases
    that name a second trip are the ones that would notice"""
    shapes = [(fc.LINE_NX, P) for P in fc.MAPPING_P + (65,)] + [(fc.STRIDED_NX, 17), (fc.LONG_NX, 2)]
    shapes += [(10, n) for n in fc.SHRINK_SIZES[:-1]]
    for S, n in shapes:
        lanes = 16 if S == 10 else 64
        tiles = fc.launch(S, lanes, n, 256)['tiles']
        want = sorted((i, t) for i in range(n) for t in range(tiles))
        assert sorted(_walk(S, lanes, n, 256)) == want, (S, n)
        missed = set(want) - set(_walk(S, lanes, n, 256, stride_factor=2))
        assert bool(missed) == (S in (fc.STRIDED_NX, fc.LONG_NX)), (S, n)
    # the strided case: the second and third member of every XCD lose tiles to the wrong stride (units 256 .. 511), and
    # the GPU test compares all 17 x 515 nodes
    all_tiles = {(i, t) for i in range(17) for t in range(129)}
    assert {i for i, _ in all_tiles - set(_walk(fc.STRIDED_NX, 64, 17, 256, 2))} == set(range(8, 17))
    with open(os.path.join(codegen.CSRC, 'sdp_family_kernel.h')) as f:
        kernel = f.read()
    for line in ('const int parts = a.n_active >= 8 ? 1 : 8 / max(a.n_active, 1);', 'const int first = xcd / parts;',
                 'const int part = xcd % parts;', 'const int mine = first < a.n_active ? (a.n_active - first + 7) / 8 : 0;',
                 'const int64_t per_part = (tiles + parts - 1) / parts;', 'const int64_t stride = gridDim.x >> 3;',
                 'const int64_t tile = (int64_t)part * per_part + unit % per_part;',
                 'const int64_t p = members[first + 8 * (int)(unit / per_part)];'):
        assert line in kernel, line
