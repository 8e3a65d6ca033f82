"""Policy evaluation and iteration of families on the CPU (tests/family_policy_cases.py): the evaluation unit
cross-compiles for gfx950 with exactly its two kernels, free of scratch memory and vector spills, and the resident
kernel takes the LDS and the workgroup the host's fit rule assumes; the sweep unit keeps its text; the form rule and
the launch geometry, restated; what the two methods refuse before a device is touched; and the inputs of the GPU tests
have the properties those tests rely on, by oracle/vi_numpy.py alone.  No GPU."""
import hashlib
import os
import re

import numpy as np
import pytest

import family_cases as fc
import family_policy_cases as pc
from test_family_plan import _kernels, _digests, ROOT
from stodynprog_amd import SolverFamily, codegen, _native as nat

BY_NAME = {c.name: c for c in fc.CASES}
UNITS = [('inventory P=3', None), ('storage_ar1 f64', None), ('storage_ar1 f32', None), ('three_d', None),
         ('finite_horizon', 0), ('pv', 0)]


@pytest.mark.parametrize('name,t_k', UNITS, ids=[u[0] for u in UNITS])
def test_evaluation_unit_compiles_with_its_two_kernels(name, t_k, tmp_path):
    fam = SolverFamily(BY_NAME[name].solvers())
    tabs = fam._tables(t_k)
    source = codegen.family_policy_unit(tabs['model'], fam.dtype)
    assert '#define SDP_FAMILY 1' in source and '#define SDP_FAMILY_POLICY 1' in source
    assert '#include "sdp_family_policy_kernel.h"' in source and 'sdp_model_cell_at(' in source
    assert '#include "sdp_family_kernel.h"' not in source and '#include "sdp_sweep_kernel.h"' not in source
    # one unit per model structure and real type: no lane count of the members in it
    assert '#define SDP_LANES 1\n' in source
    kernels = _kernels(source, tmp_path)
    assert sorted(kernels) == ['sdp_family_evalpol', 'sdp_family_evalpol_resident'], sorted(kernels)
    for k, f in kernels.items():
        print(name, k, {n: f[n] for n in ('.vgpr_count', '.sgpr_count', '.private_segment_fixed_size', '.vgpr_spill_count',
                                          '.sgpr_spill_count', '.group_segment_fixed_size', '.max_flat_workgroup_size')})
        assert f['.private_segment_fixed_size'] == 0 and f['.vgpr_spill_count'] == 0, (k, f)
    step, res = kernels['sdp_family_evalpol'], kernels['sdp_family_evalpol_resident']
    assert step['.group_segment_fixed_size'] == 0 and step['.max_flat_workgroup_size'] == pc.STEPS_TILE
    # what the fit rule assumes: two buffers of resident_nodes reals, the reduction within its share, the budget kept
    rs = fam.dtype.itemsize
    nodes = pc.resident_nodes(fam.dtype)
    assert nodes == codegen.family_resident_nodes(fam.dtype)
    assert res['.max_flat_workgroup_size'] == pc.RESIDENT_THREADS == codegen.FAMILY_RESIDENT_THREADS
    lds = res['.group_segment_fixed_size']
    assert 2 * nodes * rs < lds <= 2 * nodes * rs + pc.RESIDENT_REDUCTION_BYTES <= pc.RESIDENT_LDS_BYTES == codegen.COLUMN_LDS_MAX
    assert 2 * (nodes + 1) * rs + pc.RESIDENT_REDUCTION_BYTES > pc.RESIDENT_LDS_BYTES
    # the sweep unit of the same family keeps the text of the parent: its digest is on record
    digest = hashlib.sha256(tabs['source'].encode('utf-8')).hexdigest()[:16]
    assert digest in _digests(), name
    assert hashlib.sha256(source.encode('utf-8')).hexdigest()[:16] in _digests(), name
    assert codegen.source_key(source) != codegen.source_key(tabs['source'])


def test_the_unit_does_not_depend_on_the_lane_count_and_its_key_covers_its_headers(monkeypatch, tmp_path):
    fam = SolverFamily(BY_NAME['storage_ar1 f64'].solvers())
    tabs = fam._tables()
    assert tabs['lanes'] == 16
    one = SolverFamily(BY_NAME['storage_ar1 f64'].solvers()[:1])
    assert one._tables()['lanes'] == 8 and one._tables()['source'] != tabs['source']
    source = codegen.family_policy_unit(tabs['model'], fam.dtype)
    assert codegen.family_policy_unit(one._tables()['model'], one.dtype) == source
    assert 'sdp_family_policy_kernel.h' not in codegen._HEADERS and 'sdp_family_kernel.h' not in codegen._HEADERS
    # an edit of either header changes the key of the evaluation unit; one of the evaluation header leaves the sweep unit's
    keys = codegen.source_key(source), codegen.source_key(tabs['source'])
    csrc = tmp_path / 'csrc'
    csrc.mkdir()
    for fn in os.listdir(codegen.CSRC):
        if fn.endswith('.h'):
            (csrc / fn).write_bytes(open(os.path.join(codegen.CSRC, fn), 'rb').read())
    monkeypatch.setattr(codegen, 'CSRC', str(csrc))
    codegen._digest_cache.clear()
    assert (codegen.source_key(source), codegen.source_key(tabs['source'])) == keys
    with open(str(csrc / 'sdp_family_policy_kernel.h'), 'a') as f:
        f.write('// edited\n')
    assert codegen.source_key(source) != keys[0] and codegen.source_key(tabs['source']) == keys[1]
    with open(str(csrc / 'sdp_family_kernel.h'), 'a') as f:
        f.write('// edited\n')
    assert codegen.source_key(tabs['source']) != keys[1]
    codegen._digest_cache.clear()


def test_the_unit_says_what_it_is_and_the_library_checks_it():
    with open(os.path.join(codegen.CSRC, 'sdp_family_policy_kernel.h')) as f:
        header = f.read()
    with open(os.path.join(codegen.CSRC, 'sdp_kernel_args.h')) as f:
        args = f.read()
    with open(os.path.join(codegen.CSRC, 'sdp_hip.hip')) as f:
        library = f.read()
    assert 'SDP_META_F_FAMILY_POLICY = 2048' in args
    assert 'SDP_META_F_FAMILY | SDP_META_F_FAMILY_POLICY, 0, 0, SDP_FPOL_THREADS, SDP_FPOL_NODES' in header
    assert '!(m[SDP_META_FLAGS] & SDP_META_F_FAMILY_POLICY)' in library
    # the constants the host states are the kernel's
    assert '#define SDP_FPOL_THREADS {}'.format(codegen.FAMILY_RESIDENT_THREADS) in header
    assert '#define SDP_FPOL_LDS_BYTES (160 * 1024)' in header and codegen.FAMILY_RESIDENT_LDS_BYTES == 160 * 1024
    assert '#define SDP_FPOL_RED_BYTES {}'.format(codegen.FAMILY_RESIDENT_REDUCTION_BYTES) in header
    assert '#define SDP_FPOL_TILE {}'.format(pc.STEPS_TILE) in header
    # the fit rule is asserted before the launch
    assert 'if (form == SDP_FAMILY_EVAL_RESIDENT && f->S > f->res_nodes)' in library
    # the ABI: header, library and binding move together
    with open(os.path.join(ROOT, 'include', 'sdp_hip.h')) as f:
        abi = f.read()
    real_lib = nat.lib()
    for name in ('load_policy_unit', 'set_policy', 'take_policy', 'compare_policy', 'set_members', 'eval_policy',
                 'eval_policy_until'):
        name = 'sdp_family_' + name
        assert re.search(r'^int {}\('.format(name), abi, re.M) and 'extern "C" int {}('.format(name) in library
        assert name in nat.EXPORTS and hasattr(real_lib, name)
    assert real_lib.sdp_family_eval_policy(None, 1, 0, 0, 0, None) == -1
    assert real_lib.sdp_family_set_members(None, None, 0) == -1


def _line_family(n_x, dtype=np.float64):
    return SolverFamily([fc.line(0.55, 1.21, -0.37, n_x, dtype)()])


def test_the_form_rule_restated():
    assert pc.resident_nodes(np.float64) == 10208 and pc.resident_nodes(np.float32) == 20416
    for dtype in (np.float64, np.float32):
        S = pc.resident_nodes(dtype)
        assert S == codegen.family_resident_nodes(dtype)
        fits, over = _line_family(S, dtype), _line_family(S + 1, dtype)
        assert fits.evaluation == 'auto'
        # 'auto': resident up to one node per thread of the resident workgroup, from two steps on
        one_trip, two_trips = _line_family(pc.RESIDENT_THREADS, dtype), _line_family(pc.RESIDENT_THREADS + 1, dtype)
        assert one_trip._evaluation_form(5) == 'resident' == pc.form(pc.RESIDENT_THREADS, dtype, 5)
        assert one_trip._evaluation_form(2) == 'resident' and one_trip._evaluation_form(1) == 'steps' == pc.form(1024, dtype, 1)
        assert two_trips._evaluation_form(5) == 'steps' == pc.form(pc.RESIDENT_THREADS + 1, dtype, 5)
        assert fits._evaluation_form(5) == 'steps' == pc.form(S, dtype, 5)
        assert over._evaluation_form(5) == 'steps' == pc.form(S + 1, dtype, 5)
        fits.evaluation = over.evaluation = 'resident'
        assert fits._evaluation_form(1) == 'resident'
        with pytest.raises(ValueError) as err:
            over._evaluation_form(5)
        rs = np.dtype(dtype).itemsize
        assert str(2 * (S + 1) * rs) in str(err.value) and str(pc.RESIDENT_LDS_BYTES - pc.RESIDENT_REDUCTION_BYTES) in str(err.value)
        fits.evaluation = 'steps'
        assert fits._evaluation_form(5) == 'steps'


def test_the_launch_geometry_of_both_kernels_on_256_compute_units():
    # the steps kernel: workgroups an XCD wanted against the cap
    assert pc.launch_steps(35, 3, 256) == dict(tiles=1, parts=2, wanted=1, per_xcd=1, units=[1] * 6 + [0] * 2)
    assert pc.launch_steps(41 * 61, 64, 256) == dict(tiles=10, parts=1, wanted=80, per_xcd=80, units=[80] * 8)
    long_, strided = pc.launch_steps(pc.LONG_NX, 2, 256), pc.launch_steps(pc.STRIDED_NX, 17, 256)
    assert long_ == dict(tiles=1025, parts=4, wanted=257, per_xcd=256, units=[257] * 8)
    assert strided == dict(tiles=86, parts=1, wanted=258, per_xcd=256, units=[258] + [172] * 7)
    # family_cases' own long and strided cases stay below this kernel's cap: the cases here are larger
    assert pc.launch_steps(fc.LONG_NX, 2, 256)['wanted'] == 17 and pc.launch_steps(fc.STRIDED_NX, 17, 256)['wanted'] == 9
    # the resident kernel: one workgroup a listed member, one a compute unit at most
    assert pc.launch_resident(64, 256) == dict(wanted=64, blocks=64)
    assert pc.launch_resident(259, 256) == dict(wanted=259, blocks=256)
    with open(os.path.join(codegen.CSRC, 'sdp_hip.hip')) as f:
        library = f.read()
    for line in ('const int64_t tiles = (f->S + 255) / 256;', 'if (blocks > f->cus) blocks = f->cus;'):
        assert line in library, line
    with open(os.path.join(codegen.CSRC, 'sdp_family_policy_kernel.h')) as f:
        kernel = f.read()
    for line in ('const int64_t tile = (int64_t)part * per_part + unit % per_part;',
                 'const int64_t p = members[first + 8 * (int)(unit / per_part)];',
                 'for (int at = blockIdx.x; at < a.n_active; at += gridDim.x) {'):
        assert line in kernel, line
    # the many-member case never repeats a constant, so every member has the family's structure
    fam = SolverFamily(pc.many(259).solvers())
    prm = fam._tables()['prm']
    assert prm.shape[0] == 259 and all(len(set(row)) == prm.shape[1] for row in prm.tolist())


def test_argument_checks_come_before_a_device_is_touched(monkeypatch):
    monkeypatch.setattr(nat, 'require_gpu', lambda *a, **k: pytest.fail('a device was asked for'))
    monkeypatch.setattr(nat, 'lib', lambda *a, **k: pytest.fail('the library was asked for'))
    fam = SolverFamily(BY_NAME['storage_ar1 f64'].solvers())
    good = np.zeros((3, 7, 5, 2))
    for method, args in ((fam.eval_policy, (4,)), (fam.policy_iteration, (4, 1))):
        for bad in (np.zeros((7, 5)), np.zeros((7, 5, 1)), np.zeros((2, 7, 5, 2)), np.zeros((3, 7, 5, 2, 1))):
            with pytest.raises(ValueError) as err:
                method(bad, *args)
            assert str(bad.shape) in str(err.value) and '(7, 5, 2)' in str(err.value) and '(3, 7, 5, 2)' in str(err.value)
        with pytest.raises(ValueError):
            method(good, *args, tol=-1.)
        with pytest.raises(ValueError):
            method(good, *args, tol=1e-6, check_every=0)
        with pytest.raises(ValueError) as err:
            method(good, 0, *args[1:], tol=1e-6)
        assert 'n_iter >= 1' in str(err.value)
    for bad in (np.zeros(7), np.zeros((2, 7, 5)), np.zeros((3, 7, 5, 1))):
        with pytest.raises(ValueError) as err:
            fam.eval_policy(good, 4, J_zero=bad)
        assert str(bad.shape) in str(err.value) and 'J_zero' in str(err.value) and '(3, 7, 5)' in str(err.value)
    fam.evaluation = 'lds'
    with pytest.raises(ValueError) as err:
        fam.eval_policy(good, 4)
    assert "'lds'" in str(err.value) and 'resident' in str(err.value)
    # what _member_bytes returns for the other methods stays; the policy buffer counts for these two alone
    fam.evaluation = 'auto'
    tabs = fam._tables()
    per = fam._member_bytes(tabs)
    assert fam._policy_bytes() == 35 * 2 * 8 + 8
    fam.chunk_bytes = 2 * per + fam._policy_bytes() // 2
    assert fam._chunks(tabs) == [(0, 2), (2, 3)] and fam._chunks(tabs, fam._policy_bytes()) == [(0, 1), (1, 2), (2, 3)]


# ----------------------------------------------------------------------------------------------------------------------
# the inputs of the GPU tests, by the oracle alone

def test_the_shrink_case_under_its_policy_runs_through_every_mapping():
    t = pc.SHRINK
    pol = pc.shrink_policies()
    steps, converged = [], []
    for p, make in enumerate(t['members']):
        _, refs, checks = pc.oracle_eval(make, pol[p], t['n_iter'], True, tol=t['tol'], check_every=t['check_every'])
        steps.append(len(refs))
        converged.append(checks[-1][2] - checks[-1][1] <= t['tol'])
    print('steps to tol by the oracle:', steps)
    assert steps == pc.SHRINK_STEPS and max(steps) < t['n_iter'] and all(converged)
    sizes = fc.list_sizes(steps, t['n_iter'])
    assert sizes == pc.SHRINK_SIZES == [16, 14, 8, 5, 4, 0]              # >= 8, >= 8, 8, 5..7, < 5
    # with every third step checked and a cap of 17 the members that need 18 steps run into the cap
    c = pc.SHRINK_CAPPED
    assert [k for k in range(1, 18) if k % c['check_every'] == 0 or k == c['n_iter']] == [3, 6, 9, 12, 15, 17]
    assert sorted(set(steps)) == [14, 15, 16, 17, 18]


def test_the_line_case_needs_different_numbers_of_steps_and_improvements():
    t = pc.LINE
    pol = pc.line_policies()
    first, improvements, later = [], [], []
    for p, make in enumerate(t['members']):
        _, _, _, steps, n_imp, stable = pc.oracle_policy_iteration(make, pol[p], t['n_val'], t['n_pol'], t['tol'], t['check_every'])
        assert stable and max(steps) < t['n_val'], p
        first.append(steps[0])
        improvements.append(n_imp)
        later += steps[1:]
    print('first evaluations:', first, 'improvements:', improvements)
    assert first == pc.LINE_STEPS and improvements == pc.LINE_IMPROVEMENTS
    assert [p for p, n in enumerate(improvements) if n == 4] == [12, 14, 16] and max(improvements) < t['n_pol']
    assert min(later) == 7 and max(later) == 20 and len(set(later)) > 4


def test_the_build_compiles_the_units_of_the_gpu_tests():
    units = pc.unit_sources()
    for case in fc.STATIONARY + [fc.CHUNKS, pc.walk_case(pc.walk_sizes()[2]), pc.many(259), pc.LONG, pc.STRIDED]:
        fam = SolverFamily(case.solvers())
        tabs = fam._tables()
        assert tabs['source'] in units and codegen.family_policy_unit(tabs['model'], fam.dtype) in units, case
    with open(os.path.join(ROOT, '__graft_entry__.py')) as f:
        assert 'family_policy_cases.unit_sources()' in f.read()
