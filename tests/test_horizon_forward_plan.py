"""DPSolver.horizon_operator on the CPU (tests/horizon_forward_cases.py): what it and DPSolver.propagate refuse before a
device is touched; the plan of parts; the launch geometry of kernel sdp_transitions_h restated against the header and
the library; the generated text of the units (unchanged: only the headers carry the kernel); and the kernel in the
cross-compiled code objects, without scratch memory.  No GPU."""
import hashlib
import os

import numpy as np
import pytest

import horizon_forward_cases as hfc
from test_family_plan import _kernels, ROOT
from stodynprog_amd import DPSolver, HorizonOperator, codegen, forward, models, _native as nat


# ----------------------------------------------------------------------------------------------------------------------
# shapes and refusals

def _storage():
    row = hfc.BY_NAME['storage']
    s = row.solver()
    return s, row.policy(s)


def test_wrong_shapes_are_refused_with_both_shapes_named():
    s, pol = _storage()
    dims = tuple(len(g) for g in s.state_grid)
    with pytest.raises(ValueError) as err:                   # a policy of another grid
        s.horizon_operator(pol[:, :-1])
    assert str(pol[:, :-1].shape) in str(err.value) and str(dims + (1,)) in str(err.value)
    with pytest.raises(ValueError) as err:                   # a stationary policy without n_steps
        s.horizon_operator(pol[0])
    assert 'n_steps' in str(err.value) and str(pol[0].shape) in str(err.value) and '(T_pol,)' in str(err.value)
    for t0 in (-1, len(pol), len(pol) + 3):                  # t0 outside the policy
        with pytest.raises(ValueError) as err:
            s.horizon_operator(pol, t0=t0)
        assert str(pol.shape) in str(err.value) and str(pol.shape[1:]) in str(err.value)
    with pytest.raises(ValueError) as err:                   # more steps than the policy has from t0
        s.horizon_operator(pol, n_steps=4, t0=len(pol) - 3)
    assert 'T_pol = {}'.format(len(pol)) in str(err.value)
    with pytest.raises(ValueError):
        s.horizon_operator(pol, t0=0.5)
    with pytest.raises(ValueError):
        s.horizon_operator(pol, n_steps=0)
    for bad in (np.zeros(dims[::-1]), np.zeros((2,) + dims + (1,)), np.zeros(dims[0] * dims[1])):        # mu0
        with pytest.raises(ValueError) as err:
            s.propagate(pol, bad)
        assert str(bad.shape) in str(err.value) and str(dims) in str(err.value)


def test_a_communicator_is_refused():
    s, pol = _storage()
    s.comm = object()                                        # (never touched: refused by its presence)
    with pytest.raises(NotImplementedError):
        s.horizon_operator(pol)
    with pytest.raises(NotImplementedError):
        s.propagate(pol, np.zeros(tuple(len(g) for g in s.state_grid)))


def test_the_cap_names_the_steps_that_fit(monkeypatch):
    s, pol = _storage()
    S, nnz, step_bytes = s._transition_size()
    assert step_bytes == forward.operator_bytes(S * 5 * 4, S, 8)
    monkeypatch.setattr(DPSolver, 'TRANSITION_MAX_BYTES', 3 * step_bytes + 17)
    with pytest.raises(ValueError) as err:
        s.horizon_operator(pol)
    text = str(err.value)
    assert 'n_steps = 3 ' in text and 'TRANSITION_MAX_BYTES' in text and '{} bytes'.format(len(pol) * step_bytes) in text
    with pytest.raises(ValueError) as err:
        s.horizon_operator(pol[0], n_steps=4)
    assert 'n_steps = 3 ' in str(err.value)


# ----------------------------------------------------------------------------------------------------------------------
# the plan of parts

def test_the_runs_of_a_forced_part_length():
    plan = lambda n: HorizonOperator.plan_parts(8, 35, 700, n)
    assert plan(1) == [(k, 1) for k in range(8)]
    assert plan(2) == [(0, 2), (2, 2), (4, 2), (6, 2)]
    assert plan(3) == [(0, 3), (3, 3), (6, 2)]
    assert plan(8) == plan(50) == [(0, 8)] == plan(None)
    assert HorizonOperator.part_steps is None
    with pytest.raises(ValueError):
        plan(0)


def test_the_automatic_cut_obeys_the_row_and_entry_limits():
    """one device operator holds n_steps * S < 2^31 rows and fewer than 2^32 entries (include/sdp_hip.h)"""
    assert HorizonOperator.MAX_ROWS == 2 ** 31 - 1 and HorizonOperator.MAX_ENTRIES == 2 ** 32 - 1
    for S, per_node, n_steps in ((1 << 20, 4, 5000), (1 << 20, 64, 300), (3 * 10 ** 6 + 1, 18, 1000), (7, 6, 10 ** 6),
                                 (2 ** 31 - 1, 2, 3), (2 ** 28, 15, 5)):
        nnz = S * per_node
        parts = HorizonOperator.plan_parts(n_steps, S, nnz)
        assert [f for f, _ in parts] == [sum(c for _, c in parts[:i]) for i in range(len(parts))]
        assert sum(c for _, c in parts) == n_steps and all(c >= 1 for _, c in parts)
        longest = max(c for _, c in parts)
        assert longest * S < 2 ** 31 and longest * nnz < 2 ** 32
        if len(parts) > 1:                                   # .. and no shorter than they must be
            assert (longest + 1) * S >= 2 ** 31 or (longest + 1) * nnz >= 2 ** 32
            assert all(c == longest for _, c in parts[:-1])
    with pytest.raises(ValueError):                          # one step beyond the entry positions
        HorizonOperator.plan_parts(2, 2 ** 29, 2 ** 32)


# ----------------------------------------------------------------------------------------------------------------------
# the launch geometry

def test_the_launch_geometry_restated():
    read = lambda *path: open(os.path.join(*path)).read()
    header = read(codegen.CSRC, 'sdp_trans_horizon_kernel.h')
    args = read(codegen.CSRC, 'sdp_kernel_args.h')
    library = read(codegen.CSRC, 'sdp_hip.hip')
    sweep = read(codegen.CSRC, 'sdp_sweep_kernel.h')
    assert '#define SDP_TRANSH_THREADS {}\n'.format(hfc.THREADS) in header
    assert '#define SDP_TRANSH_TILE (SDP_TRANSH_THREADS >> SDP_D)' in header and '#define SDP_TRANSH_V (1 << SDP_D)' in header
    assert [hfc.tile(d) for d in (1, 2, 3, 4)] == [128, 64, 32, 16]
    assert 'struct SdpTransHArgs {' in args
    assert '__launch_bounds__(SDP_TRANSH_THREADS) sdp_transitions_h(SdpTransHArgs a)' in header
    assert '__shared__' not in header and '__shfl' not in header and '__syncthreads' not in header
    # directly after sdp_horizon_kernel.h, in both branches; 'sdp_horizon_kernel.h' itself untouched by that
    assert sweep.count('#include "sdp_trans_horizon_kernel.h"') == 2
    lines = sweep.split('\n')
    for i, ln in enumerate(lines):
        if ln.startswith('#include "sdp_horizon_kernel.h"'):
            assert lines[i + 1].startswith('#include "sdp_trans_horizon_kernel.h"')
    assert 'sdp_trans_horizon_kernel.h' in codegen._HEADERS                  # (in the key of every unit)
    # the flat walk: unit = kl tiles + tile, a workgroup strides over the units; the host's grid
    for line in ('const int64_t units = (a.step_end - a.step_begin) * tiles;', 'const int64_t kl = unit / tiles;',
                 'for (int64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {',
                 'if (s >= a.S) continue;', 'const int64_t e = ((kl * a.S + s) * W + j) * SDP_TRANSH_V + v;',
                 'if (v == 0) gbar[kl * a.S + s] = acc;',
                 'const sdp_real *__restrict__ pk = pol + (step - a.chunk_first) * (int64_t)SDP_NU * a.S;',
                 'const sdp_real *prm = sdp_h_prm_row(a.prm, step);', 'const sdp_real t = (sdp_real)(a.t0 + (double)step);'):
        assert line in header, line
    for line in ('const int64_t tile = 256 >> p->d;', 'int64_t blocks = n_steps * ((S + tile - 1) / tile);',
                 'if (blocks > (int64_t)p->cus * {0}) blocks = (int64_t)p->cus * {0};'.format(hfc.BUILD_PER_CU),
                 'if (blocks > cap / B) blocks = cap / B;',
                 'chain_blocks(S, 256, (int64_t)op->cus * {}, B)'.format(hfc.BUILD_PER_CU),
                 'chain_blocks(n_mid, 16, (int64_t)op->cus * {}, B)'.format(hfc.GROUP_PER_CU),
                 'chain_blocks(n_wide, 4, (int64_t)op->cus * {}, B)'.format(hfc.GROUP_PER_CU),
                 '#define SDP_PUSH_LONG {}\n'.format(hfc.PUSH_LONG), '#define SDP_PUSH_WIDE {}\n'.format(hfc.PUSH_WIDE)):
        assert line in library, line
    # the tiles and units of the GPU rows, on 256 compute units: one trip each
    shapes = {'line': (1, 65, 1), 'line_ragged': (1, 134, 2), 'storage': (2, 35, 1), 'storage_ragged': (2, 273, 5),
              'storage_data': (2, 273, 5), 'reservoirs': (3, 60, 2), 'two_variables': (1, 9, 1), 'deterministic': (1, 9, 1),
              'inventory': (1, 10, 1)}
    for row in hfc.DEVICE_ROWS:
        s = row.solver()
        dims = tuple(len(g) for g in s.state_grid)
        d, S, tiles = shapes[row.name]
        assert (len(dims), int(np.prod(dims))) == (d, S) and -(-S // hfc.tile(d)) == tiles, row
        assert hfc.units(row.T, S, d) == row.T * tiles == hfc.build_blocks(row.T, S, d, 256)
    # the case past the caps, on the 256 compute units it is sized for: with 2 vectors the build and every push launch
    # that meets all rows want more workgroups than one trip has
    S = hfc.long_line_nodes(256)
    assert S == 262144 + 134 and hfc.units(2, S, 1) == 2 * 2050 > hfc.build_blocks(2, S, 1, 256) == 2048
    assert -(-S // 256) > hfc.push_blocks(S, 256, 256 * hfc.BUILD_PER_CU, 2) == 1024
    assert -(-(S // 2) // 16) > hfc.push_blocks(S // 2, 16, 256 * hfc.GROUP_PER_CU, 2) == 8192
    assert hfc.push_blocks(10, 256, 2048, 65535) == 1
    # the ABI: header, library and binding move together
    abi = read(ROOT, 'include', 'sdp_hip.h')
    real_lib = nat.lib()
    for name in ('sdp_chainop_create', 'sdp_chainop_destroy', 'sdp_chainop_propagate', 'sdp_chainop_get_csr',
                 'sdp_chainop_get_mean_cost', 'sdp_chainop_times'):
        assert 'int {}('.format(name) in abi and 'extern "C" int {}('.format(name) in library, name
        assert name in nat.EXPORTS and hasattr(real_lib, name), name


# ----------------------------------------------------------------------------------------------------------------------
# the generated text

def _digests():
    with open(os.path.join(ROOT, 'profiles', 'plan_source_digests.txt')) as f:
        return {ln.split()[1] for ln in f if len(ln.split()) == 2 and not ln.startswith('#')}


def test_units_keep_their_generated_text():
    table = _digests()
    sources = [getattr(models, name)()[1]._kernel_plan()['source'] for name in ('inventory', 'storage_ar1', 'searev', 'two_inflows')]
    _, fh = models.finite_horizon()
    sources.append(fh._kernel_plan(0, fh._trace_now(0))['source'])
    for source in sources + hfc.unit_sources():
        assert 'sdp_trans_horizon_kernel.h' not in source and 'sdp_transitions_h' not in source
    for source in sources:
        assert hashlib.sha256(source.encode('utf-8')).hexdigest()[:16] in table


# ----------------------------------------------------------------------------------------------------------------------
# the kernel in the code objects

@pytest.mark.parametrize('dtkey', sorted(hfc.DTYPES))
@pytest.mark.parametrize('name', ['line', 'storage_data', 'reservoirs', 'two_variables'])
def test_the_kernel_is_in_the_code_object_without_scratch(name, dtkey, tmp_path):
    """d = 1, d = 2 with data[k], d = 3 and SDP_NW = 2, in both reals"""
    row = hfc.BY_NAME[name]
    s = row.solver(hfc.DTYPES[dtkey])
    source = hfc.plan_of(s, 0)['source']
    assert ('#define SDP_NW 2' in source) == (name == 'two_variables')
    assert ('#define SDP_NPARAMS ' in source) == (row.time_index == 'int')
    kernels = _kernels(source, tmp_path)
    assert 'sdp_transitions_h' in kernels and 'sdp_transitions' in kernels and 'sdp_simulate_h' in kernels
    f = kernels['sdp_transitions_h']
    print(name, dtkey, {n: f[n] for n in ('.vgpr_count', '.sgpr_count', '.private_segment_fixed_size', '.vgpr_spill_count',
                                           '.sgpr_spill_count', '.group_segment_fixed_size', '.max_flat_workgroup_size')})
    assert f['.private_segment_fixed_size'] == 0 and f['.vgpr_spill_count'] == 0, f
    assert f['.group_segment_fixed_size'] == 0 and f['.max_flat_workgroup_size'] == hfc.THREADS, f


# ----------------------------------------------------------------------------------------------------------------------
# the rows

def test_the_rows_with_python_float_constants_are_the_models_they_restate():
    """`storage_data` and `deterministic` read their constants as Python floats where the models they restate read
    numpy.float64 scalars: the same entries bit for bit and the same units in 8-byte reals; in 4-byte reals the originals'
    callables compute in 8-byte reals on the way (numpy's promotion), which no kernel does"""
    import forward_cases as fc
    import horizon_cases as hc
    for name, original in (('storage_data', lambda: hc.storage(data=True)),
                           ('deterministic', lambda: models.pv_storage(T=6, N_E=9, u_step=0.05)[1])):
        row = hfc.BY_NAME[name]
        s, o = row.solver(), original()
        pol = row.policy(s)
        mine, theirs = (forward.chain_entries(x, pol, row.T, 0, 'int') for x in (s, o))
        assert all(fc.same(a, b) for e, f in zip(mine, theirs) for a, b in zip(e[:4], f[:4])), name
        for dt in hfc.DTYPES.values():
            assert hfc.plan_of(row.solver(dt), 0)['source'] == hfc.plan_of(fc.as_dtype(o, dt), 0)['source'], name
