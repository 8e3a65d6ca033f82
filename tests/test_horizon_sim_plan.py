"""Closed loops under a time-indexed policy, on the CPU: kernels sdp_simulate_h and sdp_montecarlo_h
(csrc/sdp_horizon_kernel.h) are part of every generated unit without scratch memory or vector spills, the table of
per-step constants of a `data[k]` model is what every step's own trace gives, and what DPSolver.simulate and
monte_carlo refuse they refuse before they touch a device.  No GPU: the units of tests/horizon_sim.py are
cross-compiled for gfx950 (the code objects the build keeps) and their notes are read."""
import os
import re
import subprocess

import numpy as np
import pytest

import horizon_cases as hc
import horizon_sim as hs
import policies as P
from stodynprog_amd import codegen, models, _native as nat
from stodynprog_amd.trace import trace_model

LLVM_BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(nat.HIPCC))), 'llvm', 'bin')
TARGET = 'hipv4-amdgcn-amd-amdhsa--gfx950'


def units():
    """the generated units of the tests of the time-indexed loops (the build compiles them ahead)"""
    return hs.unit_sources()


def _kernels(source, tmp_path):
    """{kernel name: integer fields of its code-object notes} (tests/test_forward_plan.py reads them the same way)"""
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


@pytest.mark.parametrize('dtkey', ['f64', 'f32'])
@pytest.mark.parametrize('name', sorted(hs.PLANNED))
def test_kernels_are_in_the_unit_without_scratch(name, dtkey, tmp_path):
    s = P.as_dtype(hs.PLANNED[name](), dict(f64=np.float64, f32=np.float32)[dtkey])
    kernels = _kernels(hs.plan_source(s), tmp_path)
    wanted = ['sdp_simulate_h'] + (['sdp_montecarlo_h'] if s.sys.stochastic else [])
    for k in wanted:
        assert k in kernels, (k, sorted(kernels))
        f = kernels[k]
        print(name, dtkey, k, {n: f[n] for n in ('.vgpr_count', '.sgpr_count', '.private_segment_fixed_size',
                                                 '.vgpr_spill_count', '.sgpr_spill_count')})
        assert f['.private_segment_fixed_size'] == 0 and f['.vgpr_spill_count'] == 0, (k, f)
    for k in ('sdp_simulate', 'sdp_montecarlo'):                # (the stationary twins, for comparison)
        if k in kernels:
            print(name, dtkey, k, {n: kernels[k][n] for n in ('.vgpr_count', '.sgpr_count', '.sgpr_spill_count')})
    if not s.sys.stochastic:
        assert 'sdp_montecarlo_h' not in kernels and 'sdp_montecarlo' not in kernels


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


@pytest.mark.parametrize('name', ['storage data[k]', 'reservoirs data[k]', 'pv_storage'])
@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['f64', 'f32'])
def test_parameter_table_is_every_steps_own_trace(name, dtype):
    s = P.as_dtype(hs.PLANNED[name](), dtype)
    T = 48 if name == 'pv_storage' else hc.T
    model = s._trace_now(0)
    assert model.t_value == 0 and model.param_index
    table = s._horizon_table(model, False, T, 0)
    assert table.shape == (T, len(model.param_index)) and table.dtype == np.dtype(dtype) and table.flags.c_contiguous
    sy = s.sys
    for k in range(T):
        own = trace_model(sy.dyn, sy.cost, len(sy.state), len(sy.control), len(sy.perturb), sy.params, sy.stationnary,
                          t_value=k)
        row = np.asarray(own.param_values(), dtype=float).astype(dtype)        # rounded once, as set_params does
        assert np.array_equal(_bits(table[k]), _bits(row)), k
    if name != 'pv_storage':
        # the data of TIME_DATA reach their slots with their bits: 0.0 at step 2, -0.0 at step 3, the sign change between
        # steps 0 and 1, and the steps 4 and 5 that equal another literal keep a slot of their own
        slots = [j for j in range(table.shape[1])
                 if all(_bits(table[k, j:j + 1])[0] == _bits(np.array([hc.TIME_DATA[k]], dtype=dtype))[0]
                        for k in range(T))]
        assert slots, table
        j = slots[0]
        assert not np.signbit(table[2, j]) and np.signbit(table[3, j]) and table[2, j] == 0 and table[3, j] == 0
        assert table[0, j] > 0 > table[1, j]
    # a later start: the rows of the steps that run
    part = s._horizon_table(s._trace_now(3), False, 4, 3)
    assert np.array_equal(_bits(part), _bits(table[3:7]))


def test_a_structure_change_gives_no_table():
    s = hs.switching()
    model = s._trace_now(0)
    assert model.t_value == 0
    assert s._horizon_table(model, False, hc.T, 0) is None
    assert s._horizon_table(model, True, hc.T, 0) is None
    assert s._horizon_table(model, False, 1, 0).shape[0] == 1           # one step alone has a table


def test_a_symbolic_model_needs_no_table():
    s = hc.storage()
    model = s._trace_now(0)
    assert model.t_value is None
    assert s._horizon_table(model, False, hc.T, 0) is None              # a stationary policy: today's kernels
    assert s._horizon_table(model, True, hc.T, 0).shape == (hc.T, 0)


class _Ranks(object):
    nranks = 2


def test_refusals_name_their_numbers_before_a_device_is_touched(monkeypatch):
    monkeypatch.setattr(nat, 'require_gpu', lambda *a, **k: pytest.fail('a device was asked for'))
    s = hc.storage()
    dims, nu = s._state_grid_shape, 1
    pol = np.zeros((hc.T,) + dims + (nu,))
    x0 = np.zeros((3, 2))
    w = np.zeros((hc.T, 3))
    calls = (lambda p, n, t0: s.simulate(p, x0, w, n_steps=n, t0=t0),
             lambda p, n, t0: s.monte_carlo(p, x0, n, t0=t0))
    for call in calls:
        # wrong ndim
        for bad in (pol[0, ..., 0], pol[None]):
            with pytest.raises(ValueError) as err:
                call(bad, 2, 0)
            assert str(dims + (nu,)) in str(err.value) and 'T_pol' in str(err.value) and str(bad.shape) in str(err.value)
        # wrong trailing shape
        for bad in (pol[:, :-1], pol[..., :0], np.zeros((hc.T,) + dims + (2,))):
            with pytest.raises(ValueError) as err:
                call(bad, 2, 0)
            assert str(dims + (nu,)) in str(err.value) and str(bad.shape) in str(err.value)
        # beyond the policy's steps, and before them: t0, n_steps and T_pol are in the text
        with pytest.raises(ValueError) as err:
            call(pol, 6, 3)
        assert all(n in str(err.value) for n in ('t0 = 3', 'n_steps = 6', 'T_pol = 8')), str(err.value)
        with pytest.raises(ValueError) as err:
            call(pol, 2, -1)
        assert all(n in str(err.value) for n in ('t0 = -1', 'n_steps = 2', 'T_pol = 8')), str(err.value)
    # a communicator of several ranks
    s.comm = _Ranks()
    for call in calls:
        with pytest.raises(NotImplementedError):
            call(pol, 2, 0)


def test_header_is_part_of_the_cache_key():
    assert 'sdp_horizon_kernel.h' in codegen._HEADERS


def test_units_without_lifted_constants_keep_their_source():
    for make in (hc.storage, hc.line, lambda: models.synthetic3d(N=20)[1], lambda: models.inventory()[1]):
        s = make()
        src = s._kernel_plan()['source'] if s.sys.stationnary else hs.plan_source(s)
        assert 'sdp_model_cell_at' not in src and 'SDP_NPARAMS' not in src
    # a unit with lifted constants gains the one function: the body of sdp_model_cell reading the caller's row
    src = hs.plan_source(hc.storage(data=True))
    assert src.count('SDP_DEV void sdp_model_cell_at(') == 1 and src.count('SDP_DEV void sdp_model_cell(') == 1
    cell = src.split('SDP_DEV void sdp_model_cell(')[1].split('\n}\n')[0]
    cell_at = src.split('SDP_DEV void sdp_model_cell_at(')[1].split('\n}\n')[0]
    body = lambda text: text.split('{\n', 1)[1].split('\n', 1)[1]           # (after the line of (void) casts)
    assert body(cell).replace('sdp_model_prm[', 'prm[') == body(cell_at)
    assert 'sdp_model_prm[' in cell and 'sdp_model_prm[' not in cell_at
