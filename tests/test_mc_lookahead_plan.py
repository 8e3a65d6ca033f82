"""Kernel sdp_montecarlo_lookahead on the CPU: every boxed stochastic case of tests/lookahead_cases.py cross-compiles
for gfx950 with the kernel present and free of scratch memory and vector spills; units without a box function and the
deterministic unit do not carry it; the header and the library declare the entry point; and what
DPSolver.monte_carlo_lookahead refuses it refuses before a device is touched.  No GPU."""
import os
import re

import numpy as np
import pytest

import lookahead_cases as lc
import mc_lookahead_cases as mlc
from test_lookahead_plan import _kernels, _Ranks
from stodynprog_amd import codegen, _native as nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = 'sdp_montecarlo_lookahead'
FIELDS = ('.vgpr_count', '.sgpr_count', '.private_segment_fixed_size', '.vgpr_spill_count', '.sgpr_spill_count')


@pytest.mark.parametrize('case', mlc.BOXED + mlc.NAN_CASES, ids=repr)
def test_boxed_stochastic_units_carry_the_kernel_without_scratch(case, tmp_path):
    s = case.solver()
    kernels = _kernels(lc.unit_source(s, case.times[0]), tmp_path)
    assert KERNEL in kernels, sorted(kernels)
    for k in (KERNEL, 'sdp_simulate_lookahead'):
        print(case, k, {n: kernels[k][n] for n in FIELDS})
    f = kernels[KERNEL]
    assert f['.private_segment_fixed_size'] == 0 and f['.vgpr_spill_count'] == 0, f
    assert f['.max_flat_workgroup_size'] == 256                        # no launch bound beyond the workgroup size
    # .. and the kernels the unit had keep theirs
    for k in ('sdp_lookahead', 'sdp_simulate_lookahead'):
        assert kernels[k]['.private_segment_fixed_size'] == 0 and kernels[k]['.vgpr_spill_count'] == 0, (k, kernels[k])


@pytest.mark.parametrize('name', ['data[k]', 'deterministic'])
def test_units_without_a_box_and_the_deterministic_unit_do_not_carry_it(name, tmp_path):
    case = lc.BY_NAME[name]
    kernels = _kernels(lc.unit_source(case.solver(), case.times[0]), tmp_path)
    assert 'sdp_lookahead' in kernels and KERNEL not in kernels
    assert ('sdp_simulate_lookahead' in kernels) == (name == 'deterministic')


def test_a_plain_unit_does_not_carry_it(tmp_path):
    s = lc.BY_NAME['inventory'].solver()
    s.kernel = 'generic'
    kernels = _kernels(s._kernel_plan()['source'], tmp_path)
    assert 'sdp_montecarlo' in kernels and KERNEL not in kernels


def test_the_kernel_lives_in_the_lookahead_header_and_the_arguments_in_the_shared_one():
    with open(os.path.join(codegen.CSRC, 'sdp_lookahead_kernel.h')) as f:
        assert 'void __launch_bounds__(256) {}(SdpLookMcArgs a)'.format(KERNEL) in f.read()
    with open(os.path.join(codegen.CSRC, 'sdp_kernel_args.h')) as f:
        assert 'struct SdpLookMcArgs {' in f.read()
    assert 'sdp_lookahead_kernel.h' not in codegen._HEADERS and 'sdp_kernel_args.h' in codegen._HEADERS


def test_abi_declares_the_entry_point():
    with open(os.path.join(ROOT, 'include', 'sdp_hip.h')) as f:
        header = f.read()
    with open(os.path.join(codegen.CSRC, 'sdp_hip.hip')) as f:
        library = f.read()
    name = 'sdp_problem_montecarlo_lookahead'
    assert re.search(r'^int {}\('.format(name), header, re.M)
    assert 'extern "C" int {}('.format(name) in library
    assert hasattr(nat.lib(), name)
    assert name in nat.EXPORTS


def test_refusals_come_before_a_device_is_touched(monkeypatch):
    monkeypatch.setattr(nat, 'require_gpu', lambda *a, **k: pytest.fail('a device was asked for'))
    monkeypatch.setattr(nat, 'lib', lambda *a, **k: pytest.fail('the library was asked for'))
    s = lc.symbolic_time()
    dims = tuple(len(g) for g in s.state_grid)
    J = np.zeros(dims)
    J_all = np.zeros((8,) + dims)
    x0 = np.zeros((3, 2))
    # the cost-to-go: check_horizon's messages
    for bad in (J[:-1], J_all[:, :-1], J_all[None]):
        with pytest.raises(ValueError) as err:
            s.monte_carlo_lookahead(bad, x0, 2)
        assert 'T_J' in str(err.value) and str(bad.shape) in str(err.value)
    with pytest.raises(ValueError) as err:
        s.monte_carlo_lookahead(J_all, x0, 6, t0=3)
    assert all(n in str(err.value) for n in ('t0 = 3', 'n_steps = 6', 'T_J = 8')), str(err.value)
    with pytest.raises(ValueError) as err:
        s.monte_carlo_lookahead(J_all, x0, 2, t0=-1)
    assert 'T_J = 8' in str(err.value)
    # monte_carlo's conventions
    for kw in (dict(x0=np.zeros((3, 3))), dict(x0=np.zeros(2)), dict(x0=np.zeros(3), n_traj=4), dict(n_traj=4),
               dict(n_steps=0), dict(n_burn=2), dict(n_burn=-1), dict(seed=-1), dict(seed=1 << 64), dict(traj_offset=-1),
               dict(traj_offset=(1 << 64) - 2), dict(law=(np.zeros(3), np.ones(3))), dict(law=(np.zeros(3), np.ones(2) / 2)),
               dict(law=(np.zeros(4097), np.ones(4097) / 4097)), dict(law=(np.zeros(3),)), dict(path='fast')):
        args = dict(dict(J_next=J, x0=x0, n_steps=2), **kw)
        with pytest.raises(ValueError):
            s.monte_carlo_lookahead(**args)
    s.steps_per_launch = 0
    with pytest.raises(ValueError):
        s.monte_carlo_lookahead(J, x0, 2)
    s.steps_per_launch = 1024
    # a deterministic system has nothing to draw
    with pytest.raises(ValueError) as err:
        lc.deterministic().monte_carlo_lookahead(np.zeros(11), np.zeros((3, 1)), 2)
    assert 'simulate_lookahead' in str(err.value)
    # a communicator of several ranks
    s.comm = _Ranks()
    with pytest.raises(NotImplementedError):
        s.monte_carlo_lookahead(J, x0, 2)
