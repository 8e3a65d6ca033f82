"""Closed loops of families under lookahead controls over a horizon, on the CPU
(tests/family_lookahead_horizon_cases.py): every unit cross-compiles for gfx950 with exactly its kernels, free of scratch
memory, vector spills and static LDS, says what it is and is refused by the other loaders' flag checks; the old units keep
their text; the helpers are written once; header, library and binding move together; what
`SolverFamily.simulate_lookahead` and `SolverFamily.monte_carlo_lookahead_horizon` refuse before a device is touched; the
chunk rule and the byte counts, restated; the inputs of the GPU tests have the properties those tests rely on, by the numpy
definition; and the build compiles the units of the GPU tests.  No GPU."""
import os
import re

import numpy as np
import pytest

import family_lookahead_cases as flc
import family_lookahead_horizon_cases as fhl
import lookahead_cases as lc
from test_family_plan import _kernels, _digests, ROOT
from test_family_lookahead_plan import _member, digest, NOTES
from stodynprog_amd import SolverFamily, codegen, lookahead as la, _native as nat

UNITS = fhl.PARITY + [fhl.MAPPING[9], fhl.NO_LATTICE]
read = lambda *path: open(os.path.join(*path)).read()


def _tables(case):
    fam = fhl.family(case)
    return (fam,) + fam._lookahead_horizon_tables(case.n_steps, case.t0)


@pytest.mark.parametrize('case', UNITS + [fhl.DETERMINISTIC], ids=repr)
def test_the_unit_compiles_with_its_kernels(case, tmp_path):
    fam, tabs, table, prm_timed, look = _tables(case)
    source = look['source']
    assert '#define SDP_FAMILY 1' in source and '#define SDP_FAMILY_LOOKAHEAD_HORIZON 1' in source
    assert '#define SDP_FAMILY_LOOKAHEAD ' not in source and '#include "sdp_family_lookahead_kernel.h"' not in source
    assert '#define SDP_LANES {}\n'.format(tabs['lanes']) in source and tabs['lanes'] == fhl.lanes(case)
    assert '#define SDP_NBOXPARAMS {} '.format(look['bprm'].shape[1]) in source
    assert source.rstrip().splitlines()[-1].startswith('#include "sdp_family_lookahead_horizon_kernel.h"')
    assert prm_timed == case.int_time and table.shape == (len(fam), case.n_steps if case.int_time else 1, tabs['prm'].shape[1])
    kernels = _kernels(source, tmp_path)
    both = ['sdp_family_montecarlo_lookahead_h', 'sdp_family_simulate_lookahead']
    assert sorted(kernels) == (both if fam.W else both[1:]), sorted(kernels)
    for name, f in sorted(kernels.items()):
        print(case, name, {n: f[n] for n in NOTES})
        assert f['.private_segment_fixed_size'] == 0 and f['.vgpr_spill_count'] == 0, (name, f)
        assert f['.group_segment_fixed_size'] == 0, (name, f)             # (the draw table is dynamic LDS)
        assert f['.max_flat_workgroup_size'] == fhl.THREADS == 256        # no launch bound beyond the workgroup size
    assert digest(source) in _digests() and digest(tabs['source']) in _digests(), case
    # the old units keep their text and every unit of the family has a key of its own
    old = [tabs['source']]
    if not case.int_time:
        old.append(fam._lookahead_tables(None if fam.stationnary else case.t0, 0)[1]['source'])
    for text in old:
        assert digest(text) in _digests(), case
    old.append(codegen.family_horizon_unit(tabs['model'], fam.dtype))
    assert len({codegen.source_key(t) for t in old + [source]}) == len(old) + 1


def test_pv_lookahead_is_what_the_issue_describes():
    fam, tabs, table, prm_timed, look = _tables(fhl.PV)
    boxes = fam._lookahead_boxes(0)
    assert all(len(b.param_index) == 6 and b.t_value is None for b in boxes)
    assert table.shape == (3, 6, 9) and prm_timed and tabs['lanes'] == 64 and fam.W == 0
    # (the rows of a member differ from step to step: at least four different ones among the six)
    assert all(len({table[p, k].tobytes() for k in range(6)}) >= 4 for p in range(3)), table[:, :, :]


def test_the_unit_says_what_it_is_and_the_library_checks_it():
    header = read(codegen.CSRC, 'sdp_family_lookahead_horizon_kernel.h')
    shared = read(codegen.CSRC, 'sdp_family_lookahead_kernel.h')
    args = read(codegen.CSRC, 'sdp_kernel_args.h')
    library = read(codegen.CSRC, 'sdp_hip.hip')
    assert 'SDP_META_F_FAMILY_LOOKAHEAD_HORIZON = 65536' in args
    assert 'struct SdpFamilyLookSimArgs {' in args and 'struct SdpFamilyLookMcHArgs {' in args
    assert 'SDP_META_F_FAMILY | SDP_META_F_FAMILY_LOOKAHEAD_HORIZON, SDP_NBOXPARAMS, 0, SDP_FLOOK_THREADS, SDP_LANES' in header
    # its own loader takes the flag, the workgroup size and the lanes; the other loaders' flag checks refuse the unit
    assert '!(m[SDP_META_FLAGS] & SDP_META_F_FAMILY_LOOKAHEAD_HORIZON)' in library
    own = 65536 | 1024
    for other in ('SDP_META_F_FAMILY_POLICY = 2048', 'SDP_META_F_FAMILY_MC = 4096', 'SDP_META_F_FAMILY_LOOKAHEAD = 8192',
                  'SDP_META_F_FAMILY_HORIZON = 16384', 'SDP_META_F_FAMILY_TRANS = 32768'):
        name, value = other.split(' = ')
        assert other in args and not own & int(value) and '!(m[SDP_META_FLAGS] & {})'.format(name) in library
    for kernel, block in (('sdp_family_simulate_lookahead', 'SdpFamilyLookSimArgs'), ('sdp_family_montecarlo_lookahead_h', 'SdpFamilyLookMcHArgs')):
        assert 'void __launch_bounds__(SDP_FLOOK_THREADS) {}({} a)'.format(kernel, block) in header
    # the helpers are written once: defined in the lookahead header, called here
    assert '#define SDP_FLOOK_HELPERS_ONLY 1' in header and '#include "sdp_family_lookahead_kernel.h"' in header
    assert '#if !defined(SDP_FLOOK_HELPERS_ONLY)' in shared
    for helper in ('sdp_flook_walk(', 'sdp_flook_box(', 'sdp_flook_backup('):
        define = r'^SDP_DEV \w+ ' + re.escape(helper)
        assert len(re.findall(define, shared, re.M)) == 1 and not re.search(define, header, re.M) and helper in header, helper
    assert shared.index('#if !defined(SDP_FLOOK_HELPERS_ONLY)') > shared.index('SDP_DEV void sdp_flook_backup(')
    for helper in ('sdp_family_member(', 'sdp_philox4x32_10(', 'sdp_mc_index(', 'sdp_mc_visit('):
        assert helper in header and not re.search(r'^SDP_DEV \w+ ' + re.escape(helper), header, re.M), helper
    # one grid rule for the four lookahead launches of a family
    assert library.count('static unsigned family_lookahead_grid(') == 1 and library.count('family_lookahead_grid(f, ') == 4
    for kernel in ('f->f_lh_simulate', 'f->f_lh_montecarlo'):
        assert 'family_lookahead_grid(f, {}, B, '.format(kernel) in library
    # the new header is in the key of its units alone
    assert 'sdp_family_lookahead_horizon_kernel.h' not in codegen._HEADERS
    # the ABI: header, library and binding move together
    abi = read(ROOT, 'include', 'sdp_hip.h')
    lib = nat.lib()
    for name in ('sdp_family_load_lookahead_horizon_unit', 'sdp_family_simulate_lookahead', 'sdp_family_montecarlo_lookahead_h'):
        assert re.search(r'^int {}\('.format(name), abi, re.M) and 'extern "C" int {}('.format(name) in library
        assert name in nat.EXPORTS and hasattr(lib, name)
    assert lib.sdp_family_load_lookahead_horizon_unit(None, None) == -1
    assert lib.sdp_family_simulate_lookahead(None, None, 1, 0, None, 0, 0, 1, 1, 1, None, None, 0., None, None, None, None) == -1
    assert lib.sdp_family_montecarlo_lookahead_h(None, None, 1, 0, None, 0, 0, 1, 1, 1, 0, None, 0, None, None, 1, None, 0., 1,
                                                 None, None, None, None) == -1


def test_the_keys_cover_the_headers_the_unit_includes(monkeypatch, tmp_path):
    fam, tabs, _, _, look = _tables(fhl.AR1_64)
    units = [look['source'], fam._lookahead_tables(None, 0)[1]['source'], tabs['source']]
    csrc = tmp_path / 'csrc'
    csrc.mkdir()
    for fn in os.listdir(codegen.CSRC):
        if fn.endswith('.h'):
            (csrc / fn).write_bytes(open(os.path.join(codegen.CSRC, fn), 'rb').read())
    monkeypatch.setattr(codegen, 'CSRC', str(csrc))
    codegen._digest_cache.clear()
    now = lambda: [codegen.source_key(u) for u in units]

    def edit(fn):
        before = now()
        with open(str(csrc / fn), 'a') as f:
            f.write('// edited\n')
        codegen._digest_cache.clear()
        return [a != b for a, b in zip(before, now())]
    # (the unit over a horizon, the lookahead unit, the sweep unit)
    assert edit('sdp_family_lookahead_horizon_kernel.h') == [True, False, False]
    assert edit('sdp_family_lookahead_kernel.h') == [True, True, False]
    assert edit('sdp_lattice_kernel.h') == [True, True, False]
    assert edit('sdp_family_kernel.h') == [True, True, True]
    codegen._digest_cache.clear()


# ----------------------------------------------------------------------------------------------------------------------
# refusals

def test_argument_checks_come_before_a_device_is_touched(monkeypatch):
    monkeypatch.setattr(nat, 'require_gpu', lambda *a, **k: pytest.fail('a device was asked for'))
    monkeypatch.setattr(nat, 'lib', lambda *a, **k: pytest.fail('the library was asked for'))
    monkeypatch.setattr(nat, 'compile_model', lambda *a, **k: pytest.fail('the compiler was asked for'))
    fam = fhl.family(fhl.AR1_64)
    J, x0, w = np.zeros((3, 6, 7, 5)), np.zeros((3, 4, 2)), np.zeros((3, 5, 4))
    sim = lambda J_, x_, w_=w, **kw: fam.simulate_lookahead(J_, x_, w_, **kw)
    mc = lambda J_, x_, w_=None, **kw: fam.monte_carlo_lookahead_horizon(J_, x_, kw.pop('n_steps', 5), **kw)
    for call in (sim, mc):
        for bad in (np.zeros((6, 3, 7, 5)), np.zeros((2, 6, 7, 5)), np.zeros((1, 3, 6, 7, 5)), np.zeros((7, 4)), np.zeros((2, 7, 5)),
                    np.zeros((3, 6, 7, 4)), np.zeros(5)):
            with pytest.raises(ValueError) as err:
                call(bad, x0)
            assert 'J_next' in str(err.value) and str(bad.shape) in str(err.value)
        for bad in (np.zeros(3), np.zeros((4, 3)), np.zeros((2, 4, 2)), np.zeros((3, 4, 2, 1)), np.zeros(())):
            with pytest.raises(ValueError) as err:
                call(J, bad, **({'n_traj': 4} if call is mc else {}))
            assert 'x0' in str(err.value)
        # the range of the cost-to-go, and its index
        for kw in (dict(t0=2), dict(t0=-1), dict(n_steps=7)):
            with pytest.raises(ValueError) as err:
                call(J, x0, np.zeros((3, 7, 4)), **kw)
            assert 'T_J = 6' in str(err.value), kw
        with pytest.raises(ValueError) as err:
            call(J, x0, t0=0.5)
        assert 'integer' in str(err.value) and 'time-indexed cost-to-go' in str(err.value)
    for bad in (np.zeros((5, 3)), np.zeros((2, 5, 4)), np.zeros((3, 5, 4, 1))):
        with pytest.raises(ValueError) as err:
            sim(J, x0, bad)
        assert 'w must have shape' in str(err.value)
    with pytest.raises(ValueError) as err:
        sim(J, x0, None)
    assert 'perturbation' in str(err.value)
    with pytest.raises(ValueError) as err:
        sim(J, x0, w, n_steps=6)
    assert 'w holds 5 steps' in str(err.value)
    with pytest.raises(ValueError) as err:
        mc(J, np.zeros(2))
    assert 'n_traj' in str(err.value)
    for kw in (dict(n_steps=0), dict(n_burn=5), dict(n_burn=-1)):
        with pytest.raises(ValueError) as err:
            mc(J, x0, **kw)
        assert 'n_burn' in str(err.value)
    for seed in (-1, 1 << 64, (1, 2)):
        with pytest.raises(ValueError) as err:
            mc(J, x0, seed=seed)
        assert 'seed' in str(err.value)
    with pytest.raises(ValueError) as err:
        mc(J, x0, traj_offset=-1)
    assert 'trajectory ids' in str(err.value)
    grid, proba = np.linspace(-1., 1., 5), np.full(5, 0.2)
    with pytest.raises(ValueError) as err:
        mc(J, x0, law=[(grid, proba), (grid[:4], np.full(4, 0.25)), (grid, proba)])
    assert 'member 1' in str(err.value) and '4 points' in str(err.value)
    # a data[k] model needs an integer time index
    lookup = fhl.family(fhl.LOOKUP)
    for call in (lambda: lookup.simulate_lookahead(np.zeros(9), np.zeros((4, 1)), np.zeros((3, 4)), t0=0.5),
                 lambda: lookup.monte_carlo_lookahead_horizon(np.zeros(9), np.zeros((4, 1)), 3, t0=0.5)):
        with pytest.raises(ValueError) as err:
            call()
        assert 'integer' in str(err.value) and 'data[k]' in str(err.value)
    # a control_box that does not trace, traces only at a concrete time index, or uses inexact operations
    data = np.linspace(0., 1., 16)

    def untraceable(x):
        return ((-1., float(np.asarray(x).reshape(()) * 0. + 1.)),)
    boxes = dict(untraceable=(_member(), _member(box=untraceable)),
                 concrete=(_member(stationnary=False), _member(stationnary=False, box=lambda k, x: ((-1., 1. + data[k]),))),
                 inexact=(_member(), _member(box=lambda x: ((-1., 1. + np.exp(0. * x)),))))
    for name, members in boxes.items():
        other = SolverFamily(list(members))
        for call in (lambda: other.simulate_lookahead(np.zeros(9), np.zeros((4, 1)), np.zeros((3, 4)), t0=2),
                     lambda: other.monte_carlo_lookahead_horizon(np.zeros(9), np.zeros((4, 1)), 3, t0=2)):
            with pytest.raises(NotImplementedError) as err:
                call()
            assert 'member 1' in str(err.value) and 'control_box' in str(err.value), (name, str(err.value))
    other = SolverFamily([_member(), _member(box=lambda x: ((-1., 1. + 0.5 * x),))])
    with pytest.raises(ValueError) as err:
        other.simulate_lookahead(np.zeros(9), np.zeros((4, 1)), np.zeros((3, 4)))
    assert str(err.value).startswith("member 1: the structure of the traced control_box differs from member 0's")
    # coinciding box constants: family_cases' pv_sized, refused by member
    refused = fhl.family(fhl.PV_REFUSED)
    with pytest.raises(ValueError) as err:
        refused.simulate_lookahead(np.zeros(9), np.zeros((4, 1)), n_steps=6)
    assert str(err.value).startswith('member 1: constants that coincide in member 1 make its traced control_box another structure '
                                     '(5 distinct constants against 6)')
    # deterministic members: the solo message, by member
    det = SolverFamily([_member(W=False), _member(W=False)])
    with pytest.raises(ValueError) as err:
        det.monte_carlo_lookahead_horizon(np.zeros(9), np.zeros((4, 1)), 5)
    solo = pytest.raises(ValueError, _member(W=False).monte_carlo_lookahead, np.zeros(9), np.zeros((4, 1)), 5)
    assert str(err.value) == 'member 0: ' + str(solo.value) and 'simulate_lookahead' in str(err.value)
    with pytest.raises(ValueError) as err:
        det.simulate_lookahead(np.zeros(9), np.zeros((4, 1)))
    assert 'n_steps' in str(err.value)


# ----------------------------------------------------------------------------------------------------------------------
# the cuts and the bytes, restated

def test_the_chunk_rule_and_the_byte_counts():
    library = read(codegen.CSRC, 'sdp_hip.hip')
    for line in ('const size_t step_bytes = (size_t)f->P * f->S * real_size(f->dtype);',
                 'int64_t n = V_timed ? (int64_t)((size_t)chunk_bytes / step_bytes) : T;', 'a.chunk_first = V_timed ? c : 0;'):
        assert line in library, line
    P, S, rs, T = 5, 35, 8, 6
    step = P * S * rs
    assert fhl.step_chunks(P, S, rs, T, step + 8) == [(k, k + 1) for k in range(6)]
    assert fhl.step_chunks(P, S, rs, T, step - 1) == [(k, k + 1) for k in range(6)]          # a larger step: a chunk of its own
    assert fhl.step_chunks(P, S, rs, T, 2 * step + 8) == [(0, 2), (2, 4), (4, 6)]
    assert fhl.step_chunks(P, S, rs, T, 4 * step) == [(0, 4), (4, 6)]
    assert fhl.step_chunks(P, S, rs, T, 1 << 40) == [(0, 6)] == fhl.step_chunks(P, S, rs, T, 1, timed=False)
    assert fhl.launches([(0, 4), (4, 6)]) == 2 and fhl.launches([(0, 4), (4, 6)], 3) == 3 and fhl.launches([(0, 6)], 1) == 6
    # SolverFamily._horizon_info restates the same rule on the array the call hands over
    fam = fhl.family(fhl.CUTS)
    assert (len(fam), int(np.prod(fam.dims)), fam.dtype.itemsize) == (P, S, rs)
    V_d, timed = fam._horizon_cost_to_go(fhl.cost_to_go(fhl.CUTS), T, 0)
    assert V_d.shape == (P, T, 1, S) and timed
    for chunk_bytes, spl in ((step + 8, None), (2 * step + 8, 3), (4 * step, 3), (1 << 40, 4)):
        fam.horizon_chunk_bytes = chunk_bytes
        fam.backend_info = {}
        fam._horizon_info([(0, P)], 21, T, V_d, True, False, spl)
        chunks = fhl.step_chunks(P, S, rs, T, chunk_bytes)
        info = fam.backend_info['horizon']
        assert (info['step_chunks'], info['launches']) == (len(chunks), fhl.launches(chunks, spl)), (chunk_bytes, info)
    one, timed = fam._horizon_cost_to_go(fhl.cost_to_go(fhl.CUTS, timed=False), T, 0)
    assert one.shape == (P, 1, 1, S) and not timed
    # the bytes of a member, and the member chunks they give
    tabs, table, prm_timed, look = fam._lookahead_horizon_tables(T, 0)
    n_box = look['bprm'].shape[1]
    assert look['bytes'] == 8 * (n_box + fam.nu) and n_box == 5
    B = 21
    assert fhl.sim_extra_bytes(fam, B, T, T, 1, n_box) == (T * S + 5) * 8 + (2 * B + T * B + (T + 1) * 2 * B + T * 2 * B + 2 * T * B) * 8 + 8 * 7
    assert fhl.mc_extra_bytes(fam, B, 3, True, T, 1, n_box) == flc.mc_extra_bytes(fam, B, 3, True, n_box) + (T * S + 5) * 8
    fam.chunk_bytes = flc.chunk_bytes_for(fam, 3, fhl.sim_extra_bytes(fam, B, T, T, 1, n_box))
    assert fam._chunks(tabs, fhl.sim_extra_bytes(fam, B, T, T, 1, n_box)) == [(0, 3), (3, 5)]


# ----------------------------------------------------------------------------------------------------------------------
# the inputs of the GPU tests, by the numpy definition

def _definition(s, J, x0, T, t0, tamper=None):
    """(x, u, g, q, idx per step) of stodynprog_amd.lookahead.simulate_lookahead on the host with the oracle's backup as its
    step.  tamper: None, or 'J' (every step looks ahead into J[t0]) or 'k' (the model is called with the time index t0)"""
    look = lc.Case('member', lambda: s, int_time=True)
    spec = lc.spec_of(look, s)
    seen = []

    def step(J_k, x_k, t_k):
        q, u, idx = lc.oracle_lookahead(s, spec, J[t0] if tamper == 'J' else J_k, x_k, t_k)
        seen.append(idx)
        return q, u, idx
    if tamper == 'k':
        sd, dyn, cost = s.sys, s.sys.dyn, s.sys.cost
        assert (len(sd.state), len(sd.control), len(sd.perturb)) == (1, 1, 0)
        sd.dyn = lambda k, x_, u_: dyn(t0, x_, u_)
        sd.cost = lambda k, x_, u_: cost(t0, x_, u_)
    x, u, g, q = la.simulate_lookahead(s, J, x0, None if not s.perturb_grid else lc.draws(s, T, len(x0))[0][:, None, :], T, t0,
                                       'int', step=step)
    return x, u, g, q, np.stack(seen)


@pytest.mark.parametrize('case', (fhl.FINITE, fhl.PV), ids=repr)
def test_the_inputs_discriminate(case):
    J = fhl.cost_to_go(case)
    x0 = fhl.starts(case, 9)
    T, t0 = case.n_steps, case.t0
    differ = []
    for p, s in enumerate(case.solvers()):
        x, u, g, q, idx = _definition(s, J[p], x0[p], T, t0)
        assert not np.isnan(x).any() and not np.isnan(q).any()
        lo, hi = [a[0] for a in s.state_grid], [a[-1] for a in s.state_grid]
        assert np.all((x >= lo) & (x <= hi)), p                                    # nothing outside the grid
        assert idx.max() > 0 and len(np.unique(idx)) > 1, (p, np.unique(idx))
        _, u_flat, _, _, _ = _definition(case.members[p](), J[p], x0[p], T, t0, tamper='J')
        differ.append([k for k in range(1, T) if not np.array_equal(u[k], u_flat[k])])
        if case is fhl.PV:
            _, _, g_k, _, _ = _definition(case.members[p](), J[p], x0[p], T, t0, tamper='k')
            assert not np.array_equal(g, g_k), p
    print(case, 'steps whose controls change with the cost-to-go of step t0 at every step:', differ)
    assert all(len(k) >= 1 for k in differ), differ


def test_the_build_compiles_the_units_of_the_gpu_tests():
    units = fhl.unit_sources()
    for case in fhl.FAMILIES:
        fam, tabs, _, _, look = _tables(case)
        assert tabs['source'] in units and look['source'] in units, case
    for case in fhl.PARITY + [fhl.CUTS, fhl.DETERMINISTIC]:
        times = range(case.t0, case.t0 + case.n_steps) if case.int_time else [None if case.solvers()[0].sys.stationnary else case.t0]
        for s in case.solvers():
            assert all(lc.unit_source(s, t) in units for t in times), case
    assert '#define SDP_FAMILY_LOOKAHEAD_HORIZON 1' in _tables(fhl.PV)[4]['source']
    assert 'family_lookahead_horizon_cases.unit_sources()' in read(ROOT, '__graft_entry__.py')
    table = _digests()
    assert all(digest(u) in table for u in units)
