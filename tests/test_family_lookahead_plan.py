"""Lookahead controls on families on the CPU (tests/family_lookahead_cases.py): the lookahead unit cross-compiles for
gfx950 with exactly its two kernels, free of scratch memory, vector spills and static LDS; every other unit keeps its
text; the lifted box (TracedBox.lift_constants / structure_key / param_values) and its numpy twin; the family that
cannot share a box function; the tile-to-XCD mapping and the grid bound, restated; what `SolverFamily.lookahead` and
`SolverFamily.monte_carlo_lookahead` refuse before a device is touched; and the inputs of the GPU tests have the
properties those tests rely on, by the oracle.  No GPU."""
import hashlib
import os
import re

import numpy as np
import pytest

import family_cases as fc
import family_lookahead_cases as flc
import family_mc_cases as mcc
import lookahead_cases as lc
from test_family_plan import _kernels, _digests, ROOT
from stodynprog_amd import SolverFamily, DPSolver, SysDescription, codegen, _native as nat
from stodynprog_amd.models import NormalLaw
from stodynprog_amd.trace import TraceError

UNITS = flc.PARITY + [flc.MAPPING[9]]
NOTES = ('.vgpr_count', '.sgpr_count', '.private_segment_fixed_size', '.vgpr_spill_count', '.sgpr_spill_count',
         '.group_segment_fixed_size', '.max_flat_workgroup_size')
digest = lambda text: hashlib.sha256(text.encode('utf-8')).hexdigest()[:16]


def _tables(case, t='t_k'):
    fam = flc.family(case)
    return (fam,) + fam._lookahead_tables(None if fam.stationnary else getattr(case, t), 0)


@pytest.mark.parametrize('case', UNITS, ids=repr)
def test_the_unit_compiles_with_its_two_kernels(case, tmp_path):
    fam, tabs, look = _tables(case)
    source = look['source']
    assert '#define SDP_FAMILY 1' in source and '#define SDP_FAMILY_LOOKAHEAD 1' in source
    assert '#define SDP_LANES {}\n'.format(tabs['lanes']) in source and tabs['lanes'] == flc.lanes(case)
    assert '#define SDP_NBOXPARAMS {} '.format(look['bprm'].shape[1]) in source
    assert '#include "sdp_family_lookahead_kernel.h"' in source and 'sdp_model_cell_at(' in source
    assert 'SDP_DEV void sdp_model_box_at(const double *x, double t, const double *__restrict__ bprm, double *lo, double *hi)' in source
    assert '#include "sdp_family_kernel.h"' not in source and '#include "sdp_sweep_kernel.h"' not in source
    assert 'SDP_FAMILY_POLICY' not in source and 'SDP_FAMILY_MC' not in source and 'sdp_model_box(' not in source
    kernels = _kernels(source, tmp_path)
    assert sorted(kernels) == ['sdp_family_lookahead', 'sdp_family_montecarlo_lookahead'], sorted(kernels)
    for name, f in sorted(kernels.items()):
        print(case, name, {n: f[n] for n in NOTES})
        assert f['.private_segment_fixed_size'] == 0 and f['.vgpr_spill_count'] == 0, (name, f)
        assert f['.group_segment_fixed_size'] == 0, (name, f)             # (the draw table is dynamic LDS)
        assert f['.max_flat_workgroup_size'] == flc.THREADS == 256        # no launch bound beyond the workgroup size
    # the sweep, evaluation and Monte Carlo units of the same family keep the text on record; the new unit's is on record too
    policy = codegen.family_policy_unit(tabs['model'], fam.dtype)
    mc_unit = codegen.family_mc_unit(tabs['model'], fam.dtype)
    on_record = (tabs['source'], policy, mc_unit, source) if case.name in {c.name for c in mcc.PARITY} else (tabs['source'], source)
    for text in on_record:
        assert digest(text) in _digests(), case
    assert len({codegen.source_key(t) for t in (source, policy, mc_unit, tabs['source'])}) == 4


def test_the_units_of_record_keep_their_text():
    """the sweep, evaluation and Monte Carlo units of the families on record, and the solo lookahead units"""
    table = _digests()
    for case in mcc.PARITY:
        fam = SolverFamily(case.solvers())
        tabs = fam._tables()
        for text in (tabs['source'], codegen.family_policy_unit(tabs['model'], fam.dtype), codegen.family_mc_unit(tabs['model'], fam.dtype)):
            assert digest(text) in table, case
    for case in lc.TRACED:
        assert digest(lc.unit_source(case.solver(), case.times[0])) in table, case
    # the solo lookahead unit still names its own box function and the header that now includes the shared rule
    text = lc.unit_source(lc.BY_NAME['storage_ar1'].solver())
    assert 'sdp_model_box(' in text and 'sdp_model_box_at' not in text and 'bprm' not in text


def test_the_lattice_rule_is_written_once_and_both_keys_cover_it(monkeypatch, tmp_path):
    read = lambda fn: open(os.path.join(codegen.CSRC, fn)).read()
    rule, solo, family = read('sdp_lattice_kernel.h'), read('sdp_lookahead_kernel.h'), read('sdp_family_lookahead_kernel.h')
    assert 'ceil(n_interv) + 1.0' in rule and 'n_interv < 0.1' in rule and rule.count('const double n_interv') == 1
    for text in (solo, family):
        assert '#include "sdp_lattice_kernel.h"' in text and 'const double n_interv' not in text and 'sdp_look_lattice(' in text
    assert 'SDP_DEV void sdp_look_finish_box(' in rule and 'SDP_DEV void sdp_look_finish_box(' not in solo
    for fn in ('sdp_family_lookahead_kernel.h', 'sdp_lattice_kernel.h', 'sdp_lookahead_kernel.h', 'sdp_family_kernel.h'):
        assert fn not in codegen._HEADERS
    assert 'sdp_mc_kernel.h' in codegen._HEADERS
    fam, tabs, look = _tables(flc.PARITY[0])
    units = [look['source'], tabs['source'], codegen.family_mc_unit(tabs['model'], fam.dtype),
             lc.unit_source(lc.BY_NAME['inventory'].solver())]
    plain = lc.BY_NAME['inventory'].solver()
    plain.kernel = 'generic'
    units.append(plain._kernel_plan()['source'])
    csrc = tmp_path / 'csrc'
    csrc.mkdir()
    for fn in os.listdir(codegen.CSRC):
        if fn.endswith('.h'):
            (csrc / fn).write_bytes(open(os.path.join(codegen.CSRC, fn), 'rb').read())
    keys = [codegen.source_key(u) for u in units]
    monkeypatch.setattr(codegen, 'CSRC', str(csrc))
    codegen._digest_cache.clear()
    now = lambda: [codegen.source_key(u) for u in units]
    assert now() == keys

    def edit(fn):
        before = now()
        with open(str(csrc / fn), 'a') as f:
            f.write('// edited\n')
        codegen._digest_cache.clear()
        return [a != b for a, b in zip(before, now())]
    # (the family lookahead unit, the family sweep unit, the family Monte Carlo unit, a solo lookahead unit, a plain unit)
    assert edit('sdp_family_lookahead_kernel.h') == [True, False, False, False, False]
    assert edit('sdp_lattice_kernel.h') == [True, False, False, True, False]
    assert edit('sdp_family_kernel.h') == [True, True, True, False, False]
    assert edit('sdp_lookahead_kernel.h') == [False, False, False, True, False]
    assert edit('sdp_mc_kernel.h') == [True] * 5
    codegen._digest_cache.clear()


def test_the_unit_says_what_it_is_and_the_library_checks_it():
    read = lambda *path: open(os.path.join(*path)).read()
    header = read(codegen.CSRC, 'sdp_family_lookahead_kernel.h')
    args = read(codegen.CSRC, 'sdp_kernel_args.h')
    library = read(codegen.CSRC, 'sdp_hip.hip')
    sweep = read(codegen.CSRC, 'sdp_family_kernel.h')
    assert 'SDP_META_F_FAMILY_LOOKAHEAD = 8192' in args and 'SDP_META_F_FAMILY_MC = 4096,' in args
    assert 'struct SdpFamilyLookArgs {' in args and 'struct SdpFamilyLookMcArgs {' in args
    assert 'SDP_META_F_FAMILY | SDP_META_F_FAMILY_LOOKAHEAD, SDP_NBOXPARAMS, 0, SDP_FLOOK_THREADS, SDP_LANES' in header
    assert '#define SDP_FLOOK_THREADS {}'.format(flc.THREADS) in header
    assert '!(m[SDP_META_FLAGS] & SDP_META_F_FAMILY_LOOKAHEAD)' in library
    for kernel, block in (('sdp_family_lookahead', 'SdpFamilyLookArgs'), ('sdp_family_montecarlo_lookahead', 'SdpFamilyLookMcArgs')):
        assert 'void __launch_bounds__(SDP_FLOOK_THREADS) {}({} a)'.format(kernel, block) in header
    # the member's helpers and the draw helpers are included, not restated
    assert '#define SDP_MC_HELPERS_ONLY 1' in header and '#include "sdp_mc_kernel.h"' in header and '#include "sdp_family_kernel.h"' in header
    assert '!defined(SDP_FAMILY_LOOKAHEAD)' in sweep
    for helper in ('sdp_family_member(', 'sdp_family_expected_cost(', 'sdp_philox4x32_10(', 'sdp_mc_uniform(', 'sdp_mc_index(',
                   'sdp_mc_visit(', 'sdp_better_seq(', 'sdp_seg_argmin<'):
        assert helper in header and not re.search(r'^SDP_DEV \w+ ' + re.escape(helper), header, re.M), helper
    # the ABI: header, library and binding move together
    abi = read(ROOT, 'include', 'sdp_hip.h')
    real_lib = nat.lib()
    names = ('sdp_family_load_lookahead_unit', 'sdp_family_set_lookahead_box', 'sdp_family_lookahead', 'sdp_family_montecarlo_lookahead')
    for name in names:
        assert re.search(r'^int {}\('.format(name), abi, re.M) and 'extern "C" int {}('.format(name) in library
        assert name in nat.EXPORTS and hasattr(real_lib, name)
    assert real_lib.sdp_family_load_lookahead_unit(None, None) == -1
    assert real_lib.sdp_family_set_lookahead_box(None, None, 0, None) == -1
    assert real_lib.sdp_family_lookahead(None, 1, None, 0., None, None, None) == -1
    assert real_lib.sdp_family_montecarlo_lookahead(None, 1, 1, 0, None, 0, None, None, 1, None, 0., 1, None, None, None, None) == -1
    # the grid bound and the walk the restatement restates
    for line in ('const int64_t tile = (int64_t)(64 / f->look_lanes) * 4;', 'const int64_t cap = (int64_t)f->cus * per_cu / 8;',
                 'if (per_cu > 8) per_cu = 8;'):
        assert line in library, line
    for line in ('const int64_t tile = (int64_t)w.part * w.per_part + unit % w.per_part;',
                 'const int64_t p = w.first + 8 * (int)(unit / w.per_part);', 'if (p != loaded) {'):
        assert line in header, line


# ----------------------------------------------------------------------------------------------------------------------
# the lifted box

@pytest.mark.parametrize('case', flc.FAMILIES, ids=repr)
def test_the_members_boxes_have_one_structure_and_their_own_constants(case):
    fam = flc.family(case)
    t = None if fam.stationnary else case.t_k
    boxes = fam._lookahead_boxes(t)
    keys = {b.structure_key() for b in boxes}
    assert len(keys) == 1 and all(b.param_index is not None and b.t_value is None for b in boxes)
    values = [tuple(b.param_values()) for b in boxes]
    assert all(len(v) == len(boxes[0].param_index) for v in values)
    if case.name.startswith(('storage', 'finite', 'cuts', 'outside', 'deterministic')):
        assert len(set(values)) == len(values), values                   # (the constants differ from member to member)
    # the numpy twin of the lifted box function: member 0's DAG on member p's row gives member p's bits
    rng = np.random.default_rng(3)
    x = [rng.uniform(g[0] - 1., g[-1] + 1., size=33) for g in fam.solvers[0].state_grid]
    for p, b in enumerate(boxes):
        own = b.evaluate(x, t)
        twin = boxes[0].evaluate(x, t, params=values[p])
        fresh = fam.solvers[p]._trace_box_now(t).evaluate(x, t)
        for (a_lo, a_hi), (b_lo, b_hi), (c_lo, c_hi) in zip(own, twin, fresh):
            for a, b_, c in ((a_lo, b_lo, c_lo), (a_hi, b_hi, c_hi)):
                a, b_, c = (np.broadcast_to(np.asarray(v, dtype=float), (33,)) for v in (a, b_, c))
                assert np.array_equal(a.view(np.uint64), b_.view(np.uint64)) and np.array_equal(a.view(np.uint64), c.view(np.uint64))
    with pytest.raises(ValueError):
        boxes[0].evaluate(x, t, params=values[0] + (1.,))
    # the emitted function reads every slot and no literal of the box
    text = codegen.box_function_source(boxes[0], at=True)
    assert all('bprm[{}]'.format(i) in text for i in range(len(values[0]))) and 'sdp_model_prm' not in text
    assert text.count('(double)(') == 0, text
    with pytest.raises(ValueError):
        codegen.box_function_source(boxes[0])
    with pytest.raises(ValueError):
        codegen.box_function_source(fam.solvers[0]._trace_box_now(t), at=True)


def test_a_deterministic_family_carries_the_backup_alone(tmp_path):
    fam, tabs, look = _tables(flc.DETERMINISTIC)
    assert '#define SDP_HAS_W 0' in look['source'] and fam.W == 0
    kernels = _kernels(look['source'], tmp_path)
    assert sorted(kernels) == ['sdp_family_lookahead'], sorted(kernels)
    f = kernels['sdp_family_lookahead']
    assert f['.private_segment_fixed_size'] == 0 and f['.vgpr_spill_count'] == 0 and f['.group_segment_fixed_size'] == 0, f
    assert digest(look['source']) in _digests() and digest(tabs['source']) in _digests()


def test_the_lifted_box_has_the_body_of_the_literal_one():
    s = flc.PARITY[0].solvers()[0]
    plain = s._trace_box_now(None)
    lifted = s._trace_box_now(None)
    values = lifted.lift_constants()
    assert values == plain.param_values() == lifted.param_values()
    body = lambda text: text.split('{', 1)[1]
    at = body(codegen.box_function_source(lifted, at=True)).replace('    (void)x; (void)t; (void)bprm;', '    (void)x; (void)t;')
    for i, v in enumerate(values):
        at = at.replace('bprm[{}]'.format(i), codegen.real_literal(v).replace('sdp_real', 'double'))
    assert at == body(codegen.box_function_source(plain))


def test_the_sweep_family_whose_boxes_coincide_is_refused_by_name(monkeypatch):
    monkeypatch.setattr(nat, 'require_gpu', lambda *a, **k: pytest.fail('a device was asked for'))
    monkeypatch.setattr(nat, 'lib', lambda *a, **k: pytest.fail('the library was asked for'))
    monkeypatch.setattr(nat, 'compile_model', lambda *a, **k: pytest.fail('the compiler was asked for'))
    assert [a for a in fc.AR1 if a[1] == 1] == [fc.AR1[1]]                 # P_rated == dt == 1.0 in member 1's box
    fam = flc.family(flc.REFUSED)
    assert fam._tables()['source']                                         # (the sweep's family: boxes are tables there)
    for call in (lambda: fam.lookahead(np.zeros(fam.dims), np.zeros(2)),
                 lambda: fam.monte_carlo_lookahead(np.zeros(fam.dims), np.zeros((4, 2)), 3)):
        with pytest.raises(ValueError) as err:
            call()
        msg = str(err.value)
        assert msg.startswith('member 1: constants that coincide in member 1 make its traced control_box another structure '
                              '(4 distinct constants against 5)') and 'equal values are one node of the trace' in msg


# ----------------------------------------------------------------------------------------------------------------------
# the launch plan

@pytest.mark.parametrize('n_active', (1, 2, 4, 7, 8, 9, 17))
def test_the_launch_plan_on_256_compute_units(n_active):
    for B, lanes, per_cu in ((flc.B_MAPPING, 64, 8), (17, 16, 8), (4096, 64, 7), (flc.cap_batch(256), 64, 8), (flc.cap_batch(256), 64, 3)):
        plan = flc.launch(B, lanes, n_active, 256, per_cu)
        rows = (64 // lanes) * 4
        tiles = -(-B // rows)
        assert plan['tiles'] == tiles
        # every tile of every member exactly once
        seen = sorted((p, t) for xcd in plan['visits'] for p, t, _ in xcd)
        assert seen == [(p, t) for p in range(n_active) for t in range(tiles)]
        # a member's tiles stay on its XCDs
        for xcd, visits in enumerate(plan['visits']):
            for p, t, _ in visits:
                assert (p % 8 == xcd) if n_active >= 8 else (p * plan['parts'] <= xcd < (p + 1) * plan['parts'])
            if n_active < 8 and visits:
                ts = [t for _, t, _ in visits]
                assert ts == list(range(ts[0], ts[0] + len(ts)))         # a contiguous part
        assert plan['blocks'] % 8 == 0 and 8 <= plan['blocks'] <= max(8, 256 * min(per_cu, 8))
        assert plan['per_xcd'] == max(1, min(plan['wanted'], 256 * min(per_cu, 8) // 8))
    if n_active == 9:
        # the cap case of the GPU test walks again whatever the occupancy query answers, in member 8's last tiles
        B = flc.cap_batch(256)
        assert B == 909 and B % 4 == 1 and 9 * -(-B // 4) > 8 * 256
        for per_cu in range(1, 9):
            plan = flc.launch(B, 64, 9, 256, per_cu)
            later = {(p, t) for xcd in plan['visits'] for p, t, trip in xcd if trip >= 1}
            assert {(8, t) for t in range(plan['tiles'] - 3, plan['tiles'])} <= later
        # B = 5 with 64 lanes: two tiles, the second with one live group
        assert flc.launch(flc.B_MAPPING, 64, 9, 256, 8)['tiles'] == 2 and flc.B_MAPPING % 4 == 1


# ----------------------------------------------------------------------------------------------------------------------
# refusals

def _member(box=None, dyn=None, stationnary=True, W=True):
    data = np.linspace(0., 1., 16)
    lead = () if stationnary else ('k',)
    sysd = SysDescription((1, 1, 1 if W else 0), stationnary=stationnary, name='member')
    if stationnary:
        sysd.dyn = dyn or ((lambda x, u, w: (0.9 * x + u + w,)) if W else (lambda x, u: (0.9 * x + u,)))
        sysd.cost = (lambda x, u, w: x * x + 0.25 * u * u) if W else (lambda x, u: x * x + 0.25 * u * u)
        sysd.control_box = box or (lambda x: ((-1., 1.),))
    else:
        sysd.dyn = dyn or (lambda k, x, u, w: (0.9 * x + u + w + 0.01 * k,))
        sysd.cost = lambda k, x, u, w: x * x + 0.25 * u * u
        sysd.control_box = box or (lambda k, x: ((-1., 1. + 0.25 * k),))
    if W:
        sysd.perturb_laws = [NormalLaw(0, 0.1)]
    s = DPSolver(sysd)
    s.discretize_state(-2, 2, 9)
    if W:
        s.discretize_perturb(-0.3, 0.3, 3)
    s.control_steps = (0.125,)
    return s


def test_argument_checks_come_before_a_device_is_touched(monkeypatch):
    monkeypatch.setattr(nat, 'require_gpu', lambda *a, **k: pytest.fail('a device was asked for'))
    monkeypatch.setattr(nat, 'lib', lambda *a, **k: pytest.fail('the library was asked for'))
    monkeypatch.setattr(nat, 'compile_model', lambda *a, **k: pytest.fail('the compiler was asked for'))
    fam = flc.family(flc.PARITY[0])
    J, x0 = np.zeros((3, 7, 5)), np.zeros((3, 4, 2))
    both = (lambda J_, x_, **kw: fam.lookahead(J_, x_, **kw), lambda J_, x_, **kw: fam.monte_carlo_lookahead(J_, x_, 5, **kw))
    for call in both:
        # a time-indexed cost-to-go, or any extra leading axis
        for shape in ((6, 3, 7, 5), (3, 6, 7, 5), (1, 1, 3, 7, 5)):
            with pytest.raises(NotImplementedError) as err:
                call(np.zeros(shape), x0)
            assert 'time-indexed' in str(err.value)
        for bad in (np.zeros((7, 4)), np.zeros((2, 7, 5)), np.zeros(5)):
            with pytest.raises(ValueError) as err:
                call(bad, x0)
            assert str(bad.shape) in str(err.value)
        for bad in (np.zeros(3), np.zeros((4, 3)), np.zeros((2, 4, 2)), np.zeros((3, 4, 2, 1)), np.zeros(())):
            with pytest.raises(ValueError) as err:
                call(J, bad, **({'n_traj': 4} if call is both[1] else {}))
            assert 'x' in str(err.value)
    with pytest.raises(ValueError) as err:
        fam.monte_carlo_lookahead(J, np.zeros(2), 5)
    assert 'n_traj' in str(err.value)
    with pytest.raises(ValueError) as err:
        fam.monte_carlo_lookahead(J, x0, 5, n_traj=5)
    assert 'n_traj = 5' in str(err.value)
    for kw in (dict(n_steps=0), dict(n_steps=5, n_burn=5), dict(n_steps=5, n_burn=-1)):
        with pytest.raises(ValueError) as err:
            fam.monte_carlo_lookahead(J, x0, **kw)
        assert 'n_burn' in str(err.value)
    fam.steps_per_launch = 0
    with pytest.raises(ValueError) as err:
        fam.monte_carlo_lookahead(J, x0, 5)
    assert 'steps_per_launch' in str(err.value)
    del fam.steps_per_launch
    for seed in (-1, 1 << 64, (1, 2), (1, 2, -3)):
        with pytest.raises(ValueError) as err:
            fam.monte_carlo_lookahead(J, x0, 5, seed=seed)
        assert 'seed' in str(err.value)
    for offset in (-1, (1 << 64) - 3):
        with pytest.raises(ValueError) as err:
            fam.monte_carlo_lookahead(J, x0, 5, traj_offset=offset)
        assert 'trajectory ids' in str(err.value)
    grid, proba = np.linspace(-1., 1., 5), np.full(5, 0.2)
    with pytest.raises(ValueError) as err:
        fam.monte_carlo_lookahead(J, x0, 5, law=[(grid, proba), (grid[:4], np.full(4, 0.25)), (grid, proba)])
    assert 'member 1' in str(err.value) and '4 points' in str(err.value)
    with pytest.raises(ValueError) as err:
        fam.monte_carlo_lookahead(J, x0, 5, law=[(grid, proba)] * 2)
    assert 'sequence of 3' in str(err.value)
    # a time-dependent family needs its time index
    horizon = flc.family(flc.PARITY[3])
    with pytest.raises(ValueError) as err:
        horizon.lookahead(np.zeros(horizon.dims), np.zeros(1))
    assert 't_k' in str(err.value)
    # data[k] models
    data = np.linspace(0., 1., 16)
    def lookup_dyn(c):
        return lambda k, x, u, w: (c * x + u + w + data[k],)
    lookup = SolverFamily([_member(stationnary=False, dyn=lookup_dyn(c)) for c in (0.9, 0.8)])
    for call in (lambda: lookup.lookahead(np.zeros(9), np.zeros(1), 2), lambda: lookup.monte_carlo_lookahead(np.zeros(9), np.zeros((4, 1)), 5)):
        with pytest.raises(NotImplementedError) as err:
            call()
        assert 'member 0' in str(err.value) and 'data[k]' in str(err.value)
    # a control_box that does not trace, traces only at a concrete time index, or uses inexact operations
    def untraceable(x):
        return ((-1., float(np.asarray(x).reshape(()) * 0. + 1.)),)
    boxes = dict(untraceable=(_member(), _member(box=untraceable)),
                 concrete=(_member(stationnary=False), _member(stationnary=False, box=lambda k, x: ((-1., 1. + data[k]),))),
                 inexact=(_member(), _member(box=lambda x: ((-1., 1. + np.exp(0. * x)),))))
    for name, members in boxes.items():
        other = SolverFamily(list(members))
        t = None if other.stationnary else 2
        for call in (lambda: other.lookahead(np.zeros(9), np.zeros(1), t),
                     lambda: other.monte_carlo_lookahead(np.zeros(9), np.zeros((4, 1)), 5, t0=t or 0)):
            with pytest.raises(NotImplementedError) as err:
                call()
            assert 'member 1' in str(err.value) and 'control_box' in str(err.value), (name, str(err.value))
    # boxes of different structures
    other = SolverFamily([_member(), _member(box=lambda x: ((-1., 1. + 0.5 * x),))])
    with pytest.raises(ValueError) as err:
        other.lookahead(np.zeros(9), np.zeros(1))
    assert str(err.value).startswith("member 1: the structure of the traced control_box differs from member 0's")
    # deterministic members: the solo message, by member
    det = SolverFamily([_member(W=False), _member(W=False)])
    with pytest.raises(ValueError) as err:
        det.monte_carlo_lookahead(np.zeros(9), np.zeros((4, 1)), 5)
    solo = pytest.raises(ValueError, _member(W=False).monte_carlo_lookahead, np.zeros(9), np.zeros((4, 1)), 5)
    assert str(err.value) == 'member 0: ' + str(solo.value) and 'simulate_lookahead' in str(err.value)
    # the chunks of a lookahead call count its arrays beside the handle's
    tabs, look = fam._lookahead_tables(None, 1000)
    assert look['bytes'] == 1000 + 8 * (5 + 2) and look['bprm'].shape == (3, 5) and look['steps'].shape == (3, 2)
    extra = flc.mc_extra_bytes(fam, 21, 3, True, 5)
    assert extra == 3 * 21 * 8 + 8 * 21 + 8 * 35 + 3 * 16 + 8 + 8 * 7
    fam.chunk_bytes = flc.chunk_bytes_for(fam, 2, extra)
    assert fam._chunks(tabs, extra) == [(0, 2), (2, 3)]


# ----------------------------------------------------------------------------------------------------------------------
# the inputs of the GPU tests, by the oracle

@pytest.mark.parametrize('case', flc.PARITY, ids=repr)
def test_the_parity_members_exercise_the_argmin(case):
    J = flc.cost_to_go(case)
    _, _, idx = flc.oracle_lookahead(case, J, flc.states(case))
    distinct = [len(np.unique(i)) for i in idx]
    print(case, 'distinct optimal indices per member:', distinct)
    assert min(distinct) >= 3, distinct
    # the batch of the closed loop is a workgroup's tile and one more group
    fam = flc.family(case)
    lanes = fam._tables(None if fam.stationnary else case.t0)['lanes']
    assert ((64 // lanes) * 4 + 1) % ((64 // lanes) * 4) == 1


def test_three_d_strides_the_control_loop_and_the_lane_counts_differ():
    assert flc.lanes(flc.PARITY[2]) == 64
    s = flc.PARITY[2].solvers()[0]
    assert int(np.prod(s._box_plan(None)['n'].max(axis=1))) == 81
    assert [s._box_plan(None)['lanes'] for s in flc.PARITY[0].solvers()] == [8, 8, 16]
    assert flc.PARITY[3].t_k == 2 and flc.PARITY[3].t0 == 1 and flc.OFFSET > 1 << 32 and flc.SEED > 1 << 63


def test_the_outside_case_has_a_member_inside_and_a_member_outside():
    case, x0 = flc.OUTSIDE, flc.outside_starts()
    J = flc.cost_to_go(case)
    counts = [flc.oracle_monte_carlo(case, p, J[p], x0, flc.T, 0)[1] for p in range(2)]
    print('n_outside per member:', [int(c.sum()) for c in counts])
    assert counts[0].sum() == 0 and counts[1].sum() > 0
    grids = [s.state_grid for s in case.solvers()]
    assert grids[0][0][-1] == 10. and grids[1][0][-1] == 2. and np.all((x0[:, 0] >= 3.) & (x0[:, 0] <= 8.))


def test_the_laws_are_not_the_members_own_and_reach_both_branches_of_the_index():
    fam = flc.family(flc.LAWS)
    for p, (grid, proba) in enumerate(flc.member_laws()):
        s = fam.solvers[p]
        assert len(grid) == 9 != len(s.perturb_grid[0])
    idx, _ = fam.monte_carlo_draws(flc.SEED, 9, flc.T, law=flc.member_laws(), traj_offset=flc.OFFSET)
    assert all(len(np.unique(i)) >= 5 for i in idx), [len(np.unique(i)) for i in idx]
    idx, _ = fam.monte_carlo_draws(flc.SEED, 9, flc.T, law=flc.long_law(), traj_offset=flc.OFFSET)
    assert len(flc.long_law()[0]) == 70 and len(np.unique(idx)) >= 20
    with open(os.path.join(codegen.CSRC, 'sdp_mc_kernel.h')) as f:
        assert '#define SDP_MC_COUNT_MAX 64' in f.read()
    for case in flc.PARITY + [flc.SEEDS]:
        idx, _ = flc.family(case).monte_carlo_draws(flc.SEED, 9, flc.T, law=flc.spread_laws(case), traj_offset=flc.OFFSET)
        assert all(len(np.unique(i)) == 3 for i in idx), case


def test_the_no_lattice_members_lose_their_lattice_at_one_state_only():
    case = flc.NO_LATTICE
    boxes = flc.family(case)._lookahead_boxes(None)
    assert boxes[0].param_values() == boxes[1].param_values()           # (the decays differ in the model, not in the box)
    prm = flc.family(case)._tables()['prm']
    assert not np.array_equal(prm[0], prm[1])
    (lo, hi), = boxes[0].evaluate([np.array([lc.NAN_STATE, 0.5])])
    assert np.isnan(hi[0]) and hi[1] == 1.


def test_the_build_compiles_the_units_of_the_gpu_tests():
    units = flc.unit_sources()
    for case in flc.FAMILIES:
        for t in ('t_k', 't0'):
            fam, tabs, look = _tables(case, t)
            assert tabs['source'] in units and look['source'] in units, case
    for case in flc.SOLO:
        for s in case.solvers():
            assert lc.unit_source(s, case.t_k) in units and lc.unit_source(s, case.t0 if not s.sys.stationnary else None) in units
    with open(os.path.join(ROOT, '__graft_entry__.py')) as f:
        assert 'family_lookahead_cases.unit_sources()' in f.read()
