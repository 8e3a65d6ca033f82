"""The time-dependent families and column forms of tests/horizon_cases.py still mean what they say, without a GPU: at
every step of the horizon each one plans the family, the form and the control-table capacity it claims, steps whose
lattices share a capacity share one generated source, the units compile for gfx950, and a horizon keeps one trace."""
import os

import numpy as np
import pytest

import column_forms as cf
import horizon_cases as hc
from policies import family_of
from stodynprog_amd import DPSolver, codegen, solver as solver_module
from stodynprog_amd.trace import TraceError


def step_plans(s, T):
    """the plan of every step k = 0 .. T - 1 (as bellman_recursion makes them, with the step's own trace)"""
    out = []
    for k in range(T):
        model = s._trace_now(k)
        out.append((model, None if isinstance(model, TraceError) else s._kernel_plan(k, model)))
    return out


@pytest.mark.parametrize('fam', hc.FAMILIES, ids=[f.name for f in hc.FAMILIES])
def test_family_plans_what_it_claims_at_every_step(fam):
    s = fam.solver()
    assert len(fam.sizes) == hc.T
    if fam.form == 'tabulated':
        assert all(isinstance(m, TraceError) for m, _ in step_plans(s, hc.T))
        return
    by_capacity = {}
    for k, (model, plan) in enumerate(step_plans(s, hc.T)):
        assert not isinstance(model, TraceError), (fam, k, model)
        assert (model.t_value is not None) == fam.info['time_specialized'], (fam, k)
        if model.t_value is not None:
            assert model.t_value == k and model.param_index, (fam, k)
        assert plan['max_u'] == fam.sizes[k], (fam, k, plan['max_u'])
        assert family_of(plan) == fam.form, (fam, k, family_of(plan))
        src = plan['source']
        cap = hc.capacity(fam.sizes[k])
        if fam.table:
            assert cf.macro(src, 'SDP_COL_UTAB_N') == str(cap), (fam, k, cf.macro(src, 'SDP_COL_UTAB_N'))
            assert cf.macro(src, 'SDP_COL_FILTER') == '1', (fam, k)
            shift = fam.info.get('filter_form') == 'shifted lattice'
            assert cf.macro(src, 'SDP_COL_SHIFT') == ('1' if shift else None), (fam, k)
        by_capacity.setdefault(cap, set()).add(src)
    # steps whose lattices share a capacity share one source; another capacity is another source
    assert all(len(v) == 1 for v in by_capacity.values()), fam
    sources = set.union(*by_capacity.values())
    assert len(sources) == fam.units, (fam, len(sources))
    if fam.table:
        assert sorted(by_capacity) == [1, 8, 16, 32]


def test_the_horizon_takes_the_lattice_sizes_it_is_for():
    for sizes in {f.sizes for f in hc.FAMILIES}:
        s = set(sizes)
        assert 1 in s and any(n < 8 and n > 1 for n in s)
        assert any(n % 8 == 1 and n > 1 for n in s)
        assert any(n & (n - 1) == 0 and n > 1 for n in s)
        assert any((n + 1) & n == 0 and n > 1 for n in s)                     # 2^p - 1
        assert any(n > 2 and (n - 1) & (n - 2) == 0 for n in s)               # 2^p + 1
    # the 1-control step is the midpoint rule of the reference (width / step < 0.1)
    assert hc.widths(0.125, [1])[0] / 0.125 < 0.1
    d = hc.TIME_DATA
    assert 0.0 in d and any(v == 0.0 and np.signbit(v) for v in d) and any(v < 0 for v in d)
    assert any(a * b < 0 for a, b in zip(d, d[1:]))
    assert any(a == b == hc.EQUAL_LITERAL for a, b in zip(d, d[1:]))


@pytest.mark.parametrize('case,geometry', hc.PAIRS, ids=['{}-{}'.format(c.name, g) for c, g in hc.PAIRS])
def test_case_plans_the_form_at_every_step(case, geometry, debug_defines):
    if case.debug:
        debug_defines.set(**case.debug)
    else:
        debug_defines.unset('SDP_COL_WRES')
    s = case.solver(geometry)
    sources = set()
    for k, (model, plan) in enumerate(step_plans(s, len(case.sizes))):
        assert model.t_value is None and plan['max_u'] == case.sizes[k], (case, k)
        src = plan['source']
        assert family_of(plan) == 'column' and '#include "sdp_column_kernel.h"' in src, (case, k)
        claims = case.claims(geometry)
        missing = [(m, v, cf.macro(src, m)) for m, v in sorted(claims.items()) if cf.macro(src, m) != v]
        assert not missing, '{} at {}, step {}: (macro, claimed, planned) {}'.format(case, geometry, k, missing)
        assert cf.hold_geometry(src) == case.hold, (case, geometry, k)
        if case.utab_n is not None:
            assert case.utab_n == hc.capacity(max(case.sizes))
        sources.add(src)
    assert len(sources) == case.units, (case, geometry)
    below = tuple(k for k, n in enumerate(case.sizes) if case.utab_n is not None and n < case.utab_n)
    assert below == case.below, (case, below)
    # the kernels it is compared with: the same family without the filter, and the direct kernel
    m = s._trace_now(0)
    assert cf.macro(case.solver(geometry, certified_filter=False)._kernel_plan(0, m)['source'], 'SDP_COL_FILTER') is None
    assert '#include "sdp_column_kernel.h"' not in case.solver(geometry, kernel='generic')._kernel_plan(0, m)['source']


def test_every_case_with_a_table_runs_below_its_capacity():
    for c in hc.CASES:
        if c.utab_n is not None:
            assert c.below, c
            assert hc.capacity(max(c.sizes)) == c.utab_n
    assert {c.name for c in hc.CASES} == {'hold_8x2x4', 'hold_8x2x4_noise', 'hold_16x1x4_u200', 'bnb_u57', 'res_n192',
                                          'full_n500', 'res1024_u301_noise', 'f32_n600', 'f32_n512_u601_no_table'}


def units(debug_defines=None):
    """every generated source the GPU test runs: {source: what it is for}"""
    out = {}
    for fam in hc.FAMILIES:
        if fam.form == 'tabulated':
            continue
        for kw in [dict()] + list(fam.compared().values()):
            s = fam.solver(**kw)
            for _, plan in step_plans(s, hc.T):
                out.setdefault(plan['source'], fam.name)
    saved = DPSolver.debug_defines
    try:
        for case, geometry in hc.PAIRS:
            DPSolver.debug_defines = dict(case.debug) or None
            for kw in (dict(), dict(certified_filter=False), dict(kernel='generic')):
                s = case.solver(geometry, **kw)
                for _, plan in step_plans(s, len(case.sizes)):
                    out.setdefault(plan['source'], case.name)
    finally:
        DPSolver.debug_defines = saved
    return out


@pytest.mark.timeout(1200)
def test_horizon_units_compile_for_gfx950():
    """(hipcc cross-compiles; `build()` compiles the same units ahead -- __graft_entry__._prebuild_models --, so on a
    built tree this finds them in the cache)"""
    from stodynprog_amd import _native as nat
    from concurrent.futures import ThreadPoolExecutor
    sources = units()
    with ThreadPoolExecutor(max_workers=min(6, os.cpu_count() or 1)) as pool:
        mods = list(pool.map(nat.compile_model, list(sources)))
    for (src, what), mod in zip(sources.items(), mods):
        assert mod and os.path.exists(mod), what


class _FakeProblem(object):
    """stands in for the device problem: returns the cost-to-go it was given"""
    def backup_host(self, V, t_k, rel_dp, ref_index, overlap=True):
        V = np.asarray(V, dtype=float)
        return V.copy(), np.zeros(V.shape + (1,)), 0.0


def test_a_horizon_keeps_one_trace_and_fingerprints_once_per_step(monkeypatch):
    s = hc.storage()
    T = 24
    wu = hc.widths(0.125, [9] * T)
    s.sys.control_box = lambda k, e, p: ((-1.0, -1.0 + wu[k]),)
    calls, traces, seen = [], [], []
    real_fp, real_trace = solver_module.callable_fingerprint, s._trace_now_uncached

    def fp(*fns):
        if fns and fns[0] is s.sys.dyn:
            calls.append(1)
        return real_fp(*fns)
    monkeypatch.setattr(solver_module, 'callable_fingerprint', fp)
    monkeypatch.setattr(s, '_trace_now_uncached', lambda t_k=None: traces.append(t_k) or real_trace(t_k))
    monkeypatch.setattr(s, '_problem', lambda t_k=None, model=None: seen.append((t_k, model)) or _FakeProblem())
    J_fin = np.random.default_rng(0).standard_normal(s._state_grid_shape)
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        J, _ = s.bellman_recursion(T, J_fin)
    assert np.array_equal(J[0], J_fin)
    assert [t for t, _ in seen] == list(range(T - 1, -1, -1))
    kept = [k for k in s._cache if isinstance(k, tuple) and k and k[0] == 'trace now']
    assert len(kept) <= 1, kept
    assert len(calls) == T, len(calls)
    # traced once, at the first step of the horizon; every step ran that one symbolic trace
    assert traces == [T - 1], traces
    assert all(m is seen[0][1] and m.t_value is None for _, m in seen)


def test_a_time_specialised_horizon_keeps_no_trace():
    s = hc.FAMILY['column data[k]'].solver()
    models = [s._trace_now(k) for k in range(hc.T)]
    assert [m.t_value for m in models] == list(range(hc.T))
    assert not [k for k in s._cache if isinstance(k, tuple) and k and k[0] == 'trace now']
    # (every step its own constants: the data of step k, lifted)
    assert models[0].param_values() != models[1].param_values()
