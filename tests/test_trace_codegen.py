"""Tracing of model callables and HIP source generation.  No GPU: the traced
DAG is interpreted with numpy and compared bit for bit with the callable; the
generated translation units are cross-compiled for gfx950 with hipcc."""
import os
import shutil

import numpy as np
import pytest

from stodynprog_amd import models, codegen, _native as nat
from stodynprog_amd.trace import trace_model, evaluate, TraceError, Sym
from stodynprog_amd import SysDescription, DPSolver

ALL = ['inventory', 'storage_ar1', 'searev', 'nas_demo', 'synthetic3d']


def _random_args(sysd, rng, n=257):
    x = [rng.uniform(-3, 6) for _ in sysd.state]
    u = [rng.uniform(-2, 2, n) for _ in sysd.control]
    w = [rng.uniform(-1, 1, n) for _ in sysd.perturb]
    return x, u, w


@pytest.mark.parametrize('name', ALL)
def test_trace_preserves_semantics_bitwise(name):
    sysd, solver = getattr(models, name)()
    model = solver._traced()
    assert not isinstance(model, TraceError)
    assert model.bit_exact, model.inexact_ops()
    rng = np.random.default_rng(0)
    for _ in range(5):
        x, u, w = _random_args(sysd, rng)
        xn_t, g_t = evaluate(model, x, u, w)
        xn = sysd.dyn(*(x + u + w))
        g = sysd.cost(*(x + u + w))
        for a, b in zip(xn_t, xn):
            assert np.array_equal(np.broadcast_to(a, (257,)), np.broadcast_to(b, (257,)))
        assert np.array_equal(np.broadcast_to(g_t, (257,)), np.broadcast_to(g, (257,)))


def test_trace_operator_coverage():
    def dyn(x, u, w):
        a = np.where((x > 0) & ~(u < 0) | (w == 0), np.abs(u) ** 2, np.sqrt(np.abs(w)))
        b = np.clip(x + u, -1, 1) + np.minimum(u, w) - np.maximum(u, 2 * w)
        c = np.sign(u) * np.floor(w * 3) + np.ceil(u) / (1 + u * u) + (-u) ** 0.5 * 0
        return (a + b + np.where(np.isnan(c), 0., c),)

    def cost(x, u, w):
        return (x - u) ** 2 + abs(w) + 1.0 / (1 + w ** 2) + (u > w) * 0.5

    m = trace_model(dyn, cost, 1, 1, 1)
    rng = np.random.default_rng(1)
    x, u, w = [0.3], [rng.uniform(-2, 2, 100)], [rng.uniform(-1, 1, 100)]
    with np.errstate(all='ignore'):
        xn_t, g_t = evaluate(m, x, u, w)
        assert np.array_equal(xn_t[0], dyn(x[0], u[0], w[0])[0], equal_nan=True)
        assert np.array_equal(g_t, cost(x[0], u[0], w[0]))
    assert m.bit_exact
    src = codegen.model_function_source(m)
    assert 'sdp_npmin' in src and 'sqrt(' in src


def test_inexact_ops_are_flagged():
    m = trace_model(lambda x, u, w: (x + np.sin(u) * np.exp(w),), lambda x, u, w: u ** 3, 1, 1, 1)
    assert not m.bit_exact and m.inexact_ops() == ['exp', 'pow', 'sin']


@pytest.mark.parametrize('bad', [
    lambda x, u, w: (x + u if u > 0 else x,),          # truth value of a symbol
    lambda x, u, w: (max(x, u),),                        # builtin max
    lambda x, u, w: (float(u) + x,),                     # float()
    lambda x, u, w: (np.max((x, u)),),                   # np.max on a tuple of symbols
    lambda x, u, w: (np.array([1., 2.])[0] * x + np.arange(3.) * u,),   # table operand
    lambda x, u, w: (x, u),                              # wrong number of outputs
])
def test_untraceable_callables_raise_trace_error(bad):
    with pytest.raises(TraceError):
        trace_model(bad, lambda x, u, w: 0. * u, 1, 1, 1)


def test_constants_and_params_and_time():
    def dyn(k, x, u, **p):
        return (p['a'] * x + u + k,)

    def cost(k, x, u, **p):
        return 0.

    m = trace_model(dyn, cost, 1, 1, 0, params={'a': 0.5}, stationnary=False)
    assert m.time_dep
    xn, g = evaluate(m, [2.0], [np.array([1., 2.])], [], t=3)
    assert np.array_equal(xn[0], [5., 6.]) and g == 0.0
    src = codegen.model_function_source(m)
    assert '0x1.0000000000000p-1' in src and ' t)' in src or 't;' in src
    assert codegen.real_literal(float('inf')) == '(sdp_real)INFINITY'
    assert 'NAN' in codegen.real_literal(float('nan'))
    assert codegen.real_literal(-0.0) == '(sdp_real)(-0x0.0p+0)'


def test_lanes_for():
    assert [codegen.lanes_for(n) for n in (1, 2, 3, 11, 32, 33, 64, 65, 8001)] == \
        [1, 2, 4, 16, 32, 64, 64, 64, 64]


@pytest.mark.skipif(not os.path.exists(nat.HIPCC), reason='hipcc not installed')
@pytest.mark.parametrize('name,dtype,lanes', [('inventory', np.float64, 16),
                                              ('storage_ar1', np.float64, 64),
                                              ('searev', np.float32, 32)])
def test_generated_units_compile_for_gfx950(name, dtype, lanes, tmp_path, monkeypatch):
    _, solver = getattr(models, name)()
    src = codegen.translation_unit(solver._traced(), dtype, lanes)
    assert '#define SDP_LANES {}'.format(lanes) in src
    monkeypatch.setattr(nat, 'KCACHE', str(tmp_path))
    path = nat.compile_model(src)
    assert os.path.getsize(path) > 1000
    assert nat.compile_model(src) == path                  # cache hit
    with pytest.raises(nat.NativeError):
        nat.compile_model(src + '\n#error broken\n')


def test_solver_reports_untraceable_model_without_gpu():
    s = SysDescription((1, 1, 0))

    def dyn(x, u):
        return (x + (u if u > 0 else 0.),)
    s.dyn = dyn
    s.cost = lambda x, u: u * 0.
    s.control_box = lambda x: ((0., 1.),)
    solver = DPSolver(s)
    solver.discretize_state(0, 1, 3)
    assert isinstance(solver._traced(), TraceError)


def test_hint_when_the_controlled_stock_is_not_listed_first():
    import warnings
    s = SysDescription((2, 1, 1))

    def dyn(p, e, u, w):                    # exogenous price first, stock second
        return (0.8 * p + w, e + 0.5 * u)

    def cost(p, e, u, w):
        return p * u + 0.01 * u * u
    s.dyn, s.cost = dyn, cost
    s.control_box = lambda p, e: ((-1., 1.),)
    s.perturb_laws = [models.NormalLaw(0, 0.2)]
    solver = DPSolver(s)
    solver.discretize_state(-1, 1, 9, 0, 1, 11)
    solver.discretize_perturb(-0.5, 0.5, 5)
    solver.control_steps = (0.25,)
    model = solver._traced()
    assert not model.storage_separable and model.separable_axis_hint() == 1
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        plan = solver._kernel_plan()
        solver._kernel_plan()                          # only once
    # Round 4: the order of the state variables is the user's (reference stodynprog.py:119-131) -- a stock the
    # perturbation does not reach runs the reduced-array sweep on a permuted view of the axes (stocks first for the
    # filter, the reference's own order for the second pass), without a word
    assert plan['lead_axes'] == 1 and plan['lead_perm'] == (1, 0) and plan['filtered'] and not plan['column']
    assert '#define SDP_LEAD_PERM {1, 0, 2, 3}' in plan['source'] and not rec
    # 4-byte reals (and a stock that sees the perturbation) keep the column structure the model still has as
    # written (the trailing axis depends on the control, not on the leading state: table per control -- on a grid of
    # 32 768 nodes and more, or when the column family is asked for; the direct kernel on this small one), and the
    # hint says that listing the stock first would run the much cheaper separable kernel
    solver.dtype = np.dtype(np.float32)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        plan = solver._kernel_plan()
        solver._kernel_plan()                          # only once
    assert not plan['column'] and plan['staged'] is None
    assert len(rec) == 1 and '"e"' in str(rec[0].message) and 'FIRST' in str(rec[0].message)
    solver.kernel = 'column'
    plan = solver._kernel_plan()
    assert plan['column'] and plan['per_control']
    solver.kernel = 'auto'
    # a genuinely coupled model gets no hint
    _, inv = models.inventory()
    assert inv._traced().separable_axis_hint() is None


def test_np_interp_is_traced_with_numpy_semantics():
    """np.interp(symbolic x, concrete tables): one `interp1` node, interpreted
    with np.interp on the host; the generated device function restates numpy's
    arr_interp (range checks, bisection, slope * (x - xp[j]) + fp[j])"""
    xp = np.array([-1., 0., 0.5, 2.])
    fp = np.array([0.9, 0.95, 0.8, 0.6])

    def dyn(e, p, u, w):
        return (e + u * np.interp(u, xp, fp), 0.5 * p + w)

    def cost(e, p, u, w):
        return np.interp(p + w, [0., 1.], [1., 3.], left=-1., right=7.) * u + np.interp(u, [0.25], [4.])
    m = trace_model(dyn, cost, 2, 1, 1)
    assert m.bit_exact and m.storage_separable
    assert len(m.graph.tables) == 3
    rng = np.random.default_rng(0)
    u = np.concatenate([rng.uniform(-2, 3, 200), xp, [np.nan, -np.inf, np.inf, 0.25]])
    w = rng.uniform(-1, 1, u.size)
    with np.errstate(all='ignore'):
        xn, g = evaluate(m, [0.3, 0.4], [u], [w])
        assert np.array_equal(xn[0], dyn(0.3, 0.4, u, w)[0], equal_nan=True)
        assert np.array_equal(g, cost(0.3, 0.4, u, w), equal_nan=True)
    # (a 21-row, 5-point column unit as the planner makes it for this model, without the filter)
    unit = codegen.column_table_unit(m, np.float64, (21, 9), 5, 64, box=dict(per_node=False), axis=np.linspace(0., 1., 21),
                                     certified_filter=False)
    assert unit.form == 'full table' and (unit.n0, unit.w) == (21, 5)
    src = codegen.translation_unit(m, np.float64, 64, unit)
    assert 'sdp_np_interp' in src and 'sdp_tabx_2[1]' in src and 'sdp_interp1_0(' in src
    # same table twice -> one table; a different table -> a different structure
    m2 = trace_model(lambda e, p, u, w: (e + np.interp(u, xp, fp) + np.interp(w, xp, fp), p),
                     lambda e, p, u, w: u * 0., 2, 1, 1)
    assert len(m2.graph.tables) == 1
    m3 = trace_model(dyn, lambda e, p, u, w: np.interp(p + w, [0., 1.], [1., 3.5], left=-1., right=7.) * u
                     + np.interp(u, [0.25], [4.]), 2, 1, 1)
    assert m3.structure_key() != m.structure_key()
    for bad in (lambda e, p, u, w: np.interp(u, xp, fp, period=1.),
                lambda e, p, u, w: np.interp(0.3, xp, fp * u),
                lambda e, p, u, w: np.interp(u, xp, fp[:-1])):
        with pytest.raises(TraceError):
            trace_model(lambda e, p, u, w: (e + u, p), bad, 2, 1, 1)


def test_select_and_heaviside_are_traced():
    def dyn(x, u, w):
        step = np.heaviside(u - 0.25, 0.5)
        return (x + np.select([u < -1, u < 0, u < 1], [-1. + 0 * u, 0.5 * u, u * u], default=2.) * step + w,)

    def cost(x, u, w):
        return np.select([w > 0.5], [u]) + np.heaviside(w, u)
    m = trace_model(dyn, cost, 1, 1, 1)
    assert m.bit_exact
    rng = np.random.default_rng(3)
    u = np.concatenate([rng.uniform(-2, 2, 300), [0.25, -1., 0., 1., np.nan]])
    w = np.concatenate([rng.uniform(-1, 1, 300), [0., 0.5, -0., np.nan, 0.]])
    with np.errstate(all='ignore'):
        xn, g = evaluate(m, [0.3], [u], [w])
        assert np.array_equal(xn[0], dyn(0.3, u, w)[0], equal_nan=True)
        assert np.array_equal(g, cost(0.3, u, w), equal_nan=True)


def _fuzz_expr(rng, leaves, depth):
    """random numpy expression: arithmetic, comparisons, selects, min/max, clip,
    rounding functions, np.interp and np.select"""
    if depth == 0 or rng.random() < 0.2:
        if rng.random() < 0.3:
            return repr(float(np.round(rng.uniform(-2, 2), 3)))
        return leaves[rng.integers(len(leaves))]
    a = _fuzz_expr(rng, leaves, depth - 1)
    b = _fuzz_expr(rng, leaves, depth - 1)
    c = _fuzz_expr(rng, leaves, depth - 1)
    forms = ['({a} + {b})', '({a} - {b})', '({a} * {b})', '({a} / (1.5 + np.abs({b})))',
             'np.where({a} > {b}, {a}, {c})', 'np.where(np.logical_and({a} <= {b}, np.logical_not({c} < 0.1)), {b}, {c})',
             'np.minimum({a}, {b})', 'np.maximum({a}, {b})', 'np.sqrt(np.abs({a}))',
             '(-{a}) ** 2', 'abs({a}) ** 0.5', 'np.clip({a}, -0.5, {b})', 'np.floor({a})',
             'np.ceil({a} * 3.0) / 3.0', 'np.sign({a}) * {b}', '(({a} > {b}) * 2.0 - ({a} == {b}))',
             'np.interp({a}, [-1.0, -0.2, 0.3, 1.5], [2.0, -1.0, 0.5, 0.25])',
             'np.select([{a} < -0.5, {a} < {b}], [{b}, {c}], default=1.25)',
             'np.heaviside({a}, 0.5) * {b}', 'np.fmax({a}, np.fmin({b}, {c}))',
             'np.square({a})', 'np.trunc({a} * 2.5)', 'np.rint({a} * 2.0)',
             '(1.0 / (2.0 + {a} * {a}))']
    return forms[rng.integers(len(forms))].format(a=a, b=b, c=c)


@pytest.mark.parametrize('seed', range(40))
def test_tracer_fuzz_interpreted_dag_equals_the_callable(seed):
    """random callables over (x, y, u, w): the recorded DAG, interpreted with
    numpy, must reproduce the callable bit for bit on random lattices, every
    recorded operator must be one the device evaluates exactly, and the
    generated source must contain one statement per live operator"""
    rng = np.random.default_rng(7000 + seed)
    exprs = [_fuzz_expr(rng, ['x', 'y', 'u', 'w'], 4) for _ in range(3)]
    ns = {'np': np}
    exec('def dyn(x, y, u, w):\n    return ({}, {})\n'
         'def cost(x, y, u, w):\n    return {} + 0.0 * u\n'.format(*exprs), ns)
    m = trace_model(ns['dyn'], ns['cost'], 2, 1, 1)
    # `scalar ** c` on state-only sub-expressions is libm pow in numpy (flagged, 1 ulp)
    assert m.inexact_ops() in ([], ['scalar_pow']), m.inexact_ops()
    exact = m.bit_exact

    def same(a, b):
        a, b = np.broadcast_to(a, (17, 9)), np.broadcast_to(b, (17, 9))
        if exact:
            return np.array_equal(a, b, equal_nan=True)
        with np.errstate(all='ignore'):
            return bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))
                               | (np.abs(a - b) <= 4 * np.spacing(np.maximum(np.abs(a), np.abs(b))))))
    for _ in range(3):
        x, y = rng.uniform(-1.5, 1.5, 2)
        u = np.round(rng.uniform(-2, 2, (17, 1)), 2)
        w = np.round(rng.uniform(-1, 1, (1, 9)), 2)
        with np.errstate(all='ignore'):
            xn_t, g_t = evaluate(m, [x, y], [u], [w])
            xn = ns['dyn'](x, y, u, w)
            g = ns['cost'](x, y, u, w)
        for a, b in zip(xn_t, xn):
            assert same(a, b), exprs
        assert same(g_t, g), exprs
    src = codegen.model_function_source(m)
    live_ops = [n for n in m.live_nodes() if n.op not in ('var', 'const', 'bconst')]
    assert src.count('    const ') == len(live_ops)


def test_power_follows_numpy_array_ufunc_and_scalar_rules():
    """u ** 0.5 is sqrt and u ** 2 is u*u for arrays (numpy's fast paths),
    np.power(u, 0.5) is the pow loop, np.power(u, 2) is u*u; a power of a
    state-only expression is a numpy SCALAR power in the reference (libm pow):
    kept as the correctly rounded operation but flagged"""
    m = trace_model(lambda x, u, w: (x + u ** 0.5 + u ** 2 + u ** -1.0 + np.power(u, 2),), lambda x, u, w: u * 0., 1, 1, 1)
    assert m.bit_exact and 'pow' not in {n.op for n in m.live_nodes()}
    m = trace_model(lambda x, u, w: (x + np.power(u, 0.5),), lambda x, u, w: u * 0., 1, 1, 1)
    assert m.inexact_ops() == ['pow']
    m = trace_model(lambda x, u, w: (x + u,), lambda x, u, w: (x - 0.3) ** 2 + u * u, 1, 1, 1)
    assert m.inexact_ops() == ['scalar_pow'] and not m.bit_exact
    m = trace_model(lambda x, u, w: (x + u,), lambda x, u, w: (x - 0.3) * (x - 0.3) + (u - x) ** 2, 1, 1, 1)
    assert m.bit_exact
    m = trace_model(lambda x, u, w: (x + u,), lambda x, u, w: np.square(x - 0.3) + np.power(x, 2) + u, 1, 1, 1)
    assert m.bit_exact                                   # ufunc loops: x*x for scalars too


def test_kernel_family_planning_without_a_gpu():
    """which kernel family a discretised problem gets, and the compile-time shapes the
    planners hand to the generated unit (no GPU needed: planning is host code)"""
    from stodynprog_amd import codegen
    # storage-separable, table fits LDS: full-table column kernel
    _, s = models.synthetic3d(N=64)
    plan = s._kernel_plan()
    assert plan['column'] and not plan['window'] and not plan['per_control'] and plan['staged'] is None
    assert '#define SDP_TRAIL_HAS_U 0' in plan['source'] and 'SDP_COL_ROWS' not in plan['source']
    # same model, 1024-point leading axis: 32 x 1024 x 8 B = 256 KiB > LDS -> row window
    # (kernel = 'column'; in 8-byte reals 'auto' now prefers the reduced-array sweep with one controlled axis)
    s.discretize_state(0, 1, 1024, 0, 1, 12, 0, 1, 12)
    auto = s._kernel_plan()
    assert auto['lead_axes'] == 1 and not auto['column'] and auto['filtered']
    s.kernel = 'column'
    plan = s._kernel_plan()
    s.kernel = 'auto'
    threads, lds, rows, seg = plan['window']
    assert plan['column'] and rows < 1024 and rows % 32 == 0 and seg >= 64 and seg % 64 == 0
    assert lds * (2 if threads == 512 else 1) <= codegen.COLUMN_LDS_MAX
    assert '#define SDP_COL_ROWS {}'.format(rows) in plan['source'] and plan['col_seg_nodes'] == seg
    assert rows >= seg + s._lead_reach_rows(plan['model'], s._box_plan()) + 2
    # the control also drives x1: a table per control (nodes of a column share their controls)
    _, c = models.synthetic3d_coupled(N=32)
    m = c._traced()
    assert m.column_shareable and m.trail_depends_on_u and not m.storage_separable
    plan = c._kernel_plan()
    assert plan['column'] and plan['per_control'] and '#define SDP_TRAIL_HAS_U 1' in plan['source']
    assert '#define SDP_COL_WCHUNK' in plan['source'] and plan['col_seg_nodes'] in (64, 128, 256, 512)
    # x1 also depends on x0: nothing to share along a column -> LDS-staged tiles on a large grid, the direct kernel
    # (`lanes` threads per node) on a small one (round 5: a thread per node does not fill the chip there -- 32^3: 0.87 ms
    # staged, 0.25 ms direct; 48^3, 64 x 32 lattice points per node: 0.92 / 0.88 ms; DPSolver.STAGED_MIN_NODES, STAGED_MIN_WORK)
    _, f = models.synthetic3d_coupled(N=32, cross=0.3)
    assert not f._traced().column_shareable
    plan = f._kernel_plan()
    assert not plan['column'] and plan['staged'] is None and not plan['lead_axes']
    assert models.synthetic3d_coupled(N=48, cross=0.3)[1]._kernel_plan()['staged'] is None       # 110 592 nodes x 2048 points
    _, f = models.synthetic3d_coupled(N=56, cross=0.3)
    plan = f._kernel_plan()
    st = plan['staged']
    assert not plan['column'] and st['threads'] == int(np.prod(st['tile'])) == 512
    assert 1 <= st['cu'] <= 8 and 1 <= st['cw'] <= 32 and st['cap'] * 8 <= codegen.STAGED_LDS_BYTES
    for macro in ('SDP_STG_THREADS 512', 'SDP_STG_T0 8', 'SDP_STG_CU', 'SDP_STG_CW', 'SDP_STG_CAP'):
        assert '#define ' + macro in plan['source']
    # 1-D problems (no column): the direct kernel whatever the size of the grid; the staged tiles when asked for
    _, inv = models.inventory()
    plan = inv._kernel_plan()
    assert not plan['column'] and plan['staged'] is None
    _, fine = models.inventory_fine(n_x=200000)
    assert fine._kernel_plan()['staged'] is None
    inv.kernel = 'staged'
    assert inv._kernel_plan()['staged']['tile'] == (512,)
    # forcing a family
    c.kernel = 'staged'
    assert c._kernel_plan()['staged'] is not None
    c.kernel = 'generic'
    plan = c._kernel_plan()
    assert not plan['column'] and plan['staged'] is None
    c.kernel = 'nonsense'
    with pytest.raises(ValueError):
        c._kernel_plan()


def test_percontrol_and_window_shapes():
    from stodynprog_amd import codegen
    th, lds, wc = codegen.column_percontrol_config(256, 32, 3, np.float64)
    assert th == 256 and wc == 16 and lds <= 40 * 1024           # four workgroups per CU
    th, lds, wc = codegen.column_percontrol_config(600, 5, 2, np.float64)
    assert th == 512 and 1 <= wc <= 5
    assert codegen.column_percontrol_config(40, 0, 2, np.float32)[0] == 64
    # window: rows from the LDS budget, segment from the reach
    assert codegen.column_window_config(1024, 32, 3, np.float64, 66) is not None
    assert codegen.column_window_config(1024, 32, 3, np.float64, 2000) is None     # one node spans the axis
    assert codegen.staged_row_stride(19, 8, 3, 8) == 24 and codegen.staged_row_stride(8, 8, 3, 8) == 8
    assert codegen.staged_row_stride(19, 32, 2, 8) == 19 and codegen.staged_row_stride(20, 8, 3, 4) == 21


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('n0,w,d', [(2048, 11, 2), (1024, 32, 3), (4096, 5, 2)])
def test_row_window_image_fits_its_workgroups(n0, w, d, dtype):
    """The row window sweeps unfiltered, so its LDS image (struct SdpColLds) holds a partial minimum per thread:
    the planned image must count it and fit the LDS share of its workgroups -- 512 threads used to plan past half of
    the 160 KiB of a CU (one workgroup per CU instead of two), and 1024 threads (a long reach along axis 0) 12 KiB past
    all of it, a unit hipcc rejects: that form is no longer planned (a reach that long gets no row window)"""
    from stodynprog_amd import codegen
    rs = np.dtype(dtype).itemsize
    seen = set()
    for reach in range(0, n0, 8):
        cfg = codegen.column_window_config(n0, w, d, dtype, reach)
        if cfg is None:
            continue
        threads, lds, rows, seg = cfg
        seen.add(threads)
        assert lds == codegen._column_lds(w, w, rows, d, rs, threads, partial_minima=True)
        assert lds <= codegen.COLUMN_LDS_MAX // (2 if threads == 512 else 1), (reach, cfg)
        assert seg >= 64 and rows - reach - 4 >= seg
    assert seen == {512}
    assert codegen.column_window_config(n0, w, d, dtype, n0 - 64) is None


def test_certified_filter_planning_without_a_gpu():
    """where the column kernel gets the certified expectation-first filter (SDP_COL_FILTER of
    csrc/sdp_colfilter_kernel.h) and the workgroup shape that goes with it: one lane per node"""
    from stodynprog_amd import codegen
    _, s = models.synthetic3d(N=256)
    plan = s._kernel_plan()
    assert plan['column'] and plan['filtered']
    src = plan['source']
    assert '#define SDP_COL_FILTER 1' in src and '#define SDP_COL_THREADS 256' in src
    # the benchmark grid: half of the 32 perturbation points resident (32 KiB instead of 64: four workgroups per
    # CU, registers capped to match); a table that lets three workgroups share a CU anyway stays whole
    assert '#define SDP_COL_WRES 16' in src and '#define SDP_COL_MIN_WAVES 4' in src
    _, small = models.synthetic3d(N=128)
    src128 = small._kernel_plan()['source']
    assert 'SDP_COL_WRES' not in src128 and '#define SDP_COL_MIN_WAVES 1' in src128
    s.certified_filter = False                           # every control the long way: the round-1 shape
    src = s._kernel_plan()['source']
    assert 'SDP_COL_FILTER' not in src and '#define SDP_COL_THREADS 512' in src
    s.certified_filter = True
    # 512 nodes per column: 512 lanes; beyond that the lanes of a wave share nodes as before
    _, s = models.synthetic3d(N=64)
    s.discretize_state(0, 1, 512, 0, 1, 16, 0, 1, 16)
    s.dtype = np.dtype('float32')
    assert '#define SDP_COL_THREADS 512' in s._kernel_plan()['source']
    # a perturbation in x0' other than through a final sum (that form: test_shifted_lattice_planning_without_a_gpu):
    # the expectation no longer commutes with the lerp along axis 0
    m = trace_model(lambda x, y, u, w: ((x + u) * (1.0 + 0.1 * w), 0.5 * y + w), lambda x, y, u, w: u * u, 2, 1, 1)
    assert m.storage_separable and not codegen.column_filter_applies(m, dtype=np.float64)
    # a perturbation in the COST still commutes (round 3: the first pass accumulates its expectation),
    # but the control table, which holds sub-expressions without w, is not used then
    m = trace_model(lambda x, y, u, w: (x + u, 0.5 * y + w), lambda x, y, u, w: u * w, 2, 1, 1)
    assert m.storage_separable and codegen.column_filter_applies(m)
    assert codegen.control_table_plan(m, np.float64, False, 64) is None
    m = trace_model(lambda x, y, u, w: (x + u, 0.5 * y + w), lambda x, y, u, w: u * y, 2, 1, 1)
    assert codegen.column_filter_applies(m)


def test_shifted_lattice_planning_without_a_gpu():
    """a perturbation that reaches x0' through final sums (TracedModel.lead_split): what is recognised, what
    codegen emits for it and where the plan falls back to every control the long way"""
    from stodynprog_amd import codegen
    from stodynprog_amd.trace import DEP_W, DEP_X, DEP_U
    tr = lambda dyn: trace_model(dyn, lambda x, y, u, w: u * u, 2, 1, 1)
    m = tr(lambda x, y, u, w: (x + u - w, 0.5 * y + w))                       # the inventory example next to an AR(1)
    a, terms = m.lead_split()
    assert not a.deps & DEP_W and len(terms) == 1 and terms[0][1] == -1
    assert not terms[0][0].deps & (DEP_X | DEP_U)
    m2 = tr(lambda x, y, u, w: (x + u - 0.5 * w - 0.1 * y, 0.5 * y + w))      # a chain, one term without w
    assert [sg for _, sg in m2.lead_split()[1]] == [-1, -1]
    m3 = tr(lambda x, y, u, w: ((y + w) + (x + 0.7 * u), 0.5 * y + w))        # the w-part first
    assert m3.lead_split()[1][0][1] == 1 and m3.lead_split()[0].deps & DEP_U
    for bad in (lambda x, y, u, w: ((x + u) * (1.0 + 0.1 * w), 0.5 * y + w),  # not a sum
                lambda x, y, u, w: (x + (w * u - u), 0.5 * y + w),            # the control inside a w-term (x + (w - u) is regrouped since round 5: next test)
                lambda x, y, u, w: (x + u - 0.1 * y, 0.5 * y + w),            # no perturbation in x0' at all
                lambda x, y, u, w: (x + u - w - w - w - w - w, 0.5 * y + w)): # more terms than the bound covers
        assert tr(bad).lead_split() is None
    assert codegen.column_shift_applies(m, np.float64) and not codegen.column_shift_applies(m, np.float32)
    assert codegen.column_filter_applies(m, dtype=np.float64, table=(256, 32, 2))
    assert not codegen.column_filter_applies(m, dtype=np.float32, table=(256, 32, 2))
    # LDS: the lattice gets the room two workgroups per CU leave beside the table, at least n0 + n0/8 rows
    cfg = codegen.column_config(256, 32, 3, np.float64, False, True, shift=True, utab_values=128)
    assert cfg[0] == 256 and 2 * cfg[1] <= codegen.COLUMN_LDS_MAX and 288 <= cfg[2] <= 528
    assert codegen.column_config(3, 7, 2, np.float64, False, True, shift=True)[2] >= 11
    _, s = models.inventory_markov()
    plan = s._kernel_plan()
    src = plan['source']
    assert plan['column'] and plan['filtered'] and '#define SDP_COL_SHIFT 1' in src
    assert 'sdp_model_lead_a' in src and 'sdp_model_lead_b' in src and '#define SDP_COL_SHIFT_TERMS 1' in src
    assert 'sdp_model_lead_tab' in src                   # the control table holds the parts of a(x, u)
    s.dtype = np.dtype('float32')
    plan = s._kernel_plan()
    assert plan['column'] and not plan['filtered'] and 'SDP_COL_SHIFT' not in plan['source']
    _, s = models.synthetic3d(N=256, stock_noise=0.07)
    assert '#define SDP_COL_SHIFT 1' in s._kernel_plan()['source']


def test_sums_in_another_nesting_are_regrouped_by_the_tracer():
    """TracedModel.lead_split: the final-sum form is returned as the reference adds it (nothing regrouped); a chain of
    sums in another nesting is flattened into at most 4 leaves and regrouped -- a* is a new node of the graph, the
    w-free leaves and the number of additions go to the kernel's bound; products and longer chains are refused"""
    from stodynprog_amd.trace import trace_model
    cost = lambda x, y, u, w: x * x + u * u
    def split(dyn):
        m = trace_model(dyn, cost, 2, 1, 1)
        return m, m.lead_split(), m.lead_split_chain()
    m, sp, chain = split(lambda x, y, u, w: (x + u - w, 0.8 * y + w))
    assert sp is not None and chain is None and sp[0].op == 'add' and [sg for _, sg in sp[1]] == [-1]
    m, sp, chain = split(lambda x, y, u, w: (x + (w - u), 0.8 * y + w))
    assert sp[0].op == 'sub' and [a.op for a in sp[0].args] == ['var', 'var'] and [sg for _, sg in sp[1]] == [1]
    assert [sg for _, sg in chain[0]] == [1, -1] and chain[1] == 2
    assert m.lead_split() is sp                                          # (cached: the graph grows once)
    m, sp, chain = split(lambda x, y, u, w: ((x - 0.1 * y) - (u - 0.5 * w), 0.8 * y + w))
    assert [n.op for n, _ in chain[0]] == ['sub', 'var'] and chain[1] == 2 and sp[1][0][1] == 1
    m, sp, chain = split(lambda x, y, u, w: (w - (u - x), y))             # one w-free leaf, negated: nothing to regroup but the sign
    assert sp[0].op == 'neg' and chain[1] == 1
    m, sp, chain = split(lambda x, y, u, w: (-u + (w - x), y))            # no positive w-free leaf
    assert sp[0].op == 'sub' and sp[0].args[0].op == 'neg'
    assert split(lambda x, y, u, w: ((x + u) * (1 + 0.1 * w), y))[1] is None
    assert split(lambda x, y, u, w: (x + (w - u) + (0.1 * y - 0.2 * u) + 0.3, y))[1] is None      # five leaves
    assert split(lambda x, y, u, w: (x + (w * u - u), y))[1] is None      # a leaf that sees the control and the perturbation
    # the plan: the shifted lattice without the control table, the sum of the leaves' magnitudes generated
    sysd = SysDescription((2, 1, 1))
    sysd.dyn = lambda x, y, u, w: (x + ((0.5 * w + 0.1 * y) - u), 0.8 * y + w)
    sysd.cost = lambda x, y, u, w: (x - 0.3) * (x - 0.3) + 0.1 * u * u
    sysd.control_box = lambda x, y: ((-1., 1.),)
    sysd.perturb_laws = [models.NormalLaw(0, 0.2)]
    s = DPSolver(sysd)
    s.discretize_state(-1, 1, 65, -1, 1, 17)
    s.discretize_perturb(-0.5, 0.5, 7)
    s.control_steps = (0.05,)
    src = s._kernel_plan()['source']
    assert '#define SDP_COL_SHIFT 1' in src and '#define SDP_COL_SHIFT_CHAIN 2' in src
    assert 'return fabs(x[0]) + fabs(u[0]);' in src                       # sdp_model_lead_aabs
    assert '#define SDP_COL_UTAB 2' in src and 'return fabs(x[0]) + fabs(tab[0]);' in src          # .. and from the control table
    s.dtype = np.dtype(np.float32)                                        # (8-byte reals only, like the final-sum form)
    assert '#define SDP_COL_SHIFT 1' not in s._kernel_plan()['source']


def test_controlled_axes_and_the_reduced_array_plan_without_a_gpu():
    """several controlled state variables next to an exogenous process (TracedModel.controlled_axes) and
    the kernel family planned for them (csrc/sdp_lead_kernel.h)"""
    from stodynprog_amd import codegen
    tr3 = lambda dyn, cost=None: trace_model(dyn, cost or (lambda a, b, y, u, v, w: u * u + v * v + y * u), 3, 2, 1)
    assert tr3(lambda a, b, y, u, v, w: (a + u - v, b + v, 0.8 * y + w)).controlled_axes() == 2
    assert tr3(lambda a, b, y, u, v, w: (a + u, 0.9 * b + y, 0.8 * y + w)).controlled_axes() == 1     # one stock
    assert tr3(lambda a, b, y, u, v, w: (a + u + w, b + v, 0.8 * y + w)).controlled_axes() is None    # w in a stock
    assert tr3(lambda a, b, y, u, v, w: (a + u, b + v, 0.8 * y + w + 0.1 * a)).controlled_axes() is None   # a stock drives y
    assert tr3(lambda a, b, y, u, v, w: (a + u, b + v + y, 0.8 * y + w + 0.1 * u)).controlled_axes() is None   # the control drives y, which sees w
    assert models.synthetic3d(N=8)[1]._traced().controlled_axes() == 1
    m = tr3(lambda a, b, y, u, v, w: (a + u - v, b + v, 0.8 * y + w))
    assert codegen.lead_filter_applies(m, np.float64) == 2 and codegen.lead_filter_applies(m, np.float32) == 0
    mw = tr3(lambda a, b, y, u, v, w: (a + u - v, b + v, 0.8 * y + w), lambda a, b, y, u, v, w: u * w)
    assert codegen.lead_filter_applies(mw, np.float64) == 2          # a cost that sees the perturbation: its expectation per control
    _, s = models.two_reservoirs(n_a=12, n_b=10, n_y=6, n_w=5)
    plan = s._kernel_plan()
    assert plan['lead_axes'] == 2 and plan['lanes'] == 1 and plan['filtered'] and not plan['column'] and plan['staged'] is None
    src = plan['source']
    assert '#define SDP_LEAD_AXES 2' in src and '#define SDP_LANES 1' in src
    for fn in ('sdp_model_leads', 'sdp_model_trails', 'sdp_model_cost', 'sdp_model_cell'):
        assert fn in src
    s.kernel = 'generic'
    assert not s._kernel_plan()['lead_axes']
    s.kernel = 'column'                          # the table-per-control column kernel still takes the model when asked
    assert s._kernel_plan()['column'] and s._kernel_plan()['per_control']
    s.kernel = 'lead'
    s.dtype = np.dtype('float32')                # (8-byte reals only since round 6)
    with pytest.raises(ValueError):
        s._kernel_plan()


def test_control_table_planning_without_a_gpu():
    """the sub-expressions of x0' and of the cost that depend on the control but not on the leading
    state variable (TracedModel.control_uniform_frontier) and the table codegen builds from them"""
    from stodynprog_amd.trace import DEP_X, DEP_W, DEP_U
    _, s = models.synthetic3d(N=32)
    plan = s._kernel_plan()
    fr = plan['model'].control_uniform_frontier()
    assert fr is not None and len(fr) == 2                 # b u  and  (k1 x1 - k0 - u)^2 + eps u^2
    for n in fr:
        assert n.deps & DEP_U and not n.deps & (DEP_X | DEP_W)
    src = plan['source']
    assert '#define SDP_COL_UTAB 2' in src and '#define SDP_COL_UTAB_N 64' in src
    assert 'sdp_model_utab' in src and 'sdp_model_lead_tab' in src and 'sdp_model_cost_tab' in src
    lead_tab = src[src.index('sdp_model_lead_tab'):src.index('sdp_model_cost_tab')]
    assert 'u[' not in lead_tab and 'x[0] + tab[0]' in lead_tab      # what is left per (node, control)
    # a lattice that differs from node to node (Searev, storage-AR1: the box depends on the stock): no table
    for make in (models.searev, models.storage_ar1):
        _, s2 = make()
        p2 = s2._kernel_plan()
        assert p2['filtered'] and p2['per_node'] and 'SDP_COL_UTAB' not in p2['source']
    # a lattice too long for the LDS budget: no table
    _, s3 = models.synthetic3d(N=32)
    s3.control_steps = (2.0 / 4000,)
    assert 'SDP_COL_UTAB' not in s3._kernel_plan()['source']
    # the whole cost independent of x0: it IS a table entry
    m = trace_model(lambda x, y, u, w: (x + 0.5 * u, 0.5 * y + w), lambda x, y, u, w: (y - u) * (y - u), 2, 1, 1)
    fr = m.control_uniform_frontier()
    assert fr is not None and m.cost.id in [n.id for n in fr]
    # nothing to tabulate when the control enters only together with x0
    m = trace_model(lambda x, y, u, w: (x * u, 0.5 * y + w), lambda x, y, u, w: x * u, 2, 1, 1)
    fr = m.control_uniform_frontier()
    assert fr is not None and [n.op for n in fr] == ['var']            # only u itself


def test_the_environment_does_not_reach_the_generated_source(monkeypatch):
    """the product has no hidden switches (the reference's whole configuration is stodynprog.py:332):
    diagnostic knobs exist only as an explicit dict (DPSolver.debug_defines / bench.py --debug-define),
    and what used to be read from the environment is ignored -- same source, byte for byte"""
    from stodynprog_amd import codegen, DPSolver

    def sources():
        out = []
        for make in (lambda: models.synthetic3d(N=32), lambda: models.synthetic3d(N=32, stock_noise=0.07),
                     lambda: models.synthetic3d_coupled(N=24), lambda: models.two_reservoirs(n_a=16, n_b=16, n_y=8, n_w=4),
                     lambda: models.synthetic3d_coupled(N=24, cross=0.3)):
            _, s = make()
            out.append(s._kernel_plan()['source'])
        return out

    clean = sources()
    for k, v in (('SDP_COL_FILTER_SCALE', '1e-6'), ('SDP_LEAD_FILTER_SCALE', '1e-6'), ('SDP_EXTRA_DEFINES', 'X=1'),
                 ('SDP_NO_POW2', '1'), ('SDP_COL_LEAN', '0'), ('SDP_COL_THREADS', '1024'), ('SDP_COL_FILTER', '0'),
                 ('SDP_COL_UTAB', '0'), ('SDP_STAMP', '2'), ('SDP_COL_SHIFT', '0'), ('SDP_LEAD_FILTER', '0'),
                 ('SDP_STG_CU', '1'), ('SDP_COL_WCHUNK', '3'), ('SDP_COL_WPAIR', '1')):
        monkeypatch.setenv(k, v)
    assert sources() == clean
    with open(codegen.__file__) as f:
        assert 'os.environ' not in f.read()
    # the explicit dict does reach it, is recorded, and refuses names it does not know
    _, s = models.synthetic3d(N=32)
    s.debug_defines = {'SDP_COL_FILTER_SCALE': '1e6', 'SDP_EXTRA_DEFINES': 'X=1'}
    src = s._kernel_plan()['source']
    assert '#define SDP_COL_FILTER_SCALE 1000000.0' in src and '#define X 1' in src and src != clean[0]
    s.debug_defines = {'SDP_COL_FILTRE_SCALE': '2'}
    with pytest.raises(ValueError):
        s._kernel_plan()
    # and so are the switches of A/B forks that the headers no longer have
    for retired in ('SDP_COL_TAIL_KEEP', 'SDP_COL_WMODE', 'SDP_COL_A_ORDER'):
        s.debug_defines = {retired: '1'}
        with pytest.raises(ValueError):
            s._kernel_plan()
    assert DPSolver.debug_defines is None


def _compiles(source):
    """hipcc cross-compiles the unit for gfx950 (no GPU needed); False when the static_assert on
    sizeof(SdpColLds) -- or anything else -- refuses it"""
    from stodynprog_amd import _native as nat
    try:
        nat.compile_model(source)
        return True
    except Exception:
        return False


@pytest.mark.skipif(not os.path.exists('/opt/rocm/bin/hipcc'), reason='needs hipcc')
def test_the_planned_lds_image_is_the_compiled_one():
    """codegen._column_lds lays SdpColLds out member by member: the LARGEST axis-0 length the planner
    accepts for the filtered full-table kernel must compile (static_assert sizeof(SdpColLds) <= 160 KiB),
    with the control table in the struct, and a size it refuses is planned as another family instead of
    failing at compile time (advisor finding, round 3: N0 = 543..550 at W = 32 used to raise NativeError;
    the image has since lost the members a filtered build does not use, so the edge sits near 605)."""
    from stodynprog_amd import codegen
    def plan_for(n0):
        _, s = models.synthetic3d(N=12)
        s.discretize_state(0, 1, n0, 0, 1, 12, 0, 1, 12)
        return s._kernel_plan()

    with_table = [n0 for n0 in range(580, 640, 2) if '#define SDP_COL_UTAB 2' in plan_for(n0)['source']]
    column = [n0 for n0 in range(580, 640, 2) if plan_for(n0)['column']]
    assert with_table and column and 590 <= max(with_table) < max(column) <= 620, (with_table, column)
    # the last size with the control table in the struct, the last one the column family takes at all (the
    # table is what the planner drops first), and the first one that goes to another family: all compile
    for n0 in (max(with_table), max(column), max(column) + 2):
        plan = plan_for(n0)
        assert plan['filtered'] and (plan['column'] or plan['lead_axes'] or plan['window']), n0
        assert _compiles(plan['source']), n0
    # the planner's byte count IS sizeof(SdpColLds): one unit on the edge, checked against the compiler from
    # both sides by shrinking the budget the planner may use
    cfg = codegen.column_config(256, 32, 3, np.float64, False, True, max_controls=64, n_columns=65536, utab_values=128)
    assert cfg == (256, codegen._column_lds(32, 32, 256, 3, 8, 256, reduced=True, utab_values=128))


def test_the_short_first_pass_is_planned_where_the_model_has_its_shape():
    """x0' = X(x) +- a(u) and cost = K(x) +- h(u) (TracedModel.additive_control_split): the resident-chunk kernel of
    8-byte reals then gets codegen.short_pass_source (SDP_COL_LEAN2 of csrc/sdp_colres_kernel.h)"""
    from stodynprog_amd import codegen
    from stodynprog_amd.trace import DEP_U
    _, s = models.synthetic3d(N=256)
    plan = s._kernel_plan()
    m = plan['model']
    sp = m.additive_control_split(m.control_uniform_frontier())
    (X, a_slot, a_form), (K, h_slot, h_form) = sp['lead'], sp['cost']
    assert (a_slot, a_form, h_slot, h_form) == (0, 'add', 1, 'add') and not (X.deps | K.deps) & DEP_U
    src = plan['source']
    assert '#define SDP_COL_WRES 16' in src and '#define SDP_COL_LEAN2 1' in src
    assert '#define SDP_LEAN2_LEAD(X, A) ((X) + (A))' in src and '#define SDP_LEAN2_HNEG 0' in src
    lead_x = src[src.index('sdp_model_lead_x'):src.index('sdp_model_cost_x')]
    assert 'return x[0];' in lead_x and 'u[' not in lead_x
    assert _compiles(src)
    # the switch of A/B runs, 4-byte reals, a table that stays whole: the first pass of section 3.1c
    s.debug_defines = {'SDP_COL_LEAN2': '0'}
    assert 'SDP_COL_LEAN2' not in s._kernel_plan()['source']
    s.debug_defines = None
    s.dtype = np.dtype(np.float32)             # 4-byte reals: the short WIDE pass of the full-table kernel instead
    src32 = s._kernel_plan()['source']
    assert 'SDP_COL_LEAN2' not in src32 and '#define SDP_COL_WIDE2 1' in src32 and 'SDP_COL_WRES' not in src32
    assert _compiles(src32)
    s.debug_defines = {'SDP_COL_LEAN2': '0'}
    assert 'SDP_COL_WIDE2' not in s._kernel_plan()['source']
    s.debug_defines = None
    _, s2 = models.synthetic3d(N=32)
    assert 'SDP_COL_WRES' not in s2._kernel_plan()['source'] and 'SDP_COL_LEAN2' not in s2._kernel_plan()['source']
    # the forms: X - a, a - X, K - h (the control enters negated), h alone, a cost without the control
    tm = lambda dyn0, cost: trace_model(lambda x, y, u, w: (dyn0(x, y, u), 0.5 * y + w), lambda x, y, u, w: cost(x, y, u), 2, 1, 1)
    for dyn0, cost, want in (
            (lambda x, y, u: x - 0.5 * u, lambda x, y, u: x * x - (y - u) * (y - u), ('sub', 'sub')),
            (lambda x, y, u: 0.5 * u - x, lambda x, y, u: (y - u) * (y - u) - x, ('rsub', 'rsub')),
            (lambda x, y, u: x + 0.5 * u, lambda x, y, u: (y - u) * (y - u), ('add', 'add')),
            (lambda x, y, u: x * y + y * u, lambda x, y, u: x * x + y, ('add', 'add'))):
        m = tm(dyn0, cost)
        sp = m.additive_control_split(m.control_uniform_frontier())
        assert sp is not None and (sp['lead'][2], sp['cost'][2]) == want
        assert codegen.short_pass_source(m, m.control_uniform_frontier()) is not None
    assert tm(lambda x, y, u: x + 0.5 * u, lambda x, y, u: (y - u) * (y - u))\
        .additive_control_split(tm(lambda x, y, u: x + 0.5 * u, lambda x, y, u: (y - u) * (y - u)).control_uniform_frontier())['cost'][0] is None
    m = tm(lambda x, y, u: x * y + y * u, lambda x, y, u: x * x + y)
    assert m.additive_control_split(m.control_uniform_frontier())['cost'][1] is None     # no control in the cost
    # not the shape: the control multiplies the stock; the cost couples them; the stock is scaled after the control
    for dyn0, cost in ((lambda x, y, u: x * (1.0 + 0.1 * u) + u, lambda x, y, u: x + u * u),
                       (lambda x, y, u: x + u, lambda x, y, u: (x - u) * (x - u)),
                       (lambda x, y, u: (x + u) * 0.5, lambda x, y, u: x + u * u)):
        m = tm(dyn0, cost)
        fr = m.control_uniform_frontier()
        assert fr is None or m.additive_control_split(fr) is None
    # a perturbation that reaches the stock through FINAL sums (round 6: the short pass on the shifted lattice): the w-free
    # part has the shape; a chain of sums in another nesting is regrouped -- its a is not the reference's value: not taken
    m = trace_model(lambda x, y, u, w: ((x + 0.5 * u) - 0.1 * w, 0.5 * y + w), lambda x, y, u, w: x + u * u, 2, 1, 1)
    sp = m.additive_control_split(m.control_uniform_frontier(m.lead_split()[0]))
    assert sp is not None and (sp['lead'][1], sp['lead'][2], sp['cost'][2]) == (0, 'add', 'add')
    m = trace_model(lambda x, y, u, w: (x + (0.5 * u - 0.1 * w), 0.5 * y + w), lambda x, y, u, w: x + u * u, 2, 1, 1)
    assert m.lead_split_chain() is not None and m.additive_control_split(m.control_uniform_frontier(m.lead_split()[0])) is None
    _, sn = models.synthetic3d(N=256, stock_noise=0.07)
    srcn = sn._kernel_plan()['source']
    assert '#define SDP_COL_SHIFT 1' in srcn and '#define SDP_COL_LEAN2 1' in srcn and '#define SDP_COL_BNB 1' in srcn
    sn.debug_defines = {'SDP_COL_BNB': '0'}
    assert '#define SDP_COL_LEAN2 1' in sn._kernel_plan()['source'] and 'SDP_COL_BNB' not in sn._kernel_plan()['source']
    sn.debug_defines = {'SDP_COL_LEAN2': '0'}
    assert 'SDP_COL_LEAN2' not in sn._kernel_plan()['source']


# ---------------------------------------------------------------------------
# Spill code before the execution mask is restored (codegen.spill_hazards, _native.compile_model)
# ---------------------------------------------------------------------------
_ASM_JOIN = """
\t.text
sdp_sweep_col:                          ; @sdp_sweep_col
; %bb.0:
\tscratch_store_dword off, v1, off offset:4 ; 4-byte Folded Spill
\ts_and_saveexec_b64 s[2:3], vcc
\ts_cbranch_execz .LBB3_2
; %bb.1:
\tscratch_store_dword off, v2, off offset:8 ; 4-byte Folded Spill
\tv_mov_b32_e32 v2, 0
\tscratch_load_dword v2, off, off offset:8 ; 4-byte Folded Reload
.LBB3_2:
\tv_writelane_b32 v62, s30, 55
{before}
\ts_or_b64 exec, exec, s[2:3]
{after}
\ts_endpgm
"""


def test_spill_code_before_the_mask_restore_is_found():
    """the pattern of round 5's endless kernel: a vector register stored (or reloaded) at the top of a block where
    paths join, before `s_or_b64 exec, exec, ..`; spill code anywhere else -- the entry block, inside the branch,
    after the restore -- is none of the scan's business, and SGPR spills (v_writelane) ignore the mask"""
    from stodynprog_amd import codegen
    store = '\tscratch_store_dwordx2 off, v[24:25], off offset:144 ; 8-byte Folded Spill'
    load = '\tscratch_load_dword v7, off, off offset:4 ; 4-byte Folded Reload'
    acc = '\tv_accvgpr_write_b32 a3, v9 ; Reload Reuse'
    plain = '\tscratch_load_dword v7, off, off offset:4'          # (the kernel's own scratch traffic: not spill code)
    assert codegen.spill_hazards(_ASM_JOIN.format(before='', after=store)) == []
    assert codegen.spill_hazards(_ASM_JOIN.format(before=plain, after='')) == []
    for ins in (store, load, acc):
        hz = codegen.spill_hazards(_ASM_JOIN.format(before=ins, after=''))
        assert len(hz) == 1 and hz[0][:2] == ('sdp_sweep_col', '.LBB3_2') and hz[0][3] == [ins.strip()], hz
    # another write of the mask first: not the top of a join any more
    assert codegen.spill_hazards(_ASM_JOIN.format(before='\ts_mov_b64 exec, s[4:5]\n' + store, after='')) == []


def test_code_objects_that_may_spill_are_told_from_their_metadata():
    from stodynprog_amd import codegen
    note = lambda scratch, agprs: (b'\x82\xa5.name\xa9sdp_sweep\xbb.private_segment_fixed_size' + scratch +
                                   b'\xab.agpr_count' + agprs)
    assert not codegen.code_object_may_spill(note(b'\x00', b'\x00') + note(b'\x00', b'\x00'))
    assert codegen.code_object_may_spill(note(b'\x00', b'\x00') + note(b'\xcd\x01\x28', b'\x00'))      # 296 bytes of scratch
    assert codegen.code_object_may_spill(note(b'\x00', b'\x08'))
    assert codegen.code_object_may_spill(b'no metadata at all')


@pytest.mark.skipif(not os.path.exists('/opt/rocm/bin/hipcc'), reason='needs hipcc')
def test_a_kernel_with_unsafe_spill_code_is_rebuilt_with_more_registers(monkeypatch):
    """the kernel that never ended in round 5 (resident chunks, long first pass, 2 waves, a budget of 64 registers:
    the budget is forced here, the planner no longer asks for it): the first build shows the pattern, the build with
    4 waves per SIMD asked of the allocator is clean, and <key>.build.txt says so"""
    from stodynprog_amd import codegen, _native as nat, SysDescription, DPSolver
    from stodynprog_amd.models import NormalLaw
    sysd = SysDescription((2, 1, 1), name='stock, no_u_cost')
    sysd.dyn = lambda x, y, u, w: (0.7 * u + x, 0.8 * y + w)
    sysd.cost = lambda x, y, u, w: 0.05 * x + y * y
    sysd.control_box = lambda x, y: ((-1.0, 1.0),)
    sysd.perturb_laws = [NormalLaw(0, 0.2)]
    s = DPSolver(sysd)
    s.discretize_state(0, 3, 96, -1, 1, 9)
    s.discretize_perturb(-0.5, 0.5, 7)
    s.control_steps = (0.0625,)
    monkeypatch.setattr(DPSolver, 'debug_defines', {'SDP_COL_WRES': '4', 'SDP_COL_LEAN2': '0'})
    assert '#define SDP_COL_MIN_WAVES 4' in s._kernel_plan()['source']          # (what the planner asks for)
    monkeypatch.setattr(DPSolver, 'debug_defines', {'SDP_COL_WRES': '4', 'SDP_COL_LEAN2': '0', 'SDP_COL_MIN_WAVES': '8'})
    source = s._kernel_plan()['source']
    assert '#define SDP_COL_MIN_WAVES 8' in source and '#define SDP_COL_WRES 4' in source
    base = os.path.join(nat.KCACHE, codegen.source_key(source))
    for ext in ('.hsaco', '.build.txt'):
        if os.path.exists(base + ext):
            os.unlink(base + ext)
    out = nat.compile_model(source)
    assert out == base + '.hsaco' and os.path.getsize(out) > 10000
    log = open(base + '.build.txt').read().splitlines()
    assert log[0].startswith('waves cap None: sdp_sweep_col') and 'before the mask restore' in log[0], log
    assert log[-1].endswith(': clean') and len(log) >= 2, log
