"""The CPU oracle (oracle/) pinned against golden vectors produced by the real
reference (tests/golden/make_golden.py) and against the reference's own known
answers.  No GPU needed."""
import numpy as np
import pytest

from conftest import golden, assert_sweep_parity
from oracle import c_oracle, vi_numpy
from stodynprog_amd import models


def test_interp_bit_exact_all_cases():
    g = golden('g1_interp')
    n = int(g['n_cases'])
    assert n == 16
    for c in range(n):
        p = 'c{:02d}_'.format(c)
        ref = g[p + 'out']
        for impl in (c_oracle.mlinterp, vi_numpy.mlinterp_np):
            out = impl(g[p + 'smin'], g[p + 'smax'], g[p + 'orders'], g[p + 'values'], g[p + 's'])
            assert out.dtype == ref.dtype
            assert np.array_equal(out, ref, equal_nan=True), (c, impl.__name__)


def test_interp_known_answer_of_reference_test():
    # reference stodynprog/tests/test_dolointerp.py:17-40
    s = np.linspace(0., 2., 5)[None, :]
    vals = np.array([[0., 1., 4.]])
    for impl in (c_oracle.mlinterp, vi_numpy.mlinterp_np):
        out = impl(np.array([0.]), np.array([2.]), np.array([3]), vals, s)
        assert np.all(np.abs(out - np.array([0, 0.5, 1, 2.5, 4])) < 1e-10)
    g = golden('g1_interp')
    assert np.array_equal(g['ka_out'], out)


def test_interp_extrapolation_and_cast_edge_cases():
    g = golden('g1_interp')
    vals = np.array([[0., 1., 4.]])
    for impl in (c_oracle.mlinterp, vi_numpy.mlinterp_np):
        with np.errstate(all='ignore'):
            out = impl(np.array([0.]), np.array([2.]), np.array([3]), vals, g['ex_s'])
        assert np.array_equal(out, g['ex_out'], equal_nan=True)
    assert g['ex_out'][0, 0] == -1.0 and g['ex_out'][0, 1] == 7.0


def test_interp_object_api_case():
    # reference tests/test_dolointerp.py:45-93: exact at the grid corners
    g = golden('g1_interp')
    out = c_oracle.mlinterp([1., 1.], [2., 2.], [5, 5], g['mli_values'], g['mli_pts'])
    assert np.array_equal(out, g['mli_out'])
    x = g['mli_pts']
    exact = np.vstack([np.sqrt(x[0] ** 2 + x[1] ** 2), np.power(x[0] ** 3 + x[1] ** 3, 1 / 3.)])
    assert np.all(np.abs(out[:, :4] - exact[:, :4]) < 1e-9)
    assert np.all(np.abs(out - exact) < 0.01)


def test_interp_dimension_5_raises():
    with pytest.raises(Exception):
        c_oracle.mlinterp(np.zeros(5), np.ones(5), [2] * 5, np.zeros((1, 32)), np.zeros((5, 1)))


def test_inventory_known_answers_and_golden():
    # doc/example_inventory.rst:220-239
    g = golden('g2_inventory')
    _, solver = models.inventory()
    spec = vi_numpy.Spec.from_solver(solver)
    assert np.array_equal(solver.state_grid[0], g['state_grid'])
    assert np.array_equal(solver.perturb_proba[0], g['perturb_proba'])
    J = np.zeros(10)
    expected_pol = {0: [0] * 10, 1: [4, 3, 2, 1, 0, 0, 0, 0, 0, 0],
                    2: [5, 4, 3, 2, 1, 0, 0, 0, 0, 0], 3: [5, 4, 3, 2, 1, 0, 0, 0, 0, 0]}
    for k in range(6):
        J, pol, idx, mar = vi_numpy.value_iteration(spec, J)
        assert_sweep_parity(J, idx, g['J'][k], g['idx'][k], g['margin'][k], 'inventory %d' % k)
        assert np.array_equal(pol, g['pol'][k])
        if k in expected_pol:
            assert np.array_equal(pol[:, 0], expected_pol[k])
        if k == 0:
            assert np.allclose(J, [9, 6, 3, 0, 0.5, 1, 1.5, 2, 2.5, 3], rtol=0, atol=1e-14)


def test_nas_demo_golden():
    g = golden('g7_nas')
    _, solver = models.nas_demo()
    spec = vi_numpy.Spec.from_solver(solver)
    J1, pol1, idx1, _ = vi_numpy.value_iteration(spec, np.zeros(spec.shape))
    assert_sweep_parity(J1, idx1, g['J1'], g['idx1'], g['margin1'], 'nas 1')
    J2, pol2, idx2, _ = vi_numpy.value_iteration(spec, g['J1'])
    assert_sweep_parity(J2, idx2, g['J2'], g['idx2'], g['margin2'], 'nas 2')


def test_storage_ar1_sampled_nodes_golden():
    """reference-size problem (41x61, up to 8001 controls): sampled nodes only,
    the numpy oracle costs ~2 ms per node like the reference."""
    g = golden('g3_ar1_ref')
    _, solver = models.storage_ar1()
    spec = vi_numpy.Spec.from_solver(solver)
    assert np.array_equal(solver.perturb_proba[0], g['perturb_proba'])
    rng = np.random.default_rng(3)
    nodes = np.unique(np.concatenate([rng.integers(0, 41 * 61, 120), [0, 41 * 61 - 1]]))
    J, pol, idx, _ = vi_numpy.value_iteration(spec, g['J1'], nodes=nodes)
    assert_sweep_parity(J, idx, g['J2'].ravel()[nodes], g['idx2'].ravel()[nodes],
                        g['margin2'].ravel()[nodes], 'ar1 sweep 2')
    # control counts quoted by the notebook (AR1.ipynb:362-365): 4001 .. 8001
    assert g['npts'][..., 0].min() == 4001 and g['npts'][..., 0].max() == 8001
    assert abs(g['npts'][..., 0].mean() - 6342.5) < 0.5
    assert (g['npts'][..., 1] == 1).all()


def test_searev_sampled_golden_with_c_tabulated_oracle():
    g = golden('g4_searev')
    _, solver = models.searev(n_E=128, n_S=128, n_A=128, step=2.2 / 31)
    spec = vi_numpy.Spec.from_solver(solver)
    assert np.array_equal(solver.perturb_proba[0], g['perturb_proba'])
    E, S, A = solver.state_grid_full
    V0 = np.ascontiguousarray(0.02 * (E - 5.) * (E - 5.) + 1.5 * (S * S) + 0.7 * (A * A)
                              + 0.1 * S * A - 0.01 * E)
    nodes = g['nodes'][::8]
    J, pol, idx, _ = vi_numpy.value_iteration(spec, V0, nodes=nodes)
    assert_sweep_parity(J, idx, g['J'][::8], g['idx'][::8], g['margin'][::8], 'searev c3')
    assert np.array_equal(pol, g['pol'][::8])


def test_synthetic_c_oracle_vs_reference_golden():
    """the hand-written C model of the benchmark problem against the reference
    run on 4099 sampled nodes of the 256^3 grid and on the full 20^3 grid"""
    g = golden('g5_synth')
    _, solver = models.synthetic3d()
    V0 = models.synthetic3d_V0(solver.state_grid)
    import zlib
    assert zlib.crc32(V0.tobytes()) == int(g['V0_crc'])
    assert np.array_equal(solver.perturb_proba[0], g['perturb_proba'])
    J, idx, mar = c_oracle.vi_synth3d(solver.state_grid, V0, models.SYNTH_PAR, -1., 1., 64,
                                      solver.perturb_grid[0], solver.perturb_proba[0],
                                      node_ids=g['nodes'], n_threads=4)
    err, ndiff = assert_sweep_parity(J, idx, g['J'], g['idx'], g['margin'], 'synthetic 256^3')
    assert ndiff == 0                      # strictly convex cost: unique minimiser
    _, small = models.synthetic3d(N=20)
    V0s = models.synthetic3d_V0(small.state_grid)
    J1, idx1, _ = c_oracle.vi_synth3d(small.state_grid, V0s, models.SYNTH_PAR, -1., 1., 64,
                                      small.perturb_grid[0], small.perturb_proba[0],
                                      n_nodes=V0s.size)
    assert_sweep_parity(J1.reshape(V0s.shape), idx1.reshape(V0s.shape), g['s_J1'], g['s_idx1'],
                        g['s_margin1'], 'synthetic 20^3')
    # numpy oracle with the Python callables agrees with the C model bit for bit
    spec = vi_numpy.Spec.from_solver(small)
    nodes = np.arange(0, V0s.size, 37)
    Jn, _, idxn, _ = vi_numpy.value_iteration(spec, V0s, nodes=nodes)
    assert np.array_equal(Jn, J1[nodes]) and np.array_equal(idxn, idx1[nodes])


def test_c_tabulated_oracle_matches_numpy_oracle():
    _, solver = models.nas_demo(n_E=9, n_P=7, n_w=5)
    spec = vi_numpy.Spec.from_solver(solver)
    rng = np.random.default_rng(0)
    V = rng.standard_normal(spec.shape)
    interp = vi_numpy.Interp(*spec.state_grid)
    interp.set_values(V)
    import itertools
    offs, xs, gs, Js, idxs = [0], [], [], [], []
    for x_k in itertools.product(*spec.state_grid):
        J_opt, u, flat, mar = vi_numpy.backup_node(spec, x_k, interp)
        grids, dims = vi_numpy.control_grids(spec, x_k)
        u0 = grids[0].reshape(-1, 1)
        args = tuple(x_k) + (u0,) + tuple(spec.perturb_grid)
        xn = spec.dyn(*args)
        lattice = dims + (len(spec.perturb_grid[0]),)
        xs.append(np.vstack([np.broadcast_to(a, lattice).ravel() for a in xn]))
        gs.append(np.broadcast_to(spec.cost(*args), lattice).ravel())
        offs.append(offs[-1] + gs[-1].size)
        Js.append(J_opt); idxs.append(flat)
    J, idx, _ = c_oracle.vi_tab(interp._xmin, interp._xmax, interp._xshape, V, offs,
                                len(spec.perturb_grid[0]), spec.perturb_proba[0],
                                np.concatenate(xs, axis=1), np.concatenate(gs))
    assert np.array_equal(J, np.array(Js)) and np.array_equal(idx, np.array(idxs))


def test_eval_policy_oracle_vs_reference():
    g = golden('g6_policy')
    _, solver = models.storage_ar1()
    spec = vi_numpy.Spec.from_solver(solver)
    pol = models.storage_ar1_empirical_policy(solver)
    assert np.array_equal(pol, g['ar1_pol_ini'])
    J, J_ref = vi_numpy.eval_policy(spec, pol, 50, rel_dp=True, J_ref_full=True)
    assert np.allclose(J_ref, g['ar1_J_ref'], rtol=1e-12, atol=1e-14)
    assert np.abs(J - g['ar1_J']).max() < 1e-12
    # published value (AR1.ipynb:594): reference cost of the empirical policy 0.105724
    assert '{:g}'.format(J_ref[-1]) == '0.105724'
    J7 = vi_numpy.eval_policy(spec, pol, 7)
    assert np.abs(J7 - g['ar1_J7']).max() < 1e-12


def test_bellman_recursion_oracle_vs_reference():
    g = golden('g8_bellman')
    _, solver = models.finite_horizon()
    spec = vi_numpy.Spec.from_solver(solver)
    nxt = g['J_fin']
    for t in (4, 3, 2, 1, 0):
        J, pol, _, _ = vi_numpy.value_iteration(spec, nxt, t_k=t)
        assert np.abs(J - g['J'][t]).max() <= 1e-13 * max(1.0, np.abs(g['J'][t]).max())
        assert np.array_equal(pol, g['pol'][t])
        nxt = J


def test_pv_storage_time_indexed_data_oracle_vs_reference():
    """finite horizon whose cost looks data up by time index (the shape of the
    reference's examples/01 .../pv_storage_control.py): numpy oracle against
    the reference's bellman_recursion, all 48 steps, bit for bit"""
    g = golden('g9_pv_storage')
    _, solver = models.pv_storage()
    assert np.array_equal(solver.P_prod_data, g['P_prod'])
    spec = vi_numpy.Spec.from_solver(solver)
    nxt = np.zeros(50)
    for t in range(47, -1, -1):
        J, pol, _, _ = vi_numpy.value_iteration(spec, nxt, t_k=t)
        assert np.array_equal(J, g['J'][t]), t
        assert np.array_equal(pol, g['pol'][t]), t
        nxt = J


def test_simulation_oracle_vs_reference_loop():
    """vi_numpy.simulate (the closed loop batched over trajectories, the policy looked up by mlinterp_np) against
    the reference's own loop, one trajectory and one step at a time (tests/golden/make_golden.py g10)"""
    g = golden('g10_simulation')
    _, solver = models.searev(n_E=11, n_S=15, n_A=13)
    spec = vi_numpy.Spec.from_solver(solver)
    x, u, cost = vi_numpy.simulate(spec, g['pol'], g['x0'], g['w'], 400)
    assert x.shape == (401, 5, 3) and u.shape == (400, 5, 1) and cost.shape == (400, 5)
    assert np.array_equal(x, g['x']) and np.array_equal(u, g['u'])
    # the searev cost squares a state-only sub-expression: numpy SCALAR pow in the reference loop, the array
    # power here (1 ulp at most); states and controls involve no such operation
    assert np.allclose(cost, g['g'], rtol=1e-15, atol=0)
    _, ar1 = models.storage_ar1(n_E=21, n_P=25)
    y, v, _ = vi_numpy.simulate(vi_numpy.Spec.from_solver(ar1), g['pol2'], g['y0'], g['w2'], 300)
    assert np.array_equal(y, g['y']) and np.array_equal(v, g['v'])
    # a prefix of the horizon is the prefix of the trajectories; 4-byte reals stay 4-byte
    x5, u5, c5 = vi_numpy.simulate(spec, g['pol'], g['x0'], g['w'], 5)
    assert np.array_equal(x5, x[:6]) and np.array_equal(u5, u[:5]) and np.array_equal(c5, cost[:5])
    x32, u32, c32 = vi_numpy.simulate(spec, g['pol'], g['x0'], g['w'], 50, dtype=np.float32)
    assert x32.dtype == u32.dtype == c32.dtype == np.float32
    assert np.allclose(x32, x[:51], rtol=1e-4, atol=1e-4) and not np.array_equal(x32, x[:51])


def test_simulation_oracle_time_index_and_deterministic_model():
    """a non-stationary model receives t0 + k; a deterministic one runs without w"""
    fh, solver = models.finite_horizon()
    spec = vi_numpy.Spec.from_solver(solver)
    pol = np.linspace(-0.5, 0.5, 17)[:, None]
    w = np.random.default_rng(0).normal(0, 0.1, (12, 2))
    x, u, g = vi_numpy.simulate(spec, pol, [[0.3], [-1.0]], w, 12, t0=2)
    law = vi_numpy.Interp(*spec.state_grid)
    law.set_values(pol[:, 0])
    for b in range(2):
        xs = x[0, b, 0]
        for k in range(12):
            uk = float(law(np.array([xs]))[0])
            assert u[k, b, 0] == uk and g[k, b] == fh.cost(2 + k, xs, uk, w[k, b])
            xs = fh.dyn(2 + k, xs, uk, w[k, b])[0]
            assert x[k + 1, b, 0] == xs
    from stodynprog_amd import SysDescription, DPSolver
    sysd = SysDescription((1, 1, 0), name='deterministic')
    sysd.dyn = lambda x, u: (0.5 * x + u,)
    sysd.cost = lambda x, u: x * x + u * u
    sysd.control_box = lambda x: ((-1., 1.),)
    s = DPSolver(sysd)
    s.discretize_state(-2, 2, 9)
    x, u, g = vi_numpy.simulate(vi_numpy.Spec.from_solver(s), (-0.25 * s.state_grid[0])[:, None], [[1.0], [4.0]],
                                None, 3)
    assert x.shape == (4, 2, 1) and u.shape == (3, 2, 1) and g.shape == (3, 2)
    assert np.array_equal(x[:, 0, 0], [1.0, 0.25, 0.0625, 0.015625])      # u = -x / 4 on the grid
    assert u[0, 1, 0] == -1.0 and x[1, 1, 0] == 1.0                        # extrapolated past x = 2


# ---------------------------------------------------------------- the kernel's definition restated in one real type
# (vi_numpy.value_iteration_real / eval_policy_real: what tests/test_gpu_fp32_oracle.py compares the 4-byte kernels with)
def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def test_restated_definition_in_float64_is_the_reference_path_bit_for_bit():
    """The structure of the restatement is right: in float64 it gives the bits of the functions pinned on the
    reference's fixtures -- the kernel's lattice (k * step + lo, last point hi) is numpy.linspace's arithmetic, the
    narrow lerp tree is the double tree.  On the problems of the G2, G3 and G5 fixtures, from their own inputs."""
    g2, g3, g5 = golden('g2_inventory'), golden('g3_ar1_ref'), golden('g5_synth')
    cases = []
    _, inv = models.inventory()
    cases.append((inv, g2['J'][1], None))
    _, ar1 = models.storage_ar1()
    rng = np.random.default_rng(3)
    cases.append((ar1, g3['J1'], np.unique(np.concatenate([rng.integers(0, 41 * 61, 60), [0, 41 * 61 - 1]]))))
    _, syn = models.synthetic3d(N=20)
    cases.append((syn, g5['s_J1'], np.arange(0, 8000, 13)))
    for solver, V, nodes in cases:
        spec = vi_numpy.Spec.from_solver(solver)
        old = vi_numpy.value_iteration(spec, V, nodes=nodes)
        new = vi_numpy.value_iteration(spec, V, nodes=nodes, dtype=np.float64)
        for a, b, what in zip(old, new, ('J', 'policy', 'index', 'margin')):
            assert _same_bits(a, b), (solver.sys.name, what)
        # the lattice itself, node by node
        for flat in (range(int(np.prod(spec.shape))) if nodes is None else nodes[:40]):
            x_k = tuple(g[i] for g, i in zip(spec.state_grid, np.unravel_index(flat, spec.shape)))
            ga, da = vi_numpy.control_grids(spec, x_k)
            gb, db = vi_numpy.control_lattice_real(spec, x_k, None, np.float64)
            assert da == db and all(_same_bits(a, b) for a, b in zip(ga, gb)), (solver.sys.name, flat)
    # the fixed-policy backup, with and without the relative-DP shift, on the problem of the G6 fixture
    spec = vi_numpy.Spec.from_solver(ar1)
    pol = models.storage_ar1_empirical_policy(ar1)
    for rel in (False, True):
        old = vi_numpy.eval_policy(spec, pol, 4, rel_dp=rel, J_zero=g3['J1'] * 0.1, J_ref_full=True)
        new = vi_numpy.eval_policy(spec, pol, 4, rel_dp=rel, J_zero=g3['J1'] * 0.1, J_ref_full=True, dtype=np.float64)
        if rel:
            assert _same_bits(old[0], new[0]) and _same_bits(old[1], new[1])
        else:
            assert _same_bits(old, new)
    # a time-dependent model (the G8 fixture's)
    _, fh = models.finite_horizon()
    spec = vi_numpy.Spec.from_solver(fh)
    g8 = golden('g8_bellman')
    for a, b in zip(vi_numpy.value_iteration(spec, g8['J_fin'], t_k=3),
                    vi_numpy.value_iteration(spec, g8['J_fin'], t_k=3, dtype=np.float64)):
        assert _same_bits(a, b)


def _restated_models():
    return [('synthetic3d', dict(N=24)), ('storage_ar1', dict(n_E=33, n_P=20, steps=(0.05, 0.1))),
            ('searev', dict(n_E=17, n_S=12, n_A=9, step=0.01)), ('inventory', {}), ('nas_demo', {}),
            ('two_reservoirs', dict(n_a=12, n_b=10, n_y=8)), ('synthetic3d_coupled', dict(N=16)),
            ('inventory_markov', dict(n_x=48, n_d=12))]


def _smooth_V(solver):
    V = np.zeros(solver._state_grid_shape)
    for k, g in enumerate(solver.state_grid):
        g = np.asarray(g, dtype=float)
        shape = [1] * V.ndim
        shape[k] = -1
        z = (g - g[0]) / (g[-1] - g[0])
        V = V + (1.0 + 0.5 * k) * ((z - 0.4) * (z - 0.4)).reshape(shape)
    return V


@pytest.mark.parametrize('name,kw', _restated_models(), ids=[m[0] for m in _restated_models()])
def test_restated_definition_in_float32_is_within_the_float32_bar_of_float64(name, kw):
    """float32 against the float64 oracle on sampled nodes: within 1e-5 of max |J| (the project's bar for 4-byte
    results), from a standard-normal and from a smooth cost-to-go; every result of the callables is float32
    (asserted inside), and the model is one the tracer calls bit-exact."""
    _, solver = getattr(models, name)(**kw)
    assert solver._traced().bit_exact and not solver._traced().inexact_ops()
    spec = vi_numpy.Spec.from_solver(solver)
    S = int(np.prod(spec.shape))
    nodes = np.unique(np.concatenate([np.random.default_rng(1).integers(0, S, 150), [0, S - 1]]))
    for V in (np.random.default_rng(2).standard_normal(spec.shape), _smooth_V(solver)):
        V32 = V.astype(np.float32)
        with np.errstate(all='ignore'):
            J64, _, i64, m64 = vi_numpy.value_iteration(spec, V32.astype(float), nodes=nodes)
            J32, p32, i32, _ = vi_numpy.value_iteration(spec, V32, nodes=nodes, dtype=np.float32)
        assert J32.dtype == np.float32 and p32.dtype == np.float32
        assert np.abs(J32 - J64).max() <= 1e-5 * np.abs(J64).max(), (name, np.abs(J32 - J64).max() / np.abs(J64).max())
        clear = m64 > 1e-4 * np.maximum(1.0, np.abs(J64))
        assert (i32[clear] == i64[clear]).all(), name
    # the fixed-policy backup too, on the small grids: two steps of the float32 sweep's own policy
    if S <= 2500:
        with np.errstate(all='ignore'):
            _, pol, _, _ = vi_numpy.value_iteration(spec, V32, dtype=np.float32)
            E64 = vi_numpy.eval_policy(spec, pol.astype(float), 2, J_zero=V32.astype(float))
            E32 = vi_numpy.eval_policy(spec, pol, 2, J_zero=V32, dtype=np.float32)
        assert E32.dtype == np.float32 and np.abs(E32 - E64).max() <= 1e-5 * np.abs(E64).max()


def test_restated_definition_refuses_a_model_that_widens():
    """a callable that returns float64 from float32 arguments (a numpy float64 parameter) would be rounded twice:
    the width assertion trips instead of a comparison being made"""
    from stodynprog_amd import SysDescription, DPSolver
    gain = np.float64(0.3)
    s = SysDescription((1, 1, 1), name='widening')

    def dyn(x, u, w):
        return (0.9 * x + gain * u + w,)

    def cost(x, u, w):
        return x * x + 0.1 * u * u
    s.dyn, s.cost = dyn, cost
    s.control_box = lambda x: ((-1., 1.),)
    s.perturb_laws = [models.NormalLaw(0, 0.1)]
    solver = DPSolver(s)
    solver.discretize_state(-1, 1, 9)
    solver.discretize_perturb(-0.3, 0.3, 3)
    solver.control_steps = (0.25,)
    spec = vi_numpy.Spec.from_solver(solver)
    V = np.zeros(9, dtype=np.float32)
    vi_numpy.value_iteration(spec, V, dtype=np.float64)            # nothing to widen to in float64
    with pytest.raises(AssertionError, match='float64'):
        vi_numpy.value_iteration(spec, V, dtype=np.float32)
    with pytest.raises(AssertionError, match='float64'):
        vi_numpy.eval_policy(spec, np.zeros((9, 1), dtype=np.float32), 1, dtype=np.float32)
