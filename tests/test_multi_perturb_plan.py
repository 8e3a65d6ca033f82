"""Several perturbation variables, without a GPU: the definition of the flat law (stodynprog_amd/perturb.py) against an
independent loop, what the cases of tests/multi_perturb.py plan, and their code objects cross-compiled for gfx950.

The host paths of such a system (tabulated backups, the host loops of simulate and monte_carlo) all go through the
library's interpolation kernels, so they are checked on the device: tests/test_gpu_multi_perturb.py."""
import itertools

import numpy as np
import pytest

import multi_perturb as mp
from test_montecarlo_kernel import _kernels
from stodynprog_amd import SysDescription, DPSolver, codegen, perturb
from stodynprog_amd.solver import plan_info

FAST_FAMILIES = ('column', 'lead', 'line', 'staged')


def _loop_law(grids, probas):
    """the definition as a plain loop: itertools.product runs the LAST variable fastest"""
    wtab, P = [], []
    for point in itertools.product(*[range(len(g)) for g in grids]):
        wtab.append([float(grids[i][j]) for i, j in enumerate(point)])
        p = float(probas[0][point[0]])
        for i in range(1, len(point)):
            p = p * float(probas[i][point[i]])
        P.append(p)
    return np.array(wtab).T, np.array(P)


LAWS = {
    (3, 2): [mp.LAW_3A, mp.LAW_2B],
    (2, 3, 2): [mp.LAW_2B, mp.LAW_3B, ([0.2, -0.4], [0.7, 0.3])],
}


@pytest.mark.parametrize('dims', sorted(LAWS))
@pytest.mark.parametrize('real', sorted(mp.DTYPES))
def test_product_law_is_the_loop(dims, real):
    dt = mp.DTYPES[real]
    grids, probas = [g for g, _ in LAWS[dims]], [p for _, p in LAWS[dims]]
    wtab, P = perturb.product_law(grids, probas, dt)
    want_w, want_P = _loop_law(grids, probas)
    assert wtab.shape == (len(dims), int(np.prod(dims))) and P.shape == (int(np.prod(dims)),)
    assert wtab.dtype == dt and P.dtype == dt
    assert np.array_equal(wtab, want_w.astype(dt)) and np.array_equal(P, want_P.astype(dt))    # (rounded ONCE)
    # C order, the last variable fastest: the flat index is ravel_multi_index
    for point in itertools.product(*[range(n) for n in dims]):
        j = int(np.ravel_multi_index(point, dims))
        assert all(wtab[i, j] == dt(grids[i][k]) for i, k in enumerate(point))
    # the transposed order (first variable fastest) is another table on these asymmetric laws
    index = np.unravel_index(np.arange(P.size), dims, order='F')
    other = np.array([np.asarray(g)[index[i]] for i, g in enumerate(grids)]).astype(dt)
    assert not np.array_equal(other, wtab)
    assert abs(float(want_P.sum()) - 1.0) < 1e-12


def test_one_variable_is_its_own_law():
    g, p = mp.LAW_5
    wtab, P = perturb.product_law([g], [p])
    assert np.array_equal(wtab, np.array([g])) and np.array_equal(P, np.array(p))


@pytest.mark.parametrize('case', mp.CASES, ids=repr)
@pytest.mark.parametrize('real', sorted(mp.DTYPES))
def test_case_plans_the_family(case, real):
    solver = case.solver(mp.DTYPES[real])
    assert tuple(len(g) for g in solver.perturb_grid) == case.dims
    for t in (range(case.horizon) if case.horizon else (None,)):
        plan = mp.plan_of(solver, t)
        info = plan_info(plan)
        assert info['kernel'] == 'generic' and info['perturb_vars'] == case.m and info['n_perturb'] == case.m, info
        assert not info['certified_filter'] and info['staged'] is None and not info['controlled_axes'], info
        assert plan['W'] == int(np.prod(case.dims))
        assert plan['lanes'] == codegen.lanes_for(plan['max_u']) == case.lanes, (plan['lanes'], plan['max_u'])
        src = plan['source']
        assert '#define SDP_NW {} '.format(case.m) in src and 'const sdp_real *w,' in src
        assert 'w[{}]'.format(case.m - 1) in src and 'w[{}]'.format(case.m) not in src
    if case.name == 'ragged':
        assert plan['per_node']
    if case.horizon:
        assert plan['model'].t_value is not None and plan['model'].param_index     # DATA[k]: traced per step, lifted
        assert len({mp.plan_of(solver, t)['source'] for t in range(case.horizon)}) == 1    # one code object


@pytest.mark.parametrize('family', FAST_FAMILIES)
def test_fast_families_take_one_variable(family):
    solver = mp.BY_NAME['ragged'].solver()
    solver.kernel = family
    with pytest.raises(ValueError, match='one perturbation variable'):
        solver._kernel_plan()


def test_one_variable_units_are_untouched():
    twin = mp.degenerate_twin()
    src = twin._kernel_plan()['source']
    assert 'SDP_NW' not in src and 'sdp_real w,' in src
    assert plan_info(twin._kernel_plan())['perturb_vars'] == 1


def _five():
    s = SysDescription((1, 1, 5), name='five')
    s.dyn = lambda x, u, a, b, c, d, e: (x + u + a + b + c + d + e,)
    s.cost = lambda x, u, a, b, c, d, e: x * x + a * b * c * d * e
    s.control_box = lambda x: ((0., 1.),)
    solver = DPSolver(s)
    solver.discretize_state(0, 1, 3)
    solver.perturb_grid = [np.array([0., 1.])] * 5
    solver.perturb_proba = [np.array([0.5, 0.5])] * 5
    solver.control_steps = (0.5,)
    return solver


def test_five_variables_are_not_implemented():
    solver = _five()
    with pytest.raises(NotImplementedError, match='at most 4'):
        solver._kernel_plan()
    with pytest.raises(NotImplementedError, match='at most 4'):
        solver._check_supported()
    with pytest.raises(NotImplementedError, match='at most 4'):
        codegen.model_function_source(solver._traced())


def test_several_gpus_are_not_implemented():
    solver = mp.BY_NAME['order'].solver()
    solver.comm = object()          # (any communicator: refused before it is looked at)
    with pytest.raises(NotImplementedError, match='one GPU'):
        solver._check_supported()


def test_a_law_too_large_for_the_draw_table_names_the_limit():
    solver = mp.BY_NAME['wide'].solver()
    n = 3000                        # 8 (n - 1) + 3 n 8 = 95 992 bytes
    with pytest.raises(ValueError, match='65536'):
        solver._mc_law((np.zeros((3, n)), np.full(n, 1.0 / n)))
    values, proba = solver._mc_law(None)
    assert values.shape == (3, 12) and proba.shape == (12,)
    with pytest.raises(ValueError, match='shape'):
        solver._mc_law((np.zeros((2, 4)), np.full(4, 0.25)))


def test_cache_key_covers_every_variable():
    """the second variable's grid and law are part of the problem's and the plan's keys"""
    solver = mp.BY_NAME['order'].solver()
    fp = solver._fingerprint(None)
    solver.perturb_grid[1] = solver.perturb_grid[1] + 0.25
    fp_grid = solver._fingerprint(None)
    solver.perturb_proba[1] = np.array([0.5, 0.5])
    assert len({fp, fp_grid, solver._fingerprint(None)}) == 3


@pytest.mark.parametrize('case', mp.CASES, ids=repr)
@pytest.mark.parametrize('real', sorted(mp.DTYPES))
def test_code_object_has_no_scratch(case, real, tmp_path):
    plan = mp.plan_of(case.solver(mp.DTYPES[real]), 0 if case.horizon else None)
    kernels, dis = _kernels(plan['source'], tmp_path)
    assert {'sdp_sweep', 'sdp_evalpol', 'sdp_simulate', 'sdp_montecarlo'} <= set(kernels), sorted(kernels)
    for name in ('sdp_sweep', 'sdp_evalpol', 'sdp_simulate', 'sdp_montecarlo'):
        f = kernels[name]
        print(case, real, name, {k: f[k] for k in ('.vgpr_count', '.sgpr_count', '.private_segment_fixed_size',
                                                   '.group_segment_fixed_size')})
        assert f['.private_segment_fixed_size'] == 0 and f['.vgpr_spill_count'] == 0, (name, f)
        assert f['.group_segment_fixed_size'] == 0, (name, f)         # (the draw table is dynamic LDS; the sweep uses none)
        assert 'scratch_' not in dis.split('<{}>:'.format(name))[1].split('>:\n')[0]
    # the flat law is read by scalar loads: j is the same in every lane
    sweep = dis.split('<sdp_sweep>:')[1].split('>:\n')[0]
    assert 's_load_dword' in sweep


def test_library_refuses_more_than_four_variables():
    import ctypes as C
    from stodynprog_amd import _native as nat
    lib = nat.lib()
    h = C.c_void_p()
    d = nat.sdp_problem_desc()
    d.dtype, d.d, d.nu, d.W, d.n_perturb = 0, 1, 1, 2, 5
    assert lib.sdp_problem_create(C.byref(d), C.byref(h)) == -1           # SDP_EINVAL
    assert b'at most 4' in lib.sdp_last_error()
    d.W, d.n_perturb = 0, 2
    assert lib.sdp_problem_create(C.byref(d), C.byref(h)) == -1
    assert b'no point' in lib.sdp_last_error()
