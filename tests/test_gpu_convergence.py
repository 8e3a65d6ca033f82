"""Sweep loops that stop at a tolerance (value_iterations / eval_policy / policy_iteration with `tol`), on the GPU.

The statistics the library reduces on the device (k_diff_stats) must be the bits of convergence.diff_stats over the
arrays of fresh calls, in every unit of the parameter study, with and without rel_dp; a call that stops must return
what the call with n_iter = the sweeps it ran returns; the host paths (tabulated callables, host communicator) and
several ranks through the collective stand-in must agree with the single process bit for bit."""
import io
import contextlib
import os

import numpy as np
import pytest

import policies as P
from stodynprog_amd import SysDescription, DPSolver, models, convergence as conv
from stodynprog_amd.trace import TraceError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNITS = [f for f in P.FAMILIES if not f.name.endswith(' fp32') or f.name == 'column fp32']


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def same(a, b):
    return np.array_equal(np.asarray(a, dtype=float), np.asarray(b, dtype=float), equal_nan=True)


def start(solver, V0, rel_dp):
    """J^(0) in the problem's reals, and what value_iterations takes"""
    V = np.asarray(V0, dtype=solver.dtype)
    if rel_dp:
        V = (V - V[solver._state_ref_ind]).astype(solver.dtype)
        return V, (V, 0.0)
    return V, V


def vi_fresh(solver, V0, n, rel_dp):
    """J^(0..n) and the policies / reference costs of fresh value_iterations calls"""
    J0, arg = start(solver, V0, rel_dp)
    seq, pols, refs = [J0], [None], [None]
    for k in range(1, n + 1):
        J, pol = quiet(solver.value_iterations, arg, k, rel_dp, False, True)
        if rel_dp:
            J, r = J
            refs.append(np.asarray(r))
        seq.append(J)
        pols.append(pol)
    return seq, pols, refs


def ev_fresh(solver, pol, V0, n, rel_dp):
    J0 = np.asarray(V0, dtype=solver.dtype)
    seq, refs = [J0], [None]
    for k in range(1, n + 1):
        out = quiet(solver.eval_policy, pol, k, rel_dp, V0, False, True)
        if rel_dp:
            out, r = out
            refs.append(np.asarray(r))
        seq.append(out)
    return seq, refs


def expected_stats(solver, seq):
    return [conv.diff_stats(seq[k], seq[k - 1], solver.dtype) for k in range(1, len(seq))]


def check_record(rec, stats, checked, what):
    assert rec is not None and rec.checked == checked, (what, rec and rec.checked, checked)
    assert same(rec.dmin, [stats[k - 1][0] for k in checked]), (what, rec.dmin, stats)
    assert same(rec.dmax, [stats[k - 1][1] for k in checked]), (what, rec.dmax, stats)
    assert not np.signbit(rec.dmin[rec.dmin == 0]).any() and not np.signbit(rec.dmax[rec.dmax == 0]).any(), what


def first_stop(stats, n, c, tol):
    for k in conv.check_schedule(n, c):
        if conv.converged(stats[k - 1][0], stats[k - 1][1], tol):
            return k
    return n


@pytest.mark.timeout(900)
@pytest.mark.parametrize('rel_dp', [False, True], ids=['plain', 'rel_dp'])
@pytest.mark.parametrize('unit', UNITS, ids=lambda f: f.name)
def test_value_iterations_until_in_every_unit(gpu, unit, rel_dp):
    s = unit.solver()
    V0 = np.random.default_rng(21).standard_normal(s._state_grid_shape)
    seq, pols, refs = vi_fresh(s, V0, 10, rel_dp)
    stats = expected_stats(s, seq)
    _, arg = start(s, V0, rel_dp)
    # tol = 0: every sweep checked, J and the policy those of the call without tol
    J, pol = quiet(s.value_iterations, arg, 6, rel_dp, False, True, tol=0.0)
    for k, v in unit.info.items():
        assert s.backend_info[k] == v, (unit, k, s.backend_info)
    rec = s.last_convergence
    n = rec.n_iter
    assert n == first_stop(stats, 6, 1, 0.0)
    check_record(rec, stats, list(range(1, n + 1)), (unit, rel_dp))
    if rel_dp:
        J, r = J
        assert same(r, refs[n]), (unit, 'refs')
        assert same(rec.lower, rec.dmin + refs[n][np.array(rec.checked) - 1])
    assert np.array_equal(J, seq[n]) and np.array_equal(pol, pols[n]), unit
    # a tolerance met at sweep m stops the call at the first checked sweep whose span is below it
    spans = [b - a for a, b in stats]
    for c, m in ((1, 3), (2, 3), (1, 1)):
        tol = spans[m - 1]
        J, pol = quiet(s.value_iterations, arg, 10, rel_dp, False, True, tol=tol, check_every=c)
        rec = s.last_convergence
        n = first_stop(stats, 10, c, tol)
        assert rec.n_iter == n and rec.converged == conv.converged(*stats[n - 1], tol), (unit, c, m, rec)
        check_record(rec, stats, [k for k in conv.check_schedule(10, c) if k <= n], (unit, c, m))
        if rel_dp:
            J, r = J
            assert same(r, refs[n])
        assert np.array_equal(J, seq[n]) and np.array_equal(pol, pols[n]), (unit, c, m)
    # the schedule: sweeps 3, 6, 9 and the last one
    quiet(s.value_iterations, arg, 10, rel_dp, False, True, tol=0.0, check_every=3)
    if not any(conv.converged(*stats[k - 1], 0.0) for k in (3, 6, 9)):
        check_record(s.last_convergence, stats, [3, 6, 9, 10], unit)
    # and a call without tol leaves no record
    quiet(s.value_iterations, arg, 2, rel_dp)
    assert s.last_convergence is None


@pytest.mark.timeout(900)
@pytest.mark.parametrize('kind', ['lattice', 'special'])
@pytest.mark.parametrize('rel_dp', [False, True], ids=['plain', 'rel_dp'])
@pytest.mark.parametrize('unit', UNITS, ids=lambda f: f.name)
def test_eval_policy_until_in_every_unit(gpu, unit, rel_dp, kind):
    s = unit.solver()
    V0 = np.random.default_rng(22).standard_normal(s._state_grid_shape).astype(s.dtype).astype(float)
    pol = P.policy(s, kind, seed=3, V=V0)
    seq, refs = ev_fresh(s, pol, V0, 10, rel_dp)
    stats = expected_stats(s, seq)
    spans = [b - a for a, b in stats]
    if kind == 'special':
        assert np.isnan(spans[-1]), (unit, spans)                  # NaN / inf in J: the span is NaN
    mid = 1e300 if np.isnan(spans[2]) else spans[2]
    for tol, c in ((0.0, 1), (mid, 1), (mid, 2), (0.0, 3), (np.inf, 3)):
        out = quiet(s.eval_policy, pol, 10, rel_dp, V0, False, True, tol=tol, check_every=c)
        rec = s.last_convergence
        n = first_stop(stats, 10, c, tol)
        assert rec.n_iter == n, (unit, kind, tol, c, rec)
        if np.isnan(spans).all():
            assert n == 10 and not rec.converged             # a NaN span never stops the loop
        check_record(rec, stats, [k for k in conv.check_schedule(10, c) if k <= n], (unit, kind, tol, c))
        if rel_dp:
            out, r = out
            assert same(r, refs[n]), (unit, kind, 'refs')
        assert same(out, seq[n]), (unit, kind, tol, c)


def test_real_models_converge_and_bracket_the_average_cost(gpu):
    # the inventory tutorial (doc/example_inventory.py) and storage-AR1 (the AR1 notebook), relative DP
    for name, kw, n_max, tol in (('inventory', {}, 2000, 1e-9), ('storage_ar1', {}, 3000, 1e-7)):
        _, s = getattr(models, name)(**kw)
        J0 = np.zeros(s._state_grid_shape)
        (J, refs), pol = quiet(s.value_iterations, (J0, 0.0), n_max, True, False, True, tol=tol, check_every=10)
        rec = s.last_convergence
        print(name, rec, rec.lower[-1], refs[-1], rec.upper[-1])
        assert rec.converged and rec.n_iter < n_max and rec.span[-1] <= tol, (name, rec)
        assert len(refs) == rec.n_iter
        assert rec.lower[-1] <= refs[-1] <= rec.upper[-1], (name, rec.lower[-1], refs[-1], rec.upper[-1])
        # the bounds tighten: the first check's bracket holds the last one's
        assert rec.lower[0] <= rec.lower[-1] + 1e-9 * abs(refs[-1]) and rec.upper[-1] <= rec.upper[0] + 1e-9 * abs(refs[-1])
        # the policy's evaluation to the same tolerance brackets the same average cost
        E, r = quiet(s.eval_policy, pol, n_max, True, J, False, True, tol=tol, check_every=10)
        ev = s.last_convergence
        assert ev.converged and ev.lower[-1] <= r[-1] <= ev.upper[-1], (name, ev)


def test_policy_iteration_stops_with_a_stable_policy(gpu):
    _, s = models.storage_ar1()
    pol0 = models.storage_ar1_empirical_policy(s)
    tol, n_val, n_pol = 1e-7, 3000, 8
    (J, r), pol = quiet(s.policy_iteration, pol0, n_val, n_pol, True, tol=tol, check_every=10)
    rec = s.last_convergence
    print(rec, [e.n_iter for e in rec.evaluations])
    assert rec.stable and rec.n_improvements < n_pol, rec
    assert len(rec.evaluations) == rec.n_improvements and all(e.converged for e in rec.evaluations), rec
    # the same chain by hand
    p = pol0
    Jh = quiet(s.eval_policy, p, n_val, True, tol=tol, check_every=10)
    for k in range(n_pol):
        _, p2 = quiet(s.value_iteration, Jh, rel_dp=True)
        if np.array_equal(p2, p):
            p = p2
            break
        p = p2
        Jh = quiet(s.eval_policy, p, n_val, True, tol=tol, check_every=10)
    assert k + 1 == rec.n_improvements
    assert np.array_equal(pol, p) and np.array_equal(J, Jh[0]) and r == Jh[1]


def _untraceable_twin():
    _, ref = models.nas_demo(n_E=11, n_P=9, n_w=5)
    sysd = SysDescription((2, 1, 1), name='untraceable')

    def dyn(E, P_req, P_sto, innov):
        shape = np.shape(P_sto)                     # needs a concrete array
        return ref.sys.dyn(E, P_req, np.asarray(P_sto).reshape(shape), innov)
    sysd.dyn = dyn
    sysd.cost = ref.sys.cost
    sysd.control_box = ref.sys.control_box
    sysd.perturb_laws = ref.sys.perturb_laws
    solver = DPSolver(sysd)
    solver.discretize_state(0, 7.2, 11, -6, 6, 9)
    solver.perturb_grid, solver.perturb_proba = ref.perturb_grid, ref.perturb_proba
    solver.control_steps = (.1,)
    assert isinstance(solver._traced(), TraceError)
    return solver, ref


def test_untraceable_model_takes_the_same_decisions(gpu):
    tab, ref = _untraceable_twin()
    V = np.random.default_rng(0).standard_normal((11, 9))
    for rel_dp in (False, True):
        arg = (V - V[tab._state_ref_ind], 0.0) if rel_dp else V
        for tol_from, c in ((0, 1), (3, 1), (3, 2)):
            tol = 0.0
            if tol_from:
                quiet(ref.value_iterations, arg, 8, rel_dp, False, True, tol=0.0)
                tol = ref.last_convergence.span[tol_from - 1]
            a = quiet(tab.value_iterations, arg, 8, rel_dp, False, True, tol=tol, check_every=c)
            assert tab.backend_info['mode'] == 'tabulated'
            ra = tab.last_convergence
            b = quiet(ref.value_iterations, arg, 8, rel_dp, False, True, tol=tol, check_every=c)
            rb = ref.last_convergence
            assert ra.n_iter == rb.n_iter and ra.checked == rb.checked, (rel_dp, ra, rb)
            assert same(ra.dmin, rb.dmin) and same(ra.dmax, rb.dmax), (rel_dp, ra.dmin, rb.dmin)
            assert np.array_equal(a[1], b[1])
            for x, y in zip(a[0] if rel_dp else (a[0],), b[0] if rel_dp else (b[0],)):
                assert np.array_equal(x, y)
        pol = b[1]
        Ea = quiet(tab.eval_policy, pol, 8, rel_dp, V, False, True, tol=0.0)
        ra = tab.last_convergence
        Eb = quiet(ref.eval_policy, pol, 8, rel_dp, V, False, True, tol=0.0)
        rb = ref.last_convergence
        assert ra.n_iter == rb.n_iter and same(ra.dmin, rb.dmin) and same(ra.dmax, rb.dmax), (rel_dp, ra, rb)
        for x, y in zip(Ea if rel_dp else (Ea,), Eb if rel_dp else (Eb,)):
            assert np.array_equal(x, y)


# ---------------------------------------------------------------------------------------------------------- ranks
RANK_WORKER = r'''
import os, sys
sys.path.insert(0, {root!r})
sys.path.insert(0, os.path.join({root!r}, 'tests'))
import io, contextlib
import numpy as np
from stodynprog_amd import models
if os.environ.get('SDP_TEST_GLOO'):
    import torch.distributed as tdist
    tdist.init_process_group('gloo', init_method='env://')
    from gloo_comm import GlooCommunicator
    comm = GlooCommunicator()
    EXCHANGES = ['host']
else:
    from stodynprog_amd import dist
    comm, rdv = dist.from_env()
    EXCHANGES = os.environ['SDP_TEST_EXCHANGES'].split(',')
rank = comm.rank

def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)

def same(a, b):
    return np.array_equal(np.asarray(a, dtype=float), np.asarray(b, dtype=float), equal_nan=True)

CASES = [('synthetic3d', dict(N=20), 4), ('storage_ar1', dict(), 2)]
if os.environ.get('SDP_TEST_CASES'):
    CASES = [CASES[int(k)] for k in os.environ['SDP_TEST_CASES'].split(',')]
for (name, kw, phases) in CASES:
    for exchange in EXCHANGES:
        _, one = getattr(models, name)(**kw)
        _, two = getattr(models, name)(**kw)
        two.comm = comm
        if exchange != 'host':
            two.comm_exchange = 'peer' if exchange == 'sparse' else exchange
            two.comm_sparse = exchange in ('sparse', 'direct')
            two.comm_phases = phases
        V0 = np.random.default_rng(5).standard_normal(one._state_grid_shape)
        V0s = V0 - V0[one._state_ref_ind]
        for rel_dp in (False, True):
            arg = (V0s, 0.0) if rel_dp else V0
            for tol_from, c in ((0, 1), (3, 1), (4, 3)):
                tol = 0.0
                if tol_from:
                    quiet(one.value_iterations, arg, 8, rel_dp, False, True, tol=0.0)
                    tol = one.last_convergence.span[tol_from - 1]
                a = quiet(one.value_iterations, arg, 8, rel_dp, False, True, tol=tol, check_every=c)
                ra = one.last_convergence
                b = quiet(two.value_iterations, arg, 8, rel_dp, False, True, tol=tol, check_every=c)
                rb = two.last_convergence
                what = (name, exchange, rel_dp, tol_from, c)
                if exchange != 'host':
                    prob = [v for k, v in two._cache.items() if k[0] == 'problem'][0]
                    assert prob.parts is not None and prob.node_range[1] - prob.node_range[0] == V0.size, what
                    if exchange in ('sparse', 'direct'):
                        assert two.backend_info['exchange'].endswith('-sparse'), (what, two.backend_info)
                assert ra.n_iter == rb.n_iter and ra.checked == rb.checked, (what, ra, rb)
                assert same(ra.dmin, rb.dmin) and same(ra.dmax, rb.dmax), (what, ra.dmin, rb.dmin, ra.dmax, rb.dmax)
                assert np.array_equal(a[1], b[1]), what
                for x, y in zip(a[0] if rel_dp else (a[0],), b[0] if rel_dp else (b[0],)):
                    assert np.array_equal(x, y), what
                pol = a[1]
            for tol_from, c in ((0, 1), (3, 2)):
                tol = 0.0
                if tol_from:
                    quiet(one.eval_policy, pol, 8, rel_dp, V0, False, True, tol=0.0)
                    tol = one.last_convergence.span[tol_from - 1]
                Ea = quiet(one.eval_policy, pol, 8, rel_dp, V0, False, True, tol=tol, check_every=c)
                ra = one.last_convergence
                Eb = quiet(two.eval_policy, pol, 8, rel_dp, V0, False, True, tol=tol, check_every=c)
                rb = two.last_convergence
                what = (name, exchange, rel_dp, 'eval', tol_from, c)
                assert ra.n_iter == rb.n_iter and ra.checked == rb.checked, (what, ra, rb)
                assert same(ra.dmin, rb.dmin) and same(ra.dmax, rb.dmax), (what, ra.dmin, rb.dmin)
                for x, y in zip(Ea if rel_dp else (Ea,), Eb if rel_dp else (Eb,)):
                    assert np.array_equal(x, y), what
        print('rank', rank, name, exchange, 'ok', flush=True)
        for k in [k for k in list(two._cache) if k[0] == 'problem']:
            prob = two._cache.pop(k)
            if exchange != 'host':
                prob.unmap_peers()
                comm.barrier()
            prob.close()
comm.barrier()
print('rank', rank, 'all ok', flush=True)
'''


@pytest.mark.timeout(900)
@pytest.mark.parametrize('world,exchanges,cases', [(2, 'rccl,sparse,direct', ''), (4, 'sparse', '0'), ('gloo', '', '')])
def test_several_ranks_take_the_same_decisions(gpu, tmp_path, world, exchanges, cases):
    import importlib.util
    from test_gpu_dist import _build_mock, _with_hooks, _run_ranks
    script = tmp_path / 'until_worker.py'
    script.write_text(RANK_WORKER.format(root=ROOT))
    if world == 'gloo':
        if importlib.util.find_spec('torch') is None:
            pytest.skip('torch not installed')
        outs = _run_ranks(script, 2, dict(SDP_TEST_GLOO='1'), timeout=600)
        n = 2
    else:
        mock = _build_mock(tmp_path, asynchronous=True)
        outs = _run_ranks(_with_hooks(tmp_path, script), world,
                          dict(SDP_RCCL_LIBRARY=mock, SDP_TEST_EXCHANGES=exchanges, SDP_TEST_CASES=cases), timeout=800)
        n = world
    for rank in range(n):
        assert 'rank {} all ok'.format(rank) in outs[rank], outs[rank][-2000:]


@pytest.mark.timeout(900)
def test_full_size_stop_and_statistics(gpu):
    """the benchmark model, 256^3 float64: a tolerance stops the run, and the last check's statistics are those of
    the two arrays downloaded by plain calls"""
    _, s = models.synthetic3d(N=256)
    V0 = models.synthetic3d_V0(s.state_grid)
    quiet(s.value_iterations, V0, 4, False, False, tol=0.0)
    first = s.last_convergence
    assert first.n_iter == 4 and first.checked == [1, 2, 3, 4]
    tol = first.span[2]
    J, pol = quiet(s.value_iterations, V0, 20, False, False, tol=tol, check_every=1)
    rec = s.last_convergence
    n = rec.n_iter
    assert rec.converged and n <= 3, rec
    J1 = V0 if n == 1 else quiet(s.value_iterations, V0, n - 1, False, False)[0]
    Jn, pn = quiet(s.value_iterations, V0, n, False, False)
    assert np.array_equal(J, Jn) and np.array_equal(pol, pn)
    dmin, dmax = conv.diff_stats(Jn, J1, s.dtype)
    assert rec.dmin[-1] == dmin and rec.dmax[-1] == dmax, (rec.dmin[-1], dmin, rec.dmax[-1], dmax)
    assert first.dmin[n - 1] == dmin and first.dmax[n - 1] == dmax
