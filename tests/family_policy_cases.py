"""Policy evaluation and iteration of families: the cases of tests/test_family_policy_plan.py (CPU) and
tests/test_gpu_family_policy.py (GPU), on the members and helpers of tests/family_cases.py.

eval_policy / policy_iteration against the solo calls: every case of family_cases.STATIONARY, with a policy that
differs from member to member and lies off the control lattice.
shrink          family_cases.SHRINK's 16 inventory members under the policy of the oracle's 5th relative sweep from
                zeros: eval_policy from zeros, rel_dp, tol = 1e-6, check_every = 1, n_iter = 300 takes SHRINK_STEPS
                steps by oracle/vi_numpy.py, so the list of running members goes 16 -> 14 -> 8 -> 5 -> 4 -> 0, through
                all three member-to-XCD mappings, and none reaches n_iter.
line tol        family_cases.line_members(17, 9) under the policy of the oracle's first relative sweep from zeros:
                the first evaluation takes LINE_STEPS steps, policy iteration with n_pol = 6 needs 3 improvements,
                4 for members 12, 14 and 16, and every member ends stable.
resident walk   one-member line families of 10 nodes (fewer than the workgroup), 1024 (the largest 'auto' runs
                resident), 2 x 1024 + 129, the largest resident S and that S + 1 (which the resident form refuses).
past the caps   the steps kernel's grid is capped at cus workgroups an XCD, each a tile of 256 nodes: `LONG` (2 members,
                4 XCDs each: more than 256 tiles a part) and `STRIDED` (17 members, 3 on XCD 0: more than 256 units
                there) are sized for 256 compute units and the tests assert that they are past the cap of the device
                they run on.  The resident kernel's grid is capped at one workgroup a compute unit: `many(P)` makes P
                10-node inventory members whose constants never coincide.
"""
import functools

import numpy as np

import family_cases as fc

# ---------------------------------------------------------------------------------------------------------------------
# the host's rules, restated (codegen.family_resident_nodes, SolverFamily._evaluation_form, family_evalpol_step and
# family_resident in csrc/sdp_hip.hip, csrc/sdp_family_policy_kernel.h)
RESIDENT_THREADS = 1024
RESIDENT_LDS_BYTES = 160 * 1024
RESIDENT_REDUCTION_BYTES = 512
STEPS_TILE = 256


def resident_nodes(dtype):
    """the largest member whose two value buffers fit beside the reduction's share of the LDS"""
    return (RESIDENT_LDS_BYTES - RESIDENT_REDUCTION_BYTES) // (2 * np.dtype(dtype).itemsize)


def form(S, dtype, n_iter):
    """what 'auto' picks: the resident form for two steps or more of a member that fits and has at most one node per
    thread of the resident workgroup (the measured rule)"""
    return 'resident' if S <= min(resident_nodes(dtype), RESIDENT_THREADS) and n_iter >= 2 else 'steps'


def launch_steps(S, n_active, cus):
    """the grid of one evaluation step, in the style of family_cases.launch with a tile of 256 nodes: tiles per member,
    XCDs per member, workgroups an XCD wanted and launched, and the units every XCD walks"""
    tiles = -(-S // STEPS_TILE)
    parts = 1 if n_active >= 8 else 8 // n_active
    per_part = -(-tiles // parts)
    wanted = -(-n_active // 8) * tiles if n_active >= 8 else per_part
    units = []
    for xcd in range(8):
        first = xcd // parts
        mine = (n_active - first + 7) // 8 if first < n_active else 0
        units.append(mine * per_part)
    return dict(tiles=tiles, parts=parts, wanted=wanted, per_xcd=max(1, min(wanted, cus)), units=units)


def launch_resident(n_active, cus):
    """workgroups wanted (one a listed member) against the cap (one a compute unit)"""
    return dict(wanted=n_active, blocks=min(n_active, cus))


# ---------------------------------------------------------------------------------------------------------------------
# the oracle's loops
def oracle_eval(make, pol, n_iter, rel_dp=False, J_zero=None, tol=None, check_every=1):
    """oracle/vi_numpy.py's eval_policy_real of one member, step by step (a step of the relative algorithm from the
    shifted array of the step before has the bits of the fused shift): (J, reference costs per step, checks
    [(k, dmin, dmax)]), stopping where stodynprog_amd/convergence.py's rule says so"""
    from oracle import vi_numpy
    from stodynprog_amd import convergence as conv
    s = make() if callable(make) else make
    spec = vi_numpy.Spec.from_solver(s)
    J = np.zeros(spec.shape, dtype=s.dtype) if J_zero is None else np.asarray(J_zero, dtype=s.dtype)
    refs, checks = [], []
    for k in range(1, n_iter + 1):
        out = vi_numpy.eval_policy_real(spec, pol, 1, s.dtype, rel_dp, J_zero=J)
        J_k, ref = out if rel_dp else (out, None)
        refs.append(ref)
        stop = False
        if tol is not None and conv.is_check(k, n_iter, check_every):
            dmin, dmax = conv.diff_stats(J_k, J, s.dtype)
            checks.append((k, dmin, dmax))
            stop = conv.converged(dmin, dmax, tol)
        J = J_k
        if stop:
            break
    return J, np.array(refs, dtype=float) if rel_dp else None, checks


def oracle_policy_iteration(make, pol_init, n_val, n_pol, tol, check_every=1):
    """DPSolver.policy_iteration with rel_dp and tol on the oracle: (J, J_ref, pol, steps of every evaluation,
    improvements, stable)"""
    from oracle import vi_numpy
    s = make()
    spec = vi_numpy.Spec.from_solver(s)
    pol = np.asarray(pol_init, dtype=s.dtype)
    J, refs, checks = oracle_eval(s, pol, n_val, True, tol=tol, check_every=check_every)
    steps, n_imp, stable = [len(refs)], 0, False
    for _ in range(n_pol):
        _, pol_new, _, _ = vi_numpy.value_iteration_real(spec, (J, 0.), s.dtype, True)
        n_imp += 1
        if np.array_equal(pol_new, pol):
            stable, pol = True, pol_new
            break
        pol = pol_new
        J, refs, checks = oracle_eval(s, pol, n_val, True, tol=tol, check_every=check_every)
        steps.append(len(refs))
    return J, refs[-1], pol, steps, n_imp, stable


def sweep_policy(make, sweeps):
    """the policy of the oracle's `sweeps`-th relative sweep from zeros"""
    dims = make()._shape()
    return fc.oracle_sweeps(make, np.zeros(dims), sweeps, True)[0][-1][2]


# ---------------------------------------------------------------------------------------------------------------------
# to a tolerance
SHRINK = dict(members=fc.SHRINK['members'], tol=1e-6, check_every=1, n_iter=300, policy_sweep=5)
SHRINK_STEPS = [16, 18, 16, 14, 16, 15, 17, 15, 15, 15, 18, 15, 18, 15, 18, 14]       # by the oracle (test_family_policy_plan.py)
SHRINK_SIZES = [16, 14, 8, 5, 4, 0]
SHRINK_CAPPED = dict(check_every=3, n_iter=17)       # the members that need 18 steps stop at the cap, not converged
LINE = dict(members=fc.line_members(17, fc.LINE_NX), tol=1e-6, check_every=1, n_val=100, n_pol=6, policy_sweep=1)
LINE_STEPS = [23, 23, 24, 24, 24, 24, 24, 24, 25, 25, 25, 25, 25, 25, 25, 26, 26]
LINE_IMPROVEMENTS = [3] * 12 + [4, 3, 4, 3, 4]


@functools.lru_cache(maxsize=None)
def shrink_policies():
    return np.stack([sweep_policy(make, SHRINK['policy_sweep']) for make in SHRINK['members']])


@functools.lru_cache(maxsize=None)
def line_policies():
    return np.stack([sweep_policy(make, LINE['policy_sweep']) for make in LINE['members']])


# ---------------------------------------------------------------------------------------------------------------------
# against the solo calls: a policy off the lattice
def off_lattice(pol, case):
    """a family's policy plus a small offset that differs by node and by member"""
    rng = np.random.default_rng(7 + len(case.name))
    return (np.asarray(pol) + rng.uniform(-0.01, 0.01, size=np.shape(pol))).astype(case.dtype)


# ---------------------------------------------------------------------------------------------------------------------
# shapes of the resident walk, and the cases past the launch caps
def walk_sizes():
    S_max = resident_nodes(np.float64)
    return [10, RESIDENT_THREADS, 2 * RESIDENT_THREADS + 129, S_max, S_max + 1]


def walk_case(n_x):
    return fc.Case('line walk {}'.format(n_x), [fc.line(0.55, 1.21, -0.37, n_x)], oracle=True)


LONG_NX = 4 * 256 * STEPS_TILE + 129         # 2 members, 4 XCDs each: 257 tiles a part against 256 workgroups an XCD
STRIDED_NX = 85 * STEPS_TILE + 3             # 17 members: 3 x 86 = 258 units on XCD 0
LONG = fc.Case('line eval long', fc.line_members(2, LONG_NX), oracle=True)
STRIDED = fc.Case('line eval strided', fc.line_members(17, STRIDED_NX), oracle=True)


def many(P):
    """P 10-node inventory members; no two constants of a member coincide, with each other or with another member's"""
    return fc.Case('inventory P={}'.format(P), [fc.inventory(0.3 + 0.011 * i, 2.5 + 0.013 * i, 1.1 + 0.007 * i)
                                                for i in range(P)], oracle=True)


def line_policy(case):
    """a policy inside the box that differs by node and by member, in the case's reals"""
    dims = case.members[0]()._shape()
    P = len(case.members)
    x = np.linspace(-1., 1., dims[0])
    return np.stack([0.6 * np.sin(3. * x + 0.1 * p) for p in range(P)])[..., None].astype(case.dtype)


def unit_sources():
    """the generated source of every unit the GPU tests run beside those of family_cases.unit_sources(): the
    evaluation unit of every family, the sweep unit of the walk and `many` families, and the solo 'generic' units of
    the two cases to a tolerance (those of the STATIONARY cases are family_cases')"""
    from stodynprog_amd import SolverFamily, codegen
    out = []
    to_tol = [fc.Case('shrink', SHRINK['members']), fc.Case('line tol', LINE['members'])]
    for case in fc.STATIONARY + [fc.CHUNKS] + to_tol + [walk_case(10), many(3)]:
        fam = SolverFamily(case.solvers())
        tabs = fam._tables(None)
        out += [tabs['source'], codegen.family_policy_unit(tabs['model'], fam.dtype)]
        for s in fam.solvers if case in to_tol else []:
            s.kernel = 'generic'
            out.append(s._kernel_plan(None, s._trace_now(None))['source'])
    # the evaluation units of two time-dependent families at step 0 (tests/test_family_policy_plan.py reads their notes)
    for case in fc.HORIZON[:2]:
        fam = SolverFamily(case.solvers())
        out.append(codegen.family_policy_unit(fam._tables(0)['model'], fam.dtype))
    return out
