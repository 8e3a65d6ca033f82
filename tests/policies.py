"""Policies a user might hand to eval_policy, policy_iteration and simulate, and the units they run in (test
infrastructure, like tests/column_forms.py; not a test file).

value_iteration only ever returns controls of the lattice of its box: finite, inside the box, on the grid of
control_steps.  A user's policy need not be any of these.  `policy(solver, kind)` makes one of

- 'lattice': the policy of one sweep from a standard-normal cost-to-go;
- 'smooth':  a continuous function of the state, inside the box and off its lattice;
- 'outside': a continuous function that reaches about 3 box widths beyond the box on both sides, so the next states
             leave the grid and are extrapolated;
- 'random':  uniform in the box node by node: the nodes of one column reach rows far apart, farther than any row
             window;
- 'special': the smooth policy with NaN, +inf and -inf at rows 0 and n0 - 1, in the last column and at the rows
             around the boundaries of split columns (column_forms.split_rows).

Every control component is generated independently of the others.

FAMILIES are the units of the parameter study (tests/test_gpu_call_to_call.py, whose builders are reused) and their
4-byte variants where the family plans 4-byte reals; `family_of(plan)` names what a plan is, on the CPU."""
import numpy as np

import column_forms as cf
from stodynprog_amd import DPSolver
from test_gpu_call_to_call import FAMILIES as STUDY, VALUES

KINDS = ('lattice', 'smooth', 'outside', 'random', 'special')


def _box(solver):
    """(lo, hi) of every control at every node: arrays of shape state_dims + (nu,)"""
    dims = solver._state_grid_shape
    lo, hi, _ = solver._box_table(None if solver.sys.stationnary else 0)
    S = int(np.prod(dims))
    lo = np.broadcast_to(np.asarray(lo, dtype=float), (lo.shape[0], S)).T.reshape(dims + (-1,))
    hi = np.broadcast_to(np.asarray(hi, dtype=float), (hi.shape[0], S)).T.reshape(dims + (-1,))
    return lo, hi


def _wave(solver, c, seed):
    """a smooth function of the state with values in [-1, 1], one per control component"""
    rng = np.random.default_rng(1000 * seed + c)
    dims = solver._state_grid_shape
    arg = np.full(dims, rng.uniform(0, 2 * np.pi))
    for k, g in enumerate(solver.state_grid):
        g = np.asarray(g, dtype=float)
        z = (g - g[0]) / (g[-1] - g[0]) if len(g) > 1 else np.zeros(1)
        shape = [1] * len(dims)
        shape[k] = -1
        arg = arg + rng.uniform(1.5, 7.0) * rng.choice([-1, 1]) * z.reshape(shape)
    return np.sin(arg)


def smooth_value(solver):
    """a smooth cost-to-go on the state grid: the 4-byte results are judged against the 8-byte oracle with it (from a
    standard-normal one, the rounding of the next state to 4 bytes moves J by its slope, O(rows) times that rounding)"""
    dims = solver._state_grid_shape
    V = np.zeros(dims)
    for k, g in enumerate(solver.state_grid):
        g = np.asarray(g, dtype=float)
        z = (g - g[0]) / (g[-1] - g[0]) if len(g) > 1 else np.zeros(1)
        shape = [1] * len(dims)
        shape[k] = -1
        V = V + (1.0 + 0.5 * k) * ((z - 0.4) * (z - 0.4)).reshape(shape)
    return V


def special_nodes(dims):
    """index tuples of the nodes that get NaN / +inf / -inf (in this order, cyclically)"""
    n0 = dims[0]
    if len(dims) == 1:
        rows = sorted({0, 1, n0 - 1, n0 // 3} | set(cf.split_rows(n0)))
        return [(i,) for i in rows]
    last = tuple(n - 1 for n in dims[1:])
    cols = [tuple(0 for _ in dims[1:]), last, tuple(n // 3 for n in dims[1:])]
    nodes = []
    for col in cols:
        nodes += [(0,) + col, (n0 - 1,) + col]
    nodes += [(i,) + last for i in range(0, n0, max(1, n0 // 7))]             # the last column, every n0 / 7 rows
    nodes += [(i,) + cols[2] for i in cf.split_rows(n0)]                      # the boundaries of split columns
    return sorted(set(nodes))


def policy(solver, kind, seed=0, V=None):
    """a policy array of shape state_dims + (nu,) (float64; the solver casts it to its own reals)"""
    dims = solver._state_grid_shape
    if kind == 'lattice':
        if V is None:
            V = np.random.default_rng(seed).standard_normal(dims)
        _, pol = solver.value_iteration(np.asarray(V, dtype=solver.dtype).astype(float), report_time=False)
        return np.asarray(pol, dtype=float)
    lo, hi = _box(solver)
    nu = lo.shape[-1]
    pol = np.empty(dims + (nu,))
    for c in range(nu):
        l, h = lo[..., c], hi[..., c]
        if kind == 'random':
            pol[..., c] = l + (h - l) * np.random.default_rng(100 * seed + c).random(dims)
        elif kind in ('smooth', 'special'):
            pol[..., c] = l + (h - l) * (0.5 + 0.45 * _wave(solver, c, seed))
        elif kind == 'outside':
            pol[..., c] = l + (h - l) * (0.5 + 3.5 * _wave(solver, c, seed))
        else:
            raise ValueError(kind)
    if kind == 'special':
        vals = (np.nan, np.inf, -np.inf)
        for n, ind in enumerate(special_nodes(dims)):
            for c in range(nu):
                pol[ind + (c,)] = vals[(n + c) % 3]
    return pol


def family_of(plan):
    """the family or form a plan (DPSolver._kernel_plan) selects"""
    if plan['line']:
        return 'line'
    if plan['lead_axes']:
        return 'lead'
    if plan['staged'] is not None:
        return 'staged'
    if plan['column']:
        if plan['window'] is not None:
            return 'row window'
        if plan['per_control']:
            return 'table per control'
        return 'column'
    return 'generic'


def as_dtype(solver, dtype):
    """the same problem in other reals"""
    s = DPSolver(solver.sys, dtype=dtype)
    s.state_grid, s.perturb_grid = solver.state_grid, solver.perturb_grid
    s.perturb_proba, s.control_steps = solver.perturb_proba, solver.control_steps
    s._state_grid_shape, s._state_ref_ind = solver._state_grid_shape, solver._state_ref_ind
    s.kernel, s.certified_filter = solver.kernel, solver.certified_filter
    if 'LINE_MIN_CELLS' in solver.__dict__:
        s.LINE_MIN_CELLS = solver.LINE_MIN_CELLS
    return s


class Family(object):
    """one unit of the parameter study at its first values: `plans` is what family_of must say, `info` what
    backend_info must say after a run"""

    def __init__(self, name, study, dtype, plans, info):
        self.name, self.study, self.dtype, self.plans, self.info = name, study, np.dtype(dtype), plans, dict(info)

    def __repr__(self):
        return self.name

    def solver(self, kernel=None):
        make, k, _, _ = STUDY[self.study]
        s = make(dict(zip(('g', 'rho', 'k', 'cap'), VALUES[0])))
        s.kernel = k if kernel is None else kernel
        return s if s.dtype == self.dtype else as_dtype(s, self.dtype)


_PLANS = {'column': 'column', 'column fp32': 'column', 'shifted lattice': 'column', 'line': 'line', 'lead': 'lead',
          'row window': 'row window', 'table per control': 'table per control', 'staged': 'staged',
          'generic': 'generic'}
FAMILIES = [Family(name, name, np.float32 if name.endswith('fp32') else np.float64, _PLANS[name], STUDY[name][2])
            for name in sorted(STUDY)]
# 4-byte variants of the families that plan 4-byte reals (the line and lead kernels and the row window are 8-byte only)
# (they claim the kernel: the filter of a family may take another form in 4-byte reals)
FAMILIES += [Family(name + ' fp32', name, np.float32, _PLANS[name], dict(kernel=STUDY[name][2]['kernel']))
             for name in ('shifted lattice', 'table per control', 'staged', 'generic')]
