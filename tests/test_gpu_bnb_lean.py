"""The bookkeeping of the branch and bound of the short first passes (SDP_BNB_LEAN of csrc/sdp_colfilter_kernel.h: the
32-bit block mask, the straight-line `extra` row, the evaluation trips without per-control selects and clamps) on the
device, bit for bit against the same unit with the earlier bookkeeping (SDP_BNB_LEAN=0), the direct kernel
(kernel='generic', which shares none of the table code) and the numpy oracle.

The shapes are the smallest that reach every path of sdp_short_bnb: a stock axis of 12 to 70 rows (one or two waves a
column), 3 x 3 trailing nodes, 4 perturbation points of which 2 are resident -- the resident-chunk form is FORCED by its
planning switch SDP_COL_WRES as in tests/test_gpu_uniform_bound.py, whose model this is (its gain is chosen per case so
that a block of 8 controls spans about 1.0, 2.05 or 4.1 rows of the stock axis: 0, 1 and 3 `extra` rows).  The value
array has kinks along the stock (|sin|): the rows of one column -- the lanes of one wave -- ask for 1, 2, 3 and more
blocks, so that lanes with nothing left sit through the trips of their neighbours.  That this really happens is
asserted from the diagnostic build that stores the number of blocks each node asked for (SDP_DIAG_BNB_COUNT), and
those counts are IDENTICAL with and without the switch: the set of blocks a node asks for does not change."""
import contextlib
import io

import numpy as np
import pytest

import column_forms as cf
import test_gpu_uniform_bound as tub
from stodynprog_amd import DPSolver

N1, N2, N_W, WRES = 3, 3, 4, 2
FORCED = {'SDP_COL_WRES': str(WRES)}
DIAG = {'SDP_EXTRA_DEFINES': 'SDP_DIAG_BNB_COUNT=1'}      # diagnostic build: J := blocks asked for + 100 x the guess's block
SWITCHES = ('SDP_COL_WRES', 'SDP_BNB_UNIFORM', 'SDP_BNB_LEAN', 'SDP_EXTRA_DEFINES')


class Case(object):
    def __init__(self, n0, n_u, block_rows, axis=(0., 1.), noise=0.0, dtype=np.float64, uniform=True, count=False):
        self.n0, self.n_u, self.block_rows, self.axis = n0, n_u, block_rows, axis
        self.noise, self.dtype, self.uniform, self.count = noise, np.dtype(dtype), uniform, count

    @property
    def step(self):
        return 2. / (self.n_u - 1.5)                       # n_u points on [-1, 1] (the step kept off an integer quotient)

    def debug(self, lean=True, diag=False):
        d = dict(FORCED if self.dtype.itemsize == 8 else {})     # (4-byte reals: the whole-table form has the wide pass)
        if not self.uniform:
            d['SDP_BNB_UNIFORM'] = '0'
        if not lean:
            d['SDP_BNB_LEAN'] = '0'
        if diag:
            d.update(DIAG)
        return d

    def solver(self, kernel='auto'):
        lo, hi = self.axis
        # x0' = x0 + b u: a block of 8 controls spans block_rows rows of the stock axis
        reach = self.block_rows / (8 * self.step) * (hi - lo)
        sysd = tub.system(reach * (tub.N0 - 1) / (self.n0 - 1))
        if self.noise:                                     # the perturbation reaches the stock: the shifted lattice
            dyn, noise = sysd.dyn, self.noise
            sysd.dyn = lambda x0, x1, x2, u, w: (dyn(x0, x1, x2, u, w)[0] - noise * w,) + tuple(dyn(x0, x1, x2, u, w)[1:])
        s = DPSolver(sysd, dtype=self.dtype)
        s.discretize_state(lo, hi, self.n0, 0, 1, N1, 0, 1, N2)
        s.discretize_perturb(-0.15, 0.15, N_W)
        s.control_steps = (self.step,)
        s.kernel = kernel
        return s


# control counts 5, 8, 13, 16, 40, 64, 33: one partial block; one whole block; a partial last block; one chunk of the
# bound stage; two chunks, the second with clamped ends; two whole chunks; more than 32 controls and a partial fifth block.
# Axis forms [0, 1], [1, 3] (a power-of-two span off zero) and [0, 3].  The generic bound stage, the shifted lattice and
# 4-byte reals (the wide pass: two blocks a chunk) at whole and partial lattices.
CASES = {
    'u5_rows1': Case(12, 5, 1.0),
    'u8_rows2_axis13': Case(20, 8, 2.05, (1., 3.)),
    'u13_rows2_axis03': Case(24, 13, 2.05, (0., 3.)),
    'u16_rows4': Case(40, 16, 4.1),
    'u40_rows2_axis03': Case(40, 40, 2.05, (0., 3.)),
    'u64_rows2': Case(40, 64, 2.05, count=True),
    'u33_rows4_axis13': Case(70, 33, 4.1, (1., 3.), count=True),
    'u64_rows2_generic_stage': Case(40, 64, 2.05, uniform=False, count=True),
    'u33_rows1_generic_stage_axis03': Case(40, 33, 1.0, (0., 3.), uniform=False),
    'u64_rows2_shifted': Case(40, 64, 2.05, noise=0.02, count=True),
    'u13_rows4_shifted': Case(24, 13, 4.1, noise=0.02),
    'u64_rows2_f32': Case(40, 64, 2.05, dtype=np.float32),
    'u13_rows1_f32': Case(24, 13, 1.0, dtype=np.float32),
}


def _plans(case):
    """(debug dict, kernel) of the three runs of a case, then of its two diagnostic builds"""
    runs = [(case.debug(True), 'auto'), (case.debug(False), 'auto'), (None, 'generic')]
    if case.count:
        runs += [(case.debug(True, True), 'auto'), (case.debug(False, True), 'auto')]
    return runs


def units():
    """the generated sources of this file's problems (__graft_entry__.build compiles them ahead of the run)"""
    out = []
    saved = DPSolver.debug_defines
    try:
        for case in CASES.values():
            for dbg, kernel in _plans(case):
                DPSolver.debug_defines = dbg or None
                out.append(case.solver(kernel)._kernel_plan()['source'])
    finally:
        DPSolver.debug_defines = saved
    return out


def kinked(case, seed=0):
    """|sin| along the stock with another phase in every column, on a small slope across the columns"""
    i, j, k = np.meshgrid(np.arange(case.n0), np.arange(N1), np.arange(N2), indexing='ij')
    V = 0.3 * np.abs(np.sin(0.45 * i + 0.3 + 0.7 * j + 0.4 * k)) + 0.05 * (j - k)
    return (V + 1e-3 * np.random.default_rng(seed).standard_normal(V.shape)).astype(case.dtype)


def special(case):
    """the same with a NaN row, a +inf row and a -inf row of the stock, each in one column"""
    V = kinked(case, 1)
    V[3, 1, 1] = np.nan
    V[case.n0 // 2, 0, 0] = np.inf
    V[case.n0 - 2, 2, 2] = -np.inf
    return V


def _quiet(f, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all='ignore'):
        return f(*a, **kw)


def _run(debug_defines, case, dbg, kernel, V, sweeps):
    debug_defines.unset(*SWITCHES)
    if dbg:
        debug_defines.set(**dbg)
    s = case.solver(kernel)
    try:
        src = s._kernel_plan()['source']
        if kernel == 'auto':
            assert cf.macro(src, 'SDP_COL_BNB') == '1', case.__dict__
            assert cf.macro(src, 'SDP_BNB_LEAN') == ('0' if dbg.get('SDP_BNB_LEAN') == '0' else None)
            assert (cf.macro(src, 'SDP_BNB_UNIFORM') == '1') == (case.uniform and not case.noise and case.dtype.itemsize == 8)
            assert (cf.macro(src, 'SDP_COL_SHIFT') == '1') == bool(case.noise)
            assert (cf.macro(src, 'SDP_COL_WIDE2') == '1') == (case.dtype.itemsize == 4)
        J, pol = _quiet(s.value_iterations, V, sweeps, report_time=False)
        assert s.backend_info['kernel'] == ('column' if kernel == 'auto' else 'generic')
        return J, pol, s.last_policy_index.copy()
    finally:
        tub._close(s)


def _oracle(case, V):
    from oracle import vi_numpy
    nodes = np.arange(V.size)
    with np.errstate(all='ignore'):
        # (8-byte reals: the reference's own path; 4-byte reals: the direct kernel's definition restated in float32)
        Jo, _, io_, _ = vi_numpy.value_iteration(vi_numpy.Spec.from_solver(case.solver()), V, nodes=nodes,
                                                 dtype=None if case.dtype.itemsize == 8 else np.float32)
    return Jo.reshape(V.shape), io_.reshape(V.shape)


pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', sorted(CASES))
def test_the_lean_bookkeeping_keeps_every_bit(gpu, debug_defines, name):
    case = CASES[name]
    for what, V in (('kinked', kinked(case)), ('NaN / inf', special(case))):
        Jo, io_ = _oracle(case, V)
        for sweeps in (1, 2):
            lean, parent, direct = (_run(debug_defines, case, dbg, kernel, V, sweeps) for dbg, kernel in _plans(case)[:3])
            tag = '{} {}, {} sweep(s): '.format(name, what, sweeps)
            tub._same(lean, parent, tag + 'default vs SDP_BNB_LEAN=0')
            tub._same(lean, direct, tag + 'default vs the direct kernel')
            if sweeps == 1:
                # (the planted values reach some nodes of every column through the trailing axes, and leave others alone)
                assert np.isfinite(lean[0]).any() and np.isnan(lean[0]).any() == (what != 'kinked')
                assert np.array_equal(lean[0], Jo, equal_nan=True), tag + 'J differs from the oracle'
                assert np.array_equal(lean[2], io_), tag + 'policy index differs from the oracle'


@pytest.mark.parametrize('name', sorted(n for n, c in CASES.items() if c.count))
def test_every_node_asks_for_the_same_blocks(gpu, debug_defines, name):
    """J of the diagnostic builds = blocks asked for + 100 x the block of the guess, -1 where a wave took the full pass"""
    case = CASES[name]
    V = kinked(case)
    lean, parent = (_run(debug_defines, case, dbg, kernel, V, 1)[0] for dbg, kernel in _plans(case)[3:])
    assert np.array_equal(lean, parent), name + ': the nodes ask for other blocks'
    cnt = np.round(lean).astype(int)
    assert (cnt >= 0).all(), name + ': a wave took the full first pass'
    need = cnt % 100
    n_blocks = (case.n_u + 7) // 8
    print(name, 'blocks asked for:', np.bincount(need.ravel(), minlength=n_blocks + 1))
    assert need.min() >= 1 and need.max() <= n_blocks
    # lanes of one wave -- the rows of a column -- with 1, 2 and 3 blocks: some sit out trips their neighbours run
    assert {1, 2, 3} <= set(need.ravel().tolist()), np.bincount(need.ravel())
    assert any(len(set(need[:64, j, k].tolist())) >= 3 for j in range(N1) for k in range(N2))
