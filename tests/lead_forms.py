"""The forms of the reduced-array sweep (csrc/sdp_lead_kernel.h) as a table of cases (test infrastructure, like
tests/column_forms.py and tests/line_forms.py; not a test file, and no GPU code).

The lead family is the only fast family that re-indexes the whole grid: m controlled stocks next to an exogenous
process, values stored plane-major, every node split into a lead index and a trailing index, on a permuted view of
the axes where the stocks are not listed first, with a second pass that reads the plane-major copy through strides of
its own.  The planner (DPSolver._kernel_plan_now with codegen.lead_filter_applies / lead_order) gives it m from 1 to d,
with or without an exogenous axis, in any listing order.  Each case below is one such form with the plan it claims:
`lead_axes` (SDP_LEAD_AXES), `lead_perm` (the state variables, stocks first; None where they are listed first, and
SDP_LEAD_PERM is then not defined) and `cost_w` (SDP_LEAD_COST_HAS_W).

Every case has 8-byte reals and NormalLaw(0, 0.2) discretised on (-0.5, 0.5, W).  The grids are the smallest at which
the form can still go wrong: every axis of a case has a different number of points (swapped strides change the
results), no plane holds a multiple of 64 nodes (a wave straddles planes), some axis has 3 points (not all in one
case), and the span of one stock is a power of two (2.0) where that of another is not (3.0), so that the per-axis pow2
bit of SdpLeadGeom is mixed.  `phased_permuted` is the one large case: exactly 8 MiB of float64, the size from which
value_iteration runs the backup in four phases of the node range.

The baseline rows (`listed_first`, `stock_last`, `stock_middle`) are the models of tests/test_gpu_lead.py on small
grids and, for the first, with this table's law: their generated sources are those of that file's own solvers
(tests/test_lead_forms_plan.py holds them equal), so a change to the kernel is run against the forms that were
covered before as well as against the new ones.  `flat_permuted` is the flat objective of
test_near_ties_and_a_radius_far_too_small listed as (y, a, b), on 5 x 11 x 9 nodes.

One constant was changed to meet the conditions tests/test_lead_forms_plan.py puts on the oracle's policies (at least 5
distinct policy indices on the smooth and on the random input, at most half of the nodes at index 0): the control step
of `phased_permuted` is 0.125, not 0.5 -- a lattice of 9 points per node where one of 3 cannot hold 5 distinct indices.
Every other model is as first written; the `smooth` input of `inputs` is steep enough (the factor 4) for the linear
cost of `flat_permuted` not to push every node to the same corner of its box.

tests/test_lead_forms_plan.py checks on the CPU that every case plans what it claims, that the index maps restated
here (`Geom`) are consistent, and that the oracle alone meets the conditions the GPU tests rely on;
tests/test_gpu_lead_forms.py runs every case on the GPU against the numpy oracle and the direct kernel, bit for bit."""
import re

import numpy as np

from stodynprog_amd import SysDescription, DPSolver, models
from stodynprog_amd.models import NormalLaw


class Case(object):
    """name; make() -> (sysd, solver); the plan it claims: lead_axes, lead_perm (None: stocks listed first), cost_w
    (SDP_LEAD_COST_HAS_W); `sampled`: None, or the number of nodes the oracle is run on (the large case)"""

    def __init__(self, name, make, lead_axes, lead_perm=None, cost_w=False, sampled=None):
        self.name, self.make, self.lead_axes = name, make, int(lead_axes)
        self.lead_perm = None if lead_perm is None else tuple(lead_perm)
        self.cost_w, self.sampled = bool(cost_w), sampled

    def __repr__(self):
        return self.name

    def solver(self, kernel='auto', dtype=None):
        _, s = self.make()
        s.kernel = kernel
        if dtype is not None:
            s.dtype = np.dtype(dtype)
        return s

    @property
    def permuted(self):
        return self.lead_perm is not None

    def perm_define(self):
        """the `#define SDP_LEAD_PERM {..}` line the unit must hold, or None"""
        if self.lead_perm is None:
            return None
        full = self.lead_perm + tuple(range(len(self.lead_perm), 4))
        return '#define SDP_LEAD_PERM {' + ', '.join(str(k) for k in full) + '}'

    def sample_nodes(self, shape):
        """flat C-order node ids the oracle is run on: all of them, or `sampled` seeded ones with the first and the
        last node and both sides of the three boundaries between the four phases of the node range"""
        S = int(np.prod(shape))
        if self.sampled is None:
            return np.arange(S)
        picked = set(np.random.default_rng(S).choice(S, size=self.sampled - 8, replace=False).tolist())
        picked.update((0, S - 1))
        for ph in (1, 2, 3):
            picked.update((S * ph // 4 - 1, S * ph // 4))
        extra = iter(np.random.default_rng(S + 1).permutation(S).tolist())
        while len(picked) < self.sampled:
            picked.add(next(extra))
        return np.array(sorted(picked), dtype=np.int64)


def _finish(sysd, state, W, steps):
    sysd.perturb_laws = [NormalLaw(0, 0.2)]
    s = DPSolver(sysd)
    s.discretize_state(*state)
    s.discretize_perturb(-0.5, 0.5, W)
    s.control_steps = tuple(steps)
    return sysd, s


_UNIT_BOX2 = ((0., 1.), (0., 1.))


def _all_stocks():
    """m = d = 2: no exogenous axis, only the cost sees w (the #else branches of sdp_lead_reduce)"""
    sysd = SysDescription((2, 2, 1), name='all stocks')
    sysd.dyn = lambda a, b, u, v, w: (a + 0.5 * u - 0.1 * b, b + u - v)
    sysd.cost = lambda a, b, u, v, w: (v - 0.5 - w) * (v - 0.5 - w) + 0.1 * u * u + 0.2 * (a - 1.0) * (a - 1.0)
    sysd.control_box = lambda a, b: _UNIT_BOX2
    return _finish(sysd, (0, 2, 9, 0, 3, 7), 5, (0.25, 0.25))


def all_stocks_deterministic():
    """`all_stocks` with the perturbation also removed from the cost: W = 0, which is not this family"""
    sysd = SysDescription((2, 2, 0), name='all stocks, deterministic')
    sysd.dyn = lambda a, b, u, v: (a + 0.5 * u - 0.1 * b, b + u - v)
    sysd.cost = lambda a, b, u, v: (v - 0.5) * (v - 0.5) + 0.1 * u * u + 0.2 * (a - 1.0) * (a - 1.0)
    sysd.control_box = lambda a, b: _UNIT_BOX2
    s = DPSolver(sysd)
    s.discretize_state(0, 2, 9, 0, 3, 7)
    s.control_steps = (0.25, 0.25)
    return sysd, s


def _three_stocks():
    """m = 3, d = 4: SdpLeadLerp three levels deep, pm[] and lm[] of three axes"""
    sysd = SysDescription((4, 2, 1), name='three stocks')
    sysd.dyn = lambda a, b, c, y, u, v, w: (a + 0.5 * y - u, b + u - v, c + 0.3 * v - 0.1 * a, 0.7 * y + w)
    sysd.cost = lambda a, b, c, y, u, v, w: ((v - 0.5) * (v - 0.5) + 0.1 * u * u + 0.2 * (c - 1.0) * (c - 1.0)
                                             + 0.05 * a * b)
    sysd.control_box = lambda a, b, c, y: _UNIT_BOX2
    return _finish(sysd, (0, 2, 5, 0, 3, 4, 0, 4, 6, -1, 1, 3), 3, (0.5, 0.5))


def _exo_first():
    """m = 2 permuted, (y, a, b): two stocks on the permuted view, grid.M[SDP_LP[k]] in the second pass"""
    sysd = SysDescription((3, 2, 1), name='exogenous first')
    sysd.dyn = lambda y, a, b, u, v, w: (0.7 * y + w, a + 0.5 * y - u, b + u - v)
    sysd.cost = lambda y, a, b, u, v, w: (v - 0.5) * (v - 0.5) + 0.1 * u * u + 0.2 * (a - 1.0) * (a - 1.0)
    sysd.control_box = lambda y, a, b: _UNIT_BOX2
    return _finish(sysd, (-1, 1, 4, 0, 2, 6, 0, 3, 5), 3, (0.5, 0.5))


def _exo_middle():
    """the model of `exo_first` listed as (a, y, b): a stock on either side of the exogenous axis"""
    sysd = SysDescription((3, 2, 1), name='exogenous in the middle')
    sysd.dyn = lambda a, y, b, u, v, w: (a + 0.5 * y - u, 0.7 * y + w, b + u - v)
    sysd.cost = lambda a, y, b, u, v, w: (v - 0.5) * (v - 0.5) + 0.1 * u * u + 0.2 * (a - 1.0) * (a - 1.0)
    sysd.control_box = lambda a, y, b: _UNIT_BOX2
    return _finish(sysd, (0, 2, 6, -1, 1, 4, 0, 3, 5), 3, (0.5, 0.5))


def _interleaved():
    """m = 2, d = 4, (y, a, z, b): two trailing axes, interleaved with the stocks (tm[], sdp_lead_trail_grid)"""
    sysd = SysDescription((4, 2, 1), name='interleaved')
    sysd.dyn = lambda y, a, z, b, u, v, w: (0.7 * y + w, a + 0.5 * y - u, 0.5 * z - 0.3 * w + 0.1 * y, b + u - v)
    sysd.cost = lambda y, a, z, b, u, v, w: ((v - 0.5 - 0.2 * z) * (v - 0.5 - 0.2 * z) + 0.1 * u * u
                                             + 0.2 * (a - 1.0) * (a - 1.0))
    sysd.control_box = lambda y, a, z, b: _UNIT_BOX2
    return _finish(sysd, (-1, 1, 3, 0, 2, 5, -1, 1, 4, 0, 3, 6), 3, (0.5, 0.5))


def _three_controls():
    """three controls on a per-node box, permuted, a cost that sees w: sdp_lead_walk_next carries over three digits,
    and the second control has ONE lattice point where b = 0"""
    sysd = SysDescription((3, 3, 1), name='three controls')
    sysd.dyn = lambda y, a, b, u, r, v, w: (0.7 * y + w, a + 0.5 * y - u + 0.25 * r, b + u - v)
    sysd.cost = lambda y, a, b, u, r, v, w: (((v - 0.5 - w) * (v - 0.5 - w) + 0.1 * u * u)
                                             + (0.2 * (a - 1.0) * (a - 1.0) + 0.3 * r * b))
    sysd.control_box = lambda y, a, b: ((0., 1.), (0., 0.5 * b), (-0.5, 0.5 + 0.25 * a))
    return _finish(sysd, (-1, 1, 4, 0, 2, 6, 0, 3, 5), 3, (0.5, 0.25, 0.5))


def _listed_first():
    """the form of tests/test_gpu_lead.py::_small (m = 2, d = 3, stocks listed first) on 7 x 6 x 5 nodes, the second
    stock on [0, 3]"""
    sysd, s = models.two_reservoirs(n_a=7, n_b=6, n_y=5, n_w=5, steps=(0.25, 0.25))
    s.discretize_state(0., 2., 7, 0., 3., 6, -0.2, 0.8, 5)
    sysd.perturb_laws = [NormalLaw(0, 0.2)]
    s.discretize_perturb(-0.5, 0.5, 5)
    return sysd, s


def _stock_last():
    """tests/test_gpu_lead.py::_stock_not_first(False): m = 1, (a, y) with the stock listed last, 9 x 40 nodes"""
    sysd = SysDescription((2, 1, 1), name='stock listed last')
    sysd.dyn = lambda a, y, u, w: (0.8 * a + w, y + 0.7 * u)
    sysd.cost = lambda a, y, u, w: (a - 0.3) * u + 0.2 * u * u + 0.05 * y
    sysd.control_box = lambda a, y: ((-1.0, 1.0),)
    return _finish(sysd, (-1, 1, 9, 0, 3, 40), 7, (0.0625,))


def _stock_middle():
    """tests/test_gpu_lead.py::_stock_not_first(True): m = 1, (a, y, b) with the stock in the middle and a per-node
    box, on 5 x 13 x 3 nodes"""
    sysd = SysDescription((3, 1, 1), name='stock in the middle')
    sysd.dyn = lambda a, y, b, u, w: (0.8 * a + w, y + 0.7 * u, 0.5 * b - 0.3 * w + 0.1 * a)
    sysd.cost = lambda a, y, b, u, w: (a - 0.3) * u + 0.2 * u * u + 0.05 * y + 0.1 * b * b
    sysd.control_box = lambda a, y, b: ((-1.0, 1.0 + 0.2 * a * a),)
    return _finish(sysd, (-1, 1, 5, 0, 3, 13, -1, 1, 3), 7, (0.0625,))


def _flat_permuted():
    """the flat objective of tests/test_gpu_lead.py::test_near_ties_and_a_radius_far_too_small listed as (y, a, b):
    V linear in both stocks (`flat_input`), the cost cancels its slope, the argmin hangs on the last bits"""
    sysd = SysDescription((3, 2, 1), name='flat, permuted')
    sysd.dyn = lambda y, a, b, u, v, w: (0.8 * y + w, a + 0.37 * u, b + 0.29 * v)
    sysd.cost = lambda y, a, b, u, v, w: (-1.3 * 0.37) * u + (-0.7 * 0.29) * v
    sysd.control_box = lambda y, a, b: ((-1., 1.), (-1., 1.))
    return _finish(sysd, (-1, 1, 5, 0, 3, 11, 0, 3, 9), 7, (2.0 / 11, 2.0 / 9))


def flat_input(s):
    """the cost-to-go whose slopes the cost of `flat_permuted` cancels"""
    y, a, b = [np.asarray(g) for g in s.state_grid]
    return 1.3 * a[None, :, None] + 0.7 * b[None, None, :] + np.cos(3 * y)[:, None, None]


def _phased_permuted():
    """64 x 128 x 128 nodes, exactly 8 MiB of float64, (y, a, b): value_iteration runs the backup in four phases of
    the node range, each of which walks every plane-major position and drops the nodes outside its range"""
    sysd = SysDescription((3, 1, 1), name='phased, permuted')
    sysd.dyn = lambda y, a, b, u, w: (0.7 * y + w, a + 0.5 * y - u, b + 0.5 * u - 0.1 * a)
    sysd.cost = lambda y, a, b, u, w: (u - 0.5) * (u - 0.5) + 0.2 * (a - 1.0) * (a - 1.0) + 0.1 * b * y
    sysd.control_box = lambda y, a, b: ((0., 1.),)
    return _finish(sysd, (-1, 1, 64, 0, 2, 128, 0, 3, 128), 3, (0.125,))


CASES = [
    Case('all_stocks', _all_stocks, 2, None, cost_w=True),
    Case('three_stocks', _three_stocks, 3, None),
    Case('exo_first', _exo_first, 2, (1, 2, 0)),
    Case('exo_middle', _exo_middle, 2, (0, 2, 1)),
    Case('interleaved', _interleaved, 2, (1, 3, 0, 2)),
    Case('three_controls', _three_controls, 2, (1, 2, 0), cost_w=True),
    Case('listed_first', _listed_first, 2, None),
    Case('stock_last', _stock_last, 1, (1, 0)),
    Case('stock_middle', _stock_middle, 1, (1, 0, 2)),
    Case('flat_permuted', _flat_permuted, 2, (1, 2, 0)),
    Case('phased_permuted', _phased_permuted, 2, (1, 2, 0), sampled=2000),
]
BY_NAME = {c.name: c for c in CASES}
SMALL = [c for c in CASES if c.sampled is None]
NEW_FORMS = ('all_stocks', 'three_stocks', 'exo_first', 'exo_middle', 'interleaved', 'three_controls')
INPUTS = ('zeros', 'smooth', 'random', 'non-finite')
WIDE = {'SDP_LEAD_FILTER_SCALE': '1e12'}         # every node takes the long way: the second pass alone


def macro(source, name):
    """value of `#define name value` in a generated source (the rest of the line), or None"""
    m = re.search(r'^#define {} (.+)$'.format(re.escape(name)), source, re.M)
    return m.group(1).strip() if m else None


def ref_index(shape):
    """the relative-DP reference node (reference stodynprog.py:384): the middle of every axis"""
    return tuple(n // 2 for n in shape)


def inputs(shape):
    """four cost-to-go arrays: zeros, smooth, seeded random, and one with NaN and +-inf entries, none of them at the
    relative-DP reference node (the pattern of tests/multi_perturb.py)"""
    shape = tuple(int(n) for n in shape)
    S = int(np.prod(shape))
    axes = np.meshgrid(*[np.linspace(0., 1., n) for n in shape], indexing='ij')
    smooth = np.zeros(shape)
    for k, x in enumerate(axes):                     # (a bowl off the centre, tilted differently along every axis)
        smooth = smooth + (2.0 + k) * (x - 0.3 - 0.1 * k) ** 2 + 0.2 * np.sin((3 + k) * x)
    smooth = 4.0 * (smooth + 0.5 * axes[0] * axes[-1])
    rng = np.random.default_rng(40 + len(shape))
    rand = rng.standard_normal(shape)
    bad = rng.standard_normal(shape)
    flat = bad.reshape(-1)
    ref = int(np.ravel_multi_index(ref_index(shape), shape))
    spots = []
    for p in (1, S // 3, S - 1):
        while p == ref or p in spots:
            p = (p + 1) % S
        spots.append(p)
    flat[spots[0]], flat[spots[1]], flat[spots[2]] = np.nan, np.inf, -np.inf
    return {'zeros': np.zeros(shape), 'smooth': smooth, 'random': rand, 'non-finite': bad}


def unit_sources(case):
    """{what: generated source} of every unit tests/test_gpu_lead_forms.py runs for the case"""
    out = {'lead': case.solver()._kernel_plan()['source'], 'generic': case.solver('generic')._kernel_plan()['source']}
    for what, debug in RADIUS_RUNS.get(case.name, {}).items():
        s = case.solver()
        s.debug_defines = dict(debug)
        out[what] = s._kernel_plan()['source']
    return out


# the radius runs of tests/test_gpu_lead_forms.py: {case: {what: debug defines}}
RADIUS_RUNS = {
    'all_stocks': {'wide': WIDE}, 'three_stocks': {'wide': WIDE}, 'interleaved': {'wide': WIDE},
    'flat_permuted': {'half': {'SDP_LEAD_FILTER_SCALE': '0.5'}, 'far too small': {'SDP_LEAD_FILTER_SCALE': '1e-6'}},
}


# ---------------------------------------------------------------------------------------------------------------------
# The kernel's index maps, restated from the comments and the formulas of SdpLeadGeom (csrc/sdp_lead_kernel.h):
#   logical axis j of the kernel -- stocks first, then the exogenous process -- is state variable perm[j];
#   phys[p]  node-order (C-order) stride of state variable p;   ord[j] = orders[perm[j]],  nstr[j] = phys[perm[j]];
#   tm[k]    stride of trailing axis m + k inside the trailing index (the last one fastest), ts = their product;
#   pm[k]    stride of lead axis k inside a plane (the last stock fastest), ls = their product;
#   a node with index i_j along logical axis j has  lead = sum_{j < m} i_j pm[j],  trail = sum_{j >= m} i_j tm[j - m],
#   and sits at plane-major position  trail * ls + lead;
#   the second pass reads the plane-major copy in the REFERENCE's axis order with strides per state variable:
#   M[perm[k]] = pm[k] for a stock, ls * tm[k - m] for an exogenous variable.
# ---------------------------------------------------------------------------------------------------------------------
class Geom(object):
    def __init__(self, orders, lead_axes, perm=None):
        self.orders = tuple(int(n) for n in orders)
        d = self.d = len(self.orders)
        m = self.m = int(lead_axes)
        self.perm = tuple(range(d)) if perm is None else tuple(int(p) for p in perm)
        assert sorted(self.perm) == list(range(d)) and 1 <= m <= d
        phys = [1] * d
        for p in range(d - 2, -1, -1):
            phys[p] = phys[p + 1] * self.orders[p + 1]
        self.phys = tuple(phys)
        self.ord = tuple(self.orders[p] for p in self.perm)
        self.nstr = tuple(phys[p] for p in self.perm)
        tm, acc = [0] * (d - m), 1
        for k in range(d - 1, m - 1, -1):
            tm[k - m] = acc
            acc *= self.ord[k]
        self.tm, self.ts = tuple(tm), acc
        pm, acc = [0] * m, 1
        for k in range(m - 1, -1, -1):
            pm[k] = acc
            acc *= self.ord[k]
        self.pm, self.ls = tuple(pm), acc
        self.S = self.ts * self.ls
        M = [0] * d
        for k in range(m):
            M[self.perm[k]] = self.pm[k]
        for k in range(m, d):
            M[self.perm[k]] = self.ls * self.tm[k - m]
        self.M = tuple(M)

    def digits(self, node):
        """index of `node` along every LOGICAL axis"""
        node = np.asarray(node, dtype=np.int64)
        return [(node // self.nstr[j]) % self.ord[j] for j in range(self.d)]

    def split(self, node):
        i = self.digits(node)
        lead = sum(i[j] * self.pm[j] for j in range(self.m))
        trail = sum((i[j] * self.tm[j - self.m] for j in range(self.m, self.d)), np.zeros_like(lead))
        return lead, trail

    def join(self, lead, trail):
        lead, trail = np.asarray(lead, dtype=np.int64), np.asarray(trail, dtype=np.int64)
        node = np.zeros(np.broadcast(lead, trail).shape, dtype=np.int64)
        for j in range(self.m - 1, -1, -1):
            node = node + (lead % self.ord[j]) * self.nstr[j]
            lead = lead // self.ord[j]
        for j in range(self.d - 1, self.m - 1, -1):
            node = node + (trail % self.ord[j]) * self.nstr[j]
            trail = trail // self.ord[j]
        return node

    def base(self, lead):
        lead = np.asarray(lead, dtype=np.int64)
        out = np.zeros(lead.shape, dtype=np.int64)
        for j in range(self.m - 1, -1, -1):
            out = out + (lead % self.ord[j]) * self.nstr[j]
            lead = lead // self.ord[j]
        return out

    def position(self, node):
        lead, trail = self.split(node)
        return trail * self.ls + lead

    def highest_corner(self):
        """sum(off) + sum(pm) of the highest cell of the lead lattice: q_k = ord_k - 2 on every stock axis"""
        return sum((self.ord[k] - 2) * self.pm[k] for k in range(self.m)) + sum(self.pm)


def geom_of(case, shape):
    return Geom(shape, case.lead_axes, case.lead_perm)
