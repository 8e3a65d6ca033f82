"""The forms of the LDS-staged tile kernel (csrc/sdp_staged_kernel.h) as a table of cases (test infrastructure, like
tests/column_forms.py, tests/line_forms.py and tests/lead_forms.py; not a test file, and no GPU code).

The staged kernel is the family of any traceable model that no fast family takes.  It is compiled per
(SDP_STG_CU, SDP_STG_CW): a tile of 512 nodes walks its (control x perturbation) lattice in chunks of CU controls
(unrolled) x CW perturbation points, with one box prediction, one staging copy and one gather per chunk.
codegen.staged_config picks the pair from the reach of the dynamics: `cu` in 4, 2, 1 and `cw` in W >> s.  Every model
the suite ran before this table plans (4, W): one box per control chunk, so that the carry of acc[] and outside[] from
one box to the next, the flip of `parity` inside a control chunk, a ragged last w chunk and the units with cu = 2 and
cu = 1 were never run.  Each case below is a model on a grid large enough, with a reach wide enough, to plan another
pair, with the plan it claims per real type (`plans`: {itemsize: (cu, cw)}; the tile is that of its number of state
variables, the budget 76 KiB unless the case states its own), the staging paths it claims per type (`paths`) and
what its chunks are like (`claims`):

  'boxes'      W > cw: several boxes per control chunk (acc[] carried, parity flips)
  'ragged_w'   W % cw != 0: the last w chunk is cut by w1 = min(w0 + CW, Wn)
  'ragged_u'   n_ctrl % cu != 0 and n_ctrl > cu: the last control chunk runs clamped controls
  'early'      cells miss their box in a w chunk that is not the last while those of the last chunk do not:
               outside[] carried across boxes
  'uneven'     the nodes of one tile have different control counts (a per-node box)

The staging paths of a (tile, chunk) pair, in the kernel's order: 'fit' (the box is staged whole), 'cut0' (cut on the
leading axes only, axis 0 first), 'cutlast' (cut down to the last axis, rows shortened), 'none' (fewer than 3
vertices of a row fit: nothing is staged, every cell reads global memory).

All models have state axes on [0, 1], control boxes inside (-0.5, 0.5), NormalLaw(0, 0.5) discretised on (-1, 1, W).
Axes of a case have different lengths, most are no multiple of their tile edge, and `budget_512` / `budget_32` have an
axis shorter than it.  The first ten rows are the models the planner was first measured on, with the plans found then.
One thing was changed in them: the cost's `(x0 - 0.4) ** 2` is written as a product.  A power of a sub-expression that
depends on the state alone is a numpy SCALAR power in the reference's node-by-node evaluation (libm pow, one ulp off the
correctly rounded square now and then; trace._power flags it `scalar_pow`), and the oracle is compared bit for bit.  The
plans do not see the cost.  The staging paths 'cutlast' in more than one state variable and 'none' need a row of more
than 4864 vertices, or a budget below 3 * 2^(d-1) reals: no natural shape of this size, so two cases state a budget of
their own (the hook tests/test_gpu_staged.py uses); 'cutlast' at the natural budget is reached with one state variable.

`Reach` restates steps 1 and 2 of the kernel in numpy for a planned case: the corner cells of every live lane, the
box, its cut, and per lattice cell whether it is inside.  It is a check on the table, not an oracle for the device:
the device may evaluate a traced model with a contraction numpy does not make, in 4 bytes it rounds where numpy here
does not, and a guessed cell may differ by one -- so tests/test_staged_forms_plan.py asks for every claimed path at
least 16 (tile, chunk) pairs and for early misses at least 64 (control, node) pairs that miss early ONLY.

What `Reach` finds per run (T: real type; (tile, chunk) pairs per path; lattice cells that miss their box; (control,
node) pairs with a miss; those that miss early only), as measured when the table was written:

  case              T  grid         W    controls plan    fit cut0 cutlast  none   cells   pairs   early
  one_box           f8 100x120        7       11  (4,7)    76    8       0     0     512     512       0
  one_box           f4 100x120        7       11  (4,7)    84    0       0     0       0       0       0
  two_w_chunks      f8 100x120        8       11  (4,4)   168    0       0     0       0       0       0
  two_w_chunks      f4 100x120        8       11  (4,8)    84    0       0     0       0       0       0
  ragged_w_3d       f8 24x22x26       7       11  (4,3)   324    0       0     0       0       0       0
  ragged_w_3d       f4 24x22x26       7       11  (4,7)   108    0       0     0       0       0       0
  cu2               f8 300x120        8       5   (2,4)   456    0       0     0       0       0       0
  cu2               f4 300x120        8       5   (4,4)   294   10       0     0    8448    2112       0
  cu2_w6            f8 600x40         6       3   (2,3)   281   23       0     0   33792   11264       0
  cu2_w6            f4 600x40         6       3   (4,3)   138   14       0     0   20928    6976       0
  cu2_3d            f8 40x22x26       8       11  (2,8)   292   68       0     0    6488    4584       0
  cu2_3d            f4 40x22x26       8       11  (4,8)   180    0       0     0       0       0       0
  four_w_chunks_3d  f8 40x22x26       8       5   (4,2)   449   31       0     0   20376    5496    3216
  four_w_chunks_3d  f4 40x22x26       8       5   (4,8)   120    0       0     0       0       0       0
  cu1               f8 400x120        8       3   (1,8)   300    0       0     0       0       0       0
  cu1               f4 400x120        8       3   (4,2)   393    7       0     0    4928    1056     352
  cu2_in_4_bytes    f8 300x120        8       5   (2,4)   398   58       0     0  105312   26328   11864
  cu2_in_4_bytes    f4 300x120        8       5   (2,8)   210   18       0     0   25344    3168       0
  eight_boxes       f8 400x160        8       3   (4,1)   840  160       0     0   79136   51424   51424
  eight_boxes       f4 400x160        8       3   (4,1)  1000    0       0     0       0       0       0
  line_16001        f8 16001          8       11  (4,4)   159    0      33     0   47067   47067   47067
  four_axes         f8 10x9x11x12     6       5   (2,3)   278   46       0     0   12292    4376    1720
  deterministic_cu2 f8 300x120        0       5   (2,1)   228    0       0     0       0       0       0
  two_controls      f8 300x120        8       9   (2,8)   322   58       0     0  206464   25808       0
  uneven_box        f8 300x120        8       9   (4,4)   256   42       0     0   10472    2618     568
  folded            f8 300x120        8       11  (4,2)   912    0       0     0   16560    6840    5400
  budget_512        f8 12x1001        7       11  (1,1)   638  352    1474     0  586104  129614   54286
  budget_32         f8 12x1001        7       11  (1,1)     0    0       0  2464  924924  132132       0
  budget_32         f4 12x1001        7       11  (1,1)     0  638    1826     0  867626  132132       0

tests/test_staged_forms_plan.py checks on the CPU that every case plans what it claims, that `Reach` finds the paths
it claims, and that the oracle alone meets the conditions the GPU tests rely on; tests/test_gpu_staged_forms.py runs
every case on the GPU against the numpy oracle and the direct kernel, bit for bit."""
import contextlib
import functools

import numpy as np

from stodynprog_amd import SysDescription, DPSolver, codegen
from stodynprog_amd.models import NormalLaw

TILES = {1: (512,), 2: (16, 32), 3: (8, 8, 8), 4: (4, 4, 4, 8)}
BUDGET = 76 * 1024                   # bytes of LDS for the box (codegen.STAGED_LDS_BYTES)
PATHS = ('fit', 'cut0', 'cutlast', 'none')
CLAIMS = ('boxes', 'ragged_w', 'ragged_u', 'early', 'uneven')
REALS = {8: np.float64, 4: np.float32}


class Case(object):
    """name; make() -> (sysd, solver); plans {itemsize: (cu, cw)}; paths {itemsize: paths claimed}; claims
    {itemsize: what its chunks are like}; `budget`: None, or the LDS budget in bytes the case needs
    (codegen.STAGED_LDS_BYTES for the duration of its plans and runs); `sampled`: the number of oracle nodes"""

    def __init__(self, name, make, plans, paths, claims=None, budget=None, sampled=400):
        self.name, self.make, self.budget, self.sampled = name, make, budget, int(sampled)
        self.plans = {int(rs): (int(cu), int(cw)) for rs, (cu, cw) in plans.items()}
        self.paths = {int(rs): tuple(p) for rs, p in paths.items()}
        self.claims = {int(rs): frozenset(c) for rs, c in (claims or {}).items()}
        assert set(self.paths) == set(self.plans) and set(self.claims) <= set(self.plans)
        assert all(set(p) <= set(PATHS) for p in self.paths.values())
        assert all(c <= set(CLAIMS) for c in self.claims.values())

    def __repr__(self):
        return self.name

    @property
    def sizes(self):
        return sorted(self.plans, reverse=True)

    def claimed(self, rs):
        return self.claims.get(rs, frozenset())

    def solver(self, rs=8, kernel='staged'):
        _, s = self.make()
        s.kernel = kernel
        s.dtype = np.dtype(REALS[rs])
        return s

    def plan(self, rs, d):
        """what _kernel_plan()['staged'] must equal"""
        cu, cw = self.plans[rs]
        return dict(threads=512, tile=TILES[d], cu=cu, cw=cw, cap=(self.budget or BUDGET) // rs)

    @contextlib.contextmanager
    def budgeted(self):
        """the case's LDS budget for the duration of a plan made outside a test (the tests use monkeypatch)"""
        saved = codegen.STAGED_LDS_BYTES
        if self.budget is not None:
            codegen.STAGED_LDS_BYTES = self.budget
        try:
            yield self
        finally:
            codegen.STAGED_LDS_BYTES = saved


def _finish(sysd, state, W, steps):
    if W:
        sysd.perturb_laws = [NormalLaw(0, 0.5)]
    s = DPSolver(sysd)
    s.discretize_state(*state)
    if W:
        s.discretize_perturb(-1, 1, W)
    s.control_steps = tuple(steps)
    return sysd, s


_BOX1 = ((-0.5, 0.5),)


def m2(n0, n1, W, a, b, c, e, du):
    """two state variables, one control: x0 moved by the control and the perturbation, x1 by the perturbation"""
    def make():
        sysd = SysDescription((2, 1, 1), name='m2')
        sysd.dyn = lambda x0, x1, u, w: (x0 + a * u + b * w, 0.9 * x1 + c * w + e * u)
        sysd.cost = lambda x0, x1, u, w: (x0 - 0.4) * (x0 - 0.4) + 0.3 * (u - x1) ** 2 + w * u
        sysd.control_box = lambda x0, x1: _BOX1
        return _finish(sysd, (0, 1, n0, 0, 1, n1), W, (du,))
    return make


def m3(shape, W, a, b, c, du):
    """three state variables, the last one moved by w * (1 + u)"""
    def make():
        sysd = SysDescription((3, 1, 1), name='m3')
        sysd.dyn = lambda x0, x1, x2, u, w: (x0 + a * u + 0.1 * x1 * w, 0.8 * x1 + b * w + 0.05 * x2,
                                             0.7 * x2 + c * w * (1 + u) + 0.1 * x0)
        sysd.cost = lambda x0, x1, x2, u, w: (x0 - 0.4) * (x0 - 0.4) + 0.3 * (u - x1) ** 2 + w * u * x2
        sysd.control_box = lambda x0, x1, x2: _BOX1
        n0, n1, n2 = shape
        return _finish(sysd, (0, 1, n0, 0, 1, n1, 0, 1, n2), W, (du,))
    return make


def m1(n, W, a, b, g, du):
    """one state variable: the perturbation's reach grows with x (b * w * (1 + g * x)), so that the boxes of the
    tiles at the high end are the ones beyond the budget"""
    def make():
        sysd = SysDescription((1, 1, 1), name='m1')
        sysd.dyn = lambda x, u, w: (x + a * u + b * w * (1 + g * x),)
        sysd.cost = lambda x, u, w: (x - 0.4) * (x - 0.4) + 0.3 * (u - 0.2) ** 2 + w * u * x
        sysd.control_box = lambda x: _BOX1
        return _finish(sysd, (0, 1, n), W, (du,))
    return make


def m4(shape, W, a, b, c, e, du):
    """four state variables"""
    def make():
        sysd = SysDescription((4, 1, 1), name='m4')
        sysd.dyn = lambda x0, x1, x2, x3, u, w: (x0 + a * u + 0.1 * x1 * w, 0.8 * x1 + b * w + 0.05 * x2,
                                                 0.7 * x2 + c * w * (1 + u) + 0.1 * x0, 0.9 * x3 + e * w + 0.05 * x1)
        sysd.cost = lambda x0, x1, x2, x3, u, w: (x0 - 0.4) * (x0 - 0.4) + 0.3 * (u - x1) ** 2 + w * u * x2 + 0.2 * x3 * x3
        sysd.control_box = lambda x0, x1, x2, x3: _BOX1
        return _finish(sysd, sum(((0, 1, n) for n in shape), ()), W, (du,))
    return make


def m2_deterministic(n0, n1, a, e, du):
    """`m2` without a perturbation: W = 0, Wn = 1, the `acc[j] = jc` branch"""
    def make():
        sysd = SysDescription((2, 1, 0), name='m2, deterministic')
        sysd.dyn = lambda x0, x1, u: (x0 + a * u, 0.9 * x1 + e * u)
        sysd.cost = lambda x0, x1, u: (x0 - 0.4) * (x0 - 0.4) + 0.3 * (u - x1) ** 2 + 0.1 * u
        sysd.control_box = lambda x0, x1: _BOX1
        return _finish(sysd, (0, 1, n0, 0, 1, n1), 0, (du,))
    return make


def m2_two_controls(n0, n1, W, a, b, c, e, du, dv):
    """`m2` with a control of its own for x1: SDP_NU = 2, the flat lattice walked in chunks of cu"""
    def make():
        sysd = SysDescription((2, 2, 1), name='m2, two controls')
        sysd.dyn = lambda x0, x1, u, v, w: (x0 + a * u + b * w, 0.9 * x1 + c * w + e * v)
        sysd.cost = lambda x0, x1, u, v, w: (x0 - 0.4) * (x0 - 0.4) + 0.3 * (u - x1) ** 2 + w * u + 0.2 * (v + 0.1) ** 2 + 0.1 * v * x0
        sysd.control_box = lambda x0, x1: ((-0.5, 0.5), (-0.5, 0.5))
        return _finish(sysd, (0, 1, n0, 0, 1, n1), W, (du, dv))
    return make


def m2_uneven(n0, n1, W, a, b, c, e, du):
    """`m2` on a per-node box whose upper end moves with both state variables: the nodes of one tile have different
    control counts, n_ctrl is the tile's maximum, and lanes past their own count run clamped controls"""
    def make():
        sysd = SysDescription((2, 1, 1), name='m2, uneven box')
        sysd.dyn = lambda x0, x1, u, w: (x0 + a * u + b * w, 0.9 * x1 + c * w + e * u)
        sysd.cost = lambda x0, x1, u, w: (x0 - 0.4) * (x0 - 0.4) + 0.3 * (u - x1) ** 2 + w * u
        sysd.control_box = lambda x0, x1: ((-0.5, 0.5 * x0 + 0.45 * x1 - 0.45),)
        return _finish(sysd, (0, 1, n0, 0, 1, n1), W, (du,))
    return make


def m2_fold(n0, n1, W, amp, b, c, du):
    """dynamics that fold back inside a chunk (the fold of tests/test_gpu_staged.py::_wavy, moved off the middle of
    the lattice: x0' peaks at u = -0.3, x1' turns at w = -0.45), so that the corner prediction misses cells, on a
    grid and with a reach in w that plan cw < W: the turn in w lies inside the FIRST w chunk"""
    def make():
        sysd = SysDescription((2, 1, 1), name='m2, folded')
        sysd.dyn = lambda x0, x1, u, w: (x0 + amp * (0.25 - (u + 0.3) * (u + 0.3)) * 4 - 0.2 + b * w,
                                         0.5 * x1 + c * np.abs(w + 0.45) + 0.1 * u * x0)
        sysd.cost = lambda x0, x1, u, w: (x0 - 0.4) * (x0 - 0.4) + 0.3 * (u - x1) ** 2 + w * u
        sysd.control_box = lambda x0, x1: _BOX1
        return _finish(sysd, (0, 1, n0, 0, 1, n1), W, (du,))
    return make


def inputs(shape):
    """two cost-to-go arrays.  `smooth`: waves of a different length along every axis, short enough along the first
    one (the axis the control moves) for the nodes to find their valley at different points of the control lattice.
    `random`: the same with seeded white noise of unit variance on top -- a vertex read from the wrong place changes
    the result beyond any rounding -- except on the two outermost layers of every axis: the models reach far outside
    the grid, where the reference extrapolates the last cell linearly, and noise extrapolated over hundreds of cells
    would decide every policy."""
    shape = tuple(int(n) for n in shape)
    axes = np.meshgrid(*[np.linspace(0., 1., n) for n in shape], indexing='ij')
    smooth = 0.5 * axes[0] * axes[-1]
    for k, x in enumerate(axes):
        smooth = smooth + np.cos((11.0 - 3 * k) * x + 0.7 * k + 2.0 * axes[-1]) / (1 + k)
    inner = np.ones(shape, dtype=bool)
    for k, n in enumerate(shape):
        i = np.arange(n).reshape([-1 if j == k else 1 for j in range(len(shape))])
        inner = inner & (i >= 2) & (i < n - 2)
    rand = smooth + np.where(inner, np.random.default_rng(50 + len(shape)).standard_normal(shape), 0.)
    return {'smooth': smooth, 'random': rand}


INPUTS = ('smooth', 'random')


def unit_sources(case):
    """{what: generated source} of every unit tests/test_gpu_staged_forms.py runs for the case: staged and direct,
    per real type"""
    out = {}
    with case.budgeted():
        for rs in case.sizes:
            out['staged, {} bytes'.format(rs)] = case.solver(rs)._kernel_plan()['source']
            out['generic, {} bytes'.format(rs)] = case.solver(rs, 'generic')._kernel_plan()['source']
    return out


def macro(source, name):
    import re
    m = re.search(r'^#define {} (.+)$'.format(re.escape(name)), source, re.M)
    return m.group(1).strip() if m else None


# ---------------------------------------------------------------------------------------------------------------------
# Steps 1 and 2 of sdp_sweep_lds, restated from csrc/sdp_staged_kernel.h:
#   a tile is a box of TILE nodes, lanes consecutive along the last axis, tiles walked in C order; a lane past the grid
#   reads the clamped node and is not live;  n_ctrl = the largest control count of the tile's live lanes;
#   per chunk (c0, w0): the lanes with c0 < total evaluate the dynamics at (c0 | min(c0 + CU, total) - 1) x (w0 | w1 - 1)
#   and guess the cells  q = clamp(trunc((x' - smin) * (nm1 / span)), 0, n - 2);   the box of the tile is
#   org = max(qlo - 1, 0),  top = min(qhi + 1, n - 2),  ext = top + 2 - org  vertices per axis;
#   rows of stride kernel_row_stride(ext[last]);  while the volume exceeds CAP the leading axes are cut in turn to
#   max(2, CAP / other), then the row to CAP / other, and with fewer than 3 vertices of a row nothing is staged;
#   a lattice cell  q = clamp(trunc((x' - smin) / span * nm1), 0, n - 2)  is inside iff 0 <= q - org < ext - 1 on every axis.
# ---------------------------------------------------------------------------------------------------------------------
def kernel_row_stride(length, tile_last, d, rs):
    """sdp_stg_row_stride, from the kernel's text (codegen.staged_row_stride is the planner's copy)"""
    if d == 1 or tile_last >= 32 or rs != 8:
        return length | 1
    return (length + tile_last - 1) // (2 * tile_last) * (2 * tile_last) + tile_last


class Reach(object):
    """counts[path]: (tile, chunk) pairs per staging path; missed_cells; early_pairs: (control, node) pairs missed in a
    w chunk that is not the last; early_only_pairs: those of them that do not miss in the last chunk as well (only
    outside[] carried from box to box sends them to global memory), early_nodes: their nodes; nodes[path]: flat ids of the live nodes of tiles with a chunk on that path;
    early_nodes; ext_last: every row length met; read_vertices[path]: flat ids of a few vertices that lattice cells
    read from staged boxes on that path (the lower corner of a cell inside); missed_vertices[path]: the same of cells
    that missed the box of a chunk on that path (read from global memory)"""

    def __init__(self, case, rs):
        from stodynprog_amd.trace import evaluate
        with case.budgeted():
            s = case.solver(rs)
            plan = s._kernel_plan()
        st = plan['staged']
        model = plan['model']
        self.staged = st
        shape = self.shape = s._shape()
        d = self.d = len(shape)
        tile, cu, cw, cap = st['tile'], st['cu'], st['cw'], st['cap']
        W = plan['W']
        Wn = max(W, 1)
        wg = np.asarray(s.perturb_grid[0], dtype=float) if W else np.zeros(1)
        self.W, self.Wn = W, Wn
        tiles_per = [-(-shape[k] // tile[k]) for k in range(d)]
        n_tiles = int(np.prod(tiles_per))
        # (n_tiles, 512): index of every lane's node along every axis, tiles and lanes in C order
        idx, live = [], np.ones((n_tiles, 512), dtype=bool)
        for k in range(d):
            i = (np.arange(tiles_per[k])[:, None] * tile[k] + np.arange(tile[k])[None, :])      # (tiles, in_tile)
            full = np.broadcast_to(i.reshape([tiles_per[j] if j == k else 1 for j in range(d)]
                                             + [tile[j] if j == k else 1 for j in range(d)]),
                                   tuple(tiles_per) + tuple(tile)).reshape(n_tiles, 512)
            live &= full < shape[k]
            idx.append(np.minimum(full, shape[k] - 1))
        node = np.ravel_multi_index(tuple(idx), shape)
        x = [np.asarray(s.state_grid[k], dtype=float)[idx[k]] for k in range(d)]
        lo, hi, n = plan['lo'], plan['hi'], plan['n']
        col = node if plan['per_node'] else np.zeros_like(node)
        nn = n[:, col].astype(np.int64)                        # (nu, tiles, 512)
        blo, bhi = lo[:, col], hi[:, col]
        nu = nn.shape[0]
        total = np.where(live, np.prod(nn, axis=0), 0)
        n_ctrl = total.max(axis=1)
        self.n_ctrl = n_ctrl
        self.totals = total
        self.uneven_tiles = int(((np.where(live, total, n_ctrl[:, None]) != n_ctrl[:, None]).any(axis=1)).sum())
        step = np.where(nn > 1, (bhi - blo) / np.maximum(nn - 1, 1), 0.)

        def controls_at(flat):
            out = []
            for c in range(nu - 1, -1, -1):
                k = flat % nn[c]
                flat = flat // nn[c]
                out.append(np.where(nn[c] == 1, blo[c], np.where(k == nn[c] - 1, bhi[c], k * step[c] + blo[c])))
            return out[::-1]

        smin = [float(g[0]) for g in s.state_grid]
        span = [float(g[-1] - g[0]) for g in s.state_grid]
        nm1 = [float(len(g) - 1) for g in s.state_grid]

        def cells(u, wi, guess):
            xn, _ = evaluate(model, x, u, [wg[wi]] if model.n_perturb else [], 0.0)
            out = []
            for k in range(d):
                v = np.broadcast_to(np.asarray(xn[k], dtype=float), node.shape)
                p = (v - smin[k]) * (nm1[k] / span[k]) if guess else (v - smin[k]) / span[k] * nm1[k]
                out.append(np.clip(np.trunc(np.nan_to_num(p, nan=0., posinf=1e9, neginf=-1e9)), 0, shape[k] - 2).astype(np.int64))
            return out

        counts = {p: 0 for p in PATHS}
        tiles_on = {p: np.zeros(n_tiles, dtype=bool) for p in PATHS}
        read_vertices = {p: set() for p in PATHS}
        missed_vertices = {p: set() for p in PATHS}
        self.cut_axes = set()
        ext_last = set()
        n_max = int(n_ctrl.max())
        missed_pair = np.zeros((n_max,) + node.shape, dtype=bool)
        early_pair = np.zeros((n_max,) + node.shape, dtype=bool)
        last_pair = np.zeros((n_max,) + node.shape, dtype=bool)
        missed_cells = 0
        BIG = 1 << 40
        for c0 in range(0, n_max, cu):
            act = n_ctrl > c0                                   # tiles that run this control chunk
            contrib = c0 < total                                # lanes that predict
            c_last = np.minimum(c0 + cu, np.maximum(total, 1)) - 1
            ucorner = [controls_at(np.minimum(c0, np.maximum(total, 1) - 1)), controls_at(c_last)]
            ulat = [controls_at(np.minimum(c0 + j, np.maximum(total, 1) - 1)) for j in range(cu)]
            for w0 in range(0, Wn, cw):
                w1 = min(w0 + cw, Wn)
                qlo = np.full((d, n_tiles), BIG)
                qhi = np.full((d, n_tiles), -BIG)
                for u in ucorner:
                    for wi in (w0, w1 - 1):
                        q = cells(u, wi, True)
                        for k in range(d):
                            qlo[k] = np.minimum(qlo[k], np.where(contrib, q[k], BIG).min(axis=1))
                            qhi[k] = np.maximum(qhi[k], np.where(contrib, q[k], -BIG).max(axis=1))
                assert ((qlo[0] != BIG) == act).all()
                org = np.zeros((d, n_tiles), dtype=np.int64)
                ext = np.full((d, n_tiles), 2, dtype=np.int64)
                for k in range(d):
                    o = np.maximum(qlo[k] - 1, 0)
                    top = np.minimum(qhi[k] + 1, shape[k] - 2)
                    org[k] = np.where(act, o, 0)
                    ext[k] = np.where(act, top + 2 - o, 2)
                ext_last.update(np.unique(ext[d - 1][act]).tolist())
                rowlen = np.array([kernel_row_stride(int(e), tile[-1], d, rs) for e in ext[d - 1]], dtype=np.int64)
                vol = rowlen.copy()
                for k in range(d - 1):
                    vol = vol * ext[k]
                lead_cut = np.zeros(n_tiles, dtype=bool)
                for k in range(d - 1):
                    other = vol // ext[k]
                    fit = np.maximum(2, cap // other)
                    do = (vol > cap) & (fit < ext[k])
                    if (do & act).any():
                        self.cut_axes.add(k)
                    ext[k] = np.where(do, fit, ext[k])
                    vol = np.where(do, other * fit, vol)
                    lead_cut |= do
                over = vol > cap
                other = vol // rowlen
                fit = cap // other
                none = over & (fit < 3)
                last_cut = over & ~none
                if (last_cut & act).any():
                    self.cut_axes.add(d - 1)
                ext[d - 1] = np.where(last_cut, np.minimum(ext[d - 1], fit), ext[d - 1])
                path = np.where(none, 3, np.where(last_cut, 2, np.where(lead_cut, 1, 0)))
                for p, name in enumerate(PATHS):
                    on_p = act & (path == p)
                    counts[name] += int(on_p.sum())
                    tiles_on[name] |= on_p
                staged_any = act & ~none
                # the lattice cells of the chunk
                for wi in range(w0, w1):
                    for j in range(cu):
                        ci = c0 + j
                        if ci >= n_max:
                            continue
                        on = ci < total
                        q = cells(ulat[j], wi, False)
                        inside = np.broadcast_to(staged_any[:, None], node.shape).copy()
                        for k in range(d):
                            rel = q[k] - org[k][:, None]
                            inside &= (rel >= 0) & (rel < ext[k][:, None] - 1)
                        miss = on & ~inside
                        missed_cells += int(miss.sum())
                        # a few of the vertices read: from the box per path, and from global memory by a cell that missed
                        flatq = None
                        for p, name in enumerate(PATHS):
                            for hit, found in ((on & inside, read_vertices[name]), (miss, missed_vertices[name])):
                                if len(found) < 9:
                                    tl = np.flatnonzero(act & (path == p) & hit.any(axis=1))[:3]
                                    if len(tl):
                                        flatq = np.ravel_multi_index(tuple(q), shape) if flatq is None else flatq
                                        found.update(int(flatq[t, np.argmax(hit[t])]) for t in tl)
                        missed_pair[ci] |= miss
                        if w1 < Wn:
                            early_pair[ci] |= miss
                        else:
                            last_pair[ci] |= miss
        self.counts = counts
        self.missed_cells = missed_cells
        self.missed_pairs = int(missed_pair.sum())
        self.early_pairs = int(early_pair.sum())
        early_only = early_pair & ~last_pair
        self.early_only_pairs = int(early_only.sum())
        self.early_nodes = np.unique(node[early_only.any(axis=0)])
        self.nodes = {p: np.unique(node[live & tiles_on[p][:, None]]) for p in PATHS}
        self.ext_last = sorted(ext_last)
        self.read_vertices = {p: sorted(v) for p, v in read_vertices.items()}
        self.missed_vertices = {p: sorted(v) for p, v in missed_vertices.items()}
        self.cells = int((total.sum()) * Wn)
        self.n_tiles = n_tiles
        self.S = int(np.prod(shape))


@functools.lru_cache(maxsize=None)
def reach(name, rs):
    return Reach(BY_NAME[name], rs)


def sample_nodes(case, rs):
    """flat C-order node ids the oracle is run on: `sampled` of them, with the first and the last node, 50 nodes (or all
    where fewer exist) of tiles on each path the case claims, 50 nodes with an early miss where claimed, seeded"""
    r = reach(case.name, rs)
    rng = np.random.default_rng(r.S + rs)
    picked = {0, r.S - 1}
    groups = [r.nodes[p] for p in case.paths[rs]] + ([r.early_nodes] if 'early' in case.claimed(rs) else [])
    for g in groups:
        picked.update(rng.choice(g, size=min(50, len(g)), replace=False).tolist())
    extra = iter(rng.permutation(r.S).tolist())
    while len(picked) < min(case.sampled, r.S):
        picked.add(next(extra))
    return np.array(sorted(picked), dtype=np.int64)


@functools.lru_cache(maxsize=None)
def oracle(name, rs, which):
    """(nodes, J, pol, idx) of oracle/vi_numpy.py on the case's sample: the reference's path for 8-byte reals, the
    direct kernel's definition restated in float32 for 4-byte ones (as tests/test_gpu_fp32_oracle.py)"""
    from oracle import vi_numpy
    case = BY_NAME[name]
    s = case.solver(rs)
    nodes = sample_nodes(case, rs)
    V = inputs(s._shape())[which]
    with np.errstate(all='ignore'):
        if rs == 8:
            J, pol, idx, _ = vi_numpy.value_iteration(vi_numpy.Spec.from_solver(s), V, nodes=nodes)
        else:
            J, pol, idx, _ = vi_numpy.value_iteration(vi_numpy.Spec.from_solver(s), V.astype(np.float32), nodes=nodes,
                                                      dtype=np.float32)
    return nodes, J, pol, idx.astype(np.int32)


_U, _B, _W, _E, _N = 'ragged_u', 'boxes', 'ragged_w', 'early', 'uneven'
_SHORT = m2(12, 1001, 7, .2, .3, .5, 0, .1)          # axis 0 shorter than its tile edge (16)

CASES = [
    # the ten rows the planner was first measured on
    Case('one_box', m2(100, 120, 7, .2, .3, .5, 0, .1), {8: (4, 7), 4: (4, 7)}, {8: ['fit'], 4: ['fit']},
         {8: [_U], 4: [_U]}),                                            # baseline: one box per control chunk
    Case('two_w_chunks', m2(100, 120, 8, .2, .6, .5, 0, .1), {8: (4, 4), 4: (4, 8)}, {8: ['fit'], 4: ['fit']},
         {8: [_B, _U], 4: [_U]}),                                        # 11 controls in chunks of 4, 4, 3
    Case('ragged_w_3d', m3((24, 22, 26), 7, 1, .5, .5, .1), {8: (4, 3), 4: (4, 7)}, {8: ['fit'], 4: ['fit']},
         {8: [_B, _W, _U], 4: [_U]}),                                    # w chunks 3, 3, 1; d = 3 in 4 bytes: len | 1
    Case('cu2', m2(300, 120, 8, 1, 0, .5, 0, .25), {8: (2, 4), 4: (4, 4)}, {8: ['fit'], 4: ['fit']},
         {8: [_B, _U], 4: [_B, _U]}),                                    # 5 controls in chunks of 2, 2, 1
    Case('cu2_w6', m2(600, 40, 6, 1, 0, .5, 0, .5), {8: (2, 3), 4: (4, 3)}, {8: ['fit', 'cut0'], 4: ['fit']},
         {8: [_B, _U], 4: [_B]}),
    Case('cu2_3d', m3((40, 22, 26), 8, 1, .5, 0, .1), {8: (2, 8), 4: (4, 8)}, {8: ['fit', 'cut0'], 4: ['fit']},
         {8: [_U], 4: [_U]}),
    Case('four_w_chunks_3d', m3((40, 22, 26), 8, 1, .5, 0, .25), {8: (4, 2), 4: (4, 8)}, {8: ['fit', 'cut0'], 4: ['fit']},
         {8: [_B, _U, _E], 4: [_U]}),
    Case('cu1', m2(400, 120, 8, 1, 0, .5, 0, .5), {8: (1, 8), 4: (4, 2)}, {8: ['fit'], 4: ['fit']},
         {4: [_B, _E]}),
    Case('cu2_in_4_bytes', m2(300, 120, 8, 2, 0, .5, 0, .25), {8: (2, 4), 4: (2, 8)}, {8: ['fit', 'cut0'], 4: ['fit', 'cut0']},
         {8: [_B, _U, _E], 4: [_U]}),
    Case('eight_boxes', m2(400, 160, 8, 1, 1, 1, 0, .5), {8: (4, 1), 4: (4, 1)}, {8: ['fit', 'cut0'], 4: ['fit']},
         {8: [_B, _E], 4: [_B]}),                                        # 3 controls < cu; outside[] carried over 8 boxes
    # one state variable, tile (512,): more nodes than the budget, a reach that grows with x until the boxes of the
    # last tiles are cut -- on the only axis, the last one: rows of 9728 vertices copied by 64 lanes, stride len | 1
    Case('line_16001', m1(16001, 8, .2, .15, 5.0, .1), {8: (4, 4)}, {8: ['fit', 'cutlast']}, {8: [_B, _U, _E]}),
    # four state variables, tile (4, 4, 4, 8), 11 880 nodes
    Case('four_axes', m4((10, 9, 11, 12), 6, 1, .3, .3, .3, .25), {8: (2, 3)}, {8: ['fit', 'cut0']}, {8: [_B, _U, _E]}),
    # no perturbation: Wn = 1, acc[j] = jc, with cu = 2
    Case('deterministic_cu2', m2_deterministic(300, 120, 2, 0, .25), {8: (2, 1)}, {8: ['fit']}, {8: [_U]}),
    # two controls, a flat lattice of 9 points in chunks of 2
    Case('two_controls', m2_two_controls(300, 120, 8, 1, 0, .5, .2, .5, .5), {8: (2, 8)}, {8: ['fit', 'cut0']}, {8: [_U]}),
    # a per-node box: 3 to 9 controls, 73 of 76 tiles with nodes of different counts
    Case('uneven_box', m2_uneven(300, 120, 8, 1, 0, .5, 0, .125), {8: (4, 4)}, {8: ['fit', 'cut0']}, {8: [_B, _N, _E]}),
    # folded dynamics with cw < W: misses in the first w chunk
    Case('folded', m2_fold(300, 120, 8, .35, .6, .5, .1), {8: (4, 2)}, {8: ['fit']}, {8: [_B, _U, _E]}),
    # the cut branches no natural shape of this size reaches, through the budget: down to the last axis in d = 2 ..
    Case('budget_512', _SHORT, {8: (1, 1)}, {8: ['fit', 'cut0', 'cutlast']}, {8: [_B, _E]}, budget=512),
    # (in both runs EVERY control of every node has a cell outside its boxes, in the last w chunk too: no sum of the
    # gather survives, so these two runs cannot see what is carried from box to box and do not claim 'early')
    # .. and fewer than 3 vertices of a row (8 bytes: nothing staged; 4 bytes: rows of 4 vertices)
    Case('budget_32', _SHORT, {8: (1, 1), 4: (1, 1)}, {8: ['none'], 4: ['cut0', 'cutlast']}, {8: [_B], 4: [_B]},
         budget=32),
]
BY_NAME = {c.name: c for c in CASES}
RUNS = [(c, rs) for c in CASES for rs in c.sizes]
RUN_IDS = ['{}-f{}'.format(c.name, rs) for c, rs in RUNS]
