"""The compile-time forms of the column family (csrc/sdp_column_kernel.h, sdp_colres_kernel.h,
sdp_colfilter_kernel.h) as a table of cases (test infrastructure, like tests/full_parity.py; not a test file).

codegen.column_table_unit (with column_config and column_resident_points, the arithmetic underneath) turns four
numbers -- the rows of axis 0, the perturbation points W, the number of controls and the dtype -- into one of many
units (a codegen.ColumnUnit, which codegen._column_lines prints as it is): workgroup size,
resident chunks (SDP_COL_WRES), the tail held in registers (SDP_COL_TAIL_HOLD) and its geometry, lanes per
point of the table build (SDP_COL_A_LW), the short first pass and its branch and bound, the control table,
the register cap, the knobs of 4-byte reals.  Each case below is the benchmark model (models.synthetic3d)
re-discretised at a shape that selects one form, with the macros it exists to cover.  `claims` maps a macro to
the value its #define must carry, or to None where the form must NOT define it.

tests/test_column_forms_plan.py checks on the CPU that every case still plans what it claims (a planner
change that moves a shape to another form names the case that lost its coverage) and that its units compile;
tests/test_gpu_column_forms.py runs every case on the GPU against the other kernels and the oracle."""
import re

import numpy as np

from stodynprog_amd import models, DPSolver

# trailing axes (n1, n2): 'many' = 16 384 columns, at least 64 per CU of an MI355X (256 CUs): every workgroup of the
# persistent loop claims several units and carries its state from one to the next; 'split' = 64 columns, fewer than
# CUs: column_grid (csrc/sdp_hip.hip) splits every column into row ranges, one unit each
GEOMETRIES = {'many': (128, 128), 'split': (8, 8)}


class Case(object):
    def __init__(self, name, n0, claims, n_w=32, n_u=64, dtype=np.float64, noise=0.0, wres=None,
                 hold=None, geometries=('many',), geometry_claims=None):
        self.name, self.n0, self.n_w, self.n_u = name, int(n0), int(n_w), int(n_u)
        self.dtype, self.noise, self.wres = np.dtype(dtype), float(noise), wres
        self.claims = dict(claims)
        self.geometry_claims = dict(geometry_claims or {})     # {geometry: claims that differ there}
        self.hold = hold                    # (WP, NW, NJ) of sdp_colres_tail: points side by side x per thread x row pairs
        self.geometries = tuple(geometries)

    def __repr__(self):
        return self.name

    @property
    def debug(self):
        """the forced planning switch of the case (the tests set it through the debug_defines fixture)"""
        return {'SDP_COL_WRES': str(self.wres)} if self.wres else {}

    def solver(self, geometry, kernel='auto', certified_filter=True, dtype=None):
        """a solver of the case at trailing axes GEOMETRIES[geometry] (or an explicit (n1, n2)); the switches of
        `debug` must be set by the caller"""
        n1, n2 = GEOMETRIES[geometry] if isinstance(geometry, str) else geometry
        sysd, ref = models.synthetic3d(N=8, n_w=self.n_w, stock_noise=self.noise)
        s = DPSolver(sysd, dtype=self.dtype if dtype is None else dtype)
        s.discretize_state(0, 1, self.n0, 0, 1, n1, 0, 1, n2)
        s.perturb_grid, s.perturb_proba = ref.perturb_grid, ref.perturb_proba
        # n_u points on the box [-1, 1]: ceil(2 / step) + 1 of them (the step is kept off an integer quotient)
        s.control_steps = (2. / (self.n_u - 1.5),)
        s.kernel = kernel
        s.certified_filter = certified_filter
        return s


def macro(source, name):
    """value of `#define name value` in a generated source, or None"""
    m = re.search(r'^#define {} (\S+)'.format(re.escape(name)), source, re.M)
    return m.group(1) if m else None


def claims(case, geometry):
    """what the unit of `case` must define at `geometry`: {macro: value, or None for 'not defined'}"""
    return dict(case.claims, **case.geometry_claims.get(geometry, {}))


def missing_claims(case, geometry, source):
    """the claims of `case` at `geometry` that `source` does not meet: [(macro, claimed, found)]"""
    return [(k, v, macro(source, k)) for k, v in sorted(claims(case, geometry).items()) if macro(source, k) != v]


def hold_geometry(source):
    """(WP, NW, NJ) of the held tail that `source` builds (csrc/sdp_colres_kernel.h: SDP_HOLD_WP / _NW / _NJ), or None"""
    if macro(source, 'SDP_COL_TAIL_HOLD') != '1':
        return None
    t, lw, w, wres, n0 = (int(macro(source, k)) for k in
                          ('SDP_COL_THREADS', 'SDP_COL_A_LW', 'SDP_COL_W', 'SDP_COL_WRES', 'SDP_COL_N0'))
    wp = t // lw
    return (wp, (w - wres) // wp, n0 // (2 * lw))


def _resident(threads, wres, lw, min_waves=None, hold=True, **more):
    c = {'SDP_COL_THREADS': str(threads), 'SDP_COL_WRES': str(wres), 'SDP_COL_A_LW': str(lw), 'SDP_COL_FILTER': '1',
         'SDP_COL_TAIL_HOLD': '1' if hold else None, 'SDP_COL_MIN_WAVES': None if min_waves is None else str(min_waves)}
    c.update(more)
    return c


_BNB = dict(SDP_COL_LEAN2='1', SDP_COL_BNB='1')
_SHIFT = dict(SDP_COL_SHIFT='1', SDP_COL_UNROLL_W='1')
_NO_TABLE = dict(SDP_COL_UTAB=None, SDP_COL_UTAB_N=None, SDP_COL_LEAN2=None, SDP_COL_BNB=None)
_BOTH = ('many', 'split')

CASES = [
    # ---- the tail held in registers (sdp_colres_tail), four geometries, with and without noise in the stock
    Case('hold_8x2x4', 256, _resident(256, 16, 32, 4, SDP_COL_UTAB_N='64', **_BNB), hold=(8, 2, 4), geometries=_BOTH),
    Case('hold_8x2x4_noise', 256, _resident(256, 16, 32, 3, SDP_COL_UTAB_N='64', **dict(_BNB, **_SHIFT)),
         noise=0.07, hold=(8, 2, 4), geometries=_BOTH),
    Case('hold_4x4x2_w33', 256, _resident(256, 17, 64, 4, SDP_COL_UTAB_N='64', **_BNB), n_w=33,
         hold=(4, 4, 2), geometries=_BOTH),
    Case('hold_4x4x2_w33_noise', 256, _resident(256, 17, 64, 3, SDP_COL_UTAB_N='64', **dict(_BNB, **_SHIFT)), n_w=33,
         noise=0.07, hold=(4, 4, 2), geometries=_BOTH),
    Case('hold_16x1x4_u200', 256, _resident(512, 16, 32, None, SDP_COL_UTAB_N='200', **_BNB), n_u=200,
         hold=(16, 1, 4), geometries=_BOTH),
    Case('hold_16x1x4_u200_noise', 256, _resident(512, 16, 32, None, SDP_COL_UTAB_N='200', **dict(_BNB, **_SHIFT)),
         n_u=200, noise=0.07, hold=(16, 1, 4), geometries=_BOTH),
    Case('hold_8x1x4_wres24', 256, _resident(256, 24, 32, 2, SDP_COL_UTAB_N='64', **_BNB), wres=24,
         hold=(8, 1, 4), geometries=_BOTH),
    Case('hold_8x1x4_wres24_noise', 256, _resident(256, 24, 32, 2, SDP_COL_UTAB_N='64', **dict(_BNB, **_SHIFT)),
         wres=24, noise=0.07, hold=(8, 1, 4), geometries=_BOTH),
    Case('hold_4x4x2_n128_w40_wres24', 128, _resident(128, 24, 32, 2, SDP_COL_UTAB_N='64', **_BNB), n_w=40, wres=24,
         hold=(4, 4, 2), geometries=_BOTH),
    # (301 controls on 16 384 columns: 512 threads, the held tail, no control table)
    Case('hold_16x1x4_u301_no_table', 256, _resident(512, 16, 32, None, **_NO_TABLE), n_u=301, hold=(16, 1, 4)),
    # ---- resident chunks without the held tail
    Case('res_n192', 192, _resident(192, 16, 64, 3, hold=False, SDP_COL_UTAB_N='64', **_BNB)),
    Case('res_n240', 240, _resident(256, 16, 32, 4, hold=False, SDP_COL_UTAB_N='64', **_BNB)),
    Case('res_n320', 320, _resident(320, 16, 64, None, hold=False, SDP_COL_UTAB_N='64', **_BNB)),
    Case('res_n128_w64', 128, _resident(128, 32, 32, 2, hold=False, SDP_COL_UTAB_N='64', **_BNB), n_w=64),
    Case('res_n256_w40', 256, _resident(256, 20, 32, 3, hold=False, SDP_COL_UTAB_N='64', **_BNB), n_w=40),
    # ---- 1024 threads: the plain filtered kernel with the whole table, and resident chunks without a control table
    Case('full_n384', 384, dict(SDP_COL_THREADS='1024', SDP_COL_WRES=None, SDP_COL_A_LW='32', SDP_COL_UTAB_N='64',
                                SDP_COL_FILTER='1')),
    Case('full_n500', 500, dict(SDP_COL_THREADS='1024', SDP_COL_WRES=None, SDP_COL_A_LW='32', SDP_COL_UTAB_N='64',
                                SDP_COL_FILTER='1'), geometries=_BOTH),
    Case('full_n512', 512, dict(SDP_COL_THREADS='1024', SDP_COL_WRES=None, SDP_COL_A_LW='32', SDP_COL_UTAB_N='64',
                                SDP_COL_FILTER='1')),
    Case('full_n256_w48', 256, dict(SDP_COL_THREADS='1024', SDP_COL_WRES=None, SDP_COL_A_LW='64', SDP_COL_UTAB_N='64',
                                    SDP_COL_FILTER='1'), n_w=48),
    # (301 controls on fewer than 256 columns: 1024 threads, four lanes of a node's controls each)
    Case('res1024_u301', 256, _resident(1024, 16, 32, None, hold=False, **_NO_TABLE), n_u=301, geometries=('split',)),
    Case('res1024_u301_noise', 256, _resident(1024, 16, 32, None, hold=False, SDP_COL_SHIFT='1', **_NO_TABLE),
         n_u=301, noise=0.07, geometries=('split',)),
    # ---- branch and bound over blocks of 8 controls: partial last blocks, and the largest control table of the model
    Case('bnb_u57', 256, _resident(256, 16, 32, 4, SDP_COL_UTAB_N='57', **_BNB), n_u=57, hold=(8, 2, 4)),
    Case('bnb_u65', 256, _resident(256, 16, 32, 4, SDP_COL_UTAB_N='65', **_BNB), n_u=65, hold=(8, 2, 4)),
    Case('bnb_u71', 256, _resident(256, 16, 32, 4, SDP_COL_UTAB_N='71', **_BNB), n_u=71, hold=(8, 2, 4)),
    Case('bnb_u256', 256, _resident(512, 16, 32, None, SDP_COL_UTAB_N='256', **_BNB), n_u=256, hold=(16, 1, 4)),
    # ---- 4-byte reals: the short wide first pass with four blocks' bounds per stage, grouped vertex loads
    Case('f32_n600', 600, dict(SDP_COL_THREADS='1024', SDP_COL_A_LW='64', SDP_COL_WIDE2='1', SDP_COL_BNB='1',
                               SDP_BNB_CHUNK='4', SDP_COL_A_GROUP='8', SDP_COL_UTAB_N='64'), dtype=np.float32),
    Case('f32_n1024', 1024, dict(SDP_COL_THREADS='1024', SDP_COL_A_LW='64', SDP_COL_WIDE2='1', SDP_COL_BNB='1',
                                 SDP_BNB_CHUNK='4', SDP_COL_A_GROUP='8', SDP_COL_UTAB_N='64'), dtype=np.float32),
    # (on 16 384 columns 512 threads; on fewer than 256 columns 1024)
    Case('f32_n512_u129', 512, dict(SDP_COL_THREADS='512', SDP_COL_A_LW='64', SDP_COL_WIDE2='1', SDP_COL_BNB='1',
                                    SDP_BNB_CHUNK='4', SDP_COL_A_GROUP='8', SDP_COL_UTAB_N='129'),
         n_u=129, dtype=np.float32, geometries=_BOTH, geometry_claims={'split': dict(SDP_COL_THREADS='1024')}),
    Case('f32_n512_u601_no_table', 512, dict(SDP_COL_THREADS='512', SDP_COL_A_LW='64', SDP_COL_A_GROUP='8',
                                             SDP_COL_WIDE2=None, **_NO_TABLE), n_u=601, dtype=np.float32,
         geometries=_BOTH, geometry_claims={'split': dict(SDP_COL_THREADS='1024')}),
]

# every (case, geometry) pair the GPU test runs
PAIRS = [(c, g) for c in CASES for g in c.geometries]


def split_rows(n0):
    """rows on either side of every boundary column_grid can draw when it splits a column of n0 rows into `s` row
    ranges (i_lo = n0 * part / s, s <= n0 / 64: csrc/sdp_hip.hip, sdp_colres_kernel.h)"""
    rows = set()
    for s in range(2, max(2, n0 // 64) + 1):
        for part in range(1, s):
            b = n0 * part // s
            rows.update((b - 1, b))
    return sorted(r for r in rows if 0 <= r < n0)


def sample_nodes(shape, n=500, seed=0):
    """flat C-order node ids, sorted: `n` random ones plus rows 0 and n0 - 1 of several columns, the whole last
    column, and the rows around the possible split boundaries of a few columns"""
    n0, n1, n2 = shape
    rng = np.random.default_rng(seed)
    cols = [(0, 0), (n1 - 1, n2 - 1), (n1 // 2, n2 // 3), (1, n2 - 1), (n1 - 1, 0)]
    cols += [tuple(int(v) for v in rng.integers(0, (n1, n2))) for _ in range(3)]
    picked = set(rng.choice(n0 * n1 * n2, size=n, replace=False).tolist())
    ravel = lambda i, j, k: (i * n1 + j) * n2 + k
    for j, k in cols:
        picked.update((ravel(0, j, k), ravel(n0 - 1, j, k)))
        picked.update(ravel(i, j, k) for i in split_rows(n0))
    picked.update(ravel(i, n1 - 1, n2 - 1) for i in range(n0))          # the last column, every row
    return np.array(sorted(picked), dtype=np.int64)
