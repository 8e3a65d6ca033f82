"""Time-dependent systems (`stationnary=False`, run by bellman_recursion) in every kernel family and at the shapes of the
column forms (test infrastructure, like tests/column_forms.py; not a test file).

A time-dependent system reaches the kernels through paths no stationary model runs: the time index is a kernel
argument, the control box is tabulated again at every step, every step is planned on its own, and a lattice that
changes with the time index gets a control table with room to spare -- a CAPACITY, the power of two at or above the
step's largest lattice (DPSolver._kernel_plan_now; ColumnUnit.max_controls and utab_n of the unit's record), so that
the steps of a horizon share code objects.  The kernel
then runs with fewer controls than its table holds, and the branch and bound's block size and block count come from
the capacity, not from the lattice.

In every model below the time index k reaches, each through a term of its own:
- the stock, by a drift `d * (k - k0)` large enough that a prediction made at one step (the staged box, kept under the
  box digest; the row window) is several rows off at another step with the same box;
- the exogenous process;
- the cost, by a coefficient that multiplies a control term (the filter's max |h| changes from step to step);
- the control box, whose width gives the lattice of step k its size.

FAMILIES are the time-dependent twins of tests/test_gpu_call_to_call.FAMILIES (and a model that cannot be traced: the
tabulated mode).  Over their horizon the lattice takes SIZES: 1 control (width / step < 0.1, the midpoint rule), fewer
than 8, 8 m + 1, a power of two, one less and one more than a power of two (the next capacity: a second code object).
TIME_DATA variants look their constants up as `data[k]`: every step is its own trace, specialised to k, with its
constants lifted into kernel parameters.

CASES put the time-dependent synthetic3d at the shape of a case of tests/column_forms.py (rows, W, controls, dtype,
noise, the wres switch), with a horizon whose lattices all share the case's capacity and stay below it at the steps
`Case.below` lists.

tests/test_horizon_plan.py checks on the CPU that every family and case plans, at every step, what it claims here;
tests/test_gpu_horizon.py runs them on the GPU against the long way, the direct kernel and the numpy oracle."""
import numpy as np

import column_forms as cf
from stodynprog_amd import SysDescription, DPSolver
from stodynprog_amd.models import NormalLaw, SYNTH

# lattice sizes of the horizon of a family, k = 0 .. T - 1 (bellman_recursion runs k = T - 1 first): 16 = 2^4, 9 = 8 + 1,
# 1 (midpoint rule), 17 = 2^4 + 1 (capacity 32), 5 < 8, 15 = 2^4 - 1; steps 0 / 6 and 1 / 7 have the same box at
# drifts 6 steps apart
SIZES = (16, 9, 1, 17, 5, 15, 16, 9)
T = len(SIZES)
# (n_u, n_v) of the two controls of the reduced-array family: products SIZES
SIZES_2 = ((4, 4), (3, 3), (1, 1), (17, 1), (5, 1), (5, 3), (2, 8), (9, 1))
# constants looked up as data[k]: a sign change between steps 0 and 1, 0.0 and -0.0, negative values, and steps 4 and 5
# equal to another literal of the models (0.15, the weight of u * u in the cost)
TIME_DATA = (0.3, -0.2, 0.0, -0.0, 0.15, 0.15, -0.4, 0.5)
EQUAL_LITERAL = 0.15


def capacity(n):
    """the control table's room for a lattice of n controls in a time-dependent plan (solver.py: n_controls)"""
    return 1 << max(int(n) - 1, 0).bit_length()


def widths(step, sizes):
    """box widths that make a lattice of `step` take `sizes` points: ceil(w / step) + 1 = n, or w / step < 0.1"""
    return np.array([0.05 * step if n == 1 else step * (n - 1.5) for n in sizes])


# ----------------------------------------------------------------------------------------------------------------------
# the families (the builders of tests/test_gpu_call_to_call.py with a time index)

def storage(n_E=21, n_P=13, n_w=5, E_max=4.0, noise=0.0, dtype=np.float64, data=False, drift=0.15):
    """a stock and an AR(1) exogenous process (storage-separable); `noise`: the perturbation also reaches the stock
    through a final sum (the shifted lattice); `data`: the stock's inflow and the price of u are TIME_DATA[k]"""
    s = SysDescription((2, 1, 1), stationnary=False, name='time-dependent storage')
    d = np.array(TIME_DATA)
    if data:
        lead = lambda k, e: e + d[k]
        price = lambda k: d[k]
    else:
        lead = lambda k, e: e + drift * (k - 3)
        price = lambda k: 0.1 * k - 0.35
    if noise:
        s.dyn = lambda k, e, p, u, w: ((lead(k, e) + (1.1 * u - 0.02 * abs(u))) - noise * w,
                                       (0.75 * p + 0.05 * k) + w)
    else:
        s.dyn = lambda k, e, p, u, w: (lead(k, e) + (1.1 * u - 0.02 * abs(u)), (0.75 * p + 0.05 * k) + w)
    s.cost = lambda k, e, p, u, w: 0.01 * e + (((p - u) * (p - u) + 0.15 * u * u) + price(k) * u)
    wu = widths(0.125, SIZES)
    s.control_box = lambda k, e, p: ((-1.0, -1.0 + wu[k]),)
    s.perturb_laws = [NormalLaw(0, 0.3)]
    solver = DPSolver(s, dtype=dtype)
    solver.discretize_state(0, E_max, n_E, -2, 2, n_P)
    solver.discretize_perturb(-0.9, 0.9, n_w)
    solver.control_steps = (0.125,)
    return solver


def line():
    """one state, x' = (x + 0.9 u) - 0.3 w: the filtered line kernel is stationary-only, the direct kernel runs"""
    s = SysDescription((1, 1, 1), stationnary=False, name='time-dependent line')
    s.dyn = lambda k, x, u, w: ((x + 0.1 * (k - 3)) + 0.9 * u - 0.3 * w,)
    s.cost = lambda k, x, u, w: (0.15 * u * u + (0.1 * k - 0.35) * u) + 0.1 * x * x
    wu = widths(0.125, SIZES)
    s.control_box = lambda k, x: ((-1.0, -1.0 + wu[k]),)
    s.perturb_laws = [NormalLaw(0, 0.3)]
    solver = DPSolver(s)
    solver.discretize_state(-4, 4, 65)
    solver.discretize_perturb(-0.9, 0.9, 9)
    solver.control_steps = (0.125,)
    solver.LINE_MIN_CELLS = 0                    # (the line kernel would take this size if it were stationary)
    return solver


def reservoirs(data=False):
    """two stocks driven by the controls next to an exogenous inflow (the reduced-array sweep); both control boxes
    change with k, their lattices multiply to SIZES"""
    s = SysDescription((3, 2, 1), stationnary=False, name='time-dependent reservoirs')
    d = np.array(TIME_DATA)
    inflow = (lambda k: d[k]) if data else (lambda k: 0.1 * (k - 3))
    s.dyn = lambda k, a, b, y, u, v, w: ((a + inflow(k)) + 0.5 * (0.7 + 0.5 * y) - 1.1 * u, b + 1.1 * u - v,
                                         (0.3 + 0.02 * k) + 0.75 * (y - 0.3) + w)
    s.cost = lambda k, a, b, y, u, v, w: ((v - 0.8) * (v - 0.8) + 0.15 * (u - v) * (u - v) + (0.1 * k - 0.35) * u
                                          + 4.0 * np.where(a > 1.7, a - 1.7, 0.0 * a)
                                          + 8.0 * np.where(b < 0.3, 0.3 - b, 0.0 * b))
    wu = widths(0.125, [n for n, _ in SIZES_2])
    wv = widths(0.25, [n for _, n in SIZES_2])
    s.control_box = lambda k, a, b, y: ((0., wu[k]), (0., wv[k]))
    s.perturb_laws = [NormalLaw(0, 0.1)]
    solver = DPSolver(s)
    solver.discretize_state(0., 2., 16, 0., 2., 12, -0.4, 0.8, 8)
    solver.discretize_perturb(-0.3, 0.3, 5)
    solver.control_steps = (0.125, 0.25)
    return solver


def coupled():
    """the control also reaches the trailing state variables (a table per control)"""
    s = SysDescription((3, 1, 1), stationnary=False, name='time-dependent coupled')
    s.dyn = lambda k, x0, x1, x2, u, w: ((x0 + 0.02 * (k - 3)) + 0.11 * u,
                                         (0.05 + 0.01 * k) + 0.75 * x1 + 0.1 * x2 + w + 0.1 * u,
                                         0.05 + 0.1 * x1 + 0.8 * x2 + 0.5 * w)
    s.cost = lambda k, x0, x1, x2, u, w: ((1.8 * x1 - 0.9 - u) * (1.8 * x1 - 0.9 - u) + 0.15 * u * u
                                          + (0.1 * k - 0.35) * u) + 0.25 * x0
    wu = widths(0.125, SIZES)
    s.control_box = lambda k, x0, x1, x2: ((-1.0, -1.0 + wu[k]),)
    s.perturb_laws = [NormalLaw(0, 0.05)]
    solver = DPSolver(s)
    solver.discretize_state(0, 1, 12, 0, 1, 10, 0, 1, 9)
    solver.discretize_perturb(-0.15, 0.15, 7)
    solver.control_steps = (0.125,)
    return solver


def untraceable():
    """the storage model with a dynamics that needs a concrete array (np.shape): the tabulated mode"""
    s = storage()

    def dyn(k, e, p, u, w):
        shape = np.shape(u)
        return (e + 0.15 * (k - 3) + (1.1 * np.asarray(u).reshape(shape) - 0.02 * abs(u)), (0.75 * p + 0.05 * k) + w)
    s.sys.dyn = dyn
    return s


class Family(object):
    """`make()` -> a fresh solver; `kernel` its setting; `info`: what backend_info says at every step; `units`: the
    distinct code objects the horizon compiles; `ref`: 'oracle' (8-byte reals, bit for bit, every node), 'oracle sampled'
    (the same on column_forms.sample_nodes) or 'oracle32' (4-byte reals, within 1e-5 of the 8-byte oracle from a smooth
    J_fin); `filtered`: the family has a certified filter to switch off"""
    def __init__(self, name, make, kernel, info, units, ref='oracle', filtered=True, sizes=SIZES, form=None):
        self.name, self.make, self.kernel, self.info, self.units = name, make, kernel, dict(info), units
        self.ref, self.filtered, self.sizes = ref, filtered, tuple(sizes)
        self.form = form or info.get('kernel')          # policies.family_of of every step's plan
        # the unit carries a control table sized by the capacity (the column family's reduced table)
        self.table = self.form == 'column' and info.get('filter_form') in ('reduced table', 'shifted lattice')

    def __repr__(self):
        return self.name

    def compared(self):
        """{label: solver settings} of the kernels the family is compared with: the same family without the filter
        (every control the long way) where it has one, the direct kernel where it is not the direct kernel"""
        out = {}
        if self.filtered:
            out['long way'] = dict(certified_filter=False)
        if self.kernel != 'generic' and self.form != 'tabulated':
            out['direct kernel'] = dict(kernel='generic')
        return out

    def solver(self, **kw):
        s = self.make()
        s.kernel = self.kernel
        for k, v in kw.items():
            setattr(s, k, v)
        return s


_TIME = dict(time_specialized=True)
_SYMBOLIC = dict(time_specialized=False, lifted_constants=0)
# units: the distinct capacities (1, 8, 16, 32) for the column family; lanes per node (1, 8, 16, 32) for the direct,
# staged and per-control kernels (codegen.lanes_for); one reduced-array unit (a lane per node).  With data[k] the same:
# every step's constants are lifted, 0.0, -0.0 and the data equal to another literal included (no two leaves merge)
FAMILIES = [
    Family('column', storage, 'column',
           dict(kernel='column', filter_form='reduced table', certified_filter=True, **_SYMBOLIC), 4),
    Family('column fp32', lambda: storage(dtype=np.float32), 'column',
           dict(kernel='column', filter_form='reduced table', certified_filter=True, **_SYMBOLIC), 4, ref='oracle32'),
    Family('shifted lattice', lambda: storage(noise=0.05), 'column',
           dict(kernel='column', filter_form='shifted lattice', **_SYMBOLIC), 4),
    Family('line', line, 'auto', dict(kernel='generic', **_SYMBOLIC), 4, filtered=False),
    # (the reduced-array sweep has no unfiltered form: kernel = 'lead' needs the filter)
    Family('lead', reservoirs, 'lead', dict(kernel='lead', filter_form='reduced array', **_SYMBOLIC), 1,
           sizes=[a * b for a, b in SIZES_2], filtered=False),
    Family('row window', lambda: storage(n_E=2048, n_P=5, n_w=11, E_max=20.0, drift=1.5), 'column',
           dict(kernel='column', table_per_control=False, **_SYMBOLIC), 4, ref='oracle sampled', form='row window'),
    Family('table per control', coupled, 'column', dict(kernel='column', table_per_control=True, **_SYMBOLIC), 4,
           form='table per control'),
    Family('staged', storage, 'staged', dict(kernel='staged', **_SYMBOLIC), 4, filtered=False),
    Family('generic', storage, 'generic', dict(kernel='generic', **_SYMBOLIC), 4, filtered=False),
    # constants looked up as data[k]
    Family('column data[k]', lambda: storage(data=True), 'column',
           dict(kernel='column', filter_form='reduced table', **_TIME), 4),
    Family('shifted lattice data[k]', lambda: storage(noise=0.05, data=True), 'column',
           dict(kernel='column', filter_form='shifted lattice', **_TIME), 4),
    Family('lead data[k]', lambda: reservoirs(data=True), 'lead', dict(kernel='lead', filter_form='reduced array', **_TIME), 1,
           sizes=[a * b for a, b in SIZES_2], filtered=False),
    Family('staged data[k]', lambda: storage(data=True), 'staged', dict(kernel='staged', **_TIME), 4, filtered=False),
    Family('generic data[k]', lambda: storage(data=True), 'generic', dict(kernel='generic', **_TIME), 4, filtered=False),
    # no trace at all: the host evaluates the callables node by node, the device reduces
    Family('tabulated', untraceable, 'auto', dict(mode='tabulated'), 0, filtered=False, form='tabulated'),
]
FAMILY = {f.name: f for f in FAMILIES}


# ----------------------------------------------------------------------------------------------------------------------
# the column forms with a time index

def synthetic3d_t(case, sizes, geometry, dtype=None, kernel='auto', certified_filter=True, drift=0.02):
    """models.synthetic3d with a time index, discretised like column_forms.Case.solver: the lattice of step k has
    sizes[k] points of the case's control step"""
    p = SYNTH
    b, a11, a12, a21, a22, c = p['b'], p['a11'], p['a12'], p['a21'], p['a22'], p['c']
    m1, m2, k1, k0, eps, kx = p['m1'], p['m2'], p['k1'], p['k0'], p['eps'], p['kx']
    noise = case.noise
    step = 2. / (case.n_u - 1.5)
    s = SysDescription((3, 1, 1), stationnary=False, name='time-dependent synthetic 3-D')

    def dyn(k, x0, x1, x2, u, w):
        x0n = (x0 + drift * (k - 2)) + b * u
        if noise:
            x0n = x0n - noise * w
        return (x0n, (m1 + 0.01 * k) + a11 * x1 + a12 * x2 + w, m2 + a21 * x1 + a22 * x2 + c * w)

    def cost(k, x0, x1, x2, u, w):
        e = (k1 * x1 - k0) - u
        return kx * x0 + ((e * e + eps * (u * u)) + (0.05 * k - 0.1) * u)
    s.dyn, s.cost = dyn, cost
    wu = widths(step, sizes)
    s.control_box = lambda k, x0, x1, x2: ((-1.0, -1.0 + wu[k]),)
    s.perturb_laws = [NormalLaw(0, p['sigma'])]
    solver = DPSolver(s, dtype=case.dtype if dtype is None else dtype)
    n1, n2 = cf.GEOMETRIES[geometry]
    solver.discretize_state(0, 1, case.n0, 0, 1, n1, 0, 1, n2)
    solver.discretize_perturb(-3 * p['sigma'], 3 * p['sigma'], case.n_w)
    solver.control_steps = (step,)
    solver.kernel = kernel
    solver.certified_filter = certified_filter
    return solver


class Case(object):
    """column_forms case `form` over a horizon of lattices `sizes` (k = 0 ..); `utab_n`: the SDP_COL_UTAB_N every step
    plans (None: no control table), the capacity; `below`: the steps with fewer controls than that; one code object"""
    def __init__(self, form, sizes, utab_n, below):
        self.form = {c.name: c for c in cf.CASES}[form]
        self.name, self.sizes, self.utab_n, self.below = form, tuple(sizes), utab_n, tuple(below)
        self.units = 1
        self.dtype, self.hold, self.geometries = self.form.dtype, self.form.hold, self.form.geometries

    def __repr__(self):
        return self.name

    def claims(self, geometry):
        """the macros of every step's unit: the form's, with the capacity for its control table"""
        c = cf.claims(self.form, geometry)
        c['SDP_COL_UTAB_N'] = None if self.utab_n is None else str(self.utab_n)
        return c

    @property
    def debug(self):
        return self.form.debug

    def solver(self, geometry, **kw):
        return synthetic3d_t(self.form, self.sizes, geometry, **kw)


CASES = [
    Case('hold_8x2x4', (64, 57, 63, 49), 64, below=(1, 2, 3)),
    Case('hold_8x2x4_noise', (64, 57, 63, 49), 64, below=(1, 2, 3)),
    Case('hold_16x1x4_u200', (200, 129, 255, 193), 256, below=(0, 1, 2, 3)),
    # (blocks of 8: 8, 6, 5 and 8 of the table's 8, the last one short at steps 0, 1, 2)
    Case('bnb_u57', (57, 41, 33, 64), 64, below=(0, 1, 2)),
    Case('res_n192', (64, 57, 63, 49), 64, below=(1, 2, 3)),
    Case('full_n500', (64, 57, 63, 49), 64, below=(1, 2, 3)),
    Case('res1024_u301_noise', (301, 257, 300, 289), None, below=()),
    Case('f32_n600', (64, 57, 63, 33), 64, below=(1, 2, 3)),
    Case('f32_n512_u601_no_table', (601, 513, 600, 577), None, below=()),
]
PAIRS = [(c, g) for c in CASES for g in c.geometries]
