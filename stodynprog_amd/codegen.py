"""HIP source generation for a traced model.

Turns the expression DAG recorded by trace.py into the device function
`sdp_model_cell` (one statement per recorded operator, in recording order) and
wraps it in a translation unit that includes the hand-written kernels of
csrc/sdp_sweep_kernel.h.  The unit is compiled to a gfx950 code object with
    hipcc --genco --offload-arch=gfx950 -O3 -ffp-contract=off
so that every operator is one IEEE operation, as in numpy on the host
(reference stodynprog.py:674-677 evaluates the same expressions with numpy).
"""
import collections
import hashlib
import re
import math
import os

import numpy as np

from .trace import TracedModel, DEP_X

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'csrc')
MAX_PERTURB = 4          # perturbation variables of a generated unit (perturb.MAX_PERTURB)


# ---------------------------------------------------------------------------
# Diagnostic / A-B switches.  The product has none: nothing in this module reads
# the environment.  Tests and the tools under tools/ hand an explicit dict
# (`DPSolver.debug_defines`, `bench.py --debug-define K=V`) to the planning
# functions below as `debug`; the names are those of the macros of csrc/*.h they
# set (plus a few planning switches: SDP_COL_FILTER / SDP_COL_SHIFT / SDP_COL_UTAB /
# SDP_LEAD_FILTER = 0 switch a form off, SDP_COL_THREADS / SDP_COL_WCHUNK /
# SDP_STG_CU / SDP_COL_WPAIR force a shape).  A solver that carries such a dict says
# so in backend_info['debug_defines'], and bench.py in config.debug_defines.
# Only switches that a header still reads are listed: the A/B forks whose outcome is settled (docs/NOTEBOOK.md,
# "Retired switches") are gone from the headers, and their names are refused here like any typo.
# ---------------------------------------------------------------------------
# macros copied into the generated unit as they are (integers): tuning parameters and the forms tests and tools select
DEBUG_INT_MACROS = ('SDP_COL_MIN_WAVES', 'SDP_COL_BATCH', 'SDP_COL_UNROLL_U', 'SDP_COL_UNROLL_W',
                    'SDP_COL_A_GROUP', 'SDP_COL_FILTER_UNROLL', 'SDP_COL_FILTER_TOP2', 'SDP_COL_FILTER_RUNROLL',
                    'SDP_COL_A_WIDE_LOADS', 'SDP_COLU_WIDE_LOADS', 'SDP_COLU_A_GROUP',
                    'SDP_COL_TAIL_HOLD', 'SDP_SHORT_GROUP', 'SDP_BNB_CHUNK', 'SDP_BNB_LEAN')
# the reductions of the plain resident-chunk form (table_phase_plan): 0 leaves an item out of the plan -- the A/B switches
TABLE_PHASE_MACROS = ('SDP_COL_REDUCE_FUSED', 'SDP_COL_DMAX_HI')
# (SDP_COL_LEAN2 = 0 keeps the resident-chunk kernel on the first pass of section 3.1c: an A/B switch of short_pass_source)
# (SDP_COL_WRES is a planning switch: it sizes the LDS image -- column_config)
# (SDP_BNB_UNIFORM = 0 keeps the branch and bound on the bound stage that locates every block end per node: an A/B switch)
# (SDP_BNB_LEAN = 0 keeps the branch and bound's bookkeeping of before round 9 -- the 64-bit block mask, the per-control
#  selects of the evaluation: an A/B switch that nothing plans, copied into the unit only when a caller sets it)
# (SDP_BNB_UNIFORM_EVAL = 0 keeps the branch and bound on the evaluation that locates every control per node, with its radius
#  of before: an A/B switch of uniform_eval_plan)
# every name a `debug` dict may carry (a typo must not pass silently)
DEBUG_NAMES = frozenset(DEBUG_INT_MACROS + (
    'SDP_STAMP', 'SDP_NO_POW2', 'SDP_EXTRA_DEFINES', 'SDP_COL_FILTER_SCALE', 'SDP_LEAD_FILTER_SCALE',
    'SDP_LEAD_UNROLL', 'SDP_COL_A_LW', 'SDP_COL_FILTER', 'SDP_COL_SHIFT', 'SDP_COL_UTAB', 'SDP_LEAD_FILTER',
    'SDP_COL_THREADS', 'SDP_COL_WCHUNK', 'SDP_STG_CU', 'SDP_COL_WPAIR', 'SDP_COL_WRES', 'SDP_COL_LEAN2', 'SDP_COL_BNB',
    'SDP_LINE_FILTER', 'SDP_LINE_FILTER_SCALE', 'SDP_LINE_TOP2', 'SDP_BNB_UNIFORM', 'SDP_BNB_UNIFORM_EVAL')
    + TABLE_PHASE_MACROS)


def check_debug(debug):
    """normalised copy of a debug dict (values as strings), or None; unknown names raise"""
    if not debug:
        return None
    unknown = sorted(set(debug) - DEBUG_NAMES)
    if unknown:
        raise ValueError('unknown debug define(s): {}'.format(', '.join(unknown)))
    return {k: str(v) for k, v in debug.items() if v is not None and str(v) != ''} or None


def _dbg(debug, name, default=None):
    if not debug:
        return default
    v = debug.get(name)
    return default if v is None or str(v) == '' else str(v)

_BIN_INFIX = {'add': '+', 'sub': '-', 'mul': '*', 'div': '/',
              'lt': '<', 'le': '<=', 'gt': '>', 'ge': '>=', 'eq': '==', 'ne': '!=',
              'and': '&&', 'or': '||', 'xor': '!='}
_FUNC1 = {'abs': 'fabs', 'sqrt': 'sqrt', 'floor': 'floor', 'ceil': 'ceil', 'trunc': 'trunc',
          'rint': 'rint', 'exp': 'exp', 'exp2': 'exp2', 'expm1': 'sdp_npexpm1', 'log': 'log',
          'log2': 'log2', 'log10': 'log10', 'log1p': 'sdp_nplog1p', 'sin': 'sin', 'cos': 'cos',
          'tan': 'tan', 'asin': 'asin', 'acos': 'acos', 'atan': 'atan', 'sinh': 'sinh',
          'cosh': 'cosh', 'tanh': 'tanh', 'cbrt': 'cbrt'}
_FUNC2 = {'pow': 'pow', 'atan2': 'atan2', 'hypot': 'hypot', 'fmod': 'fmod',
          'min': 'sdp_npmin', 'max': 'sdp_npmax', 'fmin': 'sdp_npfmin', 'fmax': 'sdp_npfmax',
          'pymod': 'sdp_nppymod', 'floordiv': 'sdp_npfloordiv'}


def real_literal(value):
    """Exact C++ literal for a double constant (cast to the kernel's real)."""
    if math.isnan(value):
        return '(sdp_real)NAN'
    if math.isinf(value):
        return '(sdp_real)INFINITY' if value > 0 else '(-(sdp_real)INFINITY)'
    return '(sdp_real)({})'.format(float(value).hex())


def _emit_node(n, name, param_index=None, vector_w=False):
    a = [name(x) for x in n.args]
    op = n.op
    if op == 'const':
        if param_index is not None and n.id in param_index:
            return 'sdp_model_prm[{}]'.format(param_index[n.id])     # lifted constant
        return real_literal(n.value)
    if op == 'bconst':
        return 'true' if n.value else 'false'
    if op == 'var':
        v = n.value
        if v == 't':
            return 't'
        if v[0] == 'w' and vector_w:         # several perturbation variables: the model entry takes them as w[SDP_NW]
            return 'w[{}]'.format(v[1:])
        return '{}[{}]'.format(v[0], v[1:]) if v[0] in 'xu' else 'w'
    if op in _BIN_INFIX:
        return '({} {} {})'.format(a[0], _BIN_INFIX[op], a[1])
    if op in _FUNC1:
        return '{}({})'.format(_FUNC1[op], a[0])
    if op in _FUNC2:
        return '{}({}, {})'.format(_FUNC2[op], a[0], a[1])
    if op == 'neg':
        return '(-{})'.format(a[0])
    if op == 'square':
        return '({0} * {0})'.format(a[0])
    if op == 'recip':
        return '((sdp_real)1 / {})'.format(a[0])
    if op == 'sign':
        return 'sdp_npsign({})'.format(a[0])
    if op == 'not':
        return '(!{})'.format(a[0])
    if op == 'isnan':
        return '({0} != {0})'.format(a[0])
    if op == 'isinf':
        return '(fabs({}) == (sdp_real)INFINITY)'.format(a[0])
    if op == 'isfinite':
        return '(fabs({}) < (sdp_real)INFINITY)'.format(a[0])
    if op in ('select', 'bselect'):
        return '({} ? {} : {})'.format(a[0], a[1], a[2])
    if op == 'b2r':
        return '({} ? (sdp_real)1 : (sdp_real)0)'.format(a[0])
    if op == 'interp1':
        return 'sdp_interp1_{}({})'.format(n.value, a[0])
    raise NotImplementedError(op)


# np.interp on the device: numpy's arr_interp (compiled_base.c) restated --
# range checks first (binary_search_with_guess), the largest j with
# xp[j] <= x, then the same three floating-point operations and the same
# fall-backs for non-finite results.
INTERP_SOURCE = '''SDP_DEV sdp_real sdp_np_interp(sdp_real x, const sdp_real *xp, const sdp_real *fp, int n,
                                sdp_real left, sdp_real right)
{
    if (n == 1) return x < xp[0] ? left : (x > xp[0] ? right : fp[0]);
    if (x != x) return x;
    if (x > xp[n - 1]) return right;
    if (x < xp[0]) return left;
    int imin = 0, imax = n;
    while (imin < imax) {
        const int imid = imin + ((imax - imin) >> 1);
        if (x >= xp[imid]) imin = imid + 1; else imax = imid;
    }
    const int j = imin - 1;
    if (j == n - 1) return fp[j];
    if (xp[j] == x) return fp[j];
    const sdp_real slope = (fp[j + 1] - fp[j]) / (xp[j + 1] - xp[j]);
    sdp_real r = slope * (x - xp[j]) + fp[j];
    if (r != r) {
        r = slope * (x - xp[j + 1]) + fp[j + 1];
        if (r != r && fp[j] == fp[j + 1]) r = fp[j];
    }
    return r;
}
'''


def interp_tables_source(model):
    """Tables and per-table wrappers of the np.interp nodes of `model`."""
    used = sorted({n.value for n in model.live_nodes() if n.op == 'interp1'})
    if not used:
        return ''
    out = [INTERP_SOURCE]
    for tid in used:
        xp, fp, left, right = model.graph.tables[tid][:4]
        out.append('__constant__ sdp_real sdp_tabx_{}[{}] = {{{}}};'.format(
            tid, xp.size, ', '.join(real_literal(v) for v in xp)))
        out.append('__constant__ sdp_real sdp_tabf_{}[{}] = {{{}}};'.format(
            tid, fp.size, ', '.join(real_literal(v) for v in fp)))
        out.append('SDP_DEV sdp_real sdp_interp1_{0}(sdp_real x)\n{{\n    return sdp_np_interp('
                   'x, sdp_tabx_{0}, sdp_tabf_{0}, {1}, {2}, {3});\n}}'.format(
                       tid, xp.size, real_literal(left), real_literal(right)))
    return '\n'.join(out) + '\n'


def _emit_body(model, nodes, lines, names=None):
    """statements for `nodes` (topological order); returns the name map
    (`names`: nodes that already have a name -- leaves of a partial evaluation)"""
    names = dict(names or {})

    def name(n):
        return names[n.id]

    for n in nodes:
        expr = _emit_node(n, name, getattr(model, 'param_index', None), getattr(model, 'n_perturb', 0) >= 2)
        if n.op in ('const', 'bconst', 'var'):
            names[n.id] = expr              # inline leaves
            continue
        var = 'v{}'.format(n.id)
        ctype = 'bool' if n.kind == 'b' else 'sdp_real'
        lines.append('    const {} {} = {};'.format(ctype, var, expr))
        names[n.id] = var
    return names


def model_function_source(model, at=False):
    """C++ text of sdp_model_cell for a TracedModel: the whole dyn + cost.
    at: sdp_model_cell_at instead, the same body with the lifted constants read from a row `prm` the caller hands
    over (csrc/sdp_horizon_kernel.h: a table with one row per time step) instead of the unit's __constant__ array."""
    assert isinstance(model, TracedModel)
    if model.n_perturb > MAX_PERTURB:
        raise NotImplementedError('{} perturbation variables: at most {} are supported'.format(model.n_perturb, MAX_PERTURB))
    # (several perturbation variables, csrc/sdp_multiw_kernel.h: variable w<i> is w[i])
    w_arg = 'const sdp_real *w' if model.n_perturb >= 2 else 'sdp_real w'
    if at:
        lines = ['SDP_DEV void sdp_model_cell_at(const sdp_real *x, const sdp_real *u, {},'.format(w_arg),
                 '                               sdp_real t, const sdp_real *__restrict__ prm, sdp_real *xn, sdp_real &g)',
                 '{',
                 '    (void)x; (void)u; (void)w; (void)t; (void)prm;']
        body = []
        names = _emit_body(model, model.live_nodes(), body)
        lines += [ln.replace('sdp_model_prm[', 'prm[') for ln in body]
        names = {k: v.replace('sdp_model_prm[', 'prm[') for k, v in names.items()}
    else:
        lines = ['SDP_DEV void sdp_model_cell(const sdp_real *x, const sdp_real *u, {},'.format(w_arg),
                 '                            sdp_real t, sdp_real *xn, sdp_real &g)',
                 '{',
                 '    (void)x; (void)u; (void)w; (void)t;']
        names = _emit_body(model, model.live_nodes(), lines)
    for k, n in enumerate(model.x_next):
        lines.append('    xn[{}] = {};'.format(k, names[n.id]))
    lines.append('    g = {};'.format(names[model.cost.id]))
    lines.append('}')
    return '\n'.join(lines)


def separable_functions_source(model):
    """C++ text of the three slices used by the column kernel
    (csrc/sdp_column_kernel.h) for a storage-separable model."""
    assert model.column_shareable
    out = []
    lines = ['SDP_DEV sdp_real sdp_model_lead(const sdp_real *x, const sdp_real *u, sdp_real w,',
             '                                sdp_real t)',
             '{', '    (void)x; (void)u; (void)w; (void)t;']
    names = _emit_body(model, model.slice_nodes([model.x_next[0]]), lines)
    lines += ['    return {};'.format(names[model.x_next[0].id]), '}']
    out.append('\n'.join(lines))
    lines = ['SDP_DEV void sdp_model_trail(const sdp_real *x, const sdp_real *u, sdp_real w, sdp_real t,',
             '                                sdp_real *xn)',
             '{', '    (void)x; (void)u; (void)w; (void)t;']
    names = _emit_body(model, model.slice_nodes(model.x_next[1:]), lines)
    for k, n in enumerate(model.x_next[1:]):
        lines.append('    xn[{}] = {};'.format(k + 1, names[n.id]))
    lines.append('}')
    out.append('\n'.join(lines))
    lines = ['SDP_DEV sdp_real sdp_model_cost(const sdp_real *x, const sdp_real *u, sdp_real w,',
             '                                sdp_real t)',
             '{', '    (void)x; (void)u; (void)w; (void)t;']
    names = _emit_body(model, model.slice_nodes([model.cost]), lines)
    lines += ['    return {};'.format(names[model.cost.id]), '}']
    out.append('\n'.join(lines))
    split = model.lead_split()
    if split is not None:
        # x0' = a(x, u) +- b_1(x_1.., w) +- b_2 ..: a, the sum B of the signed b_i in the reference's order, and
        # the sum of the |b_i| (for the error bound), each b_i with the reference's own operations
        # (SDP_COL_SHIFT of csrc/sdp_colfilter_kernel.h)
        a_node, terms = split
        lines = ['SDP_DEV sdp_real sdp_model_lead_a(const sdp_real *x, const sdp_real *u, sdp_real t)',
                 '{', '    (void)x; (void)u; (void)t;']
        names = _emit_body(model, model.slice_nodes([a_node]), lines)
        lines += ['    return {};'.format(names[a_node.id]), '}']
        out.append('\n'.join(lines))
        chain = model.lead_split_chain()
        if chain is not None:
            # a chain of sums in another nesting, regrouped (TracedModel.lead_split): a is the sum of the chain's w-free
            # leaves, no value of the reference's; the sum of their magnitudes bounds what the regrouping costs
            # (SDP_COL_SHIFT_CHAIN of csrc/sdp_colfilter_kernel.h)
            leaves = [n for n, _ in chain[0]]
            lines = ['SDP_DEV sdp_real sdp_model_lead_aabs(const sdp_real *x, const sdp_real *u, sdp_real t)',
                     '{', '    (void)x; (void)u; (void)t;']
            names = _emit_body(model, model.slice_nodes(leaves), lines)
            lines += ['    return {};'.format(' + '.join('fabs({})'.format(names[n.id]) for n in leaves)), '}']
            out.append('\n'.join(lines))
        lines = ['SDP_DEV void sdp_model_lead_b(const sdp_real *x, sdp_real w, sdp_real t, sdp_real &b, sdp_real &babs)',
                 '{', '    (void)x; (void)w; (void)t;']
        names = _emit_body(model, model.slice_nodes([b for b, _ in terms]), lines)
        b0, s0 = terms[0]
        lines.append('    b = {}{};'.format('-' if s0 < 0 else '', names[b0.id]))
        lines.append('    babs = fabs({});'.format(names[b0.id]))
        for bn, sg in terms[1:]:
            lines.append('    b = b {} {};'.format('+' if sg > 0 else '-', names[bn.id]))
            lines.append('    babs = babs + fabs({});'.format(names[bn.id]))
        lines.append('}')
        out.append('\n'.join(lines))
    return '\n\n'.join(out)


def lead_functions_source(model, m, order=None):
    """C++ text of the slices csrc/sdp_lead_kernel.h uses for a model with `m` controlled stocks next to an
    exogenous process (TracedModel.controlled_order): `order` lists the state variables, stocks first
    (default: as they are listed)."""
    d = model.n_state
    order = tuple(order) if order is not None else tuple(range(d))
    leads = [model.x_next[k] for k in order[:m]]
    trails = [model.x_next[k] for k in order[m:]]
    out = []
    lines = ['SDP_DEV void sdp_model_leads(const sdp_real *x, const sdp_real *u, sdp_real t, sdp_real *xl)',
             '{', '    (void)x; (void)u; (void)t;']
    names = _emit_body(model, model.slice_nodes(leads), lines)
    for k, n in enumerate(leads):
        lines.append('    xl[{}] = {};'.format(k, names[n.id]))
    lines.append('}')
    out.append('\n'.join(lines))
    if m < d:
        lines = ['SDP_DEV void sdp_model_trails(const sdp_real *x, sdp_real w, sdp_real t, sdp_real *xt)',
                 '{', '    (void)x; (void)w; (void)t;']
        names = _emit_body(model, model.slice_nodes(trails), lines)
        for k, n in enumerate(trails):
            lines.append('    xt[{}] = {};'.format(k, names[n.id]))
        lines.append('}')
        out.append('\n'.join(lines))
    lines = ['SDP_DEV sdp_real sdp_model_cost(const sdp_real *x, const sdp_real *u, sdp_real w,',
             '                                sdp_real t)',
             '{', '    (void)x; (void)u; (void)w; (void)t;']
    names = _emit_body(model, model.slice_nodes([model.cost]), lines)
    lines += ['    return {};'.format(names[model.cost.id]), '}']
    out.append('\n'.join(lines))
    return '\n\n'.join(out)


def lead_filter_applies(model, dtype, min_axes=2, debug=None):
    """Several controlled state variables next to an exogenous process (TracedModel.controlled_axes
    >= 2; one stock is the column kernel's case), a perturbation that does not reach them (the cost may see
    it), 8-byte reals (a form for 4-byte reals existed in round 5: its radius of ~1e-5 of the values kept so many
    controls that the sweep was 3 x SLOWER than every control the long way, 8.9 against 2.6 ms; removed in round 6):
    the node-order sweep with the certified filter on an array reduced over w (csrc/sdp_lead_kernel.h).  Returns the
    number of controlled axes, or 0.  (`debug`: SDP_LEAD_FILTER = 0 switches it off, A/B runs.)"""
    if _dbg(debug, 'SDP_LEAD_FILTER', '1') == '0':
        return 0
    if model.n_perturb != 1 or np.dtype(dtype).itemsize != 8:
        return 0
    m = model.controlled_axes()
    return int(m) if m is not None and m >= min_axes else 0


def lead_order(model, dtype, debug=None):
    """(m, order) for the reduced-array sweep of a model whose stocks are NOT listed first (the order of the
    state variables is the user's: reference stodynprog.py:119-131), or None: TracedModel.controlled_order
    with at least one exogenous variable, 8-byte reals, one perturbation."""
    if _dbg(debug, 'SDP_LEAD_FILTER', '1') == '0' or model.n_perturb != 1 or np.dtype(dtype).itemsize != 8:
        return None
    co = model.controlled_order()
    if co is None or co[1] == tuple(range(model.n_state)) or co[0] >= model.n_state:
        return None
    return co


UTAB_MAX_VALUES = 4          # tabulated sub-expressions per control
UTAB_MAX_BYTES = 4096        # per parity buffer of the table in LDS


def control_table_plan(model, dtype, per_node, max_controls, debug=None):
    """Can the column-uniform sub-expressions of x0' and of the cost be tabulated once per
    (column, control) (SDP_COL_UTAB of csrc/sdp_colfilter_kernel.h)?  Needs a control lattice that
    is the same at every node (constant box) and small enough for LDS.  Returns the frontier
    nodes (TracedModel.control_uniform_frontier) or None.  (`debug`: SDP_COL_UTAB = 0 switches it
    off, A/B runs.)"""
    if _dbg(debug, 'SDP_COL_UTAB', '1') == '0' or per_node or model.cost_depends_on_w:
        return None
    lead = None
    if model.lead_depends_on_w:
        split = model.lead_split()
        if split is None:
            return None
        lead = split[0]
    fr = model.control_uniform_frontier(lead)
    if fr is None or len(fr) > UTAB_MAX_VALUES:
        return None
    if len(fr) * int(max_controls) * np.dtype(dtype).itemsize > UTAB_MAX_BYTES:
        return None
    return fr


def control_table_source(model, frontier):
    """C++ text of sdp_model_utab (the tabulated values of one control) and of
    sdp_model_lead_tab / sdp_model_cost_tab (x0' and the cost from them)."""
    slot = {n.id: k for k, n in enumerate(frontier)}
    out = []
    lines = ['SDP_DEV void sdp_model_utab(const sdp_real *x, const sdp_real *u, sdp_real t, sdp_real *tab)',
             '{', '    (void)x; (void)u; (void)t;']
    names = _emit_body(model, model.slice_nodes(frontier), lines)
    for n in frontier:
        lines.append('    tab[{}] = {};'.format(slot[n.id], names[n.id]))
    lines.append('}')
    out.append('\n'.join(lines))
    pre = {n.id: 'tab[{}]'.format(slot[n.id]) for n in frontier}
    split = model.lead_split() if model.lead_depends_on_w else None
    for fname, node in (('sdp_model_lead_tab', split[0] if split else model.x_next[0]),     # (shifted table: the w-free half)
                        ('sdp_model_cost_tab', model.cost)):
        lines = ['SDP_DEV sdp_real {}(const sdp_real *x, const sdp_real *tab, sdp_real t)'.format(fname),
                 '{', '    (void)x; (void)tab; (void)t;']
        names = _emit_body(model, model.slice_nodes_until([node], set(slot)), lines, pre)
        lines += ['    return {};'.format(names[node.id]), '}']
        out.append('\n'.join(lines))
    chain = model.lead_split_chain() if split else None
    if chain is not None:              # (a regrouped chain of sums: the sum of the w-free leaves' magnitudes, from the table too)
        leaves = [n for n, _ in chain[0]]
        lines = ['SDP_DEV sdp_real sdp_model_lead_aabs_tab(const sdp_real *x, const sdp_real *tab, sdp_real t)',
                 '{', '    (void)x; (void)tab; (void)t;']
        names = _emit_body(model, model.slice_nodes_until(leaves, set(slot)), lines, pre)
        lines += ['    return {};'.format(' + '.join('fabs({})'.format(names[n.id]) for n in leaves)), '}']
        out.append('\n'.join(lines))
    return '\n\n'.join(out)


def short_pass_source(model, frontier, macro='SDP_COL_LEAN2'):
    """C++ text for the short first pass of the resident-chunk kernel (SDP_COL_LEAN2 of csrc/sdp_colres_kernel.h), or
    None when the model does not have the shape: x0' = X(x, t) +- a, cost = K(x, t) +- h with a, h in the control
    table (TracedModel.additive_control_split).  X and K as functions of the node alone, the slots of a and h, and
    how they enter."""
    sp = model.additive_control_split(frontier)
    if sp is None:
        return None
    (x_node, a_slot, a_form), (k_node, h_slot, h_form) = sp['lead'], sp['cost']
    out = ['#define {} 1          // x0\' = X(x) +- a(u), cost = K(x) +- h(u): the short first pass'.format(macro),
           '#define SDP_LEAN2_A_SLOT {}'.format(int(a_slot)),
           '#define SDP_LEAN2_H_SLOT {}'.format(-1 if h_slot is None else int(h_slot)),
           '#define SDP_LEAN2_LEAD(X, A) {}'.format({'add': '((X) + (A))', 'sub': '((X) - (A))', 'rsub': '((A) - (X))'}[a_form]),
           '#define SDP_LEAN2_FORM {}            // 0: X + a, 1: X - a, 2: a - X'.format({'add': 0, 'sub': 1, 'rsub': 2}[a_form]),
           '#define SDP_LEAN2_A_FIXED {}         // a depends on the control alone: the same lattice of positions in every column'.format(
               0 if (frontier[int(a_slot)].deps & DEP_X) else 1),
           '#define SDP_LEAN2_HNEG {}           // the part of the cost that depends on the control enters negated (K - h)'.format(
               1 if (h_slot is not None and h_form == 'sub') else 0)]
    for fname, node in (('sdp_model_lead_x', x_node), ('sdp_model_cost_x', k_node)):
        lines = ['SDP_DEV sdp_real {}(const sdp_real *x, sdp_real t)'.format(fname), '{', '    (void)x; (void)t;']
        if node is None:
            lines += ['    return (sdp_real)0;', '}']
        else:
            names = _emit_body(model, model.slice_nodes([node]), lines)
            lines += ['    return {};'.format(names[node.id]), '}']
        out.append('\n'.join(lines))
    return '\n'.join(out)


def lanes_for(max_controls):
    """Lanes per state node: the power of two covering the largest control
    lattice, capped at the 64 lanes of a wavefront."""
    lanes = 1
    while lanes < max_controls and lanes < 64:
        lanes *= 2
    return lanes


def _prologue_lines(model, real, lanes, debug, peer_stores=False):
    """what every generated unit starts with: the type and shape macros, the diagnostic
    switches of an explicit `debug` dict (none in the product), the device helpers, the
    lifted constants, the interpolation tables and sdp_model_cell"""
    lines = ['// generated by stodynprog_amd.codegen -- do not edit',
             '#define SDP_REAL {}'.format(real),
             '#define SDP_D {}'.format(model.n_state),
             '#define SDP_NU {}'.format(model.n_control),
             '#define SDP_HAS_W {}'.format(1 if model.n_perturb else 0),
             '#define SDP_LANES {}'.format(int(lanes)),
             '#define SDP_PEER_STORES {}     // the backup kernels also store J into other ranks (direct exchange)'.format(
                 1 if peer_stores else 0)]
    if model.n_perturb >= 2:
        lines.append('#define SDP_NW {}         // perturbation variables: the kernels of sdp_multiw_kernel.h on their flat law'.format(
            int(model.n_perturb)))
    if _dbg(debug, 'SDP_STAMP') in ('1', '2', '3'):
        lines.append('#define SDP_STAMP {}     // diagnostic build: in-kernel clock stamps (tools/clock_probe.py, '
                     'tools/phase_probe.py)'.format(int(_dbg(debug, 'SDP_STAMP'))))
    if _dbg(debug, 'SDP_NO_POW2') == '1':
        lines.append('#define SDP_NO_POW2 1  // A/B: true division also for power-of-two spans')
    for kv in (_dbg(debug, 'SDP_EXTRA_DEFINES') or '').split(','):
        if '=' in kv:
            lines.append('#define {} {}   // SDP_EXTRA_DEFINES (diagnostic builds)'.format(*kv.split('=', 1)))
    lines += ['#include "sdp_device.h"', 'typedef SDP_REAL sdp_real;', '']
    if getattr(model, 'param_index', None):
        # lifted constants (TracedModel.lift_constants): set per launch through
        # sdp_problem_set_params; uniform loads from constant memory
        lines += ['#define SDP_NPARAMS {}'.format(len(model.param_index)),
                  'extern "C" { __constant__ sdp_real sdp_model_prm[SDP_NPARAMS]; }     // a definition', '']
    tables = interp_tables_source(model)
    if tables:
        lines.append(tables)
    lines += [model_function_source(model), '']
    if getattr(model, 'param_index', None):
        # the same model with the constants of a step of the caller's choice (sdp_simulate_h, sdp_montecarlo_h)
        lines += [model_function_source(model, at=True), '']
    return lines


def uniform_rows_axis(axis, dtype, n0=None):
    """Does node r of a column sit at row r of the stock axis, as the branch and bound's bound stage locates it?  The
    kernel forms the position of X_r as fl(fl(X_r - smin) k), k = fl((n - 1) / fl(X_last - smin)); here the product of the
    STORED values is taken exactly (rationals), the two roundings are bounded by 2^-52 of it each, and the sum has to stay
    within 2^-23 rows of r for every r -- half of what the kernel itself accepts when it checks the same thing, node by
    node, before it relies on it (SDP_BNB_UNIFORM of csrc/sdp_colres_kernel.h).  8-byte reals only."""
    from fractions import Fraction
    if np.dtype(dtype).itemsize != 8:
        return False
    x = np.asarray(axis, dtype=np.float64).ravel()
    n = x.size
    if n < 2 or (n0 is not None and n != int(n0)) or not np.all(np.isfinite(x)):
        return False
    span = x[-1] - x[0]
    if not (span > 0):
        return False
    k = Fraction(float(np.float64(n - 1) / span))
    smin, tol, u2 = Fraction(float(x[0])), Fraction(1, 2 ** 23), Fraction(1, 2 ** 51)
    for r in range(n):
        p = (Fraction(float(x[r])) - smin) * k
        if abs(p - r) + u2 * (abs(p) + 1) > tol:
            return False
    return True


def uniform_stage_model(model, frontier):
    """x0' = X +- a with X the stock ITSELF (not a function of it, of the column or of the time index): a node of row r
    then sits at row r wherever the stock axis is uniform -- what the uniform bound stage of the branch and bound needs
    of the model (the kernel checks the rows node by node all the same)"""
    sp = model.additive_control_split(frontier) if frontier is not None else None
    if sp is None:
        return False
    x_node, _, a_form = sp['lead']
    return bool(a_form in ('add', 'sub') and x_node is not None and x_node.op == 'var' and x_node.value == 'x0')


uniform_define = ('\n#define SDP_BNB_UNIFORM 1      // node r of a column sits at row r of the stock axis: the block ends of the '
                  'branch and bound at the same offsets in every lane')


def uniform_stage_reach(model, frontier, lattice, k_rows):
    """Rows of the stock axis that the control lattice reaches on either side of a node under x0' = x0 +- a(u): the
    largest |a| over the lattice (`lattice`: one array of values per control; a is evaluated with numpy on their
    product) times `k_rows`, or None where a is not a function of the controls alone."""
    from . import trace
    a_node = frontier[int(model.additive_control_split(frontier)['lead'][1])]
    mesh = np.meshgrid(*[np.asarray(v, dtype=float) for v in lattice], indexing='ij')
    env = {}
    with np.errstate(all='ignore'):
        for n in model.slice_nodes([a_node]):
            if n.op == 'var':
                if not (isinstance(n.value, str) and n.value[0] == 'u'):
                    return None
                env[n.id] = mesh[int(n.value[1:])]
            elif n.op == 'const':
                env[n.id] = np.float64(n.value)
            elif n.op == 'bconst':
                env[n.id] = np.bool_(n.value)
            elif n.op == 'interp1':
                xp, fp, left, right = model.graph.tables[n.value][:4]
                env[n.id] = np.interp(env[n.args[0].id], xp, fp, left, right)
            else:
                env[n.id] = trace._NP_EVAL[n.op](*[env[a.id] for a in n.args])
    a = np.abs(np.asarray(env[a_node.id], dtype=float))
    if not np.all(np.isfinite(a)):
        return None
    return float(a.max()) * abs(float(k_rows))


def uniform_stage_pad(model, dtype, unit, axis, box):
    """THE place that decides the uniform bound stage of the branch and bound (SDP_BNB_UNIFORM of
    csrc/sdp_colfilter_kernel.h): the rows the reduced table is padded by on either side -- BNB_PAD where a unit plans
    the stage, 0 where it keeps the bound stage that locates every block end per node.  `unit`: the ColumnUnit as
    `column_table_unit` has planned it so far, without the padding.  Planned only when ALL hold: the short first pass
    of the resident-chunk form with its branch and bound (`unit.short`, `unit.bnb`), not the shifted lattice;
    x0' = x0 +- a(u) (`uniform_stage_model`); a stock axis on which every node provably sits at its row
    (`uniform_rows_axis`); the two rows either end of the table is continued from reduced by one wave
    ((n0 - 1) % 64 != 0); a control lattice (`box`: the table of admissible boxes, the same at every node where a unit
    has a control table) whose reach, max |a| k rows plus the cell partner, the end's margin and the row below, fits
    the padding; and 2 BNB_PAD rows more that cost the CU no workgroup.  The kernel checks rows and reach again where
    it runs (a failure there is the full first pass): with this plan neither fails."""
    rs = np.dtype(dtype).itemsize
    n0 = unit.n0
    if unit.short != 'lean2' or not unit.bnb or unit.shift:
        return 0
    if n0 < 2 or (n0 - 1) % 64 == 0 or not uniform_stage_model(model, unit.frontier):
        return 0
    if not uniform_rows_axis(axis, dtype, n0):
        return 0
    x = np.asarray(axis, dtype=np.float64).ravel()
    # (the lattice of every control as the kernels form it: n points from lo to hi, sdp_control_value)
    lattice = [np.linspace(float(box['lo'][c, 0]), float(box['hi'][c, 0]), int(box['n'][c, 0]))
               for c in range(box['lo'].shape[0])]
    reach = uniform_stage_reach(model, unit.frontier, lattice, np.float64(n0 - 1) / (x[-1] - x[0]))
    if reach is None or not reach * (1.0 + 2.0 ** -30) + 2.0 ** -19 <= BNB_PAD - 3:
        return 0
    per_cu = lambda size: min(COLUMN_LDS_MAX // size, max(1, 2048 // unit.threads))      # (LDS, and 32 waves per CU)
    if per_cu(unit.lds_bytes + 2 * BNB_PAD * rs) != per_cu(unit.lds_bytes):
        return 0
    return BNB_PAD


# rows: 2 delta D = 4096 u D at most, against a radius of (160 + 256) u S_node >= 1248 u D at W = 32 and 64 controls -- the
# position term may reach 3.3 times the radius of before (the benchmark: 2180 u D, 1.7 times: the radius grows 2.7-fold at
# most); beyond that the filter would be given away for the instructions saved, and the unit keeps the evaluation it had
EVAL_DELTA_CAP = 2.0 ** -42


def uniform_eval_delta(axis, n0):
    """(delta, dx, unit_axis) of `uniform_eval_plan` for a stock axis of `n0` rows: the arithmetic alone"""
    x = np.asarray(axis, dtype=np.float64).ravel()
    n0 = int(n0)
    smin, span = x[0], x[-1] - x[0]
    k = np.float64(n0 - 1) / span
    unit_axis = bool(smin == 0.0 and span == 1.0)
    dx = float(np.max(np.abs((x - smin) * k - np.arange(n0, dtype=np.float64))))
    # (.. rounded up to a power of two, 2^-60 at least: the check compares against an immediate operand)
    dx = max(float(2.0 ** math.ceil(math.log2(dx))) if dx > 0.0 else 0.0, 2.0 ** -60)
    u = 2.0 ** -53
    m = n0 + BNB_PAD
    count = (2 * m + n0) if unit_axis else (6 * m + abs(float(smin)) * float(k) + 2 * n0)
    return (dx + u * (count + 2 * BNB_PAD + 2)) * (1.0 + 2.0 ** -20), dx, unit_axis


def uniform_eval_plan(model, dtype, unit, axis, debug=None):
    """THE place that decides the uniform EVALUATION stage of the branch and bound (SDP_BNB_UNIFORM_EVAL of
    csrc/sdp_column_kernel.h), on a unit that `uniform_stage_pad` has padded: None, or (delta, dx, unit_axis).

    delta bounds, in rows, the distance between the position the reference's chain forms for control c of row r
    (sdp_lean2_cell: fl(X_r +- a_c), - smin, / span or * rspan, * nm1, and the rounding of lam0 where the cell is clamped)
    and  r + pa_c,  pa_c = fl(+-a_c k) as the control table's wave forms it, k = fl((n - 1) / span), for EVERY a_c whose
    pa_c stays inside the padding (the wave checks that) -- so for every control of every lattice the unit runs on:

      * dx: the largest |fl(fl(X_r - smin) k) - r| over the rows of the stored axis, in the kernel's own arithmetic; the
        kernel checks every node against it, so a node that passes sits within dx + c n u of its row in real numbers (the
        two roundings of the check, one on the unit axis where X - 0 is exact);
      * the chain's roundings, each at most u of a position (|p| <= M = n + PAD rows) or of x0' itself (|smin| k more): two
        on the unit axis (the sum, the product; k = n - 1 exactly), six otherwise (sum, difference, quotient or product
        with an exact reciprocal, product, and k's own: counted as in the division form);
      * u |pa_c| <= u PAD for pa_c, u (PAD + 1) for lam0 beyond either end, u where phi_c rounds to 1.

    The roundings are COUNTED, on purpose, where one could enumerate every (row, control) pair of the planned lattice on the
    host (496 u on the benchmark against the 1 090 u counted): the enumeration says nothing about a lattice whose values the
    kernel forms an ulp away from numpy's, or about the box of another call; the count holds for whatever lies inside the
    padding.  tests/test_uniform_eval_exact.py measures the true distance pair by pair against it.  Planned where delta stays below
    EVAL_DELTA_CAP and a depends on the control alone: the records then lie where the control tables of the two parities
    held a, which such a unit reads from no table, and the LDS image is what it was.  (The record says so whether or not the
    A/B switch SDP_BNB_UNIFORM = 0 leaves both uniform stages out of the text.)"""
    if not unit.bnb_pad or _dbg(debug, 'SDP_BNB_UNIFORM_EVAL') == '0':
        return None
    # (the records take the slots a has in the control tables and serve every column: a of x0' = x0 +- a has to follow from
    # the control alone, SDP_LEAN2_A_FIXED)
    a_slot = int(model.additive_control_split(unit.frontier)['lead'][1])
    if unit.frontier[a_slot].deps & DEP_X:
        return None
    delta, dx, unit_axis = uniform_eval_delta(axis, unit.n0)
    if not (np.isfinite(delta) and delta <= EVAL_DELTA_CAP):
        return None
    return delta, dx, unit_axis


def shift_chain(model):
    """additions of a chain of sums that the shifted lattice regrouped (SDP_COL_SHIFT_CHAIN / SDP_LINE_CHAIN; 0: the
    final-sum form)"""
    chain = model.lead_split_chain()
    return chain[1] if chain is not None else 0


def _column_lines(model, dtype, unit, debug):
    """the macros and model slices of a unit that includes csrc/sdp_column_kernel.h: `unit` (a ColumnUnit) printed as
    it was planned -- nothing is decided here"""
    lines = ['#define SDP_COST_HAS_W {}'.format(1 if model.cost_depends_on_w else 0),
             '#define SDP_LEAD_HAS_W {}'.format(1 if model.lead_depends_on_w else 0),
             '#define SDP_TRAIL_HAS_U {}'.format(1 if model.trail_depends_on_u else 0),
             '#define SDP_COL_N0 {}'.format(unit.n0),
             '#define SDP_COL_W {}'.format(max(unit.w, 1)),
             '#define SDP_COL_THREADS {}'.format(unit.threads),
             '#define SDP_COL_WPAIR {}'.format(1 if unit.wpair else 0)]
    if unit.wres:
        lines.append('#define SDP_COL_WRES {}         // resident-chunk form: perturbation points the table holds at a time'.format(unit.wres))
    if unit.unroll_w:
        lines.append('#define SDP_COL_UNROLL_W {}'.format(unit.unroll_w))
    if unit.min_waves and unit.wres:
        lines.append('#define SDP_COL_MIN_WAVES {}    // as many waves per SIMD as the LDS image admits workgroups per CU, at most 4'.format(
            unit.min_waves))
    elif unit.min_waves:
        lines.append('#define SDP_COL_MIN_WAVES {}    // small workgroups of the filtered kernel: no register cap'.format(unit.min_waves))
    if unit.filtered:
        lines.append('#define SDP_COL_FILTER 1')
        if unit.shift:
            lines += ['#define SDP_COL_SHIFT 1        // x0\' = a(x, u) +- b_1(x_1.., w) +- ..: first pass on the shifted lattice',
                      '#define SDP_COL_SHIFT_TERMS {}'.format(len(model.lead_split()[1])),
                      '#define SDP_COL_SHIFT_CHAIN {}        // additions of a chain of sums that was regrouped (0: the final-sum form)'.format(
                          shift_chain(model)),
                      '#define SDP_COL_SHIFT_ROWS {}'.format(unit.shift_rows)]
        if _dbg(debug, 'SDP_COL_FILTER_SCALE'):
            lines.append('#define SDP_COL_FILTER_SCALE {}'.format(float(_dbg(debug, 'SDP_COL_FILTER_SCALE'))))
    if unit.a_lw:                 # how the table build deals its entries to the threads (else round-robin)
        lines += ['#define SDP_COL_A_ORDER 2',
                  '#define SDP_COL_A_LW {}'.format(unit.a_lw)]
        if unit.a_group:
            lines.append('#define SDP_COL_A_GROUP {}      // table entries per thread whose vertex loads are issued together'.format(unit.a_group))
        if unit.wide_loads:
            lines.append('#define SDP_COL_A_WIDE_LOADS 1')
        if unit.tail_hold:
            lines.append('#define SDP_COL_TAIL_HOLD 1    // the tail of the table is built once and held in registers')
    # (table_phase_plan: the reductions of the plain resident-chunk form)
    if unit.reduce_fused:
        lines.append('#define SDP_COL_REDUCE_FUSED 1 // A[r] by fused multiply-adds, one rounding per point')
    if unit.dmax_hi:
        lines.append('#define SDP_COL_DMAX_HI 1      // the column bound\'s maximum over the high words, rounded up')
    if unit.form == 'row window':
        lines.append('#define SDP_COL_ROWS {}'.format(unit.window_rows))
    if unit.form == 'table per control':
        lines.append('#define SDP_COL_WCHUNK {}'.format(unit.wchunk))
        if unit.colu_wide_loads:
            lines.append('#define SDP_COLU_WIDE_LOADS 1')
    for k in DEBUG_INT_MACROS:                                   # tuning knobs of A/B runs (explicit dict only)
        if _dbg(debug, k):
            lines.append('#define {} {}'.format(k, int(_dbg(debug, k))))
    lines += [separable_functions_source(model), '']
    if unit.frontier is not None:
        lines += ['#define SDP_COL_UTAB {}'.format(len(unit.frontier)),
                  '#define SDP_COL_UTAB_N {}'.format(unit.utab_n),
                  control_table_source(model, unit.frontier), '']
    if unit.short == 'lean2':
        short = short_pass_source(model, unit.frontier, 'SDP_COL_LEAN2')
        if unit.bnb:
            short += ('\n#define SDP_COL_BNB 1          // the short first pass as a certified branch and bound over '
                      'blocks of controls (sdp_lean2_bnb)')
        if unit.bnb_pad:               # (uniform_stage_pad: the LDS image counts these rows)
            short += '\n#define SDP_BNB_PAD_ROWS {}    // the reduced table continued linearly on either side'.format(unit.bnb_pad)
        if unit.uniform:
            short += uniform_define
        if unit.eval_delta and unit.uniform:          # (uniform_eval_plan; the stage needs the uniform bound stage)
            short += ('\n#define SDP_BNB_UNIFORM_EVAL 1       // controls evaluated at row r + k_c + phi_c, the same offsets in every lane'
                      '\n#define SDP_BNB_UNIFORM_EVAL_DELTA {}    // rows between that position and the reference\'s, at most: added to the radius'
                      '\n#define SDP_BNB_UNIFORM_EVAL_DX {}       // .. of which the node\'s own distance from its row, checked per node'
                      '\n#define SDP_BNB_UNIFORM_EVAL_UNIT {}     // the roundings were counted for the axis [0, 1]').format(
                          float(unit.eval_delta).hex(), float(unit.eval_dx).hex(), 1 if unit.eval_unit_axis else 0)
        lines += [short, '']
    elif unit.short == 'wide2':
        short = short_pass_source(model, unit.frontier, 'SDP_COL_WIDE2')
        if unit.bnb:
            short += ('\n#define SDP_COL_BNB 1          // the short wide first pass as a certified branch and bound over '
                      'blocks of controls (sdp_short_bnb)')
        if unit.bnb_chunk:
            short += '\n#define SDP_BNB_CHUNK {}        // blocks whose bounds are evaluated together (see SDP_COL_A_GROUP above)'.format(unit.bnb_chunk)
        lines += [short, '']
    lines += ['#include "sdp_column_kernel.h"    // also brings in sdp_sweep_kernel.h', '']
    return lines


def line_filter_applies(model, dtype, W, debug=None):
    """ONE state variable whose perturbation enters x' through final sums (`x + u - w`, the shop inventory of the
    reference's tutorial, doc/example_inventory.py:31-33), a cost that does not see the perturbation, 8-byte reals:
    the certified filter on the shifted lattice with the value array itself as the table (csrc/sdp_line_kernel.h).
    (`debug`: SDP_LINE_FILTER = 0 switches it off, A/B runs.)"""
    if _dbg(debug, 'SDP_LINE_FILTER', '1') == '0':
        return False
    return bool(model.n_state == 1 and model.n_perturb == 1 and 1 <= int(W) <= 1024 and np.dtype(dtype).itemsize == 8
                and not model.time_dep and model.lead_depends_on_w and not model.cost_depends_on_w
                and model.lead_split() is not None)


def line_functions_source(model):
    """C++ text of the slices csrc/sdp_line_kernel.h uses: a, the signed sum B of the b_i with the sum of their
    magnitudes, the cost -- each with the reference's own operations (as separable_functions_source emits them
    for the column kernel's shifted lattice)"""
    a_node, terms = model.lead_split()
    out = []
    lines = ['SDP_DEV sdp_real sdp_model_lead_a(const sdp_real *x, const sdp_real *u, sdp_real t)',
             '{', '    (void)x; (void)u; (void)t;']
    names = _emit_body(model, model.slice_nodes([a_node]), lines)
    lines += ['    return {};'.format(names[a_node.id]), '}']
    out.append('\n'.join(lines))
    chain = model.lead_split_chain()
    if chain is not None:
        leaves = [n for n, _ in chain[0]]
        lines = ['SDP_DEV sdp_real sdp_model_lead_aabs(const sdp_real *x, const sdp_real *u, sdp_real t)',
                 '{', '    (void)x; (void)u; (void)t;']
        names = _emit_body(model, model.slice_nodes(leaves), lines)
        lines += ['    return {};'.format(' + '.join('fabs({})'.format(names[n.id]) for n in leaves)), '}']
        out.append('\n'.join(lines))
    lines = ['SDP_DEV void sdp_model_lead_b(const sdp_real *x, sdp_real w, sdp_real t, sdp_real &b, sdp_real &babs)',
             '{', '    (void)x; (void)w; (void)t;']
    names = _emit_body(model, model.slice_nodes([b for b, _ in terms]), lines)
    b0, s0 = terms[0]
    lines.append('    b = {}{};'.format('-' if s0 < 0 else '', names[b0.id]))
    lines.append('    babs = fabs({});'.format(names[b0.id]))
    for bn, sg in terms[1:]:
        lines.append('    b = b {} {};'.format('+' if sg > 0 else '-', names[bn.id]))
        lines.append('    babs = babs + fabs({});'.format(names[bn.id]))
    lines.append('}')
    out.append('\n'.join(lines))
    lines = ['SDP_DEV sdp_real sdp_model_cost(const sdp_real *x, const sdp_real *u, sdp_real w,',
             '                                sdp_real t)',
             '{', '    (void)x; (void)u; (void)w; (void)t;']
    names = _emit_body(model, model.slice_nodes([model.cost]), lines)
    lines += ['    return {};'.format(names[model.cost.id]), '}']
    out.append('\n'.join(lines))
    return '\n\n'.join(out)


def box_function_source(box, at=False):
    """C++ text of `sdp_model_box(const double *x, double t, double *lo, double *hi)` for a TracedBox: the ends of the
    admissible box of every control at a state, in DOUBLE whatever the unit's reals (csrc/sdp_lookahead_kernel.h
    widens a 4-byte state first, as the host's scalar calls do).  The body is `_emit_body`'s and the np.interp tables
    are `interp_tables_source`'s, printed once more under names of their own with `double` for `sdp_real`: every
    helper the emitter names is a template or has a double overload (csrc/sdp_device.h), so no box that traces is
    left without its function.
    at: `sdp_model_box_at(const double *x, double t, const double *bprm, double *lo, double *hi)` instead, for a box
    with lifted constants (TracedBox.lift_constants): the same body with `bprm[slot]` in the place of each literal
    (csrc/sdp_family_lookahead_kernel.h hands over the row of a family's member)."""
    if at != (getattr(box, 'param_index', None) is not None):
        raise ValueError('sdp_model_box_at is the function of a box with lifted constants, sdp_model_box of one without')
    if at:
        lines = ['SDP_DEV void sdp_model_box_at(const sdp_real *x, sdp_real t, const sdp_real *__restrict__ bprm, sdp_real *lo, sdp_real *hi)',
                 '{',
                 '    (void)x; (void)t; (void)bprm;']
        body = []
        names = _emit_body(box, box.live_nodes(), body)
        lines += [ln.replace('sdp_model_prm[', 'bprm[') for ln in body]
        names = {k: v.replace('sdp_model_prm[', 'bprm[') for k, v in names.items()}
    else:
        lines = ['SDP_DEV void sdp_model_box(const sdp_real *x, sdp_real t, sdp_real *lo, sdp_real *hi)',
                 '{',
                 '    (void)x; (void)t;']
        names = _emit_body(box, box.live_nodes(), lines)
    for c, (lo, hi) in enumerate(box.ends):
        lines.append('    lo[{}] = {};'.format(c, names[lo.id]))
        lines.append('    hi[{}] = {};'.format(c, names[hi.id]))
    lines.append('}')
    text = interp_tables_source(box) + '\n'.join(lines)
    for old, new in (('sdp_np_interp', 'sdp_box_np_interp'), ('sdp_interp1_', 'sdp_box_interp1_'),
                     ('sdp_tabx_', 'sdp_box_tabx_'), ('sdp_tabf_', 'sdp_box_tabf_'), ('sdp_real', 'double')):
        text = text.replace(old, new)
    return text


def lookahead_unit(model, dtype, lanes, box=None, debug=None):
    """The generated source of a LOOKAHEAD unit (csrc/sdp_lookahead_kernel.h): a direct-family unit -- node order,
    `lanes` lanes per state, several perturbation variables through csrc/sdp_multiw_kernel.h -- that also carries
    kernel `sdp_lookahead`, and, when `box` is the TracedBox of control_box (symbolic in the state and the time
    index), the box function and kernel `sdp_simulate_lookahead`."""
    if box is not None and (box.t_value is not None or box.inexact_ops()):
        raise ValueError('the box function of a lookahead unit is a trace with a symbolic time index and exact operations')
    return translation_unit(model, dtype, lanes, None, debug=debug, lookahead=box if box is not None else True)


def family_unit(model, dtype, lanes):
    """The generated source of a FAMILY unit (csrc/sdp_family_kernel.h, kernel `sdp_family_sweep`): the direct
    prologue of a model with lifted constants, marked SDP_FAMILY, and the family header in the place of
    sdp_sweep_kernel.h.  The kernel reads the constants of member p from row p of a table through
    sdp_model_cell_at; `lanes` is the largest lane count of the members."""
    if model.param_index is None:
        raise ValueError('a family unit takes a model with lifted constants (TracedModel.lift_constants)')
    if model.n_perturb >= 2:
        raise NotImplementedError('a family unit takes one perturbation variable at most')
    real = {'float64': 'double', 'float32': 'float'}[np.dtype(dtype).name]
    head = _prologue_lines(model, real, lanes, None)
    at = head.index('#include "sdp_device.h"')
    head.insert(at, '#define SDP_FAMILY 1          // the unit carries sdp_family_sweep alone (csrc/sdp_family_kernel.h)')
    head += ['#include "sdp_family_kernel.h"    // brings in the helpers of sdp_sweep_kernel.h', '']
    return '\n'.join(head)


# the resident evaluation kernel of a family (csrc/sdp_family_policy_kernel.h: SDP_FPOL_THREADS, SDP_FPOL_LDS_BYTES,
# SDP_FPOL_RED_BYTES): its workgroup, its LDS budget -- the whole LDS of a CU -- and what of it the reduction takes
FAMILY_RESIDENT_THREADS = 1024
FAMILY_RESIDENT_LDS_BYTES = 160 * 1024
FAMILY_RESIDENT_REDUCTION_BYTES = 512


def family_resident_nodes(dtype):
    """the fit rule of kernel sdp_family_evalpol_resident: a member is resident when two buffers of S reals, plus
    what the reduction needs, fit the LDS budget the kernel is built for.  The largest such S."""
    return (FAMILY_RESIDENT_LDS_BYTES - FAMILY_RESIDENT_REDUCTION_BYTES) // (2 * np.dtype(dtype).itemsize)


def family_policy_unit(model, dtype):
    """The generated source of a family EVALUATION unit (csrc/sdp_family_policy_kernel.h, kernels
    `sdp_family_evalpol` and `sdp_family_evalpol_resident`): the direct prologue of a model with lifted constants,
    marked SDP_FAMILY and SDP_FAMILY_POLICY, and the evaluation header in the place of sdp_sweep_kernel.h.  A
    fixed-policy backup has no control lattice, so there is one unit per model structure and real type (the lane
    count the prologue prints is 1 and nothing reads it)."""
    if model.param_index is None:
        raise ValueError('a family unit takes a model with lifted constants (TracedModel.lift_constants)')
    if model.n_perturb >= 2:
        raise NotImplementedError('a family unit takes one perturbation variable at most')
    real = {'float64': 'double', 'float32': 'float'}[np.dtype(dtype).name]
    head = _prologue_lines(model, real, 1, None)
    at = head.index('#include "sdp_device.h"')
    head.insert(at, '#define SDP_FAMILY 1          // the helpers of csrc/sdp_family_kernel.h ..')
    head.insert(at + 1, '#define SDP_FAMILY_POLICY 1   // .. and the two evaluation kernels in the place of sdp_family_sweep')
    head += ['#include "sdp_family_policy_kernel.h"    // brings in sdp_family_kernel.h', '']
    return '\n'.join(head)


def family_mc_unit(model, dtype):
    """The generated source of a family MONTE CARLO unit (csrc/sdp_family_mc_kernel.h, kernel
    `sdp_family_montecarlo`): the direct prologue of a model with lifted constants, marked SDP_FAMILY and
    SDP_FAMILY_MC, and the Monte Carlo header in the place of sdp_sweep_kernel.h.  A closed loop has no control
    lattice, so there is one unit per model structure and real type (the lane count the prologue prints is 1 and
    nothing reads it)."""
    if model.param_index is None:
        raise ValueError('a family unit takes a model with lifted constants (TracedModel.lift_constants)')
    if model.n_perturb != 1:
        raise NotImplementedError('a family Monte Carlo unit draws one perturbation variable')
    real = {'float64': 'double', 'float32': 'float'}[np.dtype(dtype).name]
    head = _prologue_lines(model, real, 1, None)
    at = head.index('#include "sdp_device.h"')
    head.insert(at, '#define SDP_FAMILY 1          // the helpers of csrc/sdp_family_kernel.h ..')
    head.insert(at + 1, '#define SDP_FAMILY_MC 1       // .. and sdp_family_montecarlo in the place of sdp_family_sweep')
    head += ['#include "sdp_family_mc_kernel.h"    // brings in sdp_family_kernel.h and the draw helpers of sdp_mc_kernel.h', '']
    return '\n'.join(head)


def family_horizon_unit(model, dtype):
    """The generated source of a family HORIZON unit (csrc/sdp_family_horizon_kernel.h, kernels `sdp_family_simulate`
    and, for a stochastic model, `sdp_family_montecarlo_h`): the direct prologue of a model with lifted constants,
    marked SDP_FAMILY and SDP_FAMILY_HORIZON, and the horizon header in the place of sdp_sweep_kernel.h.  A closed
    loop has no control lattice, so there is one unit per model structure and real type (the lane count the prologue
    prints is 1 and nothing reads it); the steps of a model traced per step (`data[k]`) share it, each with its row
    of constants."""
    if model.param_index is None:
        raise ValueError('a family unit takes a model with lifted constants (TracedModel.lift_constants)')
    if model.n_perturb >= 2:
        raise NotImplementedError('a family unit takes one perturbation variable at most')
    real = {'float64': 'double', 'float32': 'float'}[np.dtype(dtype).name]
    head = _prologue_lines(model, real, 1, None)
    at = head.index('#include "sdp_device.h"')
    head.insert(at, '#define SDP_FAMILY 1          // the helpers of csrc/sdp_family_kernel.h ..')
    head.insert(at + 1, '#define SDP_FAMILY_HORIZON 1  // .. and the closed loops over a horizon in the place of sdp_family_sweep')
    head += ['#include "sdp_family_horizon_kernel.h"    // brings in sdp_family_kernel.h and the draw helpers of sdp_mc_kernel.h', '']
    return '\n'.join(head)


# kernel sdp_family_transitions (csrc/sdp_family_trans_kernel.h: SDP_FTRANS_THREADS): its workgroup
FAMILY_TRANS_THREADS = 256


def family_trans_tile(d):
    """nodes of one member a workgroup of kernel sdp_family_transitions holds (SDP_FTRANS_TILE): 2^d lanes a node"""
    return FAMILY_TRANS_THREADS >> int(d)


def family_trans_unit(model, dtype):
    """The generated source of a family TRANSITION unit (csrc/sdp_family_trans_kernel.h, kernel
    `sdp_family_transitions`): the direct prologue of a model with lifted constants, marked SDP_FAMILY and
    SDP_FAMILY_TRANS, and the transition header in the place of sdp_sweep_kernel.h.  The entries of a policy's
    operator have no control lattice, so there is one unit per model structure and real type (the lane count the
    prologue prints is 1 and nothing reads it)."""
    if model.param_index is None:
        raise ValueError('a family unit takes a model with lifted constants (TracedModel.lift_constants)')
    if model.n_perturb >= 2:
        raise NotImplementedError('a family unit takes one perturbation variable at most')
    real = {'float64': 'double', 'float32': 'float'}[np.dtype(dtype).name]
    head = _prologue_lines(model, real, 1, None)
    at = head.index('#include "sdp_device.h"')
    head.insert(at, '#define SDP_FAMILY 1          // the helpers of csrc/sdp_family_kernel.h ..')
    head.insert(at + 1, '#define SDP_FAMILY_TRANS 1    // .. and sdp_family_transitions in the place of sdp_family_sweep')
    head += ['#include "sdp_family_trans_kernel.h"    // brings in sdp_family_kernel.h', '']
    return '\n'.join(head)


def family_lookahead_unit(model, box, dtype, lanes):
    """The generated source of a family LOOKAHEAD unit (csrc/sdp_family_lookahead_kernel.h, kernels
    `sdp_family_lookahead` and `sdp_family_montecarlo_lookahead`): the direct prologue of a model with lifted
    constants, marked SDP_FAMILY and SDP_FAMILY_LOOKAHEAD, the box function of a TracedBox with lifted constants
    (`sdp_model_box_at`, SDP_NBOXPARAMS of them per member) and the lookahead header in the place of
    sdp_sweep_kernel.h.  `lanes` is the largest lane count of the members: the lanes of a state's control loop."""
    if model.param_index is None or getattr(box, 'param_index', None) is None:
        raise ValueError('a family lookahead unit takes a model and a box with lifted constants (lift_constants)')
    if model.n_perturb >= 2:
        raise NotImplementedError('a family unit takes one perturbation variable at most')
    if box.t_value is not None or box.inexact_ops():
        raise ValueError('the box function of a lookahead unit is a trace with a symbolic time index and exact operations')
    real = {'float64': 'double', 'float32': 'float'}[np.dtype(dtype).name]
    head = _prologue_lines(model, real, lanes, None)
    at = head.index('#include "sdp_device.h"')
    head.insert(at, '#define SDP_FAMILY 1          // the helpers of csrc/sdp_family_kernel.h ..')
    head.insert(at + 1, '#define SDP_FAMILY_LOOKAHEAD 1   // .. and the two lookahead kernels in the place of sdp_family_sweep')
    head += ['#define SDP_NBOXPARAMS {}     // constants of the box function, read from the member\'s row'.format(len(box.param_index)),
             box_function_source(box, at=True), '',
             '#include "sdp_family_lookahead_kernel.h"    // brings in sdp_family_kernel.h, the lattice rule and the draw helpers', '']
    return '\n'.join(head)


def family_lookahead_horizon_unit(model, box, dtype, lanes):
    """The generated source of a family LOOKAHEAD unit OVER A HORIZON (csrc/sdp_family_lookahead_horizon_kernel.h,
    kernels `sdp_family_simulate_lookahead` and, for a stochastic model, `sdp_family_montecarlo_lookahead_h`): what
    `family_lookahead_unit` generates, marked SDP_FAMILY_LOOKAHEAD_HORIZON, with the horizon header in the place of
    the lookahead header (which it includes for the walk, the box and the backup).  The steps of a model traced per
    step (`data[k]`) share the unit, each with its row of constants; the box function is one for all steps."""
    if model.param_index is None or getattr(box, 'param_index', None) is None:
        raise ValueError('a family lookahead unit takes a model and a box with lifted constants (lift_constants)')
    if model.n_perturb >= 2:
        raise NotImplementedError('a family unit takes one perturbation variable at most')
    if box.t_value is not None or box.inexact_ops():
        raise ValueError('the box function of a lookahead unit is a trace with a symbolic time index and exact operations')
    real = {'float64': 'double', 'float32': 'float'}[np.dtype(dtype).name]
    head = _prologue_lines(model, real, lanes, None)
    at = head.index('#include "sdp_device.h"')
    head.insert(at, '#define SDP_FAMILY 1          // the helpers of csrc/sdp_family_kernel.h ..')
    head.insert(at + 1, '#define SDP_FAMILY_LOOKAHEAD_HORIZON 1   // .. and the two closed loops under lookahead controls in the place of sdp_family_sweep')
    head += ['#define SDP_NBOXPARAMS {}     // constants of the box function, read from the member\'s row'.format(len(box.param_index)),
             box_function_source(box, at=True), '',
             '#include "sdp_family_lookahead_horizon_kernel.h"    // brings in sdp_family_lookahead_kernel.h: its helpers, the lattice rule, the draw helpers', '']
    return '\n'.join(head)


def translation_unit(model, dtype, lanes, family=None, debug=None, peer_stores=False, lookahead=None):
    """The generated source of one model code object.  `family`: what the unit is to hold beside the direct node-order
    kernels of csrc/sdp_sweep_kernel.h --
    None: nothing else;
    a ColumnUnit (`column_table_unit`, `column_percontrol_unit`, `column_window_unit`): the column kernels of
    csrc/sdp_column_kernel.h, printed as the record says;
    a dict of `staged_config`: the LDS-staged generic kernel of csrc/sdp_staged_kernel.h (node order, any traceable model);
    a pair (lead_axes, lead_perm) of `lead_filter_applies` / `lead_order`: the reduced-array sweep of
    csrc/sdp_lead_kernel.h (lead_perm None: the stocks are listed first);
    an int W: the line kernel of csrc/sdp_line_kernel.h on W perturbation points.
    debug: None (the product), or a dict of diagnostic switches (see DEBUG_NAMES).
    peer_stores: the unit's backup kernels also store J into the buffers of other ranks (the direct exchange,
    SdpSweepArgs.peer_J); without it they hold no code for that, and the library refuses the direct exchange.
    lookahead: None, or what `lookahead_unit` hands over (True, or the TracedBox of the unit's box function)."""
    debug = check_debug(debug)
    if lookahead is not None and family is not None:
        raise ValueError('a lookahead unit is a direct-family unit')
    real = {'float64': 'double', 'float32': 'float'}[np.dtype(dtype).name]
    if model.n_perturb >= 2 and (family is not None or peer_stores):
        raise ValueError('the column, lead, line and staged families and the direct exchange take one perturbation variable')
    head = _prologue_lines(model, real, lanes, debug, peer_stores)
    column = family if isinstance(family, ColumnUnit) else None
    staged = family if isinstance(family, dict) else None
    line = family if isinstance(family, (int, np.integer)) else 0
    lead_axes, lead_perm = family if (column is None and isinstance(family, tuple)) else (0, None)
    if column is not None:
        assert model.column_shareable
        head += _column_lines(model, dtype, column, debug)
    elif staged is not None:
        tile = tuple(staged['tile']) + (1,) * (4 - len(staged['tile']))
        head += ['#define SDP_STG_THREADS {}'.format(int(staged['threads']))] + [
            '#define SDP_STG_T{} {}'.format(k, int(tile[k])) for k in range(4)] + [
            '#define SDP_STG_CU {}'.format(int(staged['cu'])),
            '#define SDP_STG_CW {}'.format(int(staged['cw'])),
            '#define SDP_STG_CAP {}'.format(int(staged['cap'])),
            '#include "sdp_staged_kernel.h"    // also brings in sdp_sweep_kernel.h',
            '']
    elif line:
        # one state variable with noise in its sums: the filter on the shifted lattice, the value array as its table
        head += ['#define SDP_LINE 1',
                 '#define SDP_LINE_W {}'.format(int(line)),
                 '#define SDP_LINE_CHAIN {}        // additions of a chain of sums that was regrouped (0: the final-sum form)'.format(
                     shift_chain(model))]
        if _dbg(debug, 'SDP_LINE_FILTER_SCALE'):
            head.append('#define SDP_LINE_FILTER_SCALE {}'.format(float(_dbg(debug, 'SDP_LINE_FILTER_SCALE'))))
        if _dbg(debug, 'SDP_LINE_TOP2') is not None:
            head.append('#define SDP_LINE_TOP2 {}'.format(int(_dbg(debug, 'SDP_LINE_TOP2'))))
        head += [line_functions_source(model), '',
                 '#include "sdp_sweep_kernel.h"    // brings in sdp_line_kernel.h', '']
    elif lead_axes:
        # several controlled state variables: node-order sweep with the filter on an array reduced over w
        head += ['#define SDP_LEAD_AXES {}'.format(int(lead_axes)),
                 '#define SDP_LEAD_COST_HAS_W {}'.format(1 if model.cost_depends_on_w else 0)]
        if lead_perm is not None and tuple(lead_perm) != tuple(range(model.n_state)):
            full = tuple(lead_perm) + tuple(range(model.n_state, 4))
            head.append('#define SDP_LEAD_PERM {{{}}}     // state variable of logical axis j: the stocks are not listed first'.format(
                ', '.join(str(int(k)) for k in full)))
        if _dbg(debug, 'SDP_LEAD_FILTER_SCALE'):
            head.append('#define SDP_LEAD_FILTER_SCALE {}'.format(float(_dbg(debug, 'SDP_LEAD_FILTER_SCALE'))))
        if _dbg(debug, 'SDP_LEAD_UNROLL'):
            head.append('#define SDP_LEAD_UNROLL {}'.format(int(_dbg(debug, 'SDP_LEAD_UNROLL'))))
        head += [lead_functions_source(model, int(lead_axes), lead_perm), '',
                 '#include "sdp_sweep_kernel.h"    // brings in sdp_lead_kernel.h', '']
    elif lookahead is not None:
        head.append('#define SDP_LOOKAHEAD 1        // the unit also carries sdp_lookahead (csrc/sdp_lookahead_kernel.h)')
        if lookahead is not True:
            head += [box_function_source(lookahead),
                     '#define SDP_LOOKAHEAD_BOX 1    // .. its own box function, and sdp_simulate_lookahead']
        head += ['#include "sdp_sweep_kernel.h"    // brings in sdp_lookahead_kernel.h', '']
    else:
        head += ['#include "sdp_sweep_kernel.h"', '']
    return '\n'.join(head)


# ---------------------------------------------------------------------------
# LDS-staged generic kernel (csrc/sdp_staged_kernel.h): tile / chunk planning
# ---------------------------------------------------------------------------
STAGED_TILES = {1: (512,), 2: (16, 32), 3: (8, 8, 8), 4: (4, 4, 4, 8)}
STAGED_LDS_BYTES = 76 * 1024         # per workgroup: two 512-thread workgroups per CU


def staged_row_stride(length, tile_last, d, rs):
    """sdp_stg_row_stride of csrc/sdp_staged_kernel.h"""
    if d == 1 or tile_last >= 32 or rs != 8:
        return length | 1
    return (length + tile_last - 1) // (2 * tile_last) * (2 * tile_last) + tile_last


def staged_config(model, state_grid, perturb_grid, box, dtype, t_value=0.0, n_samples=24, debug=None):
    """Tile shape, chunk sizes and LDS budget of the staged kernel for `model`
    on this discretisation.  The chunk (controls x perturbation points whose
    next states share one staged box) is the largest whose box -- measured by
    evaluating the traced dynamics with numpy at the corners of sample tiles
    and chunks, exactly what the kernel does per chunk -- fits the budget for
    most samples.  A bad choice costs time only: cells outside the staged box
    read global memory (csrc/sdp_staged_kernel.h).
    box: dict with lo, hi, n ([nu][S] or [nu][1]) and per_node."""
    from .trace import evaluate
    d = model.n_state
    rs = np.dtype(dtype).itemsize
    shape = tuple(len(g) for g in state_grid)
    tile = STAGED_TILES[d]
    cap = STAGED_LDS_BYTES // rs
    W = len(perturb_grid[0]) if perturb_grid and model.n_perturb else 0
    wg = np.asarray(perturb_grid[0], dtype=float) if W else np.zeros(1)
    Wn = max(W, 1)
    nu = model.n_control
    lo, hi, n = box['lo'], box['hi'], box['n']
    S = int(np.prod(shape))
    rng = np.random.default_rng(2024)
    smin = np.array([g[0] for g in state_grid], dtype=float)
    span = np.array([g[-1] - g[0] for g in state_grid], dtype=float)
    nm1 = np.array([len(g) - 1 for g in state_grid], dtype=float)
    tiles_per = [-(-shape[k] // tile[k]) for k in range(d)]

    def control_values(flat_nodes, ci):
        """numpy.linspace point `ci` (flat C-order lattice index, clipped) of each node"""
        col = flat_nodes if box['per_node'] else np.zeros_like(flat_nodes)
        nn = n[:, col].astype(np.int64)
        tot = np.prod(nn, axis=0)
        flat = np.minimum(ci, tot - 1)
        out = []
        for c in range(nu - 1, -1, -1):
            k = flat % nn[c]
            flat = flat // nn[c]
            l, h = lo[c, col], hi[c, col]
            step = np.where(nn[c] > 1, (h - l) / np.maximum(nn[c] - 1, 1), 0.0)
            out.append(np.where(k == nn[c] - 1, h, k * step + l))
        return out[::-1], tot

    def volume(cu, cw):
        vols = []
        for _ in range(n_samples):
            torg = [int(rng.integers(0, tiles_per[k])) * tile[k] for k in range(d)]
            # corner nodes of the tile (clipped to the grid)
            idx = np.array(np.meshgrid(*[[torg[k], min(torg[k] + tile[k], shape[k]) - 1]
                                         for k in range(d)], indexing='ij')).reshape(d, -1)
            flat = np.ravel_multi_index(tuple(idx), shape)
            x = [np.asarray(state_grid[k], dtype=float)[idx[k]] for k in range(d)]
            _, tot = control_values(flat, 0)
            c0 = int(rng.integers(0, max(int(tot.max()) - cu, 0) + 1))
            w0 = int(rng.integers(0, max(Wn - cw, 0) + 1))
            qlo = np.full(d, np.inf)
            qhi = np.full(d, -np.inf)
            for ci in (c0, c0 + cu - 1):
                u, _ = control_values(flat, ci)
                for wi in (w0, min(w0 + cw, Wn) - 1):
                    with np.errstate(all='ignore'):
                        xn, _ = evaluate(model, x, u, [wg[wi]] if model.n_perturb else [], t_value)
                    for k in range(d):
                        p = (np.asarray(xn[k], dtype=float) - smin[k]) / span[k] * nm1[k]
                        q = np.clip(np.floor(np.nan_to_num(p, nan=0.0, posinf=1e9, neginf=-1e9)),
                                    0, shape[k] - 2)
                        qlo[k] = min(qlo[k], q.min())
                        qhi[k] = max(qhi[k], q.max())
            ext = [min(qhi[k] + 1, shape[k] - 2) + 2 - max(qlo[k] - 1, 0) for k in range(d)]
            ext[-1] = staged_row_stride(int(ext[-1]), tile[-1], d, rs)
            vols.append(float(np.prod(ext)))
        return float(np.percentile(vols, 80))

    cws = sorted({max(1, Wn >> s) for s in range(0, 8)}, reverse=True)
    best = None
    # controls interleaved per chunk (what depends on w alone is shared by them).  Measured on
    # the control-coupled 256^3 x 64 x 32 problem: 4 -> 93.7 ms, 2 -> 120.3 ms (4 spills five
    # registers at the 128-VGPR bound two workgroups per CU impose; still faster)
    cus = (4, 2, 1)
    if _dbg(debug, 'SDP_STG_CU'):                       # A/B runs
        cus = (int(_dbg(debug, 'SDP_STG_CU')),)
    for cu in cus:
        for cw in cws:
            if best is not None and cu * cw <= best[0] * best[1]:
                continue
            if volume(cu, cw) <= cap:
                best = (cu, cw)
                break                          # smaller cw only shrinks the chunk
    if best is None:
        best = (1, 1)
    return dict(threads=int(np.prod(tile)), tile=tile, cu=best[0], cw=best[1], cap=int(cap))


COLUMN_LDS_MAX = 160 * 1024          # LDS of one gfx950 CU


def use_wpair(model, dtype, debug=None):
    """float32 tables interleave perturbation points 2k and 2k+1 (SDP_COL_WPAIR of
    csrc/sdp_column_kernel.h): one 8-byte LDS read serves two lattice cells.
    Needs a perturbation and an x0' that does not depend on it (one axis-0 cell
    per control).  Same bits as the plain layout; measured on 256^3 x 64 x 32:
    exact 6.05 -> 5.77 ms, fused 4.43 -> 3.66 ms.  (A table of (T[r], T[r+1])
    pairs was also measured for 4-byte reals and did not pay: not kept.)"""
    if _dbg(debug, 'SDP_COL_WPAIR'):                    # A/B runs
        return bool(int(_dbg(debug, 'SDP_COL_WPAIR')))
    return (np.dtype(dtype).itemsize == 4 and model.n_perturb > 0
            and not model.lead_depends_on_w and not model.trail_depends_on_u)


def column_shift_applies(model, dtype, table=None, debug=None):
    """The certified filter with a perturbation that reaches x0' additively (`x + u - w`): the first
    pass then reads a table reduced over w on a lattice that the perturbation points have SHIFTED
    (SDP_COL_SHIFT of csrc/sdp_colfilter_kernel.h).  8-byte reals only: in 4-byte reals the rounding of
    the positions alone would put most controls inside the radius.  (`debug`: SDP_COL_SHIFT = 0 switches
    it off, A/B runs.)"""
    if _dbg(debug, 'SDP_COL_SHIFT', '1') == '0':
        return False
    ok = bool(model.n_perturb > 0 and model.lead_depends_on_w and model.lead_split() is not None
              and dtype is not None and np.dtype(dtype).itemsize == 8)
    if ok and table is not None:       # (n0, w, n_state): the shifted lattice must fit LDS beside the table
        ok = column_config(table[0], table[1], table[2], dtype, False, True, shift=True,
                           utab_values=UTAB_MAX_BYTES // np.dtype(dtype).itemsize + 256,    # (whatever the control table takes, block statistics included)
                           debug=debug) is not None
    return ok


def column_filter_applies(model, window=None, per_control=None, dtype=None, table=None, debug=None):
    """Can phase B of the column kernel run the certified expectation-first filter
    (SDP_COL_FILTER of csrc/sdp_colfilter_kernel.h)?  It needs a perturbation that reaches
    neither x0' nor the cost -- then the expectation commutes with the lerp along axis 0 and
    all but the surviving controls of a node are decided on a table reduced over w -- and the
    plain full-column table with the reference's arithmetic.  Same bits as without it
    (the survivors are re-evaluated with the reference's operations).  (`debug`: SDP_COL_FILTER = 0
    switches it off, A/B runs.)"""
    if _dbg(debug, 'SDP_COL_FILTER', '1') == '0':
        return False
    # (a cost that depends on the perturbation is fine since round 3: the first pass accumulates its
    # expectation with the reference's own values, sdp_col_cost_expect; x0' must still not depend on it)
    # (and so is a perturbation that reaches x0' through a final sum, in 8-byte reals: column_shift_applies)
    return bool(model.n_perturb > 0 and (not model.lead_depends_on_w or column_shift_applies(model, dtype, table, debug))
                and not model.trail_depends_on_u and window is None
                and per_control is None)


def column_config(n0, w, n_state, dtype, wpair=False, filtered=False, max_controls=None, n_columns=None,
                  shift=False, utab_values=0, debug=None, wres=0):
    """Compile-time shape of the column kernel for a grid with n0 points along
    axis 0 and w perturbation points: (threads, lds_bytes), or None if the
    table does not fit the LDS of a CU.  512-thread workgroups while two of
    them fit a CU, else 1024 threads (one workgroup then has to fill the CU's
    wave slots alone).  `wpair`: the table holds whole pairs of perturbation
    points (an odd count is rounded up).  `utab_values`: reals per parity buffer of the
    control table (SDP_COL_UTAB x SDP_COL_UTAB_N; 0: none).  `lds_bytes` is sizeof(SdpColLds)
    of the unit these arguments generate (`_column_lds` lays the struct out member by member;
    tests/test_trace_codegen.py compiles the largest accepted sizes against the struct's
    static_assert).
    `filtered` (certified filter, SDP_COL_FILTER): one lane per node of the column where that
    fits a workgroup (n0 <= 512) -- the lanes of a node then share nothing, the second pass
    is not repeated on them and fewer waves meet at the barriers; measured on 256^3 x 64 x 32
    fp64: 2.56 ms with 512 threads, 2.32 ms with 256 (and no register cap: 165 VGPRs).
    Long control lattices (`max_controls`, with `n_columns` columns in the grid) get more lanes per
    node: a lane walks its share of a node's controls one after the other, and at the reference's own
    problem sizes that share is what takes the time -- storage-AR1 41 x 61 nodes x <= 8001 controls:
    64 threads 4.13 ms, 512: 0.59, 1024: 0.37 (61 columns: one workgroup per CU at most anyway); Searev
    31 x 61 x 61 x <= 2201: 64 threads 1.91 ms, 512: 0.65, 1024: 0.74.  About 128 controls per lane,
    512 threads at most while the grid has columns for every CU, else 1024."""
    rs = np.dtype(dtype).itemsize
    w = max(int(w), 1)
    tw = w + (w & 1) if wpair else w
    sizes = (512, 1024)
    if filtered and n0 <= 512:
        first = max(64, (int(n0) + 63) // 64 * 64)
        if max_controls:
            lanes = 1
            while lanes * 128 < int(max_controls) and lanes < 64:
                lanes *= 2
            cap = 1024 if (n_columns is not None and int(n_columns) < 256) else 512
            first = max(first, min(first * lanes, cap))
        sizes = (first,) + tuple(t for t in sizes if t > first)
    if _dbg(debug, 'SDP_COL_THREADS'):                  # A/B runs (a CU then holds as many workgroups as fit)
        sizes = (int(_dbg(debug, 'SDP_COL_THREADS')),)
    if shift:
        # (threads, lds_bytes, rows of the shifted lattice): as many rows as LDS has room for beside the table
        # and the control table while two workgroups share a CU -- at least n0 + n0 / 8, so that
        # shifts spread over an eighth of the axis still fit --, else one workgroup per CU and 2 n0 rows
        # (`wres`: the resident-chunk form -- the table holds that many points -- may get a third workgroup per CU)
        for per_cu in ((3, 2, 1) if wres else (2, 1)):
            for threads in sizes:
                if per_cu >= 2 and threads > 512:
                    continue
                base = _column_lds(int(wres) or tw, w, n0, n_state, rs, threads, shift=True, shift_rows=0, utab_values=utab_values)
                rows = min(2 * int(n0) + 16, (COLUMN_LDS_MAX // per_cu - base - 1024) // (2 * rs))
                if rows >= int(n0) + max(8, int(n0) // 8):
                    return (threads, _column_lds(int(wres) or tw, w, n0, n_state, rs, threads, shift=True, shift_rows=rows,
                                                 utab_values=utab_values), int(rows))
        return None
    for threads in sizes:
        # (`wres`: the resident-chunk form, whose table holds that many perturbation points; its workgroup has
        # one lane per node, as many of them per CU as the image allows)
        lds = _column_lds(int(wres) or tw, w, n0, n_state, rs, threads, reduced=filtered, utab_values=utab_values,
                          partial_minima=not filtered)
        if lds * (2 if threads <= 512 else 1) <= COLUMN_LDS_MAX:
            return threads, lds
    return None


def column_resident_points(model, n0, w, n_state, dtype, filtered, shift, wpair, threads, utab_values=0, debug=None):
    """Perturbation points the LDS table of the filtered column kernel holds at a time (SDP_COL_WRES of
    csrc/sdp_colres_kernel.h), or 0 for the plain kernel with the whole W x n0 table.
    The whole table lets a CU hold two workgroups when it takes 64 KiB, and the kernel is bound by what there
    is to overlap (one workgroup per CU: 3.39 ms, two: 1.67 on the benchmark problem).  Half of the points
    resident -- the rest built twice -- halves the table: chosen when it takes the CU from < 3 to >= 3
    workgroups.  Needs the lean first pass of 8-byte reals without the shifted lattice, a cost that does not
    see the perturbation, one lane per node.  (`debug`: SDP_COL_WRES = 0 switches it off, k > 0 forces k.)"""
    rs = np.dtype(dtype).itemsize
    w = int(w)
    ok = (filtered and rs == 8 and not wpair and not model.cost_depends_on_w and w >= 4
          and int(threads) >= int(n0))
    forced = _dbg(debug, 'SDP_COL_WRES')
    if forced is not None:
        k = int(forced)
        return k if (ok and 0 < k < w and 2 * k >= w) else 0
    if not ok:
        return 0
    half = (w + 1) // 2
    if shift:
        # (the shifted lattice sits beside the table: ask the planner of that image)
        both = [column_config(n0, w, n_state, dtype, wpair, True, shift=True, utab_values=utab_values, debug=debug, wres=k)
                for k in (0, half)]
        if None in both:
            return 0
        whole, part = both[0][1], both[1][1]
    else:
        whole = _column_lds(w, w, n0, n_state, rs, threads, reduced=True, utab_values=utab_values)
        part = _column_lds(half, w, n0, n_state, rs, threads, reduced=True, utab_values=utab_values)
    if COLUMN_LDS_MAX // whole < 3 <= COLUMN_LDS_MAX // part:
        return half if RESIDENT_CHUNKS_DEFAULT else 0
    return 0


# measured on the benchmark problem (256^3 x 64 x 32, 8-byte reals), same box: whole table, two workgroups per CU
# 1.65 - 1.67 ms; 16 of 32 points resident, four per CU 1.555 ms (three: 1.62, two: 1.92 -- the chunked form costs
# 15 % at equal occupancy and wins by what it lets overlap); profiles/r04_column_ab.txt
RESIDENT_CHUNKS_DEFAULT = True


def column_wide_loads(n0, dtype, window, debug=None):
    """16-byte vertex loads in the table build (SDP_COL_A_WIDE_LOADS of csrc/sdp_column_kernel.h): a lane
    takes 16 / sizeof(real) adjacent rows.  Needs whole groups of rows, no row window, exact arithmetic.
    (`debug`: SDP_COL_A_WIDE_LOADS = 0 switches it off, 1 forces it for 4-byte reals: A/B runs.)"""
    if _dbg(debug, 'SDP_COL_A_WIDE_LOADS', '1') == '0':
        return False
    rpl = 16 // np.dtype(dtype).itemsize
    if rpl != 2 and _dbg(debug, 'SDP_COL_A_WIDE_LOADS') != '1':
        # 4-byte reals: four rows per lane, but the pair layout of their table scatters the stores --
        # measured on 512^3 fp32: 11.5 ms against 11.2 without (not used)
        return False
    return int(n0) % rpl == 0 and window is None


def column_build_order(threads, w, rows, rows_per_lane=1):
    """How phase A of the column kernel deals the W x rows table entries to the threads
    (SDP_COL_A_ORDER / SDP_COL_A_LW of csrc/sdp_column_kernel.h, generated): (2, lanes_per_w) when the
    perturbation points fill the workgroup's thread groups -- a thread then keeps its w, reads
    the trailing cell once and walks the rows with constant address steps (measured on MI355X:
    256^3 x 64 x 32 fp64 -2 %, fp32 -3.5 %) -- else (0, 0): entries dealt round-robin (with 9
    points on 16 groups of 32 lanes the first form leaves 44 % of the threads idle: +3 %)."""
    w = max(int(w), 1)
    best = (0, 0, 0.0)
    # (with 16-byte loads 32 lanes per point measured best: 256^3 x 64 x 32 fp64 1.65 ms, 64: 1.74, 16: 1.74)
    for lw in ((32, 64, 16, 8) if rows_per_lane > 1 else (64, 32, 16, 8)):
        if lw * rows_per_lane > rows or threads % lw:
            continue
        groups = threads // lw
        util = w / float(-(-w // groups) * groups)
        if util > best[2] + 1e-9:
            best = (2, lw, util)
    return (best[0], best[1]) if best[2] >= 0.85 else (0, 0)


BNB_PAD = 16                 # SDP_BNB_PAD_ROWS of csrc/sdp_column_kernel.h where a unit pads its reduced table




def bnb_words(n_controls):
    """reals of block statistics kept beside a control table of `n_controls` controls (SDP_BNB_WORDS of
    csrc/sdp_column_kernel.h: four per block of 8 controls, larger blocks beyond 64 of them)"""
    n = max(int(n_controls), 1)
    block = 8
    while (n + block - 1) // block > 64:
        block *= 2
    return 4 * ((n + block - 1) // block + 1)


def utab_reals(n_values, n_controls):
    """reals per parity buffer of a control table of `n_values` sub-expressions x `n_controls` controls, with the
    block statistics of the branch and bound (what `utab_values` of the planning functions counts; 0: no table)"""
    return int(n_values) * int(n_controls) + bnb_words(n_controls) if n_values else 0


def _column_lds(tw, w, rows, n_state, rs, threads, reduced=False, shift=False, shift_rows=0, utab_values=0,
                partial_minima=False, bnb_pad=False):
    """sizeof(SdpColLds) of csrc/sdp_column_kernel.h, member by member with the alignment rules of
    the C++ struct.  tw: perturbation points the table holds (SDP_COL_TW; SDP_COL_WRES of the resident-chunk
    form; SDP_COL_WCHUNK of the table per control); rows: rows of axis 0 the table holds;
    reduced: with the reduced table `ad` of the certified filter (full-column table) -- one real per row in the
    lean form of 8-byte reals, 16 bytes per row otherwise;
    shift: the shifted lattice -- `ad` then has `shift_rows` rows of two reals -- and the shifts of the
    perturbation points; utab_values: reals per parity buffer of the control table (0: the struct's two);
    partial_minima: the unfiltered sweep's per-thread partial minima (SDP_COL_LDS_PART);
    bnb_pad: the resident-chunk form of 8-byte reals without the shifted lattice -- `ad` is padded by BNB_PAD rows on
    either side (SDP_BNB_PAD: the uniform bound stage of the branch and bound)."""
    dt = n_state - 1
    part = threads if partial_minima else 1
    members = [(rs, tw * rows, 16),                          # T
               (rs, w * dt, rs), (rs, w * dt, rs),           # w_lam, w_oml
               (rs, 2, rs),                                  # reserve_
               (rs, part, rs), (4, part, 4),                 # part_J, part_i
               (4, w * dt, 4),                               # w_off
               (4, 4, 4), (4, 1, 4), (8, 2, 8),              # win, next_unit, dcol
               (rs, 2 * (int(utab_values) + 4 if utab_values else 2), 16)]        # utab[2][.. + 4 column statistics]
    if reduced or shift:
        per_row = 4 if rs == 4 else (2 if shift else 1)      # SDP_COL_LDS_AD (8-byte reals: the lean form is the default)
        members.append((rs, per_row * int(shift_rows if shift else rows) + (2 * BNB_PAD if bnb_pad and not shift else 0), 16))    # ad
    if shift:
        members += [(4, 2 * w, 4), (rs, 2 * w, rs), (rs, 2 * w, rs), (4, 8, 4)]                   # sh_q, sh_f, sh_c, sh_k
    off = 0
    for size, count, align in members:
        off = (off + align - 1) // align * align + size * int(count)
    return (off + 15) // 16 * 16


def column_percontrol_config(n0, w, n_state, dtype, debug=None):
    """Shape of the column kernel with a table per control (SDP_TRAIL_HAS_U of
    csrc/sdp_column_kernel.h): (threads, lds_bytes, w_chunk).  One thread per node of
    a column (at most 512; longer columns are split over workgroups), and a table of
    `w_chunk` perturbation points at a time, about 32 KiB: four to five workgroups
    then share a CU and hide each other's barriers and load latencies."""
    rs = np.dtype(dtype).itemsize
    w = max(int(w), 1)
    threads = min(512, max(64, (int(n0) + 63) // 64 * 64))
    wchunk = max(1, min(w, (32 * 1024) // (int(n0) * rs)))
    if _dbg(debug, 'SDP_COL_WCHUNK'):                   # A/B runs
        wchunk = max(1, min(w, int(_dbg(debug, 'SDP_COL_WCHUNK'))))
    lds = _column_lds(wchunk, w, n0, n_state, rs, threads)
    if lds > COLUMN_LDS_MAX:
        return None
    return threads, lds, wchunk


def column_window_config(n0, w, n_state, dtype, reach_rows):
    """Row-window shape of the column kernel for a grid whose full W x n0 table
    does not fit the LDS of a CU (SDP_COL_ROWS of csrc/sdp_column_kernel.h):
    (threads, lds_bytes, rows, seg_nodes) or None.  A unit is a segment of
    `seg_nodes` nodes of a column; its table holds `rows` rows of axis 0, enough
    for the segment plus `reach_rows` (the rows the controls of ONE node span,
    measured by the caller) plus the interpolation partner and a margin.  Two
    512-thread workgroups per CU, where that leaves segments of >= 64 nodes.
    (A 1024-thread form with one workgroup per CU is not planned: its image
    never fitted the LDS before its partial minima were counted, and once they
    were, its first run gave a wrong J -- tests/test_gpu_call_to_call.py.)"""
    rs = np.dtype(dtype).itemsize
    w = max(int(w), 1)
    for threads, wgs in ((512, 2),):
        budget = COLUMN_LDS_MAX // wgs
        # (the row window sweeps unfiltered: the image holds a partial minimum per thread, SDP_COL_LDS_PART)
        fixed = _column_lds(w, w, 0, n_state, rs, threads, partial_minima=True)
        rows = (budget - fixed) // (w * rs)
        rows = min(rows // 32 * 32, n0)
        seg = (rows - int(reach_rows) - 4) // 64 * 64
        if rows >= 128 and seg >= 64:
            return (threads, _column_lds(w, w, rows, n_state, rs, threads, partial_minima=True), int(rows),
                    int(min(seg, n0)))
    return None


def column_lds_bytes(n0, w, n_state, dtype):
    """LDS bytes of the column kernel's image (struct SdpColLds), plain table."""
    cfg = column_config(n0, w, n_state, dtype)
    return cfg[1] if cfg else COLUMN_LDS_MAX + 1


# ---------------------------------------------------------------------------
# One column unit, planned once: everything `_column_lines` prints and `solver.plan_info` reports.
#   form            'full table' / 'resident chunks' / 'row window' / 'table per control'
#   n0, w           rows of axis 0, perturbation points (0: none)
#   max_controls    capacity of a node's control lattice (a horizon's steps share a unit), n_columns: columns of the grid
#   threads, lds_bytes          workgroup size, sizeof(SdpColLds)
#   filtered        the certified filter (SDP_COL_FILTER); wpair: SDP_COL_WPAIR
#   shift, shift_rows           first pass on the shifted lattice (SDP_COL_SHIFT) and the rows of that lattice
#   wres            perturbation points resident at a time (SDP_COL_WRES; 0: the whole table)
#   frontier, utab_n            the control table's sub-expressions (None: no table) and its capacity in controls
#   short           the short first pass: 'none' / 'lean2' (resident chunks, 8-byte reals) / 'wide2' (full table, 4-byte)
#   bnb             .. as a branch and bound over blocks of controls (SDP_COL_BNB)
#   bnb_pad, uniform            rows the reduced table is padded by (SDP_BNB_PAD_ROWS) and the uniform bound stage on them
#   eval_delta, eval_dx, eval_unit_axis     the uniform evaluation stage (SDP_BNB_UNIFORM_EVAL; eval_delta 0.0: not planned): the
#                   rows its positions may lie from the reference's, the node's share of them that the kernel checks, and
#                   whether the roundings were counted for the axis [0, 1] (uniform_eval_plan)
#   window_rows, seg_nodes      rows of the row window's table; nodes of a column per unit (0: the whole column)
#   wchunk          perturbation points per table of the table per control (SDP_COL_WCHUNK)
#   unroll_w, min_waves, a_lw, a_group, wide_loads, tail_hold, bnb_chunk, colu_wide_loads
#                   the tuning macros the planner defines (SDP_COL_UNROLL_W .. SDP_COLU_WIDE_LOADS); None: not defined -- the
#                   header's default, or the value an explicit `debug` dict carries (copied as it is); a_lw None: the build
#                   deals its entries round-robin (no SDP_COL_A_ORDER)
#   reduce_fused, dmax_hi
#                   the reductions of the plain resident-chunk form (SDP_COL_REDUCE_FUSED, SDP_COL_DMAX_HI; None: not planned) --
#                   table_phase_plan
# ---------------------------------------------------------------------------
ColumnUnit = collections.namedtuple('ColumnUnit', (
    'form', 'n0', 'w', 'max_controls', 'n_columns', 'threads', 'lds_bytes',
    'filtered', 'wpair', 'shift', 'shift_rows', 'wres', 'frontier', 'utab_n', 'short', 'bnb', 'bnb_pad', 'uniform',
    'window_rows', 'seg_nodes', 'wchunk',
    'unroll_w', 'min_waves', 'a_lw', 'a_group', 'wide_loads', 'tail_hold', 'bnb_chunk', 'colu_wide_loads',
    'eval_delta', 'eval_dx', 'eval_unit_axis', 'reduce_fused', 'dmax_hi'),
    defaults=(False, False, False, 0, 0, None, 0, 'none', False, 0, False, 0, 0, 0) + (None,) * 8 + (0.0, 0.0, False)
    + (None,) * 2)


def _with_build_order(unit, dtype, debug):
    """`unit` with how phase A deals the table's entries to the threads (every form but the table per control)"""
    rs = np.dtype(dtype).itemsize
    window = unit.window_rows or None
    wide = column_wide_loads(unit.n0, dtype, window, debug)
    order, lw = column_build_order(unit.threads, unit.w, unit.window_rows or unit.n0, (16 // rs) if wide else 1)
    if order != 2:
        return unit
    lw = int(_dbg(debug, 'SDP_COL_A_LW') or lw)
    more = dict(a_lw=lw)
    if rs == 4 and unit.n0 >= 512 and not unit.wres and window is None and not _dbg(debug, 'SDP_COL_A_GROUP'):
        # (config 5, 512^3 in 4-byte reals, same box: 7.50 -> 7.36 ms, with four blocks' bounds per stage of
        # the branch and bound 7.24 ms -- boxes 25-26 of profiles/r06_column_ab.txt; 8-byte reals: worse)
        more['a_group'] = 8
    if wide and not _dbg(debug, 'SDP_COL_A_WIDE_LOADS'):
        more['wide_loads'] = 1
        # resident chunks: the tail is built once, its entries wait in the registers of the threads that made
        # them (SDP_COL_TAIL_HOLD of csrc/sdp_colres_kernel.h; round 6: 1.235 -> 1.048 ms on the benchmark, same
        # bits) -- where they are whole rounds of points and rows and at most 32 registers per thread
        # (on the shifted lattice too since the second pass is no longer unrolled there: 2.23 -> 2.12 ms, box 11 of
        # profiles/r06_column_ab.txt; with the unrolled pass it had lost, 2.96 against 2.71 ms)
        if unit.wres and rs == 8 and not unit.wpair and window is None and _dbg(debug, 'SDP_COL_TAIL_HOLD') is None:
            tail, groups = unit.w - unit.wres, unit.threads // lw
            if (tail > 0 and tail % groups == 0 and unit.n0 % (2 * lw) == 0
                    and (tail // groups) * (unit.n0 // (2 * lw)) * 4 <= 32):
                more['tail_hold'] = 1
    return unit._replace(**more)


def table_phase_plan(unit, dtype, debug=None):
    """THE place that decides the lean reductions of a unit (round 11): `unit` with reduce_fused and dmax_hi set where they
    apply -- the plain resident-chunk form of 8-byte reals, not the shifted lattice.  A[r] and the column's bound feed the
    certified filter only: no value of the result depends on either.  (`debug`: NAME = 0 leaves an item out.)"""
    rs = np.dtype(dtype).itemsize
    if not (unit.form == 'resident chunks' and unit.wres and rs == 8 and unit.filtered and not unit.shift and not unit.wpair):
        return unit
    on = lambda name: _dbg(debug, name) != '0'
    return unit._replace(reduce_fused=1 if on('SDP_COL_REDUCE_FUSED') else None,
                         dmax_hi=1 if on('SDP_COL_DMAX_HI') else None)


def _short_pass(model, dtype, unit, debug):
    """(short, bnb, bnb_chunk) of a full-table or resident-chunk unit: the short first passes -- 8-byte reals in the
    resident-chunk kernel, 4-byte reals (wide form) in the full-table one -- of a model x0' = X(x) +- a(u),
    cost = K(x) +- h(u) with a control table (round 6: on the shifted lattice too -- final sums only,
    additive_control_split).  (`debug`: SDP_COL_LEAN2 = 0 takes them away, SDP_COL_BNB = 0 their branch and bound.)"""
    rs = np.dtype(dtype).itemsize
    short = 'none'
    if (unit.frontier is not None and not model.cost_depends_on_w and _dbg(debug, 'SDP_COL_LEAN2') != '0'
            and (not unit.shift or rs == 8)):
        if rs == 8 and unit.wres:
            short = 'lean2'
        elif rs == 4 and not unit.wres and _dbg(debug, 'SDP_COL_FILTER_TOP2') in (None, '1'):
            short = 'wide2'
    if short != 'none' and model.additive_control_split(unit.frontier) is None:
        short = 'none'
    bnb = short != 'none' and _dbg(debug, 'SDP_COL_BNB') != '0'
    chunk = 4 if (short == 'wide2' and bnb and unit.n0 >= 512 and not _dbg(debug, 'SDP_BNB_CHUNK')) else None
    return short, bnb, chunk


def column_table_unit(model, dtype, shape, W, max_controls, box, axis, certified_filter=True, debug=None):
    """The column kernel whose table holds every row of axis 0 (all W points of it, or a resident chunk), for a
    storage-separable model on a grid of `shape`: a ColumnUnit, or None where the table does not fit the LDS of a CU.
    The shape is planned ONCE, with everything that sizes its LDS image (the control table, the padding of the
    uniform bound stage), and printed as it is.  `box`: the table of admissible boxes (lo, hi, n, per_node), `axis`:
    the grid of the stock, `certified_filter`: whether the solver wants the filter where it applies."""
    rs = np.dtype(dtype).itemsize
    n0, n_state, n_columns = int(shape[0]), len(shape), int(np.prod(shape[1:]))
    filtered = bool(certified_filter and column_filter_applies(model, dtype=dtype, table=(n0, W, n_state), debug=debug))
    wpair = bool(use_wpair(model, dtype, debug))
    shift = bool(filtered and column_shift_applies(model, dtype, debug=debug))
    fr = control_table_plan(model, dtype, box['per_node'], max_controls, debug) if filtered else None
    for frontier in ((fr, None) if fr is not None else (None,)):
        kw = dict(max_controls=max_controls, n_columns=n_columns, shift=shift,
                  utab_values=utab_reals(len(frontier), max_controls) if frontier else 0, debug=debug)
        cfg = column_config(n0, W, n_state, dtype, wpair, filtered, **kw)
        if cfg is not None:                   # (else once more without the control table)
            break
    else:
        return None
    # the table a chunk of perturbation points at a time, where that lets more workgroups share a CU
    wres = column_resident_points(model, n0, W, n_state, dtype, filtered, shift, wpair, cfg[0], kw['utab_values'], debug)
    if wres:
        cfg = column_config(n0, W, n_state, dtype, wpair, filtered, wres=wres, **kw)
        if cfg is None:
            return None
    unit = ColumnUnit('resident chunks' if wres else 'full table', n0, int(W), int(max_controls), n_columns,
                      int(cfg[0]), int(cfg[1]), filtered=filtered, wpair=wpair, shift=shift,
                      shift_rows=int(cfg[2]) if shift else 0, wres=int(wres), frontier=frontier,
                      utab_n=int(max_controls) if frontier is not None else 0)
    short, bnb, chunk = _short_pass(model, dtype, unit, debug)
    unit = unit._replace(short=short, bnb=bnb, bnb_chunk=chunk)
    # (a uniform stock axis under x0' = x0 +- a: the branch and bound's uniform bound stage, which pads the reduced
    # table -- the last member of the image -- where that costs the CU no workgroup.  SDP_BNB_UNIFORM = 0 keeps the
    # PADDING and leaves the stage out: the A/B switch)
    pad = uniform_stage_pad(model, dtype, unit, axis, box)
    if pad:
        unit = unit._replace(bnb_pad=pad, uniform=_dbg(debug, 'SDP_BNB_UNIFORM') != '0',
                             lds_bytes=_column_lds(unit.wres, max(unit.w, 1), n0, n_state, rs, unit.threads, reduced=True,
                                                   utab_values=kw['utab_values'], bnb_pad=True))
        # (.. and its uniform evaluation stage, at no cost in LDS; SDP_BNB_UNIFORM_EVAL = 0 leaves it out: the A/B switch)
        ev = uniform_eval_plan(model, dtype, unit, axis, debug)
        if ev:
            unit = unit._replace(eval_delta=ev[0], eval_dx=ev[1], eval_unit_axis=ev[2])
    if wres and rs == 8 and shift and not _dbg(debug, 'SDP_COL_UNROLL_W'):
        # the second pass of the shifted lattice's resident-chunk kernel one batch of perturbation points at a time: unrolled
        # four times it kept 8 points' cells, table entries and weights per survivor in flight (two survivors in half of the
        # waves), in registers the kernel does not have at three waves per SIMD -- round 6, same box: 2.45 -> 2.23 ms, and
        # with the tail held on top 2.12 ms (boxes 9-11 of profiles/r06_column_ab.txt: 48 -> 22 spilled registers).  The
        # benchmark's kernel (no cell per point, one survivor) does not care: 948.8 against 954.3 sweeps/s over 50 steps
        # (box 20; the 5 % of box 12 were the A/B tool's first-position penalty); 4-byte reals: 7.51 against 7.72 ms.
        unit = unit._replace(unroll_w=1)
    if filtered and unit.threads <= 256 and not _dbg(debug, 'SDP_COL_MIN_WAVES'):
        # resident chunks: as many waves per SIMD as the LDS image admits workgroups per CU, at most 4 (128 registers
        # per lane.  Round 4 asked for up to 8 for small tables -- 64 registers, which these kernels do not fit in:
        # 90 - 200 spilled registers in the suite's small models, and spill code the compiler got wrong, see
        # spill_hazards); else the small workgroups of the filtered kernel, without a register cap
        unit = unit._replace(min_waves=(max(1, min(4, (COLUMN_LDS_MAX // unit.lds_bytes) * unit.threads // 256))
                                        if wres else 1))
    return table_phase_plan(_with_build_order(unit, dtype, debug), dtype, debug)


def column_percontrol_unit(model, dtype, shape, W, max_controls, debug=None):
    """The column kernel with a table per control, for trailing next states that depend on the control but not on x0
    (the nodes of a column still share a table, control by control: SDP_TRAIL_HAS_U of csrc/sdp_column_kernel.h): a
    ColumnUnit, or None.  The caller sees to it that the nodes of a column share their control values."""
    if not (model.column_shareable and model.trail_depends_on_u):
        return None
    n0 = int(shape[0])
    cfg = column_percontrol_config(n0, W, len(shape), dtype, debug)
    if cfg is None:
        return None
    wide = n0 % (16 // np.dtype(dtype).itemsize) == 0 and not _dbg(debug, 'SDP_COLU_WIDE_LOADS')
    return ColumnUnit('table per control', n0, int(W), int(max_controls), int(np.prod(shape[1:])), int(cfg[0]), int(cfg[1]),
                      wpair=bool(use_wpair(model, dtype, debug)), seg_nodes=int(cfg[0]), wchunk=int(cfg[2]),
                      colu_wide_loads=1 if wide else None)


def column_window_unit(model, dtype, shape, W, max_controls, reach_rows, debug=None):
    """The column kernel of a storage-separable model whose W x N0 table exceeds the LDS of a CU: a window of rows
    per segment of the column (SDP_COL_ROWS of csrc/sdp_column_kernel.h; `reach_rows`: the rows the controls of one
    node span).  A ColumnUnit, or None."""
    n0 = int(shape[0])
    cfg = column_window_config(n0, W, len(shape), dtype, reach_rows)
    if cfg is None:
        return None
    unit = ColumnUnit('row window', n0, int(W), int(max_controls), int(np.prod(shape[1:])), int(cfg[0]), int(cfg[1]),
                      window_rows=int(cfg[2]), seg_nodes=int(cfg[3]))
    return _with_build_order(unit, dtype, debug)


HIPCC_FLAGS = ['--genco', '--offload-arch=gfx950', '-O3', '-ffp-contract=off',
               '-fno-fast-math', '-std=c++17', '-I', CSRC]


_HEADERS = ('sdp_kernel_args.h', 'sdp_device.h', 'sdp_sweep_kernel.h', 'sdp_mc_kernel.h', 'sdp_trans_kernel.h', 'sdp_column_kernel.h', 'sdp_colfilter_kernel.h', 'sdp_colres_kernel.h',
            'sdp_colfull_kernel.h', 'sdp_colu_kernel.h',
            'sdp_lead_kernel.h', 'sdp_staged_kernel.h', 'sdp_horizon_kernel.h', 'sdp_trans_horizon_kernel.h')
_digest_cache = {}


def _headers_digest():
    """sha256 state over the kernel headers (re-read only when a file changes)"""
    stamp = tuple(os.stat(os.path.join(CSRC, fn)).st_mtime_ns for fn in _HEADERS)
    h = _digest_cache.get(stamp)
    if h is None:
        h = hashlib.sha256()
        for fn in _HEADERS:
            with open(os.path.join(CSRC, fn), 'rb') as f:
                h.update(f.read())
        _digest_cache.clear()
        _digest_cache[stamp] = h
    return h.copy()


_compiler_id = None
HIPCC_PATH = '/opt/rocm/bin/hipcc'       # (_native.py, which reads HIPCC from the environment, sets it)


def compiler_identity():
    """What `hipcc --version` prints (HIP version, clang version and commit), once per process: part of every
    cache key, so that code objects built by another compiler -- a cache that travelled from a container with a
    different ROCm -- are never picked up (the key named the source, headers and flags only).
    Without a runnable hipcc the identity is a fixed string: nothing can be compiled then anyway."""
    global _compiler_id
    if _compiler_id is None:
        import subprocess
        try:
            out = subprocess.run([HIPCC_PATH, '--version'], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                                 timeout=60).stdout.decode(errors='replace')
            # (the lines that name the compiler; not the installation directory, which may be a symlink)
            keep = [ln.strip() for ln in out.splitlines() if ln.startswith(('HIP version', 'AMD clang version', 'clang version'))]
            _compiler_id = '\n'.join(keep) or 'hipcc without a version'
        except (OSError, subprocess.SubprocessError):
            _compiler_id = 'no hipcc'
    return _compiler_id


BUILD_RULES = 'spill fence 1'       # what _native.compile_model does beyond one hipcc call (below): part of the key


def source_key(source):
    """Cache key of a code object: generated text + kernel headers + flags + the compiler's identity."""
    h = _headers_digest()
    # (headers only some units include enter the key of those units alone: an edit there leaves the other code objects valid)
    if '#define SDP_LINE ' in source:
        with open(os.path.join(CSRC, 'sdp_line_kernel.h'), 'rb') as f:
            h.update(f.read())
    if '#define SDP_NW ' in source:
        with open(os.path.join(CSRC, 'sdp_multiw_kernel.h'), 'rb') as f:
            h.update(f.read())
    if '#define SDP_LOOKAHEAD ' in source:
        for fn in ('sdp_lookahead_kernel.h', 'sdp_lattice_kernel.h'):
            with open(os.path.join(CSRC, fn), 'rb') as f:
                h.update(f.read())
    if '#define SDP_FAMILY ' in source:
        with open(os.path.join(CSRC, 'sdp_family_kernel.h'), 'rb') as f:
            h.update(f.read())
    if '#define SDP_FAMILY_POLICY ' in source:
        with open(os.path.join(CSRC, 'sdp_family_policy_kernel.h'), 'rb') as f:
            h.update(f.read())
    if '#define SDP_FAMILY_MC ' in source:
        with open(os.path.join(CSRC, 'sdp_family_mc_kernel.h'), 'rb') as f:
            h.update(f.read())
    if '#define SDP_FAMILY_HORIZON ' in source:
        # (it includes sdp_family_kernel.h, above, and sdp_mc_kernel.h, one of _HEADERS)
        with open(os.path.join(CSRC, 'sdp_family_horizon_kernel.h'), 'rb') as f:
            h.update(f.read())
    if '#define SDP_FAMILY_TRANS ' in source:
        with open(os.path.join(CSRC, 'sdp_family_trans_kernel.h'), 'rb') as f:
            h.update(f.read())
    if '#define SDP_FAMILY_LOOKAHEAD ' in source:
        # (it includes sdp_family_kernel.h, above, sdp_mc_kernel.h, one of _HEADERS, and the lattice rule)
        for fn in ('sdp_family_lookahead_kernel.h', 'sdp_lattice_kernel.h'):
            with open(os.path.join(CSRC, fn), 'rb') as f:
                h.update(f.read())
    if '#define SDP_FAMILY_LOOKAHEAD_HORIZON ' in source:
        # (it includes sdp_family_lookahead_kernel.h for its helpers, and with it what that header includes)
        for fn in ('sdp_family_lookahead_horizon_kernel.h', 'sdp_family_lookahead_kernel.h', 'sdp_lattice_kernel.h'):
            with open(os.path.join(CSRC, fn), 'rb') as f:
                h.update(f.read())
    h.update(source.encode())
    h.update(' '.join(HIPCC_FLAGS[:-1]).encode())
    h.update(compiler_identity().encode())
    h.update(BUILD_RULES.encode())
    return h.hexdigest()[:24]


# ---------------------------------------------------------------------------
# Spill code and the execution mask.  Round 5 found a kernel of the test suite (resident chunks, long first pass,
# 128 threads under a budget of 64 vector registers) that never ended: the compiler (ROCm 7.2's clang 20) had put the
# store of a spilled vector register -- threadIdx.x -- at the top of a block where divergent paths JOIN, before the
# instruction that restores the execution mask (`s_or_b64 exec, exec, s[..]`).  A store to scratch memory writes the
# active lanes only: a wavefront that had skipped the branch altogether stored nothing, reloaded whatever its scratch
# memory held, took itself for wave 0 and never claimed the workgroup's next unit.  Which kernels are hit depends on
# the register allocation alone -- three unrelated one-line changes each made it come and go -- so the build LOOKS:
# a code object whose kernels use scratch memory or accumulation registers (the two places spilled vector registers
# go) is compiled to assembly once more and scanned for exactly this pattern; a kernel that shows it is rebuilt with
# fewer waves per SIMD asked of the register allocator (more registers, less spill code) until it is clean, or refused.
# ---------------------------------------------------------------------------
_ASM_FUNC = re.compile(r'^([A-Za-z_]\w*):\s*; @')
_ASM_BLOCK = re.compile(r'^(\.LBB\d+_\d+):|^; %bb\.(\d+):')
_ASM_SPILL = re.compile(r'^\s+(?:scratch_(?:store|load)\w*|buffer_(?:store|load)\w*|v_accvgpr_(?:write|read)\w*)\b.*;.*\b(?:Spill|Reload)\b')
_ASM_END_CF = re.compile(r'^\s+s_or_b64\s+exec,\s*exec,')
_ASM_EXEC_WRITE = re.compile(r'^\s+s_\w+\s+exec(?:_lo|_hi)?\b|^\s+s_\w*saveexec\w*\b|^\s+v_cmpx')


def spill_hazards(asm):
    """[(kernel, block, line number of the mask restore, [spill instructions before it]), ...] of an assembly listing
    (hipcc -S): spill stores / reloads of vector registers between the top of a basic block and the `s_or_b64 exec,
    exec, ..` that re-activates the lanes joining there.  Those instructions run for the lanes of ONE incoming path."""
    out, func, block, pending, at_top = [], None, None, [], False
    for n, line in enumerate(asm.splitlines(), 1):
        m = _ASM_FUNC.match(line)
        if m:
            func, block, pending, at_top = m.group(1), 'entry', [], False     # (the entry block: every launched lane is active)
            continue
        m = _ASM_BLOCK.match(line)
        if m:
            block, pending, at_top = m.group(1) or '%bb.' + m.group(2), [], True
            continue
        if not at_top:
            continue
        if _ASM_SPILL.match(line):
            pending.append(line.strip())
        elif _ASM_END_CF.match(line):
            if pending:
                out.append((func, block, n, pending))
            at_top = False
        elif _ASM_EXEC_WRITE.match(line):
            at_top = False
    return out


def _msgpack_ints_after(blob, key):
    out, i = [], blob.find(key)
    while i >= 0:
        j = i + len(key)
        b = blob[j] if j < len(blob) else 0
        out.append(b if b <= 0x7f else int.from_bytes(blob[j + 1:j + 1 + {0xcc: 1, 0xcd: 2, 0xce: 4}.get(b, 0)], 'big') if b in (0xcc, 0xcd, 0xce) else -1)
        i = blob.find(key, j)
    return out


def code_object_may_spill(blob):
    """True when a kernel of the code object (its bytes) uses scratch memory or accumulation registers, by its own
    metadata (the msgpack note: .private_segment_fixed_size, .agpr_count), or when the metadata cannot be read."""
    scratch = _msgpack_ints_after(blob, b'.private_segment_fixed_size')
    agprs = _msgpack_ints_after(blob, b'.agpr_count')
    if not scratch or len(agprs) != len(scratch):
        return True
    return any(v != 0 for v in scratch) or any(v != 0 for v in agprs)
