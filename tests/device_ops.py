"""The operators of trace._OPS as a table: which numpy / Python spellings reach each of them, on which operands the
device is compared with numpy, and how (tests/test_device_ops_table.py checks the table itself without a GPU,
tests/test_gpu_device_ops.py runs it on the device; __graft_entry__.build compiles its units ahead).

The harness: sdp_simulate hands x0[:, b] and w[0, b] to the generated sdp_model_cell unchanged, so a model whose
dynamics are the identity and whose cost is  where(t == 0, f_0(a, b, c), where(t == 1, f_1(a, b, c), ..))  yields, from
ONE launch of T steps,  g[k, b] = f_k(x0[b, 0], x0[b, 1], w[b])  for arbitrary operands: NaN, infinities, signed zeros,
denormals.  The reference is the very same Python callable on numpy arrays of the problem's real type.

A row's first spelling is what runs on the device; the others must trace to the SAME graph (hence the same C++), which
the CPU test asserts, so they need no launch of their own."""
import collections
import math

import numpy as np

from stodynprog_amd import SysDescription, DPSolver, models

DTYPES = {'f8': np.float64, 'f4': np.float32}
UINT = {'f8': np.uint64, 'f4': np.uint32}
ROWS_PER_UNIT = 12

Row = collections.namedtuple('Row', 'name op arity exact spellings names dtypes mp domain')


def _num(cond, like):
    """a boolean as a number of `like`'s real type (np.where of two Python floats would be float64)"""
    return np.where(cond, np.ones_like(like), np.zeros_like(like))


# ---------------------------------------------------------------------------------------------------------- np.interp tables
# (8-byte problems only: numpy evaluates np.interp in float64 whatever the type of x, so a 4-byte model that uses it
# has no float32 restatement in numpy -- the width assertion of the reference refuses it)
_XP = np.array([-1.0, -0.5, 0.0, 0.5, 1.0])
_FP = np.array([1.0, -2.0, 0.25, 3.0, -0.75])
_XP_REP = np.array([-1.0, 0.0, 0.0, 0.5, 0.5, 0.5, 1.0])
_FP_REP = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0])
_FP_INF = np.array([0.0, np.inf, np.inf, 1.0, -np.inf])      # slope NaN, +-inf: every fall-back of INTERP_SOURCE
_FP_INF2 = np.array([-np.inf, 1.0, np.inf, -np.inf, 2.0])

ROWS = []


def _row(name, op, arity, exact, spellings, names=(), dtypes=('f8', 'f4'), mp=None, domain=None):
    if callable(spellings):
        spellings = [spellings]
    ROWS.append(Row(name, op, arity, exact, list(spellings), tuple(names), tuple(dtypes), mp, domain))


# ---- arithmetic --------------------------------------------------------------------------------------------------------
_row('add', 'add', 2, True, [lambda a, b, c: np.add(a, b), lambda a, b, c: a + b, lambda a, b, c: np.positive(a) + (+b)],
     ['add', '+', 'positive', 'pos'])
_row('add const', 'add', 1, True, [lambda a, b, c: a + 1.5, lambda a, b, c: np.add(a, 1.5)], ['+'])
_row('radd const', 'add', 1, True, lambda a, b, c: 1.5 + a, ['r+'])
_row('sub', 'sub', 2, True, [lambda a, b, c: np.subtract(a, b), lambda a, b, c: a - b], ['subtract', '-'])
_row('rsub const', 'sub', 1, True, lambda a, b, c: 1.5 - a, ['r-'])
_row('mul', 'mul', 2, True, [lambda a, b, c: np.multiply(a, b), lambda a, b, c: a * b], ['multiply', '*'])
_row('rmul const', 'mul', 1, True, lambda a, b, c: 3.0 * a, ['r*'])
_row('div', 'div', 2, True, [lambda a, b, c: np.divide(a, b), lambda a, b, c: np.true_divide(a, b),
                             lambda a, b, c: a / b], ['divide', 'true_divide', '/'])
_row('rdiv const', 'div', 1, True, [lambda a, b, c: 1.0 / a, lambda a, b, c: np.reciprocal(a)], ['r/', 'reciprocal'])
_row('neg', 'neg', 1, True, [lambda a, b, c: np.negative(a), lambda a, b, c: -a], ['negative', 'neg'])
_row('abs', 'abs', 1, True, [lambda a, b, c: np.absolute(a), lambda a, b, c: np.abs(a), lambda a, b, c: np.fabs(a),
                             lambda a, b, c: abs(a)], ['absolute', 'fabs', 'abs'])
_row('sqrt', 'sqrt', 1, True, lambda a, b, c: np.sqrt(a), ['sqrt'])
_row('square', 'square', 1, True, [lambda a, b, c: np.square(a), lambda a, b, c: np.power(a, 2)], ['square', 'power'])
_row('floor', 'floor', 1, True, lambda a, b, c: np.floor(a), ['floor'])
_row('ceil', 'ceil', 1, True, lambda a, b, c: np.ceil(a), ['ceil'])
_row('trunc', 'trunc', 1, True, lambda a, b, c: np.trunc(a), ['trunc'])
_row('rint', 'rint', 1, True, lambda a, b, c: np.rint(a), ['rint'])
_row('sign', 'sign', 1, True, lambda a, b, c: np.sign(a), ['sign'])
_row('min', 'min', 2, True, lambda a, b, c: np.minimum(a, b), ['minimum'])
_row('max', 'max', 2, True, lambda a, b, c: np.maximum(a, b), ['maximum'])
_row('fmin', 'fmin', 2, True, lambda a, b, c: np.fmin(a, b), ['fmin'])
_row('fmax', 'fmax', 2, True, lambda a, b, c: np.fmax(a, b), ['fmax'])
_row('fmod', 'fmod', 2, True, lambda a, b, c: np.fmod(a, b), ['fmod'])
_row('pymod', 'pymod', 2, True, [lambda a, b, c: np.remainder(a, b), lambda a, b, c: np.mod(a, b),
                                 lambda a, b, c: a % b], ['remainder', 'mod', '%'])
_row('rpymod const', 'pymod', 1, True, lambda a, b, c: 5.0 % a, ['r%'])
_row('floordiv', 'floordiv', 2, True, [lambda a, b, c: np.floor_divide(a, b), lambda a, b, c: a // b],
     ['floor_divide', '//'])
_row('rfloordiv const', 'floordiv', 1, True, lambda a, b, c: 5.0 // a, ['r//'])
# ---- clip, heaviside ---------------------------------------------------------------------------------------------------
_row('clip', 'min', 3, True, [lambda a, b, c: np.clip(a, b, c), lambda a, b, c: a.clip(b, c)], ['clip', '.clip'])
# (constant bounds run another loop of numpy's than bounds that are arrays: a value equal to a bound keeps its own sign)
_row('clip const', 'select', 1, True, [lambda a, b, c: np.clip(a, -1.0, 1.0), lambda a, b, c: a.clip(-1.0, 1.0)], ['clip'])
_row('clip zeros', 'select', 1, True, lambda a, b, c: np.clip(a, -0.0, 0.0), ['clip'])
_row('clip zeros 2', 'select', 1, True, lambda a, b, c: np.clip(a, 0.0, -0.0), ['clip'])
_row('clip one const', 'min', 2, True, lambda a, b, c: np.clip(a, 0.0, b), ['clip'])
_row('clip below', 'max', 2, True, lambda a, b, c: np.clip(a, b, None), ['clip'])
_row('clip above', 'min', 2, True, lambda a, b, c: np.clip(a, None, b), ['clip'])
_row('heaviside', 'select', 2, True, lambda a, b, c: np.heaviside(a, b), ['heaviside'])
# ---- comparisons (a NaN operand in every position), logic ---------------------------------------------------------------
for _name, _uf, _op in (('lt', np.less, lambda a, b: a < b), ('le', np.less_equal, lambda a, b: a <= b),
                        ('gt', np.greater, lambda a, b: a > b), ('ge', np.greater_equal, lambda a, b: a >= b),
                        ('eq', np.equal, lambda a, b: a == b), ('ne', np.not_equal, lambda a, b: a != b)):
    _row(_name, _name, 2, True, [lambda a, b, c, f=_uf: _num(f(a, b), a), lambda a, b, c, f=_op: _num(f(a, b), a)],
         [_uf.__name__, _name])
_row('and', 'and', 3, True, [lambda a, b, c: _num(np.logical_and(a > b, b > c), a),
                             lambda a, b, c: _num((a > b) & (b > c), a),
                             lambda a, b, c: _num(np.bitwise_and(a > b, b > c), a)], ['logical_and', '&', 'bitwise_and'])
_row('or', 'or', 3, True, [lambda a, b, c: _num(np.logical_or(a > b, b > c), a),
                           lambda a, b, c: _num((a > b) | (b > c), a),
                           lambda a, b, c: _num(np.bitwise_or(a > b, b > c), a)], ['logical_or', '|', 'bitwise_or'])
_row('xor', 'xor', 3, True, [lambda a, b, c: _num(np.logical_xor(a > b, b > c), a),
                             lambda a, b, c: _num((a > b) ^ (b > c), a),
                             lambda a, b, c: _num(np.bitwise_xor(a > b, b > c), a),
                             lambda a, b, c: _num((a > b) != (b > c), a)], ['logical_xor', '^', 'bitwise_xor', 'ne'])
_row('not', 'not', 2, True, [lambda a, b, c: _num(np.logical_not(a > b), a), lambda a, b, c: _num(~(a > b), a),
                             lambda a, b, c: _num(np.invert(a > b), a)], ['logical_not', '~', 'invert'])
_row('bool eq', 'not', 3, True, lambda a, b, c: _num((a > b) == (b > c), a), ['eq'])
# (numpy's truth value of a real: NaN is true, both zeros are false)
_row('and of reals', 'and', 2, True, lambda a, b, c: _num(np.logical_and(a, b), a), ['logical_and'])
_row('or of reals', 'or', 2, True, lambda a, b, c: _num(np.logical_or(a, b), a), ['logical_or'])
_row('xor of reals', 'xor', 2, True, lambda a, b, c: _num(np.logical_xor(a, b), a), ['logical_xor'])
_row('not of a real', 'not', 1, True, lambda a, b, c: _num(np.logical_not(a), a), ['logical_not'])
_row('isnan', 'isnan', 1, True, lambda a, b, c: _num(np.isnan(a), a), ['isnan'])
_row('isinf', 'isinf', 1, True, lambda a, b, c: _num(np.isinf(a), a), ['isinf'])
_row('isfinite', 'isfinite', 1, True, lambda a, b, c: _num(np.isfinite(a), a), ['isfinite'])
_row('select', 'select', 3, True, lambda a, b, c: np.where(a > b, b, c), ['where'])
_row('select on a real', 'select', 3, True, lambda a, b, c: np.where(a, b, c), ['where'])
_row('np.select', 'select', 3, True, lambda a, b, c: np.select([a > b, b > c], [a, b], c), ['select'])
_row('bselect', 'bselect', 3, True, lambda a, b, c: _num(np.where(a > 0, b > 0, c > 0), a), ['where'])
_row('b2r', 'b2r', 3, True, lambda a, b, c: (a < b) + c, ['+'])
_row('b2r product', 'b2r', 2, True, lambda a, b, c: (a >= b) * b, ['*'])
# ---- np.interp ----------------------------------------------------------------------------------------------------------
_row('interp', 'interp1', 1, True, lambda a, b, c: np.interp(a, _XP, _FP), ['interp'], dtypes=('f8',))
_row('interp left right', 'interp1', 1, True, lambda a, b, c: np.interp(a, _XP, _FP, left=-7.0, right=9.0), ['interp'],
     dtypes=('f8',))
_row('interp one knot', 'interp1', 1, True, lambda a, b, c: np.interp(a, [0.5], [2.0]), ['interp'], dtypes=('f8',))
_row('interp one knot left right', 'interp1', 1, True, lambda a, b, c: np.interp(a, [0.5], [2.0], left=-1.0, right=4.0),
     ['interp'], dtypes=('f8',))
_row('interp repeated knots', 'interp1', 1, True, lambda a, b, c: np.interp(a, _XP_REP, _FP_REP), ['interp'],
     dtypes=('f8',))
_row('interp infinite values', 'interp1', 1, True, lambda a, b, c: np.interp(a, _XP, _FP_INF), ['interp'], dtypes=('f8',))
_row('interp infinite values 2', 'interp1', 1, True, lambda a, b, c: np.interp(a, _XP, _FP_INF2, left=np.inf), ['interp'],
     dtypes=('f8',))
# ---- the exponent special cases of ** (c is the perturbation: an ARRAY power in the reference, see trace._power) -----------
_row('pow 2', 'square', 1, True, lambda a, b, c: c ** 2, ['**'])
_row('pow 1', 'add', 1, True, lambda a, b, c: c ** 1 + 0.5, ['**'])
_row('pow 0', 'add', 1, True, lambda a, b, c: c ** 0 + c, ['**'])
_row('pow 0.5', 'sqrt', 1, True, lambda a, b, c: c ** 0.5, ['**'])
_row('pow -1', 'recip', 1, True, lambda a, b, c: c ** -1, ['**'])


# ---- inexact rows: result class everywhere, error in ulps against mpmath on `domain` ---------------------------------------
def _finite(*v):
    return all(np.isfinite(x) for x in v)


def _mp(name):
    import mpmath
    mp = mpmath.mp
    two, ten = mpmath.mpf(2), mpmath.mpf(10)

    def power(x, y):
        # exp(y log|x|), never mpmath's own power: that one raises integers to integer exponents exactly, digit by digit
        if x == 0:
            raise ValueError
        if x < 0:
            if y != mp.floor(y):
                raise ValueError
            odd = mp.fmod(y, 2) != 0
            return -mp.exp(y * mp.log(-x)) if odd else mp.exp(y * mp.log(-x))
        return mp.exp(y * mp.log(x))
    table = {
        'exp': mp.exp, 'exp2': lambda x: mp.exp(x * mp.log(two)), 'expm1': mp.expm1, 'log': mp.log,
        'log2': lambda x: mp.log(x) / mp.log(two), 'log10': lambda x: mp.log(x) / mp.log(ten), 'log1p': mp.log1p,
        'sin': mp.sin, 'cos': mp.cos, 'tan': mp.tan, 'asin': mp.asin, 'acos': mp.acos, 'atan': mp.atan,
        'sinh': mp.sinh, 'cosh': mp.cosh, 'tanh': mp.tanh,
        'cbrt': lambda x: -mp.cbrt(-x) if x < 0 else mp.cbrt(x),
        'pow': power, 'atan2': mp.atan2, 'hypot': mp.hypot,
        'pow 3': lambda x: x * x * x, 'rpow': lambda x: mp.exp(x * mp.log(two)), 'pow half': mp.sqrt,
        'square': lambda x: x * x,
    }
    return table[name]


_ALL = 'every finite operand with a finite non-zero result'
for _name, _uf, _dom, _text in (
        ('exp', np.exp, None, _ALL), ('exp2', np.exp2, None, _ALL), ('expm1', np.expm1, None, _ALL),
        ('log', np.log, None, 'x > 0'), ('log2', np.log2, None, 'x > 0'), ('log10', np.log10, None, 'x > 0'),
        ('log1p', np.log1p, None, 'x > -1'),
        ('sin', np.sin, lambda x: abs(x) <= 1e6, '|x| <= 1e6'), ('cos', np.cos, lambda x: abs(x) <= 1e6, '|x| <= 1e6'),
        ('tan', np.tan, lambda x: abs(x) <= 1e6, '|x| <= 1e6'),
        ('asin', np.arcsin, lambda x: abs(x) <= 1, '|x| <= 1'), ('acos', np.arccos, lambda x: abs(x) <= 1, '|x| <= 1'),
        ('atan', np.arctan, None, _ALL), ('sinh', np.sinh, None, _ALL), ('cosh', np.cosh, None, _ALL),
        ('tanh', np.tanh, None, _ALL), ('cbrt', np.cbrt, None, _ALL)):
    _row(_name, _name, 1, False, lambda a, b, c, f=_uf: f(a), [_uf.__name__], mp=_name, domain=(_dom, _text))
_row('pow', 'pow', 2, False, [lambda a, b, c: a ** b, lambda a, b, c: np.power(a, b)], ['**', 'power'], mp='pow',
     domain=(None, _ALL))
_row('float_power', 'pow', 2, False, lambda a, b, c: np.float_power(a, b), ['float_power'], dtypes=('f8',), mp='pow',
     domain=(None, _ALL))       # (numpy's float_power is float64 whatever its operands)
_row('pow 3', 'pow', 1, False, lambda a, b, c: c ** 3, ['**'], mp='pow 3', domain=(None, _ALL))
_row('rpow', 'pow', 1, False, lambda a, b, c: 2.0 ** a, ['r**'], mp='rpow', domain=(None, _ALL))
_row('np.power 0.5', 'pow', 1, False, lambda a, b, c: np.power(c, 0.5), ['power'], mp='pow half', domain=(None, _ALL))
# (a power of the STATE alone is a numpy scalar power in the reference's node-by-node evaluation: flagged scalar_pow)
_row('pow 2 of a state', 'square', 1, False, lambda a, b, c: a ** 2, ['**'], mp='square', domain=(None, _ALL))
_row('atan2', 'atan2', 2, False, lambda a, b, c: np.arctan2(a, b), ['arctan2'], mp='atan2', domain=(None, _ALL))
_row('hypot', 'hypot', 2, False, lambda a, b, c: np.hypot(a, b), ['hypot'], mp='hypot', domain=(None, _ALL))

# operand of a unary row that is not `a`
OPERAND = {'pow 2': 2, 'pow 1': 2, 'pow 0': 2, 'pow 0.5': 2, 'pow -1': 2, 'pow 3': 2, 'np.power 0.5': 2}

# Largest distance, in representable numbers of the real type, between the device's result and the correctly rounded
# one (mpmath, 300 bits, on the exact operand) over this table's operands inside the row's domain, measured on an
# MI355X with ROCm 7's device library; the test asserts  distance <= measured + 1  (the sample is finite: one ulp
# covers arguments it does not hold).  numpy's own distance is printed next to it, never asserted.
MEASURED_ULPS = {
    ('exp', 'f8'): 1, ('exp', 'f4'): 1,
    ('exp2', 'f8'): 1, ('exp2', 'f4'): 1,
    ('expm1', 'f8'): 2, ('expm1', 'f4'): 1,
    ('log', 'f8'): 1, ('log', 'f4'): 2,
    ('log2', 'f8'): 1, ('log2', 'f4'): 1,
    ('log10', 'f8'): 1, ('log10', 'f4'): 2,
    ('log1p', 'f8'): 1, ('log1p', 'f4'): 1,
    ('sin', 'f8'): 1, ('sin', 'f4'): 1,
    ('cos', 'f8'): 1, ('cos', 'f4'): 1,
    ('tan', 'f8'): 1, ('tan', 'f4'): 1,
    ('asin', 'f8'): 1, ('asin', 'f4'): 2,
    ('acos', 'f8'): 1, ('acos', 'f4'): 1,
    ('atan', 'f8'): 1, ('atan', 'f4'): 2,
    ('sinh', 'f8'): 1, ('sinh', 'f4'): 1,
    ('cosh', 'f8'): 1, ('cosh', 'f4'): 1,
    ('tanh', 'f8'): 1, ('tanh', 'f4'): 1,
    ('cbrt', 'f8'): 0, ('cbrt', 'f4'): 1,
    ('pow', 'f8'): 1, ('pow', 'f4'): 1,
    ('float_power', 'f8'): 1,
    ('pow 3', 'f8'): 1, ('pow 3', 'f4'): 1,
    ('rpow', 'f8'): 1, ('rpow', 'f4'): 1,
    ('np.power 0.5', 'f8'): 1, ('np.power 0.5', 'f4'): 1,
    ('pow 2 of a state', 'f8'): 0, ('pow 2 of a state', 'f4'): 0,
    ('atan2', 'f8'): 1, ('atan2', 'f4'): 2,
    ('hypot', 'f8'): 1, ('hypot', 'f4'): 1,
}
# numpy 2.2.6 (x86-64) on the same operands, for comparison only
NUMPY_ULPS = {
    ('exp', 'f8'): 1, ('exp', 'f4'): 2,
    ('exp2', 'f8'): 1, ('exp2', 'f4'): 1,
    ('expm1', 'f8'): 0, ('expm1', 'f4'): 2,
    ('log', 'f8'): 0, ('log', 'f4'): 2,
    ('log2', 'f8'): 0, ('log2', 'f4'): 1,
    ('log10', 'f8'): 1, ('log10', 'f4'): 2,
    ('log1p', 'f8'): 0, ('log1p', 'f4'): 2,
    ('sin', 'f8'): 1, ('sin', 'f4'): 1,
    ('cos', 'f8'): 1, ('cos', 'f4'): 1,
    ('tan', 'f8'): 1, ('tan', 'f4'): 2,
    ('asin', 'f8'): 1, ('asin', 'f4'): 2,
    ('acos', 'f8'): 1, ('acos', 'f4'): 1,
    ('atan', 'f8'): 0, ('atan', 'f4'): 1,
    ('sinh', 'f8'): 1, ('sinh', 'f4'): 1,
    ('cosh', 'f8'): 1, ('cosh', 'f4'): 2,
    ('tanh', 'f8'): 1, ('tanh', 'f4'): 1,
    ('cbrt', 'f8'): 1, ('cbrt', 'f4'): 2,
    ('pow', 'f8'): 1, ('pow', 'f4'): 1,
    ('float_power', 'f8'): 1,
    ('pow 3', 'f8'): 1, ('pow 3', 'f4'): 1,
    ('rpow', 'f8'): 1, ('rpow', 'f4'): 1,
    ('np.power 0.5', 'f8'): 1, ('np.power 0.5', 'f4'): 1,
    ('pow 2 of a state', 'f8'): 0, ('pow 2 of a state', 'f4'): 0,
    ('atan2', 'f8'): 1, ('atan2', 'f4'): 2,
    ('hypot', 'f8'): 1, ('hypot', 'f4'): 0,
}


def ulp_bound(row_name, dt):
    return MEASURED_ULPS[(row_name, dt)] + 1


# tuples of operands that leave the bit comparison of an exact row because numpy on the host disagrees with itself on
# them (scalar against arrays of several lengths and strides): {(row name, dtype key): [(a, b), ..]}.  Expected: none.
LEFT_OUT = {}


# -------------------------------------------------------------------------------------------------------------- operands
def specials(dt):
    dt = np.dtype(dt)
    fi = np.finfo(dt)
    big = 2.0 ** (fi.nmant)
    one = dt.type(1)
    below, above = float(np.nextafter(one, dt.type(0))), float(np.nextafter(one, dt.type(2)))
    vals = [0.0, -0.0, 1.0, -1.0, 0.5, -0.5, 1.5, -1.5, 2.5, -2.5, np.inf, -np.inf, np.nan,
            float(fi.tiny), float(fi.max), float(fi.smallest_subnormal), float(fi.smallest_subnormal) * 2.0 ** (fi.nmant // 2) * 1.25,
            big - 1.0, big + 1.0, below, -below, above, -above, 3.0, -3.0, 5.0, -5.0]
    out = np.array(vals, dtype=np.float64)
    assert np.array_equal(out.astype(dt).astype(np.float64), out, equal_nan=True)
    return out


N_RANDOM = 2048


def operands(dt):
    """(a, b, c) as float64 arrays of values that the real type `dt` holds exactly: the full cross product of the
    specials, then N_RANDOM seeded triples -- half ordinary, in [-4, 4], half spread over the exponent range"""
    sp = specials(dt)
    a, b, c = (g.reshape(-1) for g in np.meshgrid(sp, sp, sp, indexing='ij'))
    rng = np.random.default_rng(20261017)
    fi = np.finfo(dt)
    half = N_RANDOM // 2
    ordinary = rng.uniform(-4.0, 4.0, (3, half))
    spread = rng.choice([-1.0, 1.0], (3, half)) * rng.uniform(1.0, 2.0, (3, half)) \
        * 2.0 ** rng.integers(fi.minexp - fi.nmant + 1, fi.maxexp - 1, (3, half)).astype(np.float64)
    rnd = np.concatenate([ordinary, spread], axis=1).astype(dt).astype(np.float64)
    return tuple(np.concatenate([v, r]) for v, r in zip((a, b, c), rnd))


# ------------------------------------------------------------------------------------------------------------ the units
def rows_for(dtkey):
    return [r for r in ROWS if dtkey in r.dtypes]


def units(dtkey):
    rows = rows_for(dtkey)
    return [rows[i:i + ROWS_PER_UNIT] for i in range(0, len(rows), ROWS_PER_UNIT)]


def unit_cost(rows):
    fns = [r.spellings[0] for r in rows]

    def cost(k, a, b, u, c):
        out = fns[-1](a, b, c)
        for j in range(len(fns) - 2, -1, -1):
            out = np.where(k == j, fns[j](a, b, c), out)
        return out
    return cost


def unit_solver(rows, dtkey):
    s = SysDescription((2, 1, 1), stationnary=False, name='device ops')
    s.dyn = lambda k, a, b, u, c: (a, b)
    s.cost = unit_cost(rows)
    s.control_box = lambda k, a, b: ((0., 0.),)
    s.perturb_laws = [models.NormalLaw(0, 1.0)]
    solver = DPSolver(s, dtype=DTYPES[dtkey])
    solver.discretize_state(-1, 1, 3, -1, 1, 3)
    solver.discretize_perturb(-1, 1, 3)
    solver.control_steps = (1.0,)
    solver.kernel = 'generic'
    return solver


def unit_source(solver):
    return solver._kernel_plan(0, solver._trace_now(0))['source']


def reference(rows, dtkey, ops):
    """the rows' callables on numpy arrays of the problem's type: (len(rows), B)"""
    dt = DTYPES[dtkey]
    a, b, c = (v.astype(dt) for v in ops)
    cost = unit_cost(rows)
    out = []
    with np.errstate(all='ignore'):
        for k in range(len(rows)):
            g = cost(k, a, b, np.zeros_like(a), c)
            assert isinstance(g, np.ndarray) and g.dtype == dt, \
                'row {!r} returns {} from {} arguments'.format(rows[k].name, getattr(g, 'dtype', type(g)), np.dtype(dt))
            out.append(g)
    return np.stack(out)


def same_bits(x, y, dtkey):
    """elementwise: equal bit patterns, all NaNs counting as equal to each other"""
    u = UINT[dtkey]
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return (x.view(u) == y.view(u)) | (np.isnan(x) & np.isnan(y))


def ordinal(x, dtkey):
    """position of each finite value among the representable numbers of its type (both zeros at 0), as int64"""
    i = np.ascontiguousarray(x).view(np.int64 if dtkey == 'f8' else np.int32).astype(np.int64)
    return np.where(i < 0, np.int64(-2 ** 63 if dtkey == 'f8' else -2 ** 31) - i, i)


def distance(x, y, dtkey):
    """how many representable numbers lie between x and y (finite, same type); values of opposite sign: 2^62"""
    ox, oy = ordinal(x, dtkey), ordinal(y, dtkey)
    with np.errstate(over='ignore'):
        d = np.abs(ox - oy)
    return np.where((ox < 0) != (oy < 0), np.int64(2 ** 62), d)


def round_to(v, dtkey):
    """the mpmath real `v`, rounded ONCE (to nearest, ties to even) to the real type: a Python float that the type
    holds exactly, or +-inf"""
    import mpmath
    sign, man, exp, _ = mpmath.mpf(v)._mpf_
    if man == 0:
        return 0.0
    nmant, emin, emax = (52, -1022, 1023) if dtkey == 'f8' else (23, -126, 127)
    e = man.bit_length() + exp - 1                       # 2^e <= |v| < 2^(e + 1)
    q = max(e, emin) - nmant                             # exponent of the spacing there
    shift = exp - q
    if shift >= 0:
        n = man << shift
    else:
        n, rem = divmod(man, 1 << -shift)
        half = 1 << (-shift - 1)
        if rem > half or (rem == half and n & 1):
            n += 1
    if n.bit_length() + q - 1 > emax:
        out = float('inf')
    else:
        out = math.ldexp(float(n), q)
    return -out if sign else out


# ------------------------------------------------------------------------------- the sweep fuzz with the wider pool of forms
def wide_expr(rng, leaves, depth):
    """random numpy expression over the leaf names: the nine forms of test_gpu_sweep._random_expr and the other exact
    operators (rounding, sign, fmin / fmax, clip, heaviside, a comparison as a number, logic under a where)"""
    if depth == 0 or rng.random() < 0.2:
        if rng.random() < 0.3:
            return repr(float(np.round(rng.uniform(-2, 2), 3)))
        return leaves[rng.integers(len(leaves))]
    a = wide_expr(rng, leaves, depth - 1)
    b = wide_expr(rng, leaves, depth - 1)
    kind = rng.integers(24)
    if kind == 0:
        return '({} + {})'.format(a, b)
    if kind == 1:
        return '({} - {})'.format(a, b)
    if kind == 2:
        return '({} * {})'.format(a, b)
    if kind == 3:
        return '({} / (1.5 + np.abs({})))'.format(a, b)
    if kind == 4:
        return 'np.where({} > {}, {}, {})'.format(a, b, a, wide_expr(rng, leaves, depth - 1))
    if kind == 5:
        return 'np.minimum({}, {})'.format(a, b)
    if kind == 6:
        return 'np.maximum({}, {})'.format(a, b)
    if kind == 7:
        return 'np.sqrt(np.abs({}))'.format(a)
    if kind == 8:
        # (a power of an expression without control and perturbation is flagged scalar_pow, see trace._power: the
        # product is the same operation without the flag)
        if 'u' in a or 'w' in a:
            return '(-{}) ** 2'.format(a)
        return '((-{0}) * (-{0}))'.format(a)
    if kind in (9, 10, 11, 12):
        return 'np.{}(3.0 * {})'.format(('floor', 'ceil', 'rint', 'trunc')[kind - 9], a)
    if kind == 13:
        return '(np.sign({}) * {})'.format(a, b)
    if kind == 14:
        return 'np.fmin({}, {})'.format(a, b)
    if kind == 15:
        return 'np.fmax({}, {})'.format(a, b)
    if kind == 16:
        return 'np.clip({}, -0.5, {})'.format(a, b)
    if kind == 17:
        return 'np.clip({}, {}, 0.75)'.format(a, b)
    if kind == 18:
        return 'np.heaviside({}, {})'.format(a, b)
    if kind == 19:
        return '(({} > {}) + {})'.format(a, b, a)
    if kind == 20:
        return '(({} <= {}) * {})'.format(a, b, b)
    c = wide_expr(rng, leaves, depth - 1)
    if kind == 21:
        return 'np.where(np.logical_and({0} > {1}, {1} > {2}), {0}, {2})'.format(a, b, c)
    if kind == 22:
        return 'np.where(np.logical_or({0} > {1}, {1} > {2}), {0}, {2})'.format(a, b, c)
    return 'np.where(np.logical_not({0} > {1}), {0}, {2})'.format(a, b, c)


WIDE_SEEDS = tuple(range(8))
WIDE_BASE = 7016


def wide_model(seed):
    """(solver, the three expressions): 2 states, 1 control, 1 perturbation on a 13 x 11 grid, 5 perturbation points,
    9 controls, as test_gpu_sweep.test_random_models_match_numpy_bit_for_bit"""
    rng = np.random.default_rng(WIDE_BASE + seed)
    separable = seed % 2 == 0                  # exercise both kernel families
    lead = wide_expr(rng, ['x', 'y', 'u'] if separable else ['x', 'y', 'u', 'w'], 3)
    trail = wide_expr(rng, ['y', 'w'] if separable else ['x', 'y', 'u', 'w'], 3)
    cst = wide_expr(rng, ['x', 'y', 'u', 'w'], 4)
    ns = {'np': np}
    exec('def dyn(x, y, u, w):\n    return (0.5 * x + 0.2 * ({}), 0.5 * y + 0.2 * ({}))\n'
         'def cost(x, y, u, w):\n    return {} + 0.0 * u\n'.format(lead, trail, cst), ns)
    s = SysDescription((2, 1, 1), name='wide fuzz %d' % seed)
    s.dyn, s.cost = ns['dyn'], ns['cost']
    s.control_box = lambda x, y: ((-1., 1.),)
    s.perturb_laws = [models.NormalLaw(0, 0.3)]
    solver = DPSolver(s)
    solver.discretize_state(-1, 1, 13, -1, 1, 11)
    solver.discretize_perturb(-0.6, 0.6, 5)
    solver.control_steps = (0.25,)
    return solver, (lead, trail, cst)
