"""Digests of every generated source the planner produces, to compare two versions of the HOST side of the planner
without a GPU and without a compiler: the generated text is the whole contract of a code object (its cache key hashes
the text, the headers and the flags), so two checkouts whose tables are equal -- and whose csrc/ is -- run the same
kernels.  Section (a): every source `__graft_entry__._prebuild_models` would compile (`_native.compile_model` is
replaced by a collector for the duration of the call).  Section (b): the A/B switches that no table of (a) reaches, one
at a time on nine models.  One line per source: family and sha256 prefix; a plan that raises prints the exception's type.
usage: python tools/plan_digests.py [repository root, default: this one] > table.txt ; diff the two tables"""
import hashlib
import os
import re
import sys

SWITCHES = [
    'SDP_COL_FILTER=0', 'SDP_COL_SHIFT=0', 'SDP_COL_UTAB=0', 'SDP_COL_LEAN2=0', 'SDP_COL_BNB=0', 'SDP_BNB_UNIFORM=0',
    'SDP_BNB_UNIFORM_EVAL=0', 'SDP_COL_REDUCE_FUSED=0', 'SDP_COL_DMAX_HI=0',
    'SDP_COL_WRES=0', 'SDP_COL_WRES=24', 'SDP_COL_TAIL_HOLD=0',
    'SDP_COL_WPAIR=0', 'SDP_COL_WPAIR=1',
    'SDP_COL_THREADS=512', 'SDP_COL_THREADS=1024', 'SDP_COL_MIN_WAVES=2', 'SDP_COL_UNROLL_W=2',
    'SDP_COL_A_LW=16', 'SDP_COL_A_GROUP=2', 'SDP_COL_A_WIDE_LOADS=0', 'SDP_COL_A_WIDE_LOADS=1',
    'SDP_COL_FILTER_TOP2=0', 'SDP_BNB_CHUNK=2', 'SDP_COL_FILTER_SCALE=4',
    'SDP_COL_WCHUNK=4', 'SDP_COLU_WIDE_LOADS=0']

# (model, keywords, reals, DPSolver.kernel)
MODELS = [
    ('synthetic3d', dict(N=256), 'float64', 'auto'),
    ('synthetic3d', dict(N=256, stock_noise=0.07), 'float64', 'auto'),
    ('synthetic3d', dict(N=256, stock_noise=0.07, nested=True), 'float64', 'auto'),
    ('synthetic3d', dict(N=256), 'float32', 'auto'),
    ('synthetic3d', dict(N=512), 'float32', 'auto'),
    ('synthetic3d', dict(N=48), 'float64', 'auto'),
    ('synthetic3d_coupled', dict(N=24), 'float64', 'column'),
    ('storage_ar1', {}, 'float64', 'auto'),
    ('searev', {}, 'float64', 'auto')]


def digest(source):
    return hashlib.sha256(source.encode('utf-8')).hexdigest()[:16]


def family(source):
    for name, mark in (('family_policy', '#define SDP_FAMILY_POLICY 1'), ('family_lookahead', '#define SDP_FAMILY_LOOKAHEAD 1'),
                       ('family_horizon', '#define SDP_FAMILY_HORIZON 1'),
                       ('family_lookahead_horizon', '#define SDP_FAMILY_LOOKAHEAD_HORIZON 1'),
                       ('family', '#define SDP_FAMILY 1'), ('column', '#include "sdp_column_kernel.h"'), ('staged', '#include "sdp_staged_kernel.h"'),
                       ('line', '#define SDP_LINE 1'), ('lead', '#define SDP_LEAD_AXES '),
                       ('lookahead', '#define SDP_LOOKAHEAD 1')):
        if mark in source:
            return name
    return 'direct'


def macro(source, name):
    m = re.search(r'^#define {} (\S+)'.format(re.escape(name)), source, re.M)
    return m.group(1) if m else None


def forms(sources):
    """which of the forms backend_info tells apart the sources hold: the equalities of tests/test_column_unit_record.py
    are vacuous for a form that no source has"""
    out = set()
    for s in sources:
        if macro(s, 'SDP_COL_SHIFT') == '1':
            out.add('shifted lattice')
            if macro(s, 'SDP_COL_SHIFT_CHAIN') != '0':
                out.add('regrouped chain')
        if family(s) == 'line':
            out.add('line')
    return out


def prebuilt_sources(root):
    import __graft_entry__ as entry
    from stodynprog_amd import _native as nat
    got = []
    saved = nat.compile_model
    nat.compile_model = lambda source, verbose=False: got.append(source) or os.devnull
    try:
        entry._prebuild_models()
    finally:
        nat.compile_model = saved
    return sorted(set(got))


def switch_rows():
    import numpy as np
    from stodynprog_amd import models, DPSolver
    rows, sources = [], []
    for name, kw, reals, kernel in MODELS:
        sysd, ref = getattr(models, name)(**kw)
        for sw in [None] + SWITCHES:
            s = DPSolver(sysd, dtype=np.dtype(reals))
            s.state_grid, s.perturb_grid = ref.state_grid, ref.perturb_grid
            s.perturb_proba, s.control_steps = ref.perturb_proba, ref.control_steps
            s.kernel = kernel
            s.debug_defines = dict([sw.split('=')]) if sw else None
            try:
                src = s._kernel_plan()['source']
                sources.append(src)
                what = '{} {}'.format(family(src), digest(src))
            except Exception as e:
                what = 'raises {}'.format(type(e).__name__)
            rows.append('{}({}) {} {} {}: {}'.format(name, ', '.join('{}={}'.format(*kv) for kv in sorted(kw.items())),
                                                    reals, kernel, sw or '-', what))
    return rows, sources


def main():
    root = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(__file__), '..'))
    sys.path.insert(0, root)
    sys.dont_write_bytecode = True
    built = prebuilt_sources(root)
    print('# (a) the sources build() compiles')
    for row in sorted('{} {}'.format(family(s), digest(s)) for s in built):
        print(row)
    count = {}
    for s in built:
        count[family(s)] = count.get(family(s), 0) + 1
    print('# {} sources: {}; all of them {}'.format(
        len(built), ', '.join('{} {}'.format(k, v) for k, v in sorted(count.items(), key=lambda kv: -kv[1])),
        hashlib.sha256(''.join(built).encode('utf-8')).hexdigest()))
    rows, switched = switch_rows()
    print('# (b) one A/B switch at a time')
    for row in rows:
        print(row)
    print('# {} rows, {} distinct sources, {} raise'.format(len(rows), len(set(switched)), len(rows) - len(switched)))
    assert forms(built) == {'shifted lattice', 'regrouped chain', 'line'}, forms(built)
    assert forms(switched) >= {'shifted lattice', 'regrouped chain'}, forms(switched)


if __name__ == '__main__':
    main()
