"""Several perturbation variables, as a definition in numpy.

The reference accepts `SysDescription((n_state, n_perturb, n_control))` with `n_perturb >= 2`,
a list of laws and `discretize_perturb(lo1, hi1, n1, lo2, hi2, n2, ...)`, and stops at its sweep
(`# TODO : implement nD perturbation`, stodynprog.py:666, :679-683).  There is no reference result
to reproduce, so what the kernels of csrc/sdp_multiw_kernel.h compute is written down here first --
what `montecarlo.py` is to the draws and `convergence.py` to the stopping rule.

m = len(sys.perturb) INDEPENDENT variables, 2 <= m <= 4; variable i has a grid g_i of W_i points
and probabilities p_i, as `DPSolver.discretize_perturb` stores them (perturb_grid[i],
perturb_proba[i]).  They are flattened into ONE law of W = W_1 .. W_m points:

    j          = ravel_multi_index((j_1, .., j_m), (W_1, .., W_m))       C order, the LAST variable fastest
    wtab[i, j] = g_i[j_i]                                                shape (m, W)
    P[j]       = ((p_1[j_1] * p_2[j_2]) * p_3[j_3]) * ..                 float64, multiplied left to right

A problem of 4-byte reals rounds wtab and P ONCE to float32, like every other host table.  The
backup is then the sequential sum over a flat law that one variable has always had:

    cell_j = g(x, u, w_1, .., w_m) + J_next(f(x, u, w_1, .., w_m))       at w_i = wtab[i, j]
    acc    = acc + cell_j * P[j]                                         j ascending, one rounded multiply and
                                                                         one rounded add per point
    J(x)   = min_u acc,  first-occurrence argmin

m = 1 is this with wtab = grid[None, :] and P = proba: the definition every existing test pins.

Monte Carlo (`montecarlo.py`) still makes ONE Philox call and one uniform per (trajectory, step);
the index j it gives -- from the float64 running sum of P -- selects the column wtab[:, j].  A law
handed to `monte_carlo(law=...)` for m >= 2 is `(values of shape (m, n), proba of shape (n,))`: a
JOINT law, which need not be a product.
"""
import numpy as np

MAX_PERTURB = 4              # variables the model entry of a generated unit takes (SDP_NW of csrc/sdp_multiw_kernel.h)
MC_TABLE_BYTES = 65536       # dynamic LDS the Monte Carlo kernel may ask for: cum (8 (n - 1) bytes), then the values


def product_law(grids, probas, dtype=None):
    """(wtab, P) of independent variables with grids `grids` and probabilities `probas` (see the
    module's text).  float64, or rounded once to `dtype`."""
    if len(grids) != len(probas) or len(grids) < 1:
        raise ValueError('product_law needs one vector of probabilities per grid')
    grids = [np.array(g, dtype=np.float64).ravel() for g in grids]
    probas = [np.array(p, dtype=np.float64).ravel() for p in probas]
    for g, p in zip(grids, probas):
        if g.size < 1 or g.shape != p.shape:
            raise ValueError('a grid of shape {} with probabilities of shape {}'.format(g.shape, p.shape))
    dims = tuple(g.size for g in grids)
    W = int(np.prod(dims, dtype=np.int64))
    index = np.unravel_index(np.arange(W), dims)          # C order: the last variable fastest
    wtab = np.empty((len(grids), W))
    for i, g in enumerate(grids):
        wtab[i] = g[index[i]]
    P = probas[0][index[0]]
    for i in range(1, len(grids)):
        P = P * probas[i][index[i]]                       # left to right, one rounded multiply each
    if dtype is not None:
        wtab, P = wtab.astype(dtype), P.astype(dtype)
    return np.ascontiguousarray(wtab), np.ascontiguousarray(P)


def check_joint_law(values, proba, m):
    """a joint law of `m` variables for the draws: values (m, n) (a vector for m = 1), proba (n,)"""
    from . import montecarlo as mc
    p = mc.check_proba(proba)
    v = np.array(values, dtype=np.float64)
    if m == 1 and v.ndim == 1:
        v = v[None, :]
    if v.shape != (m, p.size):
        raise ValueError('law: values of shape {} but {} variable(s) and proba of shape {}'.format(v.shape, m, p.shape))
    return v, p


def mc_table_bytes(n_law, m, itemsize):
    """bytes of the draw table of `sdp_montecarlo` in LDS"""
    return (int(n_law) - 1) * 8 + int(m) * int(n_law) * int(itemsize)
