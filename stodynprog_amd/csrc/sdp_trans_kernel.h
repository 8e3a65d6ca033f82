// sdp_trans_kernel.h -- the entries of the policy's transition operator (kernel `sdp_transitions`).
//
// Included by sdp_sweep_kernel.h in every generated unit -- one perturbation variable, several, none,
// node-order, column, staged, line and lead units alike -- next to `sdp_simulate`.  The definition in
// numpy is stodynprog_amd/forward.py; this kernel gives its bits.
//
// Under a fixed policy the backup of sdp_evalpol is linear in the cost-to-go: (P J)(s) = sum_j P[j] *
// interp(J)(f(x_s, pol[s], w_j)).  Written out over the 2^d vertices of the interpolation cell, P is a
// sparse matrix with exactly W * 2^d entries per node s.  This kernel emits them -- the library sorts
// them by target into the CSR of the TRANSPOSE (sdp_hip.hip: sdp_transop), whose product moves a state
// distribution one step forward.  Per node s (flat id, the reference's C order, whatever layout the unit's
// sweep kernels store their per-node arrays in), point j of the flat law and vertex v in {0,1}^d (axis 0
// the most significant bit of v):
//
//     (x', g) = sdp_model_cell(x_s, pol[s], w_j, t_k)
//     cell q_k, lam_k, oml_k = (real)1 - lam_k             sdp_locate_axis<real, D, real>: the cast truncates,
//                                                          the index is clamped, lam is not (extrapolation)
//     tgt[e] = sum_k M_k (q_k + v_k)                       e = (s W + j) 2^d + v
//     val[e] = (((f_0 f_1) ..) f_{d-1}) P[j]               f_k = v_k ? lam_k : oml_k, one rounded multiply per product
//     gbar[s]: acc = 0; acc = acc + g_j P[j], j ascending  the sweep's own two roundings
//
// A deterministic system is W = 1 with P = [1] (the host passes that law; the model gets w = 0 as in
// sdp_evalpol).  Mapping: 2^d consecutive lanes per node, one per vertex, so the lanes of a wave store
// runs of 2^d consecutive entries (64 consecutive ones when W = 1); every lane of a node evaluates the model
// itself -- 2^d times the evaluations of sdp_evalpol, once per operator, with no LDS and no cross-lane
// traffic.  j is the same in every lane: the law is read through the constant address space (scalar loads).
// No launch bound beyond the workgroup size is asked of the register allocator (asking for
// eight waves made Searev's Monte Carlo kernel spill).
#pragma once

#define SDP_TRANS_THREADS 256
#define SDP_TRANS_V (1 << SDP_D)       // vertices of a cell

extern "C" __global__ void __launch_bounds__(SDP_TRANS_THREADS) sdp_transitions(SdpTransArgs a)
{
    SdpGrid<sdp_real, SDP_D> grid;
    const sdp_real *axes = (const sdp_real *)a.axes;
    {
        sdp_real smin[SDP_D], smax[SDP_D];
#pragma unroll
        for (int k = 0; k < SDP_D; ++k) {
            smin[k] = axes[a.axis_off[k]];
            smax[k] = axes[a.axis_off[k] + a.orders[k] - 1];
        }
        sdp_make_grid<sdp_real, SDP_D>(grid, a.orders, smin, smax);
    }
    const sdp_real *__restrict__ pol = (const sdp_real *)a.pol;
    const sdp_cst_real *wtab = (const sdp_cst_real *)a.wtab;
    const sdp_cst_real *proba = (const sdp_cst_real *)a.proba;
    int32_t *__restrict__ tgt = a.tgt;
    sdp_real *__restrict__ val = (sdp_real *)a.val;
    sdp_real *__restrict__ gbar = (sdp_real *)a.gbar;
    const int W = a.W;
    const sdp_real t = (sdp_real)a.t_k;
    const int64_t lanes = a.S * SDP_TRANS_V;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; id < lanes; id += stride) {
        const int64_t s = id / SDP_TRANS_V;
        const int v = (int)(id % SDP_TRANS_V);
        sdp_real x[SDP_D], u[SDP_NU];
        {
            int64_t r = s;
#pragma unroll
            for (int k = SDP_D - 1; k >= 0; --k) {
                const int i = (int)(r % a.orders[k]);
                r /= a.orders[k];
                x[k] = axes[a.axis_off[k] + i];
            }
        }
#pragma unroll
        for (int c = 0; c < SDP_NU; ++c) u[c] = pol[s * SDP_NU + c];
        sdp_real acc = (sdp_real)0;
        for (int j = 0; j < W; ++j) {
            sdp_real xn[SDP_D], g;
#if defined(SDP_NW) && SDP_NW >= 2
            sdp_real w[SDP_NW];
#pragma unroll
            for (int i = 0; i < SDP_NW; ++i) w[i] = wtab[i * W + j];
            sdp_model_cell(x, u, w, t, xn, g);
#elif SDP_HAS_W
            sdp_model_cell(x, u, wtab[j], t, xn, g);
#else
            sdp_model_cell(x, u, (sdp_real)0, t, xn, g);
#endif
            const sdp_real pj = proba[j];
            acc = acc + g * pj;
            SdpCell<sdp_real, SDP_D, sdp_real> cell;
            int node = 0;
            sdp_real f = (sdp_real)0;
#pragma unroll
            for (int k = 0; k < SDP_D; ++k) {
                sdp_locate_axis<sdp_real, SDP_D, sdp_real>(grid, k, xn[k], cell);
                const bool up = (v >> (SDP_D - 1 - k)) & 1;
                node += cell.off[k] + (up ? grid.M[k] : 0);
                const sdp_real fk = up ? cell.lam[k] : cell.oml[k];
                f = k == 0 ? fk : f * fk;
            }
            const int64_t e = (s * W + j) * SDP_TRANS_V + v;
            tgt[e] = node;
            val[e] = f * pj;
        }
        if (v == 0) gbar[s] = acc;
    }
}
