// sdp_trans_horizon_kernel.h -- the entries of the transition operators of the steps of a HORIZON, each under its own
// slice of a time-indexed policy: kernel `sdp_transitions_h`, the forward pass of a finite-horizon problem without
// sampling noise.
//
// Included by sdp_sweep_kernel.h directly after sdp_horizon_kernel.h, so every generated unit carries it next to
// `sdp_transitions` and `sdp_simulate_h`; it uses `sdp_model_cell_at`, `sdp_h_prm_row` and `sdp_w_arg` of that header.
// The definition in numpy is stodynprog_amd/forward.py (`chain_entries`: `entries` at every step).
//
// The kernel is `sdp_transitions` (sdp_trans_kernel.h) restated with a step index, statement for statement, as
// `sdp_family_transitions` restates it with a member index.  Per step k of [step_begin, step_end), node s, point j of the
// flat law and vertex v in {0,1}^d (axis 0 the most significant bit of v), with kl = k - step_begin:
//
//     u        = pol[k - chunk_first][.][s]                  the policy slice of the step, control axis first
//     (x', g)  = sdp_model_cell_at(x_s, u, w_j, t0 + k, prm[k])   row k of the table of lifted constants
//     cell q_i, lam_i, oml_i = (real)1 - lam_i               sdp_locate_axis<real, D, real>
//     tgt[e] = kl S + sum_i M_i (q_i + v_i)                  e = ((kl S + s) W + j) 2^d + v
//     val[e] = (((f_0 f_1) ..) f_{d-1}) P[j]                 f_i = v_i ? lam_i : oml_i, one rounded multiply per product
//     gbar[kl S + s]: acc = 0; acc = acc + g_j P[j], j ascending, stored by the lane with v == 0
//
// -- the operations of sdp_trans_kernel.h in its order, so block kl of val and gbar has the bits of `sdp_transitions`
// under pol[k] at time index t0 + k, and its targets are the solo ones plus kl S: the steps' operators are ONE
// block-diagonal operator on (step_end - step_begin) S rows, which the library sorts in one pass (sdp_hip.hip:
// sdp_chainop).  The sort is stable and steps share no row, so each step's rows keep the solo entry order.
//
// Work decomposition (that of sdp_family_trans_kernel.h).  2^d consecutive lanes per node, one per vertex; a workgroup
// of 256 lanes holds a tile of 256 >> d consecutive nodes of ONE step, so the step index is workgroup-uniform: the row
// of constants and the base of the policy slice are a kernel-argument pointer plus a multiple of it, the table and the
// law read through the constant address space (scalar loads).  No LDS, no cross-lane traffic.  Lanes past a step's last
// node are dead: no load, no store.
//
// Grid.  Bounded; workgroup b takes the units b, b + gridDim.x, .. of the steps x tiles units, unit = kl tiles + tile.
// No launch bound beyond the workgroup size is asked of the register allocator.
#pragma once

#define SDP_TRANSH_THREADS 256
#define SDP_TRANSH_V (1 << SDP_D)                              // vertices of a cell
#define SDP_TRANSH_TILE (SDP_TRANSH_THREADS >> SDP_D)          // nodes of a workgroup's tile

extern "C" __global__ void __launch_bounds__(SDP_TRANSH_THREADS) sdp_transitions_h(SdpTransHArgs a)
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
    constexpr int64_t tile_nodes = SDP_TRANSH_TILE;
    const int v = threadIdx.x & (SDP_TRANSH_V - 1);
    const int64_t slot = threadIdx.x >> SDP_D;

    // everything here is the same in every lane of the workgroup
    const int64_t tiles = (a.S + tile_nodes - 1) / tile_nodes;        // per step
    const int64_t units = (a.step_end - a.step_begin) * tiles;
    for (int64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
        const int64_t kl = unit / tiles;
        const int64_t tile = unit % tiles;
        const int64_t step = a.step_begin + kl;
        const sdp_real *__restrict__ pk = pol + (step - a.chunk_first) * (int64_t)SDP_NU * a.S;
        const sdp_real *prm = sdp_h_prm_row(a.prm, step);
        const sdp_real t = (sdp_real)(a.t0 + (double)step);
        const int64_t s = tile * tile_nodes + slot;
        if (s >= a.S) continue;                        // lanes beyond the step's last node are dead
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
        for (int c = 0; c < SDP_NU; ++c) u[c] = pk[c * a.S + s];
        const int base = (int)(kl * a.S);              // (steps x S < 2^31: the library's rule)
        sdp_real acc = (sdp_real)0;
        for (int j = 0; j < W; ++j) {
            sdp_real xn[SDP_D], g;
#if defined(SDP_NW) && SDP_NW >= 2
            sdp_real w[SDP_NW];
#pragma unroll
            for (int i = 0; i < SDP_NW; ++i) w[i] = wtab[i * W + j];
            sdp_model_cell_at(x, u, w, t, prm, xn, g);
#elif SDP_HAS_W
            sdp_model_cell_at(x, u, wtab[j], t, prm, xn, g);
#else
            sdp_model_cell_at(x, u, (sdp_real)0, t, prm, xn, g);
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
            const int64_t e = ((kl * a.S + s) * W + j) * SDP_TRANSH_V + v;
            tgt[e] = base + node;
            val[e] = f * pj;
        }
        if (v == 0) gbar[kl * a.S + s] = acc;
    }
}
