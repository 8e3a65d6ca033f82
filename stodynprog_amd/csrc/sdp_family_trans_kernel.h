// sdp_family_trans_kernel.h -- the entries of the transition operators of a FAMILY of same-shaped problems, each under
// its own policy: kernel `sdp_family_transitions`.
//
// Included LAST by a generated transition unit (codegen.family_trans_unit), after the direct prologue with
//   SDP_FAMILY 1, SDP_FAMILY_TRANS 1, SDP_REAL, SDP_D, SDP_NU, SDP_HAS_W, SDP_NPARAMS
//   sdp_model_cell_at(x, u, w, t, prm, xn, g)   the traced dyn/cost with its constants read from a row `prm`
// (SDP_LANES is printed by the prologue and not read here: one unit per model structure and real type.)
//
// The kernel is `sdp_transitions` (sdp_trans_kernel.h) restated with a member index, as `sdp_family_evalpol` restates
// `sdp_evalpol`; the definition in numpy is stodynprog_amd/forward.py on every member.  Per member p, node s, point j of
// the member's flat law and vertex v in {0,1}^d (axis 0 the most significant bit of v):
//
//     (x', g) = sdp_model_cell_at(x_s, pol[p][s], w_j, t_k, prm[p])
//     cell q_k, lam_k, oml_k = (real)1 - lam_k             sdp_locate_axis on the member's grid ends
//     tgt[e] = p S + sum_k M_k (q_k + v_k)                 e = ((p S + s) W + j) 2^d + v
//     val[e] = (((f_0 f_1) ..) f_{d-1}) P[p][j]            f_k = v_k ? lam_k : oml_k, one rounded multiply per product
//     gbar[p][s]: acc = 0; acc = acc + g_j P[p][j], j ascending, stored by the lane with v == 0
//
// -- the operations of sdp_trans_kernel.h in its order, so member p of val and gbar has the bits of `sdp_transitions`
// on problem p alone, and member p's targets are the solo ones plus p S: the P operators are ONE block-diagonal operator
// on P S rows, whose CSR the library builds with the sort it builds a solo one with (sdp_hip.hip: sdp_transop).  The sort
// is stable and members share no row, so each member's rows keep the solo entry order.  A deterministic family is W = 1
// with the one weight 1 read from memory by every member (the host passes it; the model gets w = 0).
//
// Work decomposition.  2^d consecutive lanes per node, one per vertex; a workgroup of 256 lanes holds a tile of
// 256 >> d consecutive nodes of ONE member, so a wavefront never spans two members: the member's row of constants, its
// grid ends and its law are wave-uniform and read through the constant address space (sdp_family_member,
// sdp_model_cell_at), and j is the same in every lane.  No LDS, no cross-lane traffic.  The lanes of a wave store
// 64 / 2^d runs of 2^d consecutive entries per law point (64 consecutive entries when W = 1).
//
// Grid.  Bounded; workgroup b takes the units b, b + gridDim.x, .. of the P x tiles units, unit = p tiles + tile.
// Members are NOT mapped to XCDs as sdp_family_evalpol maps them.  That mapping keeps a member's value array, which
// every node of the member gathers from, in one XCD's L2.  This kernel gathers nothing: a tile reads its own policy
// rows once and writes its own entries once, and what the tiles of a member share -- the row of constants, the axes,
// the law: a few hundred bytes -- is read through the scalar cache whatever XCD the tile runs on.  The mapping would
// only leave XCDs idle where P is no multiple of 8 (8 / P XCDs a member below 8, up to 7 idle at P = 9) in a kernel
// that runs once per operator; the flat walk loads every XCD alike for every P.
#pragma once
#include "sdp_family_kernel.h"     // (SDP_FAMILY_TRANS: SdpMember and the member helpers only)

#define SDP_FTRANS_THREADS 256
#define SDP_FTRANS_V (1 << SDP_D)                              // vertices of a cell
#define SDP_FTRANS_TILE (SDP_FTRANS_THREADS >> SDP_D)          // nodes of a workgroup's tile

extern "C" __global__ void __launch_bounds__(SDP_FTRANS_THREADS) sdp_family_transitions(SdpFamilyTransArgs e)
{
    const SdpFamilyArgs &a = e.f;
    constexpr int64_t tile_nodes = SDP_FTRANS_TILE;
    const sdp_real t = (sdp_real)a.t_k;
    const int W = e.W;
    const int v = threadIdx.x & (SDP_FTRANS_V - 1);
    const int slot = threadIdx.x >> SDP_D;
    int32_t *__restrict__ tgt = e.tgt;
    sdp_real *__restrict__ val = (sdp_real *)e.val;
    sdp_real *__restrict__ gbar = (sdp_real *)e.gbar;

    // everything here is the same in every lane of the workgroup
    const int64_t tiles = (a.S + tile_nodes - 1) / tile_nodes;        // per member
    const int64_t units = (int64_t)a.n_active * tiles;
    for (int64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
        const int64_t p = unit / tiles;
        const int64_t tile = unit % tiles;
        SdpMember m;
        SdpGrid<sdp_real, SDP_D> grid;
        sdp_family_member(a, p, m, grid);
        const int64_t s = tile * tile_nodes + slot;
        if (s >= a.S) continue;                        // lanes beyond the member's last node are dead
        sdp_real x[SDP_D], u[SDP_NU];
        sdp_family_node_coords(a, m, s, x);
        const sdp_real *__restrict__ row = (const sdp_real *)a.pol + (p * a.S + s) * SDP_NU;
#pragma unroll
        for (int c = 0; c < SDP_NU; ++c) u[c] = row[c];
        const int base = (int)(p * a.S);               // (P S < 2^31: the host's chunk rule)
        sdp_real acc = (sdp_real)0;
        for (int j = 0; j < W; ++j) {
            sdp_real xn[SDP_D], g;
#if SDP_HAS_W
            sdp_model_cell_at(x, u, m.wgrid[j], t, m.prm, xn, g);
#else
            sdp_model_cell_at(x, u, (sdp_real)0, t, m.prm, xn, g);
#endif
            const sdp_real pj = m.proba[j];
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
            const int64_t at = ((p * a.S + s) * W + j) * SDP_FTRANS_V + v;
            tgt[at] = base + node;
            val[at] = f * pj;
        }
        if (v == 0) gbar[p * a.S + s] = acc;
    }
}

// what this code object was generated for (sdp_kernel_args.h, SDP_META_*)
extern "C" {
__constant__ int32_t sdp_meta[SDP_META_WORDS] = {
    SDP_META_MAGIC, (int32_t)sizeof(sdp_real), SDP_D, SDP_NU, SDP_HAS_W, 0, 0, 1,
    SDP_META_F_FAMILY | SDP_META_F_FAMILY_TRANS, 0, 0, SDP_FTRANS_THREADS, SDP_FTRANS_TILE, 0, 0, 0};
}
