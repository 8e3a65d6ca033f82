// sdp_family_policy_kernel.h -- fixed-policy backups of a FAMILY of same-shaped problems: kernels
// `sdp_family_evalpol` (one step of every listed member, any grid size) and `sdp_family_evalpol_resident` (all
// steps of a member in one workgroup, its values in LDS).
//
// Included LAST by a generated evaluation unit (codegen.family_policy_unit), after the direct prologue with
//   SDP_FAMILY 1, SDP_FAMILY_POLICY 1, SDP_REAL, SDP_D, SDP_NU, SDP_HAS_W, SDP_NPARAMS
//   sdp_model_cell_at(x, u, w, t, prm, xn, g)   the traced dyn/cost with its constants read from a row `prm`
// (SDP_LANES is printed by the prologue and not read here: one unit per model structure and real type.)
//
// Both kernels are `sdp_evalpol` (sdp_sweep_kernel.h) restated with a member index, as `sdp_family_sweep` restates
// `sdp_sweep`: one lane per node, the control read from the member's policy row, the perturbation loop in w order
// with the same sequential `acc = acc + jc * proba[wi]`, every vertex read as V - shift (SdpLerp<.., SHIFT>: the
// relative shift of the previous step, one rounding, as the reference's in-place `J_pol -= J_ref[k]`).  Member p of
// the result has the bits of `sdp_evalpol` on problem p alone.
//
// sdp_family_evalpol.  The unit of work is a tile of 256 consecutive nodes of ONE member -- a workgroup -- so a
// wavefront never spans two members and the member's constants, grid ends and law are wave-uniform and read through
// the constant address space.  Members map to XCDs as in sdp_family_sweep (the head of sdp_family_kernel.h), with
// that tile: a member's value array stays in one XCD's L2.  Bounded grid, the workgroups stride over the tiles.
//
// sdp_family_evalpol_resident.  One workgroup per listed member (bounded grid, striding over the list).  The
// member's two value buffers [S] live in LDS: per step every thread evaluates its strided share of the nodes --
// policy row and node coordinates from global memory (step-invariant, L2-resident after the first step), vertices
// out of the LDS buffer -- then a workgroup barrier and a swap.  The relative shift (V[ref] read from LDS after the
// barrier), the reference cost of every step, the final explicit shift and, with a check, the statistics and the
// decision run inside the kernel: a step costs a barrier, not a launch.  The decision is taken by thread 0 and
// broadcast through LDS, so it is workgroup-uniform and every barrier is reached by every thread.  No grid-wide
// barrier, nothing read from another workgroup.
#pragma once
#include "sdp_family_kernel.h"     // (SDP_FAMILY_POLICY: SdpMember and the member helpers only)

#ifndef SDP_FPOL_THREADS
#define SDP_FPOL_THREADS 1024                  // workgroup of the resident kernel
#endif
#define SDP_FPOL_LDS_BYTES (160 * 1024)        // the LDS of one CU: the resident kernel's budget
#define SDP_FPOL_RED_BYTES 512                 // .. of which the reduction and the broadcast take this much
// nodes of a member whose two buffers fit
#define SDP_FPOL_NODES ((SDP_FPOL_LDS_BYTES - SDP_FPOL_RED_BYTES) / (2 * (int)sizeof(sdp_real)))
#define SDP_FPOL_TILE 256                      // nodes per workgroup step of sdp_family_evalpol
#ifndef SDP_FPOL_HOIST
// nodes of a thread whose coordinates and controls the resident kernel keeps in registers across the steps: what 16
// registers hold, three at most (at 1024 threads a lane has 128 registers; with more the 3-D unit of the tests spills)
#define SDP_FPOL_HOIST_WORDS ((SDP_D + SDP_NU) * (int)(sizeof(SDP_REAL) / 4))
#define SDP_FPOL_HOIST (16 / SDP_FPOL_HOIST_WORDS > 3 ? 3 : 16 / SDP_FPOL_HOIST_WORDS)
#endif

// sdp_expected_cost<true> of sdp_evalpol with the member's constants and law, V in any address space
SDP_DEV sdp_real sdp_family_policy_cost(const SdpFamilyArgs &a, const SdpMember &m, const SdpGrid<sdp_real, SDP_D> &grid,
                                        const sdp_real *__restrict__ V, const sdp_real *x, const sdp_real *u, sdp_real t)
{
    sdp_real xn[SDP_D], g;
#if SDP_HAS_W
    sdp_real acc = (sdp_real)0;
    for (int wi = 0; wi < a.W; ++wi) {
        sdp_model_cell_at(x, u, m.wgrid[wi], t, m.prm, xn, g);
        const sdp_real jc = g + sdp_interp_point<sdp_real, SDP_D, sdp_real, true>(V, grid, xn);
        acc = acc + jc * m.proba[wi];
    }
    return acc;
#else
    sdp_model_cell_at(x, u, (sdp_real)0, t, m.prm, xn, g);
    return g + sdp_interp_point<sdp_real, SDP_D, sdp_real, true>(V, grid, xn);
#endif
}

extern "C" __global__ void __launch_bounds__(SDP_FPOL_TILE) sdp_family_evalpol(SdpFamilyEvalArgs e)
{
    const SdpFamilyArgs &a = e.f;
    constexpr int64_t tile_nodes = SDP_FPOL_TILE;
    const sdp_real t = (sdp_real)a.t_k;
    sdp_cst_i32 *members = (sdp_cst_i32 *)a.members;

    // members -> XCDs as in sdp_family_sweep; everything here is the same in every lane of the workgroup
    const int64_t tiles = (a.S + tile_nodes - 1) / tile_nodes;        // per member
    const int xcd = blockIdx.x & 7;
    const int parts = a.n_active >= 8 ? 1 : 8 / max(a.n_active, 1);   // XCDs per member
    const int first = xcd / parts;
    const int part = xcd % parts;
    const int mine = first < a.n_active ? (a.n_active - first + 7) / 8 : 0;
    const int64_t per_part = (tiles + parts - 1) / parts;
    const int64_t units = (int64_t)mine * per_part;
    const int64_t stride = gridDim.x >> 3;

    for (int64_t unit = blockIdx.x >> 3; unit < units; unit += stride) {
        const int64_t tile = (int64_t)part * per_part + unit % per_part;
        if (tile >= tiles) continue;
        const int64_t p = members[first + 8 * (int)(unit / per_part)];
        SdpMember m;
        SdpGrid<sdp_real, SDP_D> grid;
        sdp_family_member(a, p, m, grid);
        // fused relative shift of the previous step; its value is J_ref of that step: one lane per member stores it
        grid.shift = e.shift ? m.V[e.ref_index] : (sdp_real)0;
        if (e.shift && tile == 0 && threadIdx.x == 0) e.refs[(int64_t)e.slot * e.P + p] = (double)grid.shift;
        const int64_t node = tile * tile_nodes + threadIdx.x;
        if (node < a.S) {
            sdp_real x[SDP_D], u[SDP_NU];
            sdp_family_node_coords(a, m, node, x);
            const sdp_real *__restrict__ row = (const sdp_real *)a.pol + (p * a.S + node) * SDP_NU;
#pragma unroll
            for (int c = 0; c < SDP_NU; ++c) u[c] = row[c];
            ((sdp_real *)a.J)[p * a.S + node] = sdp_family_policy_cost(a, m, grid, m.V, x, u, t);
        }
    }
}

// min / max / NaN flag of a workgroup: the wavefront by shuffles, the wavefronts through `red`; thread 0 holds the result
SDP_DEV void sdp_fpol_reduce(sdp_real &mn, sdp_real &mx, int &nan, sdp_real *red_mn, sdp_real *red_mx, int *red_nan)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const sdp_real omn = sdp_shfl_xor(mn, off), omx = sdp_shfl_xor(mx, off);
        mn = omn < mn ? omn : mn;
        mx = omx > mx ? omx : mx;
        nan |= __shfl_xor(nan, off, 64);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red_mn[wave] = mn; red_mx[wave] = mx; red_nan[wave] = nan; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < SDP_FPOL_THREADS / 64; ++w) {
            mn = red_mn[w] < mn ? red_mn[w] : mn;
            mx = red_mx[w] > mx ? red_mx[w] : mx;
            nan |= red_nan[w];
        }
    }
}

extern "C" __global__ void __launch_bounds__(SDP_FPOL_THREADS) sdp_family_evalpol_resident(SdpFamilyEvalArgs e)
{
    const SdpFamilyArgs &a = e.f;
    __shared__ sdp_real s_val[2][SDP_FPOL_NODES];
    __shared__ sdp_real s_mn[SDP_FPOL_THREADS / 64], s_mx[SDP_FPOL_THREADS / 64];
    __shared__ int s_nan[SDP_FPOL_THREADS / 64];
    __shared__ int s_stop;
    static_assert(sizeof(sdp_real) * 2 * (SDP_FPOL_THREADS / 64) + 4 * (SDP_FPOL_THREADS / 64) + 4 <= SDP_FPOL_RED_BYTES,
                  "the reduction's share of the LDS");
    sdp_trap_unless(a.S <= SDP_FPOL_NODES && blockDim.x == SDP_FPOL_THREADS);
    const sdp_real t = (sdp_real)a.t_k;
    sdp_cst_i32 *members = (sdp_cst_i32 *)a.members;
    const int S = (int)a.S;
    const int ref = (int)e.ref_index;

    for (int at = blockIdx.x; at < a.n_active; at += gridDim.x) {
        const int64_t p = members[at];
        SdpMember m;
        SdpGrid<sdp_real, SDP_D> grid;
        sdp_family_member(a, p, m, grid);
        const sdp_real *__restrict__ pol = (const sdp_real *)a.pol + p * a.S * SDP_NU;
        for (int i = threadIdx.x; i < S; i += SDP_FPOL_THREADS) s_val[0][i] = m.V[i];
        // step-invariant: the coordinates and the controls of a thread's first SDP_FPOL_HOIST nodes stay in registers
        sdp_real hx[SDP_FPOL_HOIST][SDP_D], hu[SDP_FPOL_HOIST][SDP_NU];
#pragma unroll
        for (int j = 0; j < SDP_FPOL_HOIST; ++j) {
            const int node = threadIdx.x + j * SDP_FPOL_THREADS;
            if (node < S) {
                sdp_family_node_coords(a, m, node, hx[j]);
#pragma unroll
                for (int c = 0; c < SDP_NU; ++c) hu[j][c] = pol[(int64_t)node * SDP_NU + c];
            }
        }
        __syncthreads();
        int cur = 0, done = 0, check = 0;
        for (int k = 0; k < e.n_iter; ++k) {
            const sdp_real *Vs = s_val[cur];
            sdp_real *Js = s_val[cur ^ 1];
            // step k > 0 of the relative algorithm reads V - V[ref]; that value is the reference cost of step k - 1
            const bool shifted = e.rel_dp && k > 0;
            grid.shift = shifted ? Vs[ref] : (sdp_real)0;
            if (shifted && threadIdx.x == 0) e.refs[(int64_t)(k - 1) * e.P + p] = (double)grid.shift;
#pragma unroll
            for (int j = 0; j < SDP_FPOL_HOIST; ++j) {
                const int node = threadIdx.x + j * SDP_FPOL_THREADS;
                if (node < S) Js[node] = sdp_family_policy_cost(a, m, grid, Vs, hx[j], hu[j], t);
            }
            for (int node = threadIdx.x + SDP_FPOL_HOIST * SDP_FPOL_THREADS; node < S; node += SDP_FPOL_THREADS) {
                sdp_real x[SDP_D], u[SDP_NU];
                sdp_family_node_coords(a, m, node, x);
#pragma unroll
                for (int c = 0; c < SDP_NU; ++c) u[c] = pol[(int64_t)node * SDP_NU + c];
                Js[node] = sdp_family_policy_cost(a, m, grid, Vs, x, u, t);
            }
            __syncthreads();
            done = k + 1;
            bool stop = false;
            if (e.check_every > 0 && (done % e.check_every == 0 || done == e.n_iter)) {
                // the statistics of the SHIFTED sequence (k_diff_stats with ra / rb): both buffers hold raw values
                const sdp_real ja = e.rel_dp ? Js[ref] : (sdp_real)0, vb = shifted ? Vs[ref] : (sdp_real)0;
                sdp_real mn = (sdp_real)INFINITY, mx = (sdp_real)-INFINITY;
                int nan = 0;
                for (int i = threadIdx.x; i < S; i += SDP_FPOL_THREADS) {
                    const sdp_real av = e.rel_dp ? Js[i] - ja : Js[i], bv = shifted ? Vs[i] - vb : Vs[i];
                    const sdp_real d = av == bv ? (sdp_real)0 : av - bv;
                    nan |= d != d;
                    mn = d < mn ? d : mn;
                    mx = d > mx ? d : mx;
                }
                sdp_fpol_reduce(mn, mx, nan, s_mn, s_mx, s_nan);
                if (threadIdx.x == 0) {
                    const double dmin = nan ? (double)NAN : (double)mn, dmax = nan ? (double)NAN : (double)mx;
                    double *st = e.stats + ((int64_t)check * e.P + p) * 2;
                    st[0] = dmin;
                    st[1] = dmax;
                    s_stop = (dmax - dmin <= e.tol) ? 1 : 0;            // a NaN never converges
                }
                __syncthreads();
                stop = s_stop != 0;
                ++check;
                __syncthreads();                                         // (s_stop and the partial results are free again)
            }
            if (stop) break;
            if (k + 1 < e.n_iter) cur ^= 1;
        }
        // the result: the buffer of the last step, shifted once more with rel_dp (the explicit shift after the loop)
        if (done == 0) {
            for (int i = threadIdx.x; i < S; i += SDP_FPOL_THREADS) ((sdp_real *)a.J)[p * a.S + i] = s_val[0][i];
        } else {
            const sdp_real *Js = s_val[cur ^ 1];
            const sdp_real r = e.rel_dp ? Js[ref] : (sdp_real)0;
            if (e.rel_dp && threadIdx.x == 0) e.refs[(int64_t)(done - 1) * e.P + p] = (double)r;
            for (int i = threadIdx.x; i < S; i += SDP_FPOL_THREADS)
                ((sdp_real *)a.J)[p * a.S + i] = e.rel_dp ? Js[i] - r : Js[i];
        }
        if (threadIdx.x == 0) e.n_done[p] = done;
        __syncthreads();                                                 // the buffers are the next member's
    }
}

// what this code object was generated for (sdp_kernel_args.h, SDP_META_*)
extern "C" {
__constant__ int32_t sdp_meta[SDP_META_WORDS] = {
    SDP_META_MAGIC, (int32_t)sizeof(sdp_real), SDP_D, SDP_NU, SDP_HAS_W, 0, 0, 1,
    SDP_META_F_FAMILY | SDP_META_F_FAMILY_POLICY, 0, 0, SDP_FPOL_THREADS, SDP_FPOL_NODES, 0, 0, 0};
}
