// sdp_family_mc_kernel.h -- Monte Carlo policy evaluation of a FAMILY of same-shaped problems (kernel
// `sdp_family_montecarlo`).
//
// Included LAST by a generated Monte Carlo unit (codegen.family_mc_unit), after the direct prologue with
//   SDP_FAMILY 1, SDP_FAMILY_MC 1, SDP_REAL, SDP_D, SDP_NU, SDP_HAS_W 1, SDP_NPARAMS
//   sdp_model_cell_at(x, u, w, t, prm, xn, g)   the traced dyn/cost with its constants read from a row `prm`
// (SDP_LANES is printed by the prologue and not read here: one unit per model structure and real type.)
//
// The kernel is the per-trajectory loop of `sdp_montecarlo_loop<false>` (sdp_horizon_kernel.h) restated with a member
// index, statement for statement: every axis located once, the outside test against the member's own grid ends, the
// occupancy node from that cell, the policy looked up by SdpLerp<.., double, 0, false> on the member's [nu][S] slice,
// the Philox4x32-10 draw of sdp_mc_kernel.h (its helpers, not a copy) on the member's seed, cumulative sums and
// values, the traced model with the member's row of constants, `acc = acc + g` for the counted steps.  Member p of
// every array has the bits of `sdp_montecarlo` on problem p alone: a draw is a function of (seed, id, step), so
// members that share a seed see the same uniforms (common random numbers).
//
// Work decomposition.  The unit of work is a tile of 256 trajectories of ONE member -- a workgroup -- so the member
// index is workgroup-uniform, and with it the row of constants, the grid ends, the seed and the bases of the policy
// and of the occupancy: read through the constant address space.  The member's draw table (cum[n_law - 1] doubles,
// then values[n_law] reals) lives in dynamic LDS: loaded at a workgroup's first tile, and again -- between two
// barriers -- only where its next tile is another member's.  Every loop bound around a barrier, a ballot or a shuffle
// is workgroup-uniform.  Dead lanes of a member's last tile run along on a copy of that member's last row and store
// nothing (the ballots and shuffles of the occupancy need every lane of a wave), as in the solo loop; a wavefront
// without a live lane skips the steps.  Members map to XCDs as in sdp_family_sweep (the head of sdp_family_kernel.h)
// with that tile: with 8 members or more XCD x takes members x, x + 8, ..; with fewer every member is given 8 / P
// XCDs, each a contiguous part of its tiles.  Bounded grid (a multiple of 8), the workgroups stride over the tiles.
#pragma once
#define SDP_MC_HELPERS_ONLY 1          // sdp_mc_kernel.h without the solo entry point
#include "sdp_family_kernel.h"         // (SDP_FAMILY_MC: the typedefs and sdp_model_cell_at's fallback only)
#include "sdp_mc_kernel.h"             // sdp_philox4x32_10, sdp_mc_uniform, sdp_mc_index, sdp_mc_visit

#define SDP_FMC_TILE SDP_MC_THREADS    // trajectories per tile: a workgroup

typedef const __attribute__((address_space(4))) uint64_t sdp_cst_u64;

extern "C" __global__ void __launch_bounds__(SDP_FMC_TILE) sdp_family_montecarlo(SdpFamilyMcArgs a)
{
    extern __shared__ double sdp_fmc_lds[];                // cum[W-1] (doubles), then law_grid[W] (reals)
    const int W = a.n_law;
    double *cum = sdp_fmc_lds;
    sdp_real *wtab = (sdp_real *)(sdp_fmc_lds + (W - 1));
    constexpr int64_t tile_rows = SDP_FMC_TILE;

    // members -> XCDs as in sdp_family_sweep; everything here is the same in every lane of the workgroup
    const int64_t tiles = (a.B + tile_rows - 1) / tile_rows;          // per member
    const int xcd = blockIdx.x & 7;
    const int parts = a.P >= 8 ? 1 : 8 / max(a.P, 1);                 // XCDs per member
    const int first = xcd / parts;                                    // first member of this XCD ..
    const int part = xcd % parts;                                     // .. and which part of its tiles
    const int mine = first < a.P ? (a.P - first + 7) / 8 : 0;
    const int64_t per_part = (tiles + parts - 1) / parts;
    const int64_t units = (int64_t)mine * per_part;
    const int64_t stride = gridDim.x >> 3;

    int64_t loaded = -1;                                              // the member whose draw table is in LDS
    for (int64_t unit = blockIdx.x >> 3; unit < units; unit += stride) {
        const int64_t tile = (int64_t)part * per_part + unit % per_part;
        if (tile >= tiles) continue;
        const int64_t p = first + 8 * (int)(unit / per_part);
        if (p != loaded) {                                            // (workgroup-uniform: every thread reaches both barriers)
            __syncthreads();                                          // the last tile's draws are done with the old table
            const double *pc = a.cum + p * W;
            const sdp_real *pw = (const sdp_real *)a.law_grid + p * W;
            for (int i = threadIdx.x; i < W - 1; i += SDP_FMC_TILE) cum[i] = pc[i];
            for (int i = threadIdx.x; i < W; i += SDP_FMC_TILE) wtab[i] = pw[i];
            __syncthreads();
            loaded = p;
        }
        // a wavefront beyond the member's last row has nothing to do (wave-uniform; no barrier below this line)
        const int64_t base = tile * tile_rows + (threadIdx.x & ~63);
        if (base >= a.B) continue;

        SdpGrid<sdp_real, SDP_D> grid;
        sdp_real smin[SDP_D], smax[SDP_D];
        {
            sdp_cst_real *axes = (sdp_cst_real *)a.axes + p * a.n_axes;
#pragma unroll
            for (int k = 0; k < SDP_D; ++k) {
                smin[k] = axes[a.axis_off[k]];
                smax[k] = axes[a.axis_off[k] + a.orders[k] - 1];
            }
            sdp_make_grid<sdp_real, SDP_D>(grid, a.orders, smin, smax);
        }
        const sdp_real *prm = (const sdp_real *)((sdp_cst_real *)a.prm + p * SDP_NPARAMS);
        const sdp_real *__restrict__ pol = (const sdp_real *)a.pol + p * (int64_t)SDP_NU * a.S;
        unsigned long long *occ = a.occupancy ? a.occupancy + p * a.S : nullptr;
        sdp_real *xs = (sdp_real *)a.x + p * (int64_t)SDP_D * a.B;
        sdp_real *accs = (sdp_real *)a.acc + p * a.B;
        const uint64_t seed = ((sdp_cst_u64 *)a.seed)[p];
        const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);

        const int64_t b = base + (threadIdx.x & 63);
        const bool live = b < a.B;
        // an idle lane of the member's last wave runs along on a copy of its last row and stores nothing (see the solo loop)
        const int64_t row = live ? b : a.B - 1;
        const unsigned long long id = a.traj_offset + (unsigned long long)row;
        sdp_real x[SDP_D];
#pragma unroll
        for (int k = 0; k < SDP_D; ++k) x[k] = xs[k * a.B + row];
        sdp_real acc = accs[row];
        int n_out = 0;                                     // (of this launch: fewer than 2^31 steps)
        for (int64_t step = a.step_begin; step < a.step_end; ++step) {
            const bool counted = step >= a.n_burn;
            SdpCell<sdp_real, SDP_D, double> cell;
            bool outside = false;
#pragma unroll
            for (int k = 0; k < SDP_D; ++k) {
                sdp_locate_axis<sdp_real, SDP_D, double>(grid, k, x[k], cell);
                outside = outside || !(x[k] >= smin[k] && x[k] <= smax[k]);
            }
            n_out += (counted && outside) ? 1 : 0;
            if (occ) {
                int node = 0;
#pragma unroll
                for (int k = 0; k < SDP_D; ++k) {
                    const int q = cell.off[k] + ((cell.lam[k] >= (sdp_real)0.5) ? grid.M[k] : 0);     // M[k] * (cell + 1)
                    node += max(min(q, grid.M[k] * (a.orders[k] - 1)), 0);
                }
                sdp_mc_visit(occ, node, counted && live);
            }
            sdp_real u[SDP_NU], xn[SDP_D], g;
#pragma unroll
            for (int c = 0; c < SDP_NU; ++c)               // sdp_interp_point<sdp_real, SDP_D, double>, the cell located once
                u[c] = (sdp_real)SdpLerp<sdp_real, SDP_D, double, 0, false>::eval(pol + c * a.S, grid, cell, 0);
            const SdpPhilox r = sdp_philox4x32_10((unsigned)id, (unsigned)(id >> 32), (unsigned)step,
                                                  (unsigned)((unsigned long long)step >> 32), k0, k1);
            const int j = sdp_mc_index(cum, W - 1, sdp_mc_uniform(r));     // 0 <= j <= W - 1
            const sdp_real w = wtab[j];
            sdp_model_cell_at(x, u, w, (sdp_real)(a.t0 + (double)step), prm, xn, g);
            if (counted) acc = acc + g;
#pragma unroll
            for (int k = 0; k < SDP_D; ++k) x[k] = xn[k];
        }
        if (live) {
#pragma unroll
            for (int k = 0; k < SDP_D; ++k) xs[k * a.B + b] = x[k];
            accs[b] = acc;
            a.n_outside[p * a.B + b] += n_out;
        }
    }
}

// what this code object was generated for (sdp_kernel_args.h, SDP_META_*)
extern "C" {
__constant__ int32_t sdp_meta[SDP_META_WORDS] = {
    SDP_META_MAGIC, (int32_t)sizeof(sdp_real), SDP_D, SDP_NU, SDP_HAS_W, 0, 0, 1,
    SDP_META_F_FAMILY | SDP_META_F_FAMILY_MC, 0, 0, SDP_FMC_TILE, 0, 0, 0, 0};
}
