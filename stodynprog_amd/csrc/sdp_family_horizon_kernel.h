// sdp_family_horizon_kernel.h -- closed loops of a FAMILY of same-shaped problems over a horizon (kernels
// `sdp_family_simulate` and `sdp_family_montecarlo_h`): the forward half of a finite-horizon study.
//
// Included LAST by a generated horizon unit (codegen.family_horizon_unit), after the direct prologue with
//   SDP_FAMILY 1, SDP_FAMILY_HORIZON 1, SDP_REAL, SDP_D, SDP_NU, SDP_HAS_W, SDP_NPARAMS
//   sdp_model_cell_at(x, u, w, t, prm, xn, g)   the traced dyn/cost with its constants read from a row `prm`
// (SDP_LANES is printed by the prologue and not read here: one unit per model structure and real type.)
//
// The kernels are the per-trajectory loops of `sdp_simulate_loop<true>` and `sdp_montecarlo_loop<true>`
// (sdp_horizon_kernel.h) restated with a member index, statement for statement, and with the two things that change from
// step to step addressed by strides (SdpFamilySimHArgs): member p at step k of the call reads the policy slice
//     pol + p * pol_member_stride + (k - chunk_first) * pol_step_stride        [nu][S], control axis first
// and the row of lifted constants
//     prm + p * prm_member_stride + k * prm_step_stride                        [SDP_NPARAMS]
// A step stride of 0 is a stationary policy, or a model that is symbolic in time: one slice or row per member, passed
// once.  Member p of every array has the bits of `sdp_simulate_h` / `sdp_montecarlo_h` on problem p alone.
//
// Work decomposition.  The unit of work is a tile of trajectories of ONE member -- a workgroup: 64 in
// `sdp_family_simulate` (one wavefront, no LDS, no barrier), 256 in `sdp_family_montecarlo_h` -- so the member index is
// workgroup-uniform, and the step index is the same in every lane: the row of constants, the base of the policy slice,
// the grid ends and the seed are read through the constant address space or are a kernel-argument pointer plus
// uniform offsets.  In the Monte Carlo kernel the member's draw table (cum[n_law - 1] doubles, then values[n_law]
// reals) lives in dynamic LDS: loaded at a workgroup's first tile, and again -- between two barriers -- only where its
// next tile is another member's.  Every loop bound around a barrier, a ballot or a shuffle is workgroup-uniform.  Dead
// lanes of a member's last tile run along on a copy of that member's last row and store nothing; a wavefront without
// a live lane skips the steps.  Members map to XCDs as in sdp_family_sweep (the head of sdp_family_kernel.h) with
// that tile: with 8 members or more XCD x takes members x, x + 8, ..; with fewer every member is given 8 / P XCDs,
// each a contiguous part of its tiles.  Bounded grid (a multiple of 8), the workgroups stride over the tiles.
#pragma once
#define SDP_MC_HELPERS_ONLY 1          // sdp_mc_kernel.h without the solo entry point
#include "sdp_family_kernel.h"         // (SDP_FAMILY_HORIZON: the typedefs and sdp_model_cell_at's fallback only)
#include "sdp_mc_kernel.h"             // sdp_philox4x32_10, sdp_mc_uniform, sdp_mc_index, sdp_mc_visit

#define SDP_FH_SIM_TILE 64             // trajectories per tile of sdp_family_simulate: a workgroup of one wavefront
#define SDP_FH_MC_TILE SDP_MC_THREADS  // trajectories per tile of sdp_family_montecarlo_h: a workgroup

typedef const __attribute__((address_space(4))) uint64_t sdp_cst_u64;

// The walk of a workgroup over the tiles of its XCD's members (everything here is workgroup-uniform): `units` of them,
// unit -> (member, tile) by sdp_fh_unit; a tile beyond the member's last is skipped.
struct SdpFhWalk {
    int64_t tiles, per_part, units, stride;
    int first, part;
};

SDP_DEV SdpFhWalk sdp_fh_walk(int64_t B, int P, int64_t tile_rows)
{
    SdpFhWalk k;
    k.tiles = (B + tile_rows - 1) / tile_rows;                        // per member
    const int xcd = blockIdx.x & 7;
    const int parts = P >= 8 ? 1 : 8 / max(P, 1);                     // XCDs per member
    k.first = xcd / parts;                                            // first member of this XCD ..
    k.part = xcd % parts;                                             // .. and which part of its tiles
    const int mine = k.first < P ? (P - k.first + 7) / 8 : 0;
    k.per_part = (k.tiles + parts - 1) / parts;
    k.units = (int64_t)mine * k.per_part;
    k.stride = gridDim.x >> 3;
    return k;
}

// the grid of member p and its ends (sdp_grid_from_args on the member's axes, read as scalars)
template <typename Args>
SDP_DEV void sdp_fh_grid(const Args &a, int64_t p, SdpGrid<sdp_real, SDP_D> &grid, sdp_real *smin, sdp_real *smax)
{
    sdp_cst_real *axes = (sdp_cst_real *)a.axes + p * a.n_axes;
#pragma unroll
    for (int k = 0; k < SDP_D; ++k) {
        smin[k] = axes[a.axis_off[k]];
        smax[k] = axes[a.axis_off[k] + a.orders[k] - 1];
    }
    sdp_make_grid<sdp_real, SDP_D>(grid, a.orders, smin, smax);
}

// the loop of sdp_simulate_loop<true> with a member index: one lane per trajectory, a tile of 64 of one member a workgroup
extern "C" __global__ void __launch_bounds__(SDP_FH_SIM_TILE) sdp_family_simulate(SdpFamilySimHArgs a)
{
    constexpr int64_t tile_rows = SDP_FH_SIM_TILE;
    const SdpFhWalk k = sdp_fh_walk(a.B, a.P, tile_rows);
    for (int64_t unit = blockIdx.x >> 3; unit < k.units; unit += k.stride) {
        const int64_t tile = (int64_t)k.part * k.per_part + unit % k.per_part;
        if (tile >= k.tiles) continue;
        const int64_t p = k.first + 8 * (int)(unit / k.per_part);
        SdpGrid<sdp_real, SDP_D> grid;
        sdp_real smin[SDP_D], smax[SDP_D];
        sdp_fh_grid(a, p, grid, smin, smax);
        const sdp_real *__restrict__ pol = (const sdp_real *)a.pol + p * a.pol_member_stride;
        const sdp_real *prm = (const sdp_real *)a.prm + p * a.prm_member_stride;
        const sdp_real *__restrict__ wseq = a.w ? (const sdp_real *)a.w + p * a.T * a.B : nullptr;
        sdp_real *__restrict__ xo = (sdp_real *)a.x + p * (a.T + 1) * (int64_t)SDP_D * a.B;
        sdp_real *__restrict__ uo = (sdp_real *)a.u + p * a.T * (int64_t)SDP_NU * a.B;
        sdp_real *__restrict__ go = (sdp_real *)a.g + p * a.T * a.B;
        // a tile is one wavefront: with a live lane by construction (tile < tiles); the dead lanes of the member's last
        // tile run along on a copy of its last row and store nothing
        const int64_t b = tile * tile_rows + threadIdx.x;
        const bool live = b < a.B;
        const int64_t row = live ? b : a.B - 1;
        sdp_real x[SDP_D];
#pragma unroll
        for (int i = 0; i < SDP_D; ++i) x[i] = xo[(a.step_begin * SDP_D + i) * a.B + row];
        for (int64_t step = a.step_begin; step < a.step_end; ++step) {
            const sdp_real *__restrict__ pk = pol + (step - a.chunk_first) * a.pol_step_stride;
            const sdp_real *row_prm = (const sdp_real *)((sdp_cst_real *)prm + step * a.prm_step_stride);
            sdp_real u[SDP_NU], xn[SDP_D], g;
#pragma unroll
            for (int c = 0; c < SDP_NU; ++c)
                u[c] = sdp_interp_point<sdp_real, SDP_D, double>(pk + c * a.S, grid, x);
            const sdp_real w = wseq ? wseq[step * a.B + row] : (sdp_real)0;
            sdp_model_cell_at(x, u, w, (sdp_real)(a.t0 + (double)step), row_prm, xn, g);
            if (live) {
#pragma unroll
                for (int c = 0; c < SDP_NU; ++c) uo[(step * SDP_NU + c) * a.B + b] = u[c];
                go[step * a.B + b] = g;
            }
#pragma unroll
            for (int i = 0; i < SDP_D; ++i) {
                x[i] = xn[i];
                if (live) xo[((step + 1) * SDP_D + i) * a.B + b] = xn[i];
            }
        }
    }
}

#if SDP_HAS_W
// the loop of sdp_family_montecarlo (sdp_family_mc_kernel.h) with the policy slice and the constants row of the step
extern "C" __global__ void __launch_bounds__(SDP_FH_MC_TILE) sdp_family_montecarlo_h(SdpFamilyMcHArgs a)
{
    extern __shared__ double sdp_fh_lds[];                 // cum[W-1] (doubles), then law_grid[W] (reals)
    const int W = a.n_law;
    double *cum = sdp_fh_lds;
    sdp_real *wtab = (sdp_real *)(sdp_fh_lds + (W - 1));
    constexpr int64_t tile_rows = SDP_FH_MC_TILE;
    const SdpFhWalk k = sdp_fh_walk(a.B, a.P, tile_rows);

    int64_t loaded = -1;                                              // the member whose draw table is in LDS
    for (int64_t unit = blockIdx.x >> 3; unit < k.units; unit += k.stride) {
        const int64_t tile = (int64_t)k.part * k.per_part + unit % k.per_part;
        if (tile >= k.tiles) continue;
        const int64_t p = k.first + 8 * (int)(unit / k.per_part);
        if (p != loaded) {                                            // (workgroup-uniform: every thread reaches both barriers)
            __syncthreads();                                          // the last tile's draws are done with the old table
            const double *pc = a.cum + p * W;
            const sdp_real *pw = (const sdp_real *)a.law_grid + p * W;
            for (int i = threadIdx.x; i < W - 1; i += SDP_FH_MC_TILE) cum[i] = pc[i];
            for (int i = threadIdx.x; i < W; i += SDP_FH_MC_TILE) wtab[i] = pw[i];
            __syncthreads();
            loaded = p;
        }
        // a wavefront beyond the member's last row has nothing to do (wave-uniform; no barrier below this line)
        const int64_t base = tile * tile_rows + (threadIdx.x & ~63);
        if (base >= a.B) continue;

        SdpGrid<sdp_real, SDP_D> grid;
        sdp_real smin[SDP_D], smax[SDP_D];
        sdp_fh_grid(a, p, grid, smin, smax);
        const sdp_real *__restrict__ pol = (const sdp_real *)a.pol + p * a.pol_member_stride;
        const sdp_real *prm = (const sdp_real *)a.prm + p * a.prm_member_stride;
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
        for (int i = 0; i < SDP_D; ++i) x[i] = xs[i * a.B + row];
        sdp_real acc = accs[row];
        int n_out = 0;                                     // (of this launch: fewer than 2^31 steps)
        for (int64_t step = a.step_begin; step < a.step_end; ++step) {
            const sdp_real *__restrict__ pk = pol + (step - a.chunk_first) * a.pol_step_stride;
            const sdp_real *row_prm = (const sdp_real *)((sdp_cst_real *)prm + step * a.prm_step_stride);
            const bool counted = step >= a.n_burn;
            SdpCell<sdp_real, SDP_D, double> cell;
            bool outside = false;
#pragma unroll
            for (int i = 0; i < SDP_D; ++i) {
                sdp_locate_axis<sdp_real, SDP_D, double>(grid, i, x[i], cell);
                outside = outside || !(x[i] >= smin[i] && x[i] <= smax[i]);
            }
            n_out += (counted && outside) ? 1 : 0;
            if (occ) {
                int node = 0;
#pragma unroll
                for (int i = 0; i < SDP_D; ++i) {
                    const int q = cell.off[i] + ((cell.lam[i] >= (sdp_real)0.5) ? grid.M[i] : 0);     // M[i] * (cell + 1)
                    node += max(min(q, grid.M[i] * (a.orders[i] - 1)), 0);
                }
                sdp_mc_visit(occ, node, counted && live);
            }
            sdp_real u[SDP_NU], xn[SDP_D], g;
#pragma unroll
            for (int c = 0; c < SDP_NU; ++c)               // sdp_interp_point<sdp_real, SDP_D, double>, the cell located once
                u[c] = (sdp_real)SdpLerp<sdp_real, SDP_D, double, 0, false>::eval(pk + c * a.S, grid, cell, 0);
            const SdpPhilox r = sdp_philox4x32_10((unsigned)id, (unsigned)(id >> 32), (unsigned)step,
                                                  (unsigned)((unsigned long long)step >> 32), k0, k1);
            const int j = sdp_mc_index(cum, W - 1, sdp_mc_uniform(r));     // 0 <= j <= W - 1
            const sdp_real w = wtab[j];
            sdp_model_cell_at(x, u, w, (sdp_real)(a.t0 + (double)step), row_prm, xn, g);
            if (counted) acc = acc + g;
#pragma unroll
            for (int i = 0; i < SDP_D; ++i) x[i] = xn[i];
        }
        if (live) {
#pragma unroll
            for (int i = 0; i < SDP_D; ++i) xs[i * a.B + b] = x[i];
            accs[b] = acc;
            a.n_outside[p * a.B + b] += n_out;
        }
    }
}
#define SDP_FH_MC_THREADS SDP_FH_MC_TILE
#else
#define SDP_FH_MC_THREADS 0            // a deterministic unit has sdp_family_simulate alone
#endif  // SDP_HAS_W

// what this code object was generated for (sdp_kernel_args.h, SDP_META_*)
extern "C" {
__constant__ int32_t sdp_meta[SDP_META_WORDS] = {
    SDP_META_MAGIC, (int32_t)sizeof(sdp_real), SDP_D, SDP_NU, SDP_HAS_W, 0, 0, 1,
    SDP_META_F_FAMILY | SDP_META_F_FAMILY_HORIZON, 0, 0, SDP_FH_MC_THREADS, SDP_FH_SIM_TILE, 0, 0, 0};
}
