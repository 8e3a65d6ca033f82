// sdp_family_lookahead_horizon_kernel.h -- closed loops of a FAMILY of same-shaped problems under one-step lookahead
// controls over a horizon (kernels `sdp_family_simulate_lookahead` and `sdp_family_montecarlo_lookahead_h`): the forward
// half of a finite-horizon study scored under the controller that would run.
//
// Included LAST by a generated unit (codegen.family_lookahead_horizon_unit), after the direct prologue with
//   SDP_FAMILY 1, SDP_FAMILY_LOOKAHEAD_HORIZON 1, SDP_REAL, SDP_D, SDP_NU, SDP_HAS_W, SDP_LANES, SDP_NPARAMS, SDP_NBOXPARAMS
//   sdp_model_cell_at(x, u, w, t, prm, xn, g)    the traced dyn/cost with its constants read from a row `prm`
//   sdp_model_box_at(x, t, bprm, lo, hi)         the traced control_box, in double, its constants read from a row `bprm`
//
// `sdp_family_simulate_lookahead` is `sdp_simulate_lookahead` (sdp_lookahead_kernel.h) restated with a member index,
// statement for statement; `sdp_family_montecarlo_lookahead_h` is `sdp_family_montecarlo_lookahead`
// (sdp_family_lookahead_kernel.h).  Both with the two things that change from step to step addressed by strides
// (SdpFamilyLookSimArgs): member p at step k of the call looks ahead into the cost-to-go
//     V + p * V_member_stride + (k - chunk_first) * V_step_stride             [S]
// and runs -- the backup and the plant's step -- on the row of lifted constants
//     prm + p * prm_member_stride + k * prm_step_stride                       [SDP_NPARAMS]
// A step stride of 0 is one cost-to-go for every step, or a model that is symbolic in time: one slice or row per member,
// passed once.  Both addresses are workgroup-uniform -- kernel arguments, the member index and the step -- so they are
// scalar arithmetic, and the row is read through the constant address space.  The box constants are per member, not per
// step; the box function takes the time index t0 + k.  Member p of every array has the bits of the solo kernel on
// problem p alone.
//
// Work decomposition: that of sdp_family_lookahead_kernel.h, whose helpers these kernels call (`sdp_flook_walk`,
// `sdp_flook_box`, `sdp_flook_backup`: written once, there).  A tile of (64 / SDP_LANES) x 4 trajectories of ONE member is
// a workgroup of 256; an idle group runs along on the first trajectory of its own wave and stores nothing; a wave without
// a live trajectory skips the steps (below the barriers of the Monte Carlo kernel; the closed loop has none).  Every
// loop bound around a barrier, a ballot or a shuffle is wave- or workgroup-uniform.  The draw table of the Monte Carlo
// kernel lives in dynamic LDS as there.  Plain vector stores from C++, no launch bound beyond the workgroup size.
#pragma once
#define SDP_FAMILY_LOOKAHEAD 1         // sdp_family_kernel.h without the sweep kernel, as for a family lookahead unit
#define SDP_FLOOK_HELPERS_ONLY 1       // sdp_family_lookahead_kernel.h without its two kernels and its sdp_meta
#include "sdp_family_lookahead_kernel.h"

// the cost-to-go slice and the row of constants of member p at step `step` (workgroup-uniform)
template <typename Args>
SDP_DEV void sdp_flookh_step(const Args &a, int64_t p, int64_t step, SdpMember &m)
{
    m.V = (const sdp_real *)a.f.V + p * a.V_member_stride + (step - a.chunk_first) * a.V_step_stride;
    m.prm = (const sdp_real *)((sdp_cst_real *)a.f.prm + p * a.prm_member_stride + step * a.prm_step_stride);
}

extern "C" __global__ void __launch_bounds__(SDP_FLOOK_THREADS) sdp_family_simulate_lookahead(SdpFamilyLookSimArgs a)
{
    constexpr int L = SDP_LANES;
    constexpr int NPW = 64 / L;                       // trajectories per wavefront
    constexpr int64_t tile_rows = (int64_t)NPW * (SDP_FLOOK_THREADS / 64);
    const int lane = threadIdx.x & 63;
    const int sub = lane & (L - 1);
    const int slot = lane / L;
    const int wave = threadIdx.x >> 6;

    SdpFamilyWalk w;
    sdp_flook_walk(a.B, tile_rows, a.f.n_active, w);
    for (int64_t unit = blockIdx.x >> 3; unit < w.units; unit += w.stride) {
        const int64_t tile = (int64_t)w.part * w.per_part + unit % w.per_part;
        if (tile >= w.tiles) continue;                // (workgroup-uniform)
        const int64_t p = w.first + 8 * (int)(unit / w.per_part);
        // a wavefront beyond the member's last trajectory has nothing to do (wave-uniform; the kernel has no barrier)
        const int64_t b_wave = tile * tile_rows + (int64_t)wave * NPW;
        if (b_wave >= a.B) continue;

        SdpMember m;
        SdpGrid<sdp_real, SDP_D> grid;
        sdp_family_member(a.f, p, m, grid);
        const sdp_real *__restrict__ wseq = a.w ? (const sdp_real *)a.w + p * a.T * a.B : nullptr;
        sdp_real *xo = (sdp_real *)a.x + p * (a.T + 1) * (int64_t)SDP_D * a.B;      // (row step_begin is read, the later rows written)
        sdp_real *uo = (sdp_real *)a.u + p * a.T * (int64_t)SDP_NU * a.B;
        sdp_real *go = (sdp_real *)a.g + p * a.T * a.B;
        sdp_real *qo = (sdp_real *)a.q + p * a.T * a.B;

        const int64_t b = b_wave + slot;
        const bool live = b < a.B;
        const int64_t bb = live ? b : b_wave;         // (an idle group computes on the wave's first trajectory and stores nothing)
        sdp_real x[SDP_D];
#pragma unroll
        for (int k = 0; k < SDP_D; ++k) x[k] = xo[(a.step_begin * SDP_D + k) * a.B + bb];
        // (the bound is the same in every lane of the wave: the shuffles of the argmin run with every lane in step)
        for (int64_t step = a.step_begin; step < a.step_end; ++step) {
            sdp_flookh_step(a, p, step, m);
            const double td = a.t0 + (double)step;
            const sdp_real t = (sdp_real)td;
            SdpBox box;
            const bool valid = sdp_flook_box(a.bprm, a.steps, p, x, td, box);
            sdp_real best;
            int ibest;
            sdp_flook_backup(a.f, m, grid, x, t, box, valid, sub, best, ibest);
            sdp_real u[SDP_NU], xn[SDP_D], g;
            if (valid) sdp_controls_at(box, ibest, u);
#pragma unroll
            for (int c = 0; c < SDP_NU; ++c) u[c] = valid ? u[c] : (sdp_real)NAN;
            if (!valid) best = (sdp_real)NAN;
            const sdp_real wk = wseq ? wseq[step * a.B + bb] : (sdp_real)0;
            sdp_model_cell_at(x, u, wk, t, m.prm, xn, g);
            if (live && sub == 0) {
#pragma unroll
                for (int c = 0; c < SDP_NU; ++c) uo[(step * SDP_NU + c) * a.B + b] = u[c];
                go[step * a.B + b] = g;
                qo[step * a.B + b] = best;
#pragma unroll
                for (int k = 0; k < SDP_D; ++k) xo[((step + 1) * SDP_D + k) * a.B + b] = xn[k];
            }
#pragma unroll
            for (int k = 0; k < SDP_D; ++k) x[k] = xn[k];
        }
    }
}

#if SDP_HAS_W
extern "C" __global__ void __launch_bounds__(SDP_FLOOK_THREADS) sdp_family_montecarlo_lookahead_h(SdpFamilyLookMcHArgs a)
{
    constexpr int L = SDP_LANES;
    constexpr int NPW = 64 / L;                       // trajectories per wavefront
    constexpr int64_t tile_rows = (int64_t)NPW * (SDP_FLOOK_THREADS / 64);
    extern __shared__ double sdp_flook_lds[];         // cum[n_law - 1] (doubles), then law_grid[n_law] (reals)
    const int n_law = a.n_law;
    double *cum = sdp_flook_lds;
    sdp_real *wtab = (sdp_real *)(sdp_flook_lds + (n_law - 1));
    const int lane = threadIdx.x & 63;
    const int sub = lane & (L - 1);
    const int slot = lane / L;
    const int wave = threadIdx.x >> 6;

    SdpFamilyWalk w;
    sdp_flook_walk(a.B, tile_rows, a.f.n_active, w);
    int64_t loaded = -1;                              // the member whose draw table is in LDS
    for (int64_t unit = blockIdx.x >> 3; unit < w.units; unit += w.stride) {
        const int64_t tile = (int64_t)w.part * w.per_part + unit % w.per_part;
        if (tile >= w.tiles) continue;                // (workgroup-uniform)
        const int64_t p = w.first + 8 * (int)(unit / w.per_part);
        if (p != loaded) {                            // (workgroup-uniform: every thread reaches both barriers)
            __syncthreads();                          // the last tile's draws are done with the old table
            const double *pc = a.cum + p * n_law;
            const sdp_real *pw = (const sdp_real *)a.law_grid + p * n_law;
            for (int i = threadIdx.x; i < n_law - 1; i += SDP_FLOOK_THREADS) cum[i] = pc[i];
            for (int i = threadIdx.x; i < n_law; i += SDP_FLOOK_THREADS) wtab[i] = pw[i];
            __syncthreads();
            loaded = p;
        }
        // a wavefront beyond the member's last trajectory has nothing to do (wave-uniform; no barrier below this line)
        const int64_t b_wave = tile * tile_rows + (int64_t)wave * NPW;
        if (b_wave >= a.B) continue;

        SdpMember m;
        SdpGrid<sdp_real, SDP_D> grid;
        sdp_family_member(a.f, p, m, grid);
        sdp_real smax[SDP_D];
#pragma unroll
        for (int k = 0; k < SDP_D; ++k) smax[k] = m.axes[a.f.axis_off[k] + a.f.orders[k] - 1];
        unsigned long long *occ = a.occupancy ? a.occupancy + p * a.f.S : nullptr;
        sdp_real *xs = (sdp_real *)a.x + p * (int64_t)SDP_D * a.B;     // (read at the start of a tile, written at its end: not __restrict__)
        sdp_real *accs = (sdp_real *)a.acc + p * a.B;
        const uint64_t seed = ((sdp_cst_u64 *)a.seed)[p];
        const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);

        const int64_t b = b_wave + slot;
        const bool live = b < a.B;
        // an idle group runs along on the first trajectory of its own wave and stores nothing (the shuffles of the argmin
        // and the ballots of the occupancy need every lane); a wave reads its states before it stores them
        const int64_t bb = live ? b : b_wave;
        const unsigned long long id = a.traj_offset + (unsigned long long)bb;
        sdp_real x[SDP_D];
#pragma unroll
        for (int k = 0; k < SDP_D; ++k) x[k] = xs[k * a.B + bb];
        sdp_real acc = accs[bb];
        int n_out = 0;                                // (of this launch: at most 2^30 steps)
        // (the bound is the same in every lane of the wave: the shuffles of the argmin and the ballots run with every lane in step)
        for (int64_t step = a.step_begin; step < a.step_end; ++step) {
            sdp_flookh_step(a, p, step, m);
            const bool counted = step >= a.n_burn;
            bool outside = false;
#pragma unroll
            for (int k = 0; k < SDP_D; ++k) outside = outside || !(x[k] >= grid.smin[k] && x[k] <= smax[k]);
            n_out += (counted && outside) ? 1 : 0;
            if (occ) {                                // (workgroup-uniform)
                SdpCell<sdp_real, SDP_D, double> cell;
                int node = 0;
#pragma unroll
                for (int k = 0; k < SDP_D; ++k) {
                    sdp_locate_axis<sdp_real, SDP_D, double>(grid, k, x[k], cell);
                    const int q = cell.off[k] + ((cell.lam[k] >= (sdp_real)0.5) ? grid.M[k] : 0);     // M[k] * (cell + 1)
                    node += max(min(q, grid.M[k] * (a.f.orders[k] - 1)), 0);
                }
                sdp_mc_visit(occ, node, counted && live && sub == 0);
            }
            const double td = a.t0 + (double)step;
            const sdp_real t = (sdp_real)td;
            SdpBox box;
            const bool valid = sdp_flook_box(a.bprm, a.steps, p, x, td, box);
            sdp_real best;
            int ibest;
            sdp_flook_backup(a.f, m, grid, x, t, box, valid, sub, best, ibest);
            sdp_real u[SDP_NU], xn[SDP_D], g;
            if (valid) sdp_controls_at(box, ibest, u);
#pragma unroll
            for (int c = 0; c < SDP_NU; ++c) u[c] = valid ? u[c] : (sdp_real)NAN;
            const SdpPhilox r = sdp_philox4x32_10((unsigned)id, (unsigned)(id >> 32), (unsigned)step,
                                                  (unsigned)((unsigned long long)step >> 32), k0, k1);
            const int j = sdp_mc_index(cum, n_law - 1, sdp_mc_uniform(r));     // 0 <= j <= n_law - 1
            const sdp_real wk = wtab[j];
            sdp_model_cell_at(x, u, wk, t, m.prm, xn, g);
            if (counted) acc = acc + g;
#pragma unroll
            for (int k = 0; k < SDP_D; ++k) x[k] = xn[k];
        }
        if (live && sub == 0) {
#pragma unroll
            for (int k = 0; k < SDP_D; ++k) xs[k * a.B + b] = x[k];
            accs[b] = acc;
            a.n_outside[p * a.B + b] += n_out;
        }
    }
}
#endif  // SDP_HAS_W

// what this code object was generated for (sdp_kernel_args.h, SDP_META_*)
extern "C" {
__constant__ int32_t sdp_meta[SDP_META_WORDS] = {
    SDP_META_MAGIC, (int32_t)sizeof(sdp_real), SDP_D, SDP_NU, SDP_HAS_W, 0, 0, 1,
    SDP_META_F_FAMILY | SDP_META_F_FAMILY_LOOKAHEAD_HORIZON, SDP_NBOXPARAMS, 0, SDP_FLOOK_THREADS, SDP_LANES, 0, 0, 0};
}
