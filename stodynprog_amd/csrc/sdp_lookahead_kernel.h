// sdp_lookahead_kernel.h -- one-step lookahead at ARBITRARY states (kernels `sdp_lookahead`,
// `sdp_simulate_lookahead` and `sdp_montecarlo_lookahead`): what turns a cost-to-go into a decision at the state the
// plant is in.
//
// Included by sdp_sweep_kernel.h under SDP_LOOKAHEAD -- in the one-variable branch and in the branch of several
// perturbation variables (SDP_NW >= 2) -- after the direct kernels, so only lookahead units carry it and every
// other unit compiles to the code object it compiled to before.  The definition is stodynprog_amd/lookahead.py.
//
//   sdp_lookahead            `sdp_sweep`'s mapping with the node replaced by state b of a batch: a wave owns
//                            64 / SDP_LANES consecutive states, their lanes stride the control lattice,
//                            `sdp_expected_cost` (or its twin on the flat law) unchanged, `sdp_seg_argmin`.
//                            x is read from [d][B]; J[B], idx[B] and u[nu][B] are written.
//   sdp_simulate_lookahead   (units with SDP_LOOKAHEAD_BOX) the per-trajectory loop: the SDP_LANES lanes of a
//                            trajectory run all the steps of a launch; per step the box at the carried state, the
//                            lattice, the segmented argmin, then every lane of the group evaluates the model once at
//                            u_opt and w[k][b] and lane 0 of the group stores x, u, g and q at their absolute steps.
//   sdp_montecarlo_lookahead (.. of a stochastic system) that loop with w DRAWN on the device and reduced per trajectory:
//                            the draw, the sums and the occupancy of `sdp_montecarlo`, nothing stored per step.
//
// The control lattice of a state comes from one of two places that give the same bits:
//   * host-made arrays lo, hi, n of shape [nu][B] (SdpLookArgs.box_n not null): the host evaluated the box;
//   * the unit's own `sdp_model_box(const double *x, double t, double *lo, double *hi)` (SDP_LOOKAHEAD_BOX: the
//     traced control_box, emitted in double whatever the unit's reals) and a restatement of DPSolver._box_lattice:
//     in double, n_interv = (hi - lo) / step; n_interv < 0.1: one point at (lo + hi) / 2; else n = ceil(n_interv) + 1;
//     then ONE rounding of lo and hi to sdp_real.  A 4-byte state is widened first.
// A state whose box has a non-finite end, or whose lattice total reaches 2^31, has no valid lattice: J and u are
// NaN, idx is -1 (host arrays say so with n[0][b] == 0).
//
// Launch rules: no launch bound beyond the workgroup size, the law through the constant address space (several
// variables; one variable reads it as `sdp_expected_cost` does), plain vector stores from C++.
#pragma once

#if defined(SDP_NW) && SDP_NW >= 2
#define SDP_LOOK_COST sdp_expected_cost_mw<false>
#else
#define SDP_LOOK_COST sdp_expected_cost<false>
#endif

// the fields of SdpSweepArgs that sdp_expected_cost and sdp_grid_from_args read (the rest stays zero and folds away)
template <typename Args>
SDP_DEV void sdp_look_sweep_args(const Args &a, SdpSweepArgs &s)
{
    s.axes = a.axes;
    s.wgrid = a.wgrid;
    s.proba = a.proba;
    s.W = a.W;
#pragma unroll
    for (int k = 0; k < SDP_MAXD; ++k) { s.orders[k] = a.orders[k]; s.axis_off[k] = a.axis_off[k]; }
}

#include "sdp_lattice_kernel.h"  // sdp_look_finish_box, sdp_look_lattice: the lattice rule, shared with the family lookahead kernels

// the lattice of state b from host-made arrays [nu][B]; false: the state has none
SDP_DEV bool sdp_look_box_host(const void *box_lo, const void *box_hi, const int32_t *box_n, int64_t B, int64_t b, SdpBox &box)
{
#pragma unroll
    for (int c = 0; c < SDP_NU; ++c) {
        box.lo[c] = ((const sdp_real *)box_lo)[c * B + b];
        box.hi[c] = ((const sdp_real *)box_hi)[c * B + b];
        box.n[c] = box_n[c * B + b];
    }
    const bool ok = box.n[0] > 0;
    sdp_look_finish_box(box);
    return ok;
}

#if defined(SDP_LOOKAHEAD_BOX)
// the lattice of the state x from the unit's own box function: DPSolver._box_lattice in double, one rounding
// (sdp_lattice_kernel.h)
SDP_DEV bool sdp_look_box_device(const sdp_real *x, double t, const double *steps, SdpBox &box)
{
    return sdp_look_lattice(x, steps, box, [t](const double *xd, double *lo, double *hi) { sdp_model_box(xd, t, lo, hi); });
}
#endif

// the backup of one state by the SDP_LANES lanes of its group: every lane of the group ends with (J_opt, idx)
SDP_DEV void sdp_look_backup(const SdpSweepArgs &s, const SdpGrid<sdp_real, SDP_D> &grid, const sdp_real *__restrict__ V,
                             const sdp_real *x, sdp_real t, const SdpBox &box, bool run, int sub, sdp_real &best, int &ibest)
{
    best = INFINITY;
    ibest = INT_MAX;
    if (run) {
        for (int ci = sub; ci < box.total; ci += SDP_LANES) {
            sdp_real u[SDP_NU];
            sdp_controls_at(box, ci, u);
            const sdp_real jc = SDP_LOOK_COST(s, grid, V, x, u, t);
            if (ibest == INT_MAX || sdp_better_seq(jc, best)) { best = jc; ibest = ci; }
        }
    }
    sdp_seg_argmin<sdp_real, SDP_LANES>(best, ibest);
}

extern "C" __global__ void __launch_bounds__(256) sdp_lookahead(SdpLookArgs a)
{
    constexpr int L = SDP_LANES;
    constexpr int NPW = 64 / L;                       // states per wavefront
    const int lane = threadIdx.x & 63;
    const int sub = lane & (L - 1);
    const int slot = lane / L;
    const int wave = threadIdx.x >> 6;
    const int waves = blockDim.x >> 6;
    const int64_t tile_states = (int64_t)NPW * waves;

    const sdp_real *__restrict__ V = (const sdp_real *)a.V;
    const sdp_real *__restrict__ xs = (const sdp_real *)a.x;
    SdpSweepArgs s = {};
    sdp_look_sweep_args(a, s);
    SdpGrid<sdp_real, SDP_D> grid;
    sdp_grid_from_args(s, grid);
    const sdp_real t = (sdp_real)a.t_k;

    // the direct kernel's walk: XCD x takes the x-th contiguous eighth of the tiles (states placed at
    // neighbouring nodes then share one L2, as the nodes of a sweep do)
    const int64_t n_tiles = (a.B + tile_states - 1) / tile_states;
    const int xcd = blockIdx.x & 7;
    const int64_t per_xcd = (n_tiles + 7) / 8;
    const int64_t t_end = min((int64_t)(xcd + 1) * per_xcd, n_tiles);
    const int64_t stride = gridDim.x >> 3;

    for (int64_t tile = (int64_t)xcd * per_xcd + (blockIdx.x >> 3); tile < t_end; tile += stride) {
        const int64_t b = tile * tile_states + (int64_t)wave * NPW + slot;
        const bool live = b < a.B;
        SdpBox box;
        sdp_real x[SDP_D];
        bool valid = false;
        if (live) {
#pragma unroll
            for (int k = 0; k < SDP_D; ++k) x[k] = xs[k * a.B + b];
#if defined(SDP_LOOKAHEAD_BOX)
            if (!a.box_n) valid = sdp_look_box_device(x, a.t_k, a.steps, box);
            else
#endif
            valid = sdp_look_box_host(a.box_lo, a.box_hi, a.box_n, a.B, b, box);
        }
        sdp_real best;
        int ibest;
        sdp_look_backup(s, grid, V, x, t, box, live && valid, sub, best, ibest);
        if (live && sub == 0) {
            sdp_real u[SDP_NU];
            if (valid) sdp_controls_at(box, ibest, u);
#pragma unroll
            for (int c = 0; c < SDP_NU; ++c) ((sdp_real *)a.u)[c * a.B + b] = valid ? u[c] : (sdp_real)NAN;
            ((sdp_real *)a.J)[b] = valid ? best : (sdp_real)NAN;
            a.idx[b] = valid ? ibest : -1;
        }
    }
}

#if defined(SDP_LOOKAHEAD_BOX)
extern "C" __global__ void __launch_bounds__(256) sdp_simulate_lookahead(SdpLookSimArgs a)
{
    constexpr int L = SDP_LANES;
    constexpr int NPW = 64 / L;                       // trajectories per wavefront
    const int lane = threadIdx.x & 63;
    const int sub = lane & (L - 1);
    const int slot = lane / L;
    const int wave = threadIdx.x >> 6;
    const int waves = blockDim.x >> 6;
    const int64_t tile_traj = (int64_t)NPW * waves;

    SdpSweepArgs s = {};
    sdp_look_sweep_args(a, s);
    SdpGrid<sdp_real, SDP_D> grid;
    sdp_grid_from_args(s, grid);
    const sdp_real *__restrict__ wseq = (const sdp_real *)a.w;
    sdp_real *xo = (sdp_real *)a.x;                   // (row step_begin is read, the later rows written)
    sdp_real *uo = (sdp_real *)a.u;
    sdp_real *go = (sdp_real *)a.g;
    sdp_real *qo = (sdp_real *)a.q;

    const int64_t n_tiles = (a.B + tile_traj - 1) / tile_traj;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t b = tile * tile_traj + (int64_t)wave * NPW + slot;
        const bool live = b < a.B;
        const int64_t bb = live ? b : 0;              // (a dead group computes on trajectory 0 and stores nothing)
        sdp_real x[SDP_D];
#pragma unroll
        for (int k = 0; k < SDP_D; ++k) x[k] = xo[(a.step_begin * SDP_D + k) * a.B + bb];
        // (the bound is the same in every lane of the wave: the shuffles of the argmin run with every lane in step)
        for (int64_t step = a.step_begin; step < a.step_end; ++step) {
            const sdp_real *__restrict__ V = (const sdp_real *)a.V + (step - a.chunk_first) * a.V_stride;
            const double td = a.t0 + (double)step;
            const sdp_real t = (sdp_real)td;
            SdpBox box;
            const bool valid = sdp_look_box_device(x, td, a.steps, box);
            sdp_real best;
            int ibest;
            sdp_look_backup(s, grid, V, x, t, box, valid, sub, best, ibest);
            sdp_real u[SDP_NU], xn[SDP_D], g;
            if (valid) sdp_controls_at(box, ibest, u);
#pragma unroll
            for (int c = 0; c < SDP_NU; ++c) u[c] = valid ? u[c] : (sdp_real)NAN;
            if (!valid) best = (sdp_real)NAN;
#if defined(SDP_NW) && SDP_NW >= 2
            sdp_real w[SDP_NW];
#pragma unroll
            for (int i = 0; i < SDP_NW; ++i) w[i] = wseq[(step * SDP_NW + i) * a.B + bb];
#else
            const sdp_real w = wseq ? wseq[step * a.B + bb] : (sdp_real)0;
#endif
            sdp_model_cell(x, u, w, t, xn, g);
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
// Monte Carlo evaluation under lookahead controls: the loop of `sdp_simulate_lookahead` with the perturbation of every
// step drawn as `sdp_montecarlo_loop` draws it (Philox keyed by the seed, counter = (trajectory id, step of the call),
// the cumulative table and the values staged once per workgroup in dynamic LDS) and nothing stored per step: per
// trajectory acc = acc + g_k and the steps outside the grid over k >= n_burn, optionally the occupancy.  The
// definition is stodynprog_amd/lookahead.py:monte_carlo_lookahead.
//   * EVERY lane of a group computes the draw itself: it is a function of (seed, id, step) alone, so the lanes of a
//     group get the same w without a shuffle, and a wave executes the ten rounds once whichever lanes want them.
//   * A group past the end of the batch runs along on the FIRST trajectory of its own wave (the shuffles of the argmin
//     and the ballots of the occupancy need every lane), stores nothing and counts nothing; a wave without a live
//     trajectory skips the tile.  A wave reads its states before it stores them, so nobody reads a row that another
//     wave is writing -- which trajectory 0 of the batch would be, the state being updated in place here.
extern "C" __global__ void __launch_bounds__(256) sdp_montecarlo_lookahead(SdpLookMcArgs a)
{
    constexpr int L = SDP_LANES;
    constexpr int NPW = 64 / L;                       // trajectories per wavefront
#if defined(SDP_NW) && SDP_NW >= 2
    constexpr int NW = SDP_NW;
#else
    constexpr int NW = 1;
#endif
    extern __shared__ double sdp_look_mc_lds[];       // cum[n_law - 1] (doubles), then law_grid[NW][n_law] (reals)
    const int n_law = a.n_law;
    double *cum = sdp_look_mc_lds;
    sdp_real *wtab = (sdp_real *)(sdp_look_mc_lds + (n_law - 1));
    for (int i = threadIdx.x; i < n_law - 1; i += blockDim.x) cum[i] = a.cum[i];
    for (int i = threadIdx.x; i < NW * n_law; i += blockDim.x) wtab[i] = ((const sdp_real *)a.law_grid)[i];
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const int sub = lane & (L - 1);
    const int slot = lane / L;
    const int wave = threadIdx.x >> 6;
    const int waves = blockDim.x >> 6;
    const int64_t tile_traj = (int64_t)NPW * waves;

    SdpSweepArgs s = {};
    sdp_look_sweep_args(a, s);
    SdpGrid<sdp_real, SDP_D> grid;
    sdp_grid_from_args(s, grid);
    sdp_real smax[SDP_D];
#pragma unroll
    for (int k = 0; k < SDP_D; ++k) smax[k] = ((const sdp_real *)a.axes)[a.axis_off[k] + a.orders[k] - 1];
    sdp_real *xs = (sdp_real *)a.x;                   // (read at the start of a tile, written at its end: not __restrict__)
    sdp_real *accs = (sdp_real *)a.acc;
    const unsigned k0 = (unsigned)a.seed, k1 = (unsigned)(a.seed >> 32);

    const int64_t n_tiles = (a.B + tile_traj - 1) / tile_traj;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t b_wave = tile * tile_traj + (int64_t)wave * NPW;
        if (b_wave >= a.B) continue;                  // (wave-uniform: no trajectory of this wave is live)
        const int64_t b = b_wave + slot;
        const bool live = b < a.B;
        const int64_t bb = live ? b : b_wave;
        const unsigned long long id = a.traj_offset + (unsigned long long)bb;
        sdp_real x[SDP_D];
#pragma unroll
        for (int k = 0; k < SDP_D; ++k) x[k] = xs[k * a.B + bb];
        sdp_real acc = accs[bb];
        int n_out = 0;                                // (of this launch: at most 2^30 steps)
        // (the bound is the same in every lane of the wave: the shuffles of the argmin and the ballots run with every lane in step)
        for (int64_t step = a.step_begin; step < a.step_end; ++step) {
            const sdp_real *__restrict__ V = (const sdp_real *)a.V + (step - a.chunk_first) * a.V_stride;
            const bool counted = step >= a.n_burn;
            bool outside = false;
#pragma unroll
            for (int k = 0; k < SDP_D; ++k) outside = outside || !(x[k] >= grid.smin[k] && x[k] <= smax[k]);
            n_out += (counted && outside) ? 1 : 0;
            if (a.occupancy) {                        // (wave-uniform)
                SdpCell<sdp_real, SDP_D, double> cell;
                int node = 0;
#pragma unroll
                for (int k = 0; k < SDP_D; ++k) {
                    sdp_locate_axis<sdp_real, SDP_D, double>(grid, k, x[k], cell);
                    const int q = cell.off[k] + ((cell.lam[k] >= (sdp_real)0.5) ? grid.M[k] : 0);     // M[k] * (cell + 1)
                    node += max(min(q, grid.M[k] * (a.orders[k] - 1)), 0);
                }
                sdp_mc_visit(a.occupancy, node, counted && live && sub == 0);
            }
            const double td = a.t0 + (double)step;
            const sdp_real t = (sdp_real)td;
            SdpBox box;
            const bool valid = sdp_look_box_device(x, td, a.steps, box);
            sdp_real best;
            int ibest;
            sdp_look_backup(s, grid, V, x, t, box, valid, sub, best, ibest);
            sdp_real u[SDP_NU], xn[SDP_D], g;
            if (valid) sdp_controls_at(box, ibest, u);
#pragma unroll
            for (int c = 0; c < SDP_NU; ++c) u[c] = valid ? u[c] : (sdp_real)NAN;
            const SdpPhilox r = sdp_philox4x32_10((unsigned)id, (unsigned)(id >> 32), (unsigned)step,
                                                  (unsigned)((unsigned long long)step >> 32), k0, k1);
            const int j = sdp_mc_index(cum, n_law - 1, sdp_mc_uniform(r));     // 0 <= j <= n_law - 1
#if defined(SDP_NW) && SDP_NW >= 2
            sdp_real w[SDP_NW];
#pragma unroll
            for (int i = 0; i < SDP_NW; ++i) w[i] = wtab[i * n_law + j];
#else
            const sdp_real w = wtab[j];
#endif
            sdp_model_cell(x, u, w, t, xn, g);
            if (counted) acc = acc + g;
#pragma unroll
            for (int k = 0; k < SDP_D; ++k) x[k] = xn[k];
        }
        if (live && sub == 0) {
#pragma unroll
            for (int k = 0; k < SDP_D; ++k) xs[k * a.B + b] = x[k];
            accs[b] = acc;
            a.n_outside[b] += n_out;
        }
    }
}
#endif  // SDP_HAS_W
#endif
