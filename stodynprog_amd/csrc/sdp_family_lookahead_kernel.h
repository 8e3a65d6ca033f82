// sdp_family_lookahead_kernel.h -- one-step lookahead at arbitrary states, and its Monte Carlo score, for a FAMILY of
// same-shaped problems (kernels `sdp_family_lookahead` and `sdp_family_montecarlo_lookahead`).
//
// Included LAST by a generated family lookahead unit (codegen.family_lookahead_unit), after the direct prologue with
//   SDP_FAMILY 1, SDP_FAMILY_LOOKAHEAD 1, SDP_REAL, SDP_D, SDP_NU, SDP_HAS_W, SDP_LANES, SDP_NPARAMS, SDP_NBOXPARAMS
//   sdp_model_cell_at(x, u, w, t, prm, xn, g)    the traced dyn/cost with its constants read from a row `prm`
//   sdp_model_box_at(x, t, bprm, lo, hi)         the traced control_box, in double, its constants read from a row `bprm`
//
// The kernels are `sdp_lookahead` and `sdp_montecarlo_lookahead` of sdp_lookahead_kernel.h restated with a member
// index, statement for statement, the way sdp_family_sweep restates sdp_sweep and sdp_family_montecarlo the solo loop:
// the box at the state in double on the member's row of box constants, the lattice rule of sdp_lattice_kernel.h (the
// one the solo kernels include, not a copy) with the member's control steps, `sdp_look_backup`'s control loop -- the
// SDP_LANES lanes of a state stride its lattice, `sdp_better_seq`, `sdp_seg_argmin` -- on `sdp_family_expected_cost`
// (the member's constants, law and cost-to-go), and in the closed loop the draw of sdp_mc_kernel.h (its helpers) on the
// member's seed and draw table, the traced model at u_opt, `acc = acc + g` for the counted steps.  Member p of every
// array has the bits of the solo kernel on problem p alone.
//
// Work decomposition.  The unit of work is a tile of (64 / SDP_LANES) x 4 states (trajectories) of ONE member -- a
// workgroup of 256 -- so the member index is workgroup-uniform, and with it the row of model constants, the row of box
// constants, the control steps, the grid ends, the law of the backup and the seed: read through the constant address
// space.  Members map to XCDs as in sdp_family_montecarlo (the head of sdp_family_kernel.h) with that tile: with 8
// members or more XCD x takes members x, x + 8, ..; with fewer every member is given 8 / P XCDs, each a contiguous
// part of its tiles.  Bounded grid (a multiple of 8), the workgroups stride over the tiles.  Every loop bound around
// a barrier, a ballot or a shuffle is workgroup- or wave-uniform.
//
// The closed loop.  The plant's draw table of the member (cum[n_law - 1] doubles, then values[n_law] reals) lives in
// dynamic LDS: loaded at a workgroup's first tile, and again -- between two barriers -- only where its next tile is
// another member's.  EVERY lane of a group computes the draw itself (a function of (seed, id, step) alone: the lanes of
// a group get the same w without a shuffle).  A group past the end of the member's batch runs along on the FIRST
// trajectory of its own wave and stores nothing; a wave without a live trajectory skips the steps (below the
// barriers).  The occupancy goes through `sdp_mc_visit` with the flag set in the leading lane of a group.  State, sums
// and counters stay in device buffers between launches.  Plain vector stores from C++, no launch bound beyond the
// workgroup size.
#pragma once
#define SDP_MC_HELPERS_ONLY 1          // sdp_mc_kernel.h without the solo entry point
#include "sdp_family_kernel.h"         // (SDP_FAMILY_LOOKAHEAD: SdpMember, sdp_family_member, sdp_family_expected_cost; no sweep kernel)
#include "sdp_lattice_kernel.h"        // sdp_look_lattice: DPSolver._box_lattice in double with one rounding
#if SDP_HAS_W
#include "sdp_mc_kernel.h"             // sdp_philox4x32_10, sdp_mc_uniform, sdp_mc_index, sdp_mc_visit
#endif

#define SDP_FLOOK_THREADS 256          // a workgroup: 4 waves of 64 / SDP_LANES states

typedef const __attribute__((address_space(4))) uint64_t sdp_cst_u64;
typedef const __attribute__((address_space(4))) double sdp_cst_f64;

// where a workgroup walks (sdp_family_montecarlo's mapping of members to XCDs on tiles of `tile_rows` rows): the same
// in every lane of the workgroup
struct SdpFamilyWalk {
    int64_t tiles, per_part, units, stride;
    int first, part;
};

SDP_DEV void sdp_flook_walk(int64_t B, int64_t tile_rows, int P, SdpFamilyWalk &w)
{
    w.tiles = (B + tile_rows - 1) / tile_rows;                        // per member
    const int xcd = blockIdx.x & 7;
    const int parts = P >= 8 ? 1 : 8 / max(P, 1);                     // XCDs per member
    w.first = xcd / parts;                                            // first member of this XCD ..
    w.part = xcd % parts;                                             // .. and which part of its tiles
    const int mine = w.first < P ? (P - w.first + 7) / 8 : 0;
    w.per_part = (w.tiles + parts - 1) / parts;
    w.units = (int64_t)mine * w.per_part;
    w.stride = gridDim.x >> 3;
}

// the lattice of the state x of member p: its box constants and control steps through the constant address space
SDP_DEV bool sdp_flook_box(const double *bprm, const double *steps, int64_t p, const sdp_real *x, double t, SdpBox &box)
{
    const double *row = (const double *)((sdp_cst_f64 *)bprm + p * SDP_NBOXPARAMS);
    double st[SDP_NU];
#pragma unroll
    for (int c = 0; c < SDP_NU; ++c) st[c] = ((sdp_cst_f64 *)steps)[p * SDP_NU + c];
    return sdp_look_lattice(x, st, box, [t, row](const double *xd, double *lo, double *hi) { sdp_model_box_at(xd, t, row, lo, hi); });
}

// sdp_look_backup on the member: every lane of the group ends with (J_opt, idx)
SDP_DEV void sdp_flook_backup(const SdpFamilyArgs &f, const SdpMember &m, const SdpGrid<sdp_real, SDP_D> &grid, const sdp_real *x,
                              sdp_real t, const SdpBox &box, bool run, int sub, sdp_real &best, int &ibest)
{
    best = INFINITY;
    ibest = INT_MAX;
    if (run) {
        for (int ci = sub; ci < box.total; ci += SDP_LANES) {
            sdp_real u[SDP_NU];
            sdp_controls_at(box, ci, u);
            const sdp_real jc = sdp_family_expected_cost(f, m, grid, x, u, t);
            if (ibest == INT_MAX || sdp_better_seq(jc, best)) { best = jc; ibest = ci; }
        }
    }
    sdp_seg_argmin<sdp_real, SDP_LANES>(best, ibest);
}

#if !defined(SDP_FLOOK_HELPERS_ONLY)
// (a lookahead unit over a horizon, sdp_family_lookahead_horizon_kernel.h, takes the walk, the box and the backup above and
// brings its own kernels and its own sdp_meta)
extern "C" __global__ void __launch_bounds__(SDP_FLOOK_THREADS) sdp_family_lookahead(SdpFamilyLookArgs a)
{
    constexpr int L = SDP_LANES;
    constexpr int NPW = 64 / L;                       // states per wavefront
    constexpr int64_t tile_rows = (int64_t)NPW * (SDP_FLOOK_THREADS / 64);
    const int lane = threadIdx.x & 63;
    const int sub = lane & (L - 1);
    const int slot = lane / L;
    const int wave = threadIdx.x >> 6;
    const sdp_real t = (sdp_real)a.f.t_k;

    SdpFamilyWalk w;
    sdp_flook_walk(a.B, tile_rows, a.f.n_active, w);
    for (int64_t unit = blockIdx.x >> 3; unit < w.units; unit += w.stride) {
        const int64_t tile = (int64_t)w.part * w.per_part + unit % w.per_part;
        if (tile >= w.tiles) continue;                // (workgroup-uniform)
        const int64_t p = w.first + 8 * (int)(unit / w.per_part);
        SdpMember m;
        SdpGrid<sdp_real, SDP_D> grid;
        sdp_family_member(a.f, p, m, grid);
        const sdp_real *__restrict__ xs = (const sdp_real *)a.x + p * (int64_t)SDP_D * a.B;

        const int64_t b = tile * tile_rows + (int64_t)wave * NPW + slot;
        const bool live = b < a.B;                    // groups beyond the member's last state are dead
        SdpBox box;
        sdp_real x[SDP_D];
        bool valid = false;
        if (live) {
#pragma unroll
            for (int k = 0; k < SDP_D; ++k) x[k] = xs[k * a.B + b];
            valid = sdp_flook_box(a.bprm, a.steps, p, x, a.f.t_k, box);
        }
        sdp_real best;
        int ibest;
        sdp_flook_backup(a.f, m, grid, x, t, box, live && valid, sub, best, ibest);
        if (live && sub == 0) {
            sdp_real u[SDP_NU];
            if (valid) sdp_controls_at(box, ibest, u);
#pragma unroll
            for (int c = 0; c < SDP_NU; ++c) ((sdp_real *)a.u)[(p * SDP_NU + c) * a.B + b] = valid ? u[c] : (sdp_real)NAN;
            ((sdp_real *)a.J)[p * a.B + b] = valid ? best : (sdp_real)NAN;
            a.idx[p * a.B + b] = valid ? ibest : -1;
        }
    }
}

#if SDP_HAS_W
extern "C" __global__ void __launch_bounds__(SDP_FLOOK_THREADS) sdp_family_montecarlo_lookahead(SdpFamilyLookMcArgs a)
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
    SDP_META_F_FAMILY | SDP_META_F_FAMILY_LOOKAHEAD, SDP_NBOXPARAMS, 0, SDP_FLOOK_THREADS, SDP_LANES, 0, 0, 0};
}
#endif  // !SDP_FLOOK_HELPERS_ONLY
