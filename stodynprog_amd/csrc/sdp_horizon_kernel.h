// sdp_horizon_kernel.h -- closed loops under a TIME-INDEXED policy (kernels `sdp_simulate_h` and
// `sdp_montecarlo_h`): the forward half of a finite-horizon problem.
//
// Included by sdp_sweep_kernel.h after `sdp_simulate` / `sdp_montecarlo` (and after their twins of
// sdp_multiw_kernel.h for several perturbation variables), so every generated unit carries them.  The loops are
// written ONCE, here, as device functions templated on a compile-time flag: the stationary entry points instantiate
// them with H = false (one policy, the unit's own constants), the two kernels below with H = true.  They are those
// two loops -- one lane per trajectory, the policy looked up by the lerp tree in double, then the traced model;
// the draw of stodynprog_amd/montecarlo.py, the occupancy combine and n_outside of sdp_mc_kernel.h -- with two
// things that change from step to step:
//
//     pol   [steps of the chunk][nu][S]   step k reads slice k - chunk_first  (what bellman_recursion returns,
//                                         control axis first; the host uploads a chunk of whole steps at a time)
//     prm   [steps of the call][SDP_NPARAMS]   the lifted constants of step k (a unit traced for one concrete time
//                                         index, `data[k]` models): sdp_model_cell_at reads row k where
//                                         sdp_model_cell reads the code object's one __constant__ row
//
// The step index is the same in every lane of a wave, so the row of `prm` and the base of the policy slice are
// wave-uniform: both are a kernel-argument pointer plus a multiple of the loop counter, the table read through the
// constant address space (scalar loads, like the weights of the sweep kernels).
// A launch runs the steps [step_begin, step_end) of the call; the state (and for Monte Carlo the sums) stay in
// device buffers between launches, so cutting a run at any step changes no bit.
#pragma once

#if defined(SDP_NW) && SDP_NW >= 2
typedef const sdp_real *sdp_w_arg;
#else
typedef sdp_real sdp_w_arg;
#endif

#if !defined(SDP_NPARAMS)
// a unit without lifted constants: its model is the same at every step but for the time index
SDP_DEV void sdp_model_cell_at(const sdp_real *x, const sdp_real *u, sdp_w_arg w, sdp_real t, const sdp_real *prm,
                               sdp_real *xn, sdp_real &g)
{
    (void)prm;
    sdp_model_cell(x, u, w, t, xn, g);
}
#define SDP_H_NPARAMS 0
#else
#define SDP_H_NPARAMS SDP_NPARAMS
#endif

// row `step` of the table of lifted constants (wave-uniform; null without a table)
SDP_DEV const sdp_real *sdp_h_prm_row(const void *prm, int64_t step)
{
    return (const sdp_real *)((const sdp_cst_real *)prm + step * SDP_H_NPARAMS);
}

// The per-trajectory loop of `sdp_simulate` (H = false, Args = SdpSimArgs: one policy, the unit's own constants, the
// whole run in one launch) and of `sdp_simulate_h` (H = true, Args = SdpSimHArgs).
template <bool H, typename Args>
SDP_DEV void sdp_simulate_loop(const Args &a)
{
    SdpGrid<sdp_real, SDP_D> grid;
    {
        const sdp_real *axes = (const sdp_real *)a.axes;
        sdp_real smin[SDP_D], smax[SDP_D];
#pragma unroll
        for (int k = 0; k < SDP_D; ++k) {
            smin[k] = axes[a.axis_off[k]];
            smax[k] = axes[a.axis_off[k] + a.orders[k] - 1];
        }
        sdp_make_grid<sdp_real, SDP_D>(grid, a.orders, smin, smax);
    }
    const sdp_real *__restrict__ pol = (const sdp_real *)a.pol;
    const sdp_real *__restrict__ wseq = (const sdp_real *)a.w;
    sdp_real *__restrict__ xo = (sdp_real *)a.x;         // (H: row step_begin is read, the later rows written)
    sdp_real *__restrict__ uo = (sdp_real *)a.u;
    sdp_real *__restrict__ go = (sdp_real *)a.g;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    // (the bound is the same in every lane of a wave: the step loop below then runs with wave-uniform addresses)
    const int64_t first = (int64_t)blockIdx.x * blockDim.x;
    for (int64_t base = first; base < a.B; base += stride) {
        const int64_t b = base + threadIdx.x;
        if (b >= a.B) continue;
        sdp_real x[SDP_D];
        int64_t step_begin, step_end;
        if constexpr (H) {
            step_begin = a.step_begin;
            step_end = a.step_end;
#pragma unroll
            for (int k = 0; k < SDP_D; ++k) x[k] = xo[(step_begin * SDP_D + k) * a.B + b];
        } else {
            step_begin = 0;
            step_end = a.T;
#pragma unroll
            for (int k = 0; k < SDP_D; ++k) {
                x[k] = ((const sdp_real *)a.x0)[k * a.B + b];
                xo[k * a.B + b] = x[k];
            }
        }
        for (int64_t step = step_begin; step < step_end; ++step) {
            const sdp_real *__restrict__ pk = pol;
            if constexpr (H) pk = pol + (step - a.chunk_first) * (int64_t)SDP_NU * a.S;
            sdp_real u[SDP_NU], xn[SDP_D], g;
#pragma unroll
            for (int c = 0; c < SDP_NU; ++c)
                u[c] = sdp_interp_point<sdp_real, SDP_D, double>(pk + c * a.S, grid, x);
#if defined(SDP_NW) && SDP_NW >= 2
            sdp_real w[SDP_NW];
#pragma unroll
            for (int i = 0; i < SDP_NW; ++i) w[i] = wseq[(step * SDP_NW + i) * a.B + b];
#else
            const sdp_real w = wseq ? wseq[step * a.B + b] : (sdp_real)0;
#endif
            if constexpr (H) sdp_model_cell_at(x, u, w, (sdp_real)(a.t0 + (double)step), sdp_h_prm_row(a.prm, step), xn, g);
            else sdp_model_cell(x, u, w, (sdp_real)(a.t0 + (double)step), xn, g);
#pragma unroll
            for (int c = 0; c < SDP_NU; ++c) uo[(step * SDP_NU + c) * a.B + b] = u[c];
            if (go) go[step * a.B + b] = g;
#pragma unroll
            for (int k = 0; k < SDP_D; ++k) {
                x[k] = xn[k];
                xo[((step + 1) * SDP_D + k) * a.B + b] = xn[k];
            }
        }
    }
}

extern "C" __global__ void __launch_bounds__(64) sdp_simulate_h(SdpSimHArgs a)
{
    sdp_simulate_loop<true>(a);
}

#if SDP_HAS_W
// The per-trajectory loop of `sdp_montecarlo` (H = false, Args = SdpMcArgs) and of `sdp_montecarlo_h` (H = true, Args =
// SdpMcHArgs): the draw table in LDS, the single-locate policy lookup, the occupancy combine and n_outside.
template <bool H, typename Args>
SDP_DEV void sdp_montecarlo_loop(const Args &a)
{
#if defined(SDP_NW) && SDP_NW >= 2
    constexpr int NW = SDP_NW;
#else
    constexpr int NW = 1;
#endif
    extern __shared__ double sdp_mc_lds[];                 // cum[W-1] (doubles), then law_grid[NW][W] (reals)
    const int W = a.n_law;
    double *cum = sdp_mc_lds;
    sdp_real *wtab = (sdp_real *)(sdp_mc_lds + (W - 1));
    for (int i = threadIdx.x; i < W - 1; i += blockDim.x) cum[i] = a.cum[i];
    for (int i = threadIdx.x; i < NW * W; i += blockDim.x) wtab[i] = ((const sdp_real *)a.law_grid)[i];
    __syncthreads();

    SdpGrid<sdp_real, SDP_D> grid;
    sdp_real smin[SDP_D], smax[SDP_D];
    {
        const sdp_real *axes = (const sdp_real *)a.axes;
#pragma unroll
        for (int k = 0; k < SDP_D; ++k) {
            smin[k] = axes[a.axis_off[k]];
            smax[k] = axes[a.axis_off[k] + a.orders[k] - 1];
        }
        sdp_make_grid<sdp_real, SDP_D>(grid, a.orders, smin, smax);
    }
    const sdp_real *__restrict__ pol = (const sdp_real *)a.pol;
    sdp_real *xs = (sdp_real *)a.x;
    sdp_real *accs = (sdp_real *)a.acc;
    const unsigned k0 = (unsigned)a.seed, k1 = (unsigned)(a.seed >> 32);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    // the loop bound is the same in every lane of a wave (the ballots and shuffles of the occupancy need them all)
    const int64_t first = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63);
    for (int64_t base = first; base < a.B; base += stride) {
        const int64_t b = base + (threadIdx.x & 63);
        const bool live = b < a.B;
        // An idle lane of the last wave runs along (the ballots and shuffles of the occupancy need every lane) on a copy
        // of the last row's state and stores nothing.  Whatever it reads is harmless -- its results are dropped, its
        // gathers are clamped to the grid like everyone's and its visits are not counted -- so nothing here depends on
        // the order of that read and the live lane's store at the end (xs and accs are not __restrict__ for that reason).
        const int64_t row = live ? b : a.B - 1;
        const unsigned long long id = a.traj_offset + (unsigned long long)row;
        sdp_real x[SDP_D];
#pragma unroll
        for (int k = 0; k < SDP_D; ++k) x[k] = xs[k * a.B + row];
        sdp_real acc = accs[row];
        int n_out = 0;                                     // (of this launch: fewer than 2^31 steps)
        for (int64_t step = a.step_begin; step < a.step_end; ++step) {
            const sdp_real *__restrict__ pk = pol;
            if constexpr (H) pk = pol + (step - a.chunk_first) * (int64_t)SDP_NU * a.S;
            const bool counted = step >= a.n_burn;
            SdpCell<sdp_real, SDP_D, double> cell;
            bool outside = false;
#pragma unroll
            for (int k = 0; k < SDP_D; ++k) {
                sdp_locate_axis<sdp_real, SDP_D, double>(grid, k, x[k], cell);
                outside = outside || !(x[k] >= smin[k] && x[k] <= smax[k]);
            }
            n_out += (counted && outside) ? 1 : 0;
            if (a.occupancy) {
                int node = 0;
#pragma unroll
                for (int k = 0; k < SDP_D; ++k) {
                    const int q = cell.off[k] + ((cell.lam[k] >= (sdp_real)0.5) ? grid.M[k] : 0);     // M[k] * (cell + 1)
                    node += max(min(q, grid.M[k] * (a.orders[k] - 1)), 0);
                }
                sdp_mc_visit(a.occupancy, node, counted && live);
            }
            sdp_real u[SDP_NU], xn[SDP_D], g;
#pragma unroll
            for (int c = 0; c < SDP_NU; ++c)               // sdp_interp_point<sdp_real, SDP_D, double>, the cell located once
                u[c] = (sdp_real)SdpLerp<sdp_real, SDP_D, double, 0, false>::eval(pk + c * a.S, grid, cell, 0);
            const SdpPhilox r = sdp_philox4x32_10((unsigned)id, (unsigned)(id >> 32), (unsigned)step,
                                                  (unsigned)((unsigned long long)step >> 32), k0, k1);
            const int j = sdp_mc_index(cum, W - 1, sdp_mc_uniform(r));     // 0 <= j <= W - 1
#if defined(SDP_NW) && SDP_NW >= 2
            sdp_real w[SDP_NW];
#pragma unroll
            for (int i = 0; i < SDP_NW; ++i) w[i] = wtab[i * W + j];
#else
            const sdp_real w = wtab[j];
#endif
            if constexpr (H) sdp_model_cell_at(x, u, w, (sdp_real)(a.t0 + (double)step), sdp_h_prm_row(a.prm, step), xn, g);
            else sdp_model_cell(x, u, w, (sdp_real)(a.t0 + (double)step), xn, g);
            if (counted) acc = acc + g;
#pragma unroll
            for (int k = 0; k < SDP_D; ++k) x[k] = xn[k];
        }
        if (live) {
#pragma unroll
            for (int k = 0; k < SDP_D; ++k) xs[k * a.B + b] = x[k];
            accs[b] = acc;
            a.n_outside[b] += n_out;
        }
    }
}

extern "C" __global__ void __launch_bounds__(SDP_MC_THREADS) sdp_montecarlo_h(SdpMcHArgs a)
{
    sdp_montecarlo_loop<true>(a);
}
#endif  // SDP_HAS_W
