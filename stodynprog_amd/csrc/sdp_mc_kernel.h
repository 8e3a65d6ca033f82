// sdp_mc_kernel.h -- Monte Carlo policy evaluation on the device (kernel `sdp_montecarlo`).
//
// Included by sdp_sweep_kernel.h next to `sdp_simulate`, so every generated unit of a stochastic
// system carries it.  B closed-loop trajectories, one lane each; per step exactly what
// sdp_simulate does -- the policy looked up by multilinear interpolation (lerp tree in double),
// then the traced model -- but the perturbation is DRAWN here and nothing is stored per step:
//
//     (r0, r1, ., .) = Philox4x32-10( counter = (id_lo, id_hi, step_lo, step_hi),
//                                     key = (seed_lo, seed_hi) )        id = traj_offset + row
//     u = ((r0 >> 5) * 2^26 + (r1 >> 6)) * 2^-53                        a double in [0, 1)
//     j = #{ i in [0, W-2] : u >= cum[i] }                              cum: float64 running sum (host)
//     w = law_grid[j]
//
// (the definition in numpy: stodynprog_amd/montecarlo.py).  A draw depends on (seed, id, step)
// alone: the grid size, the batch and how a run is cut into launches cannot change a bit.
// Per trajectory, over the steps k >= n_burn: acc = acc + g_k (one rounded add per step, in the
// problem's reals, k ascending) and the number of steps whose x_k lies outside the state grid (or
// is NaN).  The state, acc and the counter live in device buffers between the launches of one run.
// Occupancy (optional): one 64-bit count per grid node, incremented at the node nearest to x_k,
// from the cell and weights the policy lookup has computed anyway; the lanes of a wave that hit
// the same node are combined into one atomic (trajectories cluster: a stock sitting at its floor).
#pragma once

#ifndef SDP_MC_COMBINE
#define SDP_MC_COMBINE 1         // 0: one atomic per lane (what the in-wave combine is measured against)
#endif
#define SDP_MC_THREADS 256
#define SDP_MC_COUNT_MAX 64      // up to this many law points the index is a branch-free count

struct SdpPhilox { unsigned r0, r1; };

// Philox4x32-10 (Salmon et al., Random123): output words 0 and 1
SDP_DEV SdpPhilox sdp_philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return {c0, c1};
}

SDP_DEV double sdp_mc_uniform(SdpPhilox r)
{
    // 27 + 26 bits: every step is exact in a double
    return ((double)(r.r0 >> 5) * 67108864.0 + (double)(r.r1 >> 6)) * (1.0 / 9007199254740992.0);
}

// np.searchsorted(cum[:n], u, 'right'): the number of entries <= u (cum ascending, wave-uniform n)
SDP_DEV int sdp_mc_index(const double *cum, int n, double u)
{
    if (n <= SDP_MC_COUNT_MAX - 1) {
        int j = 0;
        for (int i = 0; i < n; ++i) j += (u >= cum[i]) ? 1 : 0;        // (the same LDS word in every lane: a broadcast)
        return j;
    }
    int lo = 0, hi = n;                                                // entries below lo are <= u, entries from hi on are > u
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (u >= cum[mid]) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// one more visit of grid node `node` by every lane with `count` set; all lanes of the wave call this
SDP_DEV void sdp_mc_visit(unsigned long long *occ, int node, bool count)
{
#if SDP_MC_COMBINE
    unsigned long long todo = __ballot(count);
    const int lane = threadIdx.x & 63;
    while (todo) {                                                     // wave-uniform: `todo` is a ballot
        const int leader = __ffsll((long long)todo) - 1;
        const int ln = __shfl(node, leader, 64);
        const unsigned long long same = __ballot(count && node == ln) & todo;
        if (lane == leader) atomicAdd(occ + ln, (unsigned long long)__popcll(same));
        todo &= ~same;
    }
#else
    if (count) atomicAdd(occ + node, 1ull);
#endif
}

extern "C" __global__ void __launch_bounds__(SDP_MC_THREADS) sdp_montecarlo(SdpMcArgs a)
{
    extern __shared__ double sdp_mc_lds[];                 // cum[W-1] (doubles), then law_grid[W] (reals)
    const int W = a.n_law;
    double *cum = sdp_mc_lds;
    sdp_real *wgrid = (sdp_real *)(sdp_mc_lds + (W - 1));
    for (int i = threadIdx.x; i < W - 1; i += blockDim.x) cum[i] = a.cum[i];
    for (int i = threadIdx.x; i < W; i += blockDim.x) wgrid[i] = ((const sdp_real *)a.law_grid)[i];
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
                u[c] = (sdp_real)SdpLerp<sdp_real, SDP_D, double, 0, false>::eval(pol + c * a.S, grid, cell, 0);
            const SdpPhilox r = sdp_philox4x32_10((unsigned)id, (unsigned)(id >> 32), (unsigned)step,
                                                  (unsigned)((unsigned long long)step >> 32), k0, k1);
            const sdp_real w = wgrid[sdp_mc_index(cum, W - 1, sdp_mc_uniform(r))];
            sdp_model_cell(x, u, w, (sdp_real)(a.t0 + (double)step), xn, g);
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
