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

#if !defined(SDP_MC_HELPERS_ONLY)
// (a family Monte Carlo unit, sdp_family_mc_kernel.h, takes the draw helpers above and brings its own kernel)
extern "C" __global__ void __launch_bounds__(SDP_MC_THREADS) sdp_montecarlo(SdpMcArgs a)
{
    sdp_montecarlo_loop<false>(a);     // (sdp_horizon_kernel.h)
}
#endif
