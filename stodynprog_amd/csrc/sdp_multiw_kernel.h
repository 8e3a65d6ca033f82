// sdp_multiw_kernel.h -- the node-order kernel family for systems with SEVERAL perturbation variables.
//
// Included by sdp_sweep_kernel.h (after its helpers: SdpBox, sdp_controls_at, sdp_node_coords,
// sdp_grid_from_args) in place of its own kernels when the generated unit defines
//   SDP_NW        number of perturbation variables m, 2..4
// and a model entry that takes them as a vector:
//   sdp_model_cell(x, u, const sdp_real *w, t, xn, g)      w[SDP_NW]
//
// The definition (stodynprog_amd/perturb.py): the m independent variables are flattened by the host
// into ONE law of W = W_1 .. W_m points, C order, the last variable fastest --
//   wtab[i][j] = g_i[j_i]            SdpSweepArgs.wgrid, [SDP_NW][W]
//   P[j]       = (p_1[j_1] p_2[j_2]) p_3[j_3] ..            SdpSweepArgs.proba, [W]
// and the backup is the sequential sum over that flat law, as for one variable:
//   acc = acc + (g(x, u, wtab[.][j]) + J_next(f(x, u, wtab[.][j]))) * P[j],     j ascending.
//
// Kernels, argument blocks and `sdp_meta` are those of sdp_sweep_kernel.h: `sdp_sweep` keeps the direct
// kernel's mapping (SDP_LANES lanes of a node stride its control lattice, the j loop runs in registers,
// sdp_seg_argmin, XCD-contiguous tile walk, sdp_store_J); `sdp_evalpol`, `sdp_simulate` and
// `sdp_montecarlo` are the one-variable kernels with a vector w.  j is the same in every lane of a
// wave, so wtab and P are read through the constant address space: m + 1 scalar loads per point, whose
// results reach the model as scalar operands -- no LDS, no barrier, no vector register per table entry.
// The model is evaluated per cell; nothing is hoisted across the variables.
//
// Layouts with a perturbation in them: SdpSimArgs.w is [T][SDP_NW][B]; SdpMcArgs.law_grid is
// [SDP_NW][n_law], staged behind `cum` in dynamic LDS (the host refuses a law that does not fit).
#pragma once

#if SDP_NW < 2 || SDP_NW > 4
#error "sdp_multiw_kernel.h: SDP_NW must be 2, 3 or 4"
#endif
#if !SDP_HAS_W
#error "sdp_multiw_kernel.h: a unit with perturbation variables defines SDP_HAS_W 1"
#endif

// expected cost of one (node, control) on the flat law
template <bool SHIFT = false>
SDP_DEV sdp_real sdp_expected_cost_mw(const SdpSweepArgs &a, const SdpGrid<sdp_real, SDP_D> &grid,
                                      const sdp_real *__restrict__ V, const sdp_real *x,
                                      const sdp_real *u, sdp_real t)
{
    const sdp_cst_real *wtab = (const sdp_cst_real *)a.wgrid;
    const sdp_cst_real *proba = (const sdp_cst_real *)a.proba;
    const int W = a.W;
    sdp_real acc = (sdp_real)0;
    for (int j = 0; j < W; ++j) {
        sdp_real w[SDP_NW], xn[SDP_D], g;
#pragma unroll
        for (int i = 0; i < SDP_NW; ++i) w[i] = wtab[i * W + j];
        sdp_model_cell(x, u, w, t, xn, g);
        const sdp_real jc = g + sdp_interp_point<sdp_real, SDP_D, sdp_real, SHIFT>(V, grid, xn);
        acc = acc + jc * proba[j];
    }
    return acc;
}

extern "C" __global__ void __launch_bounds__(256) sdp_sweep(SdpSweepArgs a)
{
    constexpr int L = SDP_LANES;
    constexpr int NPW = 64 / L;                       // nodes per wavefront
    const int lane = threadIdx.x & 63;
    const int sub = lane & (L - 1);
    const int slot = lane / L;
    const int wave = threadIdx.x >> 6;
    const int waves = blockDim.x >> 6;
    const int64_t tile_nodes = (int64_t)NPW * waves;  // nodes per workgroup step

    const sdp_real *__restrict__ V = (const sdp_real *)a.V;
    SdpGrid<sdp_real, SDP_D> grid;
    sdp_grid_from_args(a, grid);
    const sdp_real t = (sdp_real)a.t_k;

    // XCD-aware walk, as in the direct kernel: XCD x takes the x-th contiguous eighth of the tiles
    const int64_t n_nodes = a.node_end - a.node_begin;
    const int64_t n_tiles = (n_nodes + tile_nodes - 1) / tile_nodes;
    const int xcd = blockIdx.x & 7;
    const int64_t per_xcd = (n_tiles + 7) / 8;
    const int64_t t_end = min((int64_t)(xcd + 1) * per_xcd, n_tiles);
    const int64_t stride = gridDim.x >> 3;

    for (int64_t tile = (int64_t)xcd * per_xcd + (blockIdx.x >> 3); tile < t_end; tile += stride) {
        const int64_t node = a.node_begin + tile * tile_nodes + (int64_t)wave * NPW + slot;
        const bool live = node < a.node_end;
        sdp_real best = INFINITY;
        int ibest = INT_MAX;
        SdpBox box;
        sdp_real x[SDP_D];
        if (live) {
            sdp_node_coords(a, node, x);
            sdp_load_box(a, node, box);
            for (int ci = sub; ci < box.total; ci += L) {
                sdp_real u[SDP_NU];
                sdp_controls_at(box, ci, u);
                const sdp_real jc = sdp_expected_cost_mw(a, grid, V, x, u, t);
                if (ibest == INT_MAX || sdp_better_seq(jc, best)) { best = jc; ibest = ci; }
            }
        }
        sdp_seg_argmin<sdp_real, L>(best, ibest);
        if (live && sub == 0) {
            sdp_store_J<sdp_real>(a, node, 0, best);
            if (a.idx) a.idx[node] = ibest;
            if (a.pol) {
                sdp_real u[SDP_NU];
                sdp_controls_at(box, ibest, u);
#pragma unroll
                for (int c = 0; c < SDP_NU; ++c) ((sdp_real *)a.pol)[node * SDP_NU + c] = u[c];
            }
        }
    }
}

extern "C" __global__ void __launch_bounds__(256) sdp_evalpol(SdpSweepArgs a)
{
    const sdp_real *__restrict__ V = (const sdp_real *)a.V;
    SdpGrid<sdp_real, SDP_D> grid;
    sdp_grid_from_args(a, grid);
    const sdp_real t = (sdp_real)a.t_k;
    // fused relative-DP shift of the previous step (see SdpLerp<.., SHIFT>)
    grid.shift = a.shift_index >= 0 ? V[a.shift_index] : (sdp_real)0;
    if (a.ref_out && blockIdx.x == 0 && threadIdx.x == 0) *a.ref_out = (double)grid.shift;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t node = a.node_begin + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         node < a.node_end; node += stride) {
        sdp_real x[SDP_D], u[SDP_NU];
        sdp_node_coords(a, node, x);
#pragma unroll
        for (int c = 0; c < SDP_NU; ++c) u[c] = ((const sdp_real *)a.pol_in)[node * SDP_NU + c];
        sdp_store_J<sdp_real>(a, node, 0, sdp_expected_cost_mw<true>(a, grid, V, x, u, t));
    }
}

// B closed-loop trajectories of T steps, one lane each (sdp_simulate of sdp_sweep_kernel.h); the
// perturbation of step k and trajectory b is the vector w[k][.][b]
extern "C" __global__ void __launch_bounds__(64) sdp_simulate(SdpSimArgs a)
{
    sdp_simulate_loop<false>(a);       // (sdp_horizon_kernel.h: w[k][.][b] with SDP_NW defined)
}

// ---- Monte Carlo policy evaluation: sdp_montecarlo of sdp_mc_kernel.h on the flat law ----
// ONE Philox call and one uniform per (trajectory, step), exactly the draw of stodynprog_amd/montecarlo.py;
// the index j it gives selects the column j of law_grid[SDP_NW][n_law].  The draw helpers below restate
// those of sdp_mc_kernel.h, which defines its kernel next to them for the scalar-w model entry and is
// therefore not included by a unit of several variables.
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
    unsigned long long todo = __ballot(count);
    const int lane = threadIdx.x & 63;
    while (todo) {                                                     // wave-uniform: `todo` is a ballot
        const int leader = __ffsll((long long)todo) - 1;
        const int ln = __shfl(node, leader, 64);
        const unsigned long long same = __ballot(count && node == ln) & todo;
        if (lane == leader) atomicAdd(occ + ln, (unsigned long long)__popcll(same));
        todo &= ~same;
    }
}

extern "C" __global__ void __launch_bounds__(SDP_MC_THREADS) sdp_montecarlo(SdpMcArgs a)
{
    sdp_montecarlo_loop<false>(a);     // (sdp_horizon_kernel.h: column j of law_grid[SDP_NW][n_law])
}

// what this code object was generated for (sdp_kernel_args.h, SDP_META_*); word 15: perturbation variables
extern "C" {
__constant__ int32_t sdp_meta[SDP_META_WORDS] = {
    SDP_META_MAGIC, (int32_t)sizeof(sdp_real), SDP_D, SDP_NU, SDP_HAS_W, 0, 0, 1,
    SDP_META_PEER_FLAG, 0, 0, 256, 0, 0, 0,
    SDP_NW};
}
