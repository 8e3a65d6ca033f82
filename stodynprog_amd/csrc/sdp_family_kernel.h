// sdp_family_kernel.h -- one Bellman backup of a FAMILY of same-shaped problems (kernel `sdp_family_sweep`).
//
// Included LAST by a generated family unit (codegen.family_unit), after the direct prologue with
//   SDP_FAMILY 1, SDP_REAL, SDP_D, SDP_NU, SDP_HAS_W, SDP_LANES, SDP_NPARAMS
//   sdp_model_cell_at(x, u, w, t, prm, xn, g)   the traced dyn/cost with its constants read from a row `prm`
//
// A parameter study solves P problems that differ in constants only: the members share the grid's shape, the
// number of controls and of perturbation points and the structure of the traced model, and each has its own
// constants, grid ends, law and box table (SdpFamilyArgs: every array member-major).  The kernel is the backup
// of `sdp_sweep` (sdp_sweep_kernel.h), restated with a member index: per (member, node) the member's node
// coordinates and box row, SDP_LANES lanes over the control lattice, per lane the perturbation loop in w order
// with the same sequential `acc = acc + jc * proba[wi]`, then the first-occurrence argmin.  Member p of the result
// has the bits of `sdp_sweep` on problem p alone.
//
// Work decomposition.  The unit of work is a tile of (64 / SDP_LANES) x waves nodes of ONE member, so a wavefront
// never spans two members: the member index, and with it the row of constants, the grid ends, the law and the
// base of the box table, are wave-uniform and read through the constant address space (scalar loads feeding VALU
// operands instead of 64 identical vector loads).  The grid is bounded and its workgroups stride over the tiles.
// Workgroups b and b + 8 share an XCD (round-robin dispatch), and a member's tiles stay on one XCD, whose L2 then
// holds the member's value array for the whole launch: with 8 listed members or more, XCD x takes the listed
// members x, x + 8, ..; with fewer, every member is given 8 / n_active XCDs, each a contiguous part of its tiles
// (the walk of `sdp_sweep`), and the XCDs left over stay idle.
#pragma once
#include "sdp_sweep_kernel.h"      // (SDP_FAMILY: SdpBox, sdp_control_value, sdp_controls_at and the typedefs only)

#if !defined(SDP_NPARAMS)
// a model without a real constant: nothing to read from the row
#define SDP_NPARAMS 0
SDP_DEV void sdp_model_cell_at(const sdp_real *x, const sdp_real *u, sdp_real w, sdp_real t, const sdp_real *prm,
                               sdp_real *xn, sdp_real &g)
{
    (void)prm;
    sdp_model_cell(x, u, w, t, xn, g);
}
#endif

typedef const __attribute__((address_space(4))) int32_t sdp_cst_i32;

// what is the same for every node of a member (wave-uniform)
struct SdpMember {
    const sdp_real *__restrict__ V;        // [S]
    const sdp_real *axes;                  // [n_axes]
    sdp_cst_real *wgrid, *proba;           // [W]
    const sdp_real *prm;                   // [SDP_NPARAMS]
    const sdp_real *box_lo, *box_hi;       // [nu] or [nu][S]
    const int32_t *box_n;
};

SDP_DEV void sdp_family_member(const SdpFamilyArgs &a, int64_t p, SdpMember &m, SdpGrid<sdp_real, SDP_D> &grid)
{
    const int64_t nbox = (int64_t)SDP_NU * (a.box_per_node ? a.S : 1);
    m.V = (const sdp_real *)a.V + p * a.S;
    m.axes = (const sdp_real *)a.axes + p * a.n_axes;
    m.wgrid = (sdp_cst_real *)a.wgrid + p * a.W;
    m.proba = (sdp_cst_real *)a.proba + p * a.W;
    m.prm = (const sdp_real *)((sdp_cst_real *)a.prm + p * SDP_NPARAMS);
    m.box_lo = (const sdp_real *)a.box_lo + p * nbox;
    m.box_hi = (const sdp_real *)a.box_hi + p * nbox;
    m.box_n = a.box_n + p * nbox;
    // (sdp_grid_from_args on the member's axes)
    sdp_cst_real *axes = (sdp_cst_real *)a.axes + p * a.n_axes;
    sdp_real smin[SDP_D], smax[SDP_D];
#pragma unroll
    for (int k = 0; k < SDP_D; ++k) {
        smin[k] = axes[a.axis_off[k]];                       // x[0]   stodynprog.py:263
        smax[k] = axes[a.axis_off[k] + a.orders[k] - 1];     // x[-1]  stodynprog.py:264
    }
    sdp_make_grid<sdp_real, SDP_D>(grid, a.orders, smin, smax);
}

// sdp_load_box on the member's table
SDP_DEV void sdp_family_load_box(const SdpFamilyArgs &a, const SdpMember &m, int64_t node, SdpBox &b)
{
    b.total = 1;
#pragma unroll
    for (int c = 0; c < SDP_NU; ++c) {
        const int64_t at = a.box_per_node ? (int64_t)c * a.S + node : (int64_t)c;
        b.lo[c] = m.box_lo[at];
        b.hi[c] = m.box_hi[at];
        b.n[c] = m.box_n[at];
        b.delta[c] = b.hi[c] - b.lo[c];
        // numpy.linspace: step = delta / div with div = num - 1
        b.step[c] = (b.n[c] > 1) ? b.delta[c] / (sdp_real)(b.n[c] - 1) : (sdp_real)0;
        b.total *= b.n[c];
    }
}

// sdp_node_coords on the member's axes
SDP_DEV void sdp_family_node_coords(const SdpFamilyArgs &a, const SdpMember &m, int64_t node, sdp_real *x)
{
    int64_t r = node;
#pragma unroll
    for (int k = SDP_D - 1; k >= 0; --k) {
        const int i = (int)(r % a.orders[k]);
        r /= a.orders[k];
        x[k] = m.axes[a.axis_off[k] + i];
    }
}

// sdp_expected_cost with the member's constants, law and value array: sum_w p_w * (g + J_next(f))
SDP_DEV sdp_real sdp_family_expected_cost(const SdpFamilyArgs &a, const SdpMember &m, const SdpGrid<sdp_real, SDP_D> &grid,
                                          const sdp_real *x, const sdp_real *u, sdp_real t)
{
    sdp_real xn[SDP_D], g;
#if SDP_HAS_W
    sdp_real acc = (sdp_real)0;
    for (int wi = 0; wi < a.W; ++wi) {
        sdp_model_cell_at(x, u, m.wgrid[wi], t, m.prm, xn, g);
        const sdp_real jc = g + sdp_interp_point<sdp_real, SDP_D, sdp_real>(m.V, grid, xn);       // stodynprog.py:677
        acc = acc + jc * m.proba[wi];                                                             // stodynprog.py:681
    }
    return acc;
#else
    sdp_model_cell_at(x, u, (sdp_real)0, t, m.prm, xn, g);
    return g + sdp_interp_point<sdp_real, SDP_D, sdp_real>(m.V, grid, xn);                        // stodynprog.py:679-680
#endif
}

#if !defined(SDP_FAMILY_POLICY) && !defined(SDP_FAMILY_MC) && !defined(SDP_FAMILY_LOOKAHEAD) && !defined(SDP_FAMILY_HORIZON) \
    && !defined(SDP_FAMILY_TRANS)
// (an evaluation unit, sdp_family_policy_kernel.h, takes SdpMember and the helpers above and brings its own kernels; so
// do a Monte Carlo unit, sdp_family_mc_kernel.h, a lookahead unit, sdp_family_lookahead_kernel.h, a horizon unit,
// sdp_family_horizon_kernel.h, and a transition unit, sdp_family_trans_kernel.h)
extern "C" __global__ void __launch_bounds__(256) sdp_family_sweep(SdpFamilyArgs a)
{
    constexpr int L = SDP_LANES;
    constexpr int NPW = 64 / L;                       // nodes per wavefront
    const int lane = threadIdx.x & 63;
    const int sub = lane & (L - 1);
    const int slot = lane / L;
    const int wave = threadIdx.x >> 6;
    const int waves = blockDim.x >> 6;
    const int64_t tile_nodes = (int64_t)NPW * waves;  // nodes per workgroup step
    const sdp_real t = (sdp_real)a.t_k;
    sdp_cst_i32 *members = (sdp_cst_i32 *)a.members;

    // members -> XCDs (see the head of this file); everything here is the same in every lane of the workgroup
    const int64_t tiles = (a.S + tile_nodes - 1) / tile_nodes;        // per member
    const int xcd = blockIdx.x & 7;
    const int parts = a.n_active >= 8 ? 1 : 8 / max(a.n_active, 1);   // XCDs per member
    const int first = xcd / parts;                                    // first listed member of this XCD ..
    const int part = xcd % parts;                                     // .. and which part of its tiles
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

        const int64_t node = tile * tile_nodes + (int64_t)wave * NPW + slot;
        const bool live = node < a.S;                 // lanes beyond the member's last node are dead
        sdp_real best = INFINITY;
        int ibest = INT_MAX;
        SdpBox box;
        sdp_real x[SDP_D];
        if (live) {
            sdp_family_node_coords(a, m, node, x);
            sdp_family_load_box(a, m, node, box);
            for (int ci = sub; ci < box.total; ci += L) {
                sdp_real u[SDP_NU];
                sdp_controls_at(box, ci, u);
                const sdp_real jc = sdp_family_expected_cost(a, m, grid, x, u, t);
                if (ibest == INT_MAX || sdp_better_seq(jc, best)) { best = jc; ibest = ci; }
            }
        }
        sdp_seg_argmin<sdp_real, L>(best, ibest);
        if (live && sub == 0) {
            const int64_t at = p * a.S + node;
            ((sdp_real *)a.J)[at] = best;
            if (a.idx) a.idx[at] = ibest;
            if (a.pol) {
                sdp_real u[SDP_NU];
                sdp_controls_at(box, ibest, u);
#pragma unroll
                for (int c = 0; c < SDP_NU; ++c) ((sdp_real *)a.pol)[at * SDP_NU + c] = u[c];
            }
        }
    }
}

// what this code object was generated for, filled in like a node-order unit (sdp_kernel_args.h, SDP_META_*)
extern "C" {
__constant__ int32_t sdp_meta[SDP_META_WORDS] = {
    SDP_META_MAGIC, (int32_t)sizeof(sdp_real), SDP_D, SDP_NU, SDP_HAS_W, 0, 0, 1,
    SDP_META_F_FAMILY, 0, 0, 256, 0, 0, 0, 0};
}
#endif  // SDP_FAMILY_POLICY
