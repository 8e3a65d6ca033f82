// sdp_lattice_kernel.h -- the control lattice of a state from a box function, on the device: ONE statement of
// DPSolver._box_lattice for every kernel that makes its lattice itself.
//
// Included by sdp_lookahead_kernel.h (the unit's `sdp_model_box`) and by sdp_family_lookahead_kernel.h (the unit's
// `sdp_model_box_at` on a member's row of constants), after SdpBox (sdp_sweep_kernel.h) and with sdp_real, SDP_D and
// SDP_NU defined.  The rule, in double whatever the unit's reals (a 4-byte state is widened first, as the host's
// scalar calls do): n_interv = (hi - lo) / step; n_interv < 0.1: one point at (lo + hi) / 2; else
// n = ceil(n_interv) + 1; then ONE rounding of lo and hi to sdp_real.  A box with a non-finite end, or a lattice whose
// total reaches 2^31, is not valid: every n is 0 and the caller writes NaN, NaN, -1.
#pragma once

// what sdp_load_box derives from (lo, hi, n)
SDP_DEV void sdp_look_finish_box(SdpBox &b)
{
    b.total = 1;
#pragma unroll
    for (int c = 0; c < SDP_NU; ++c) {
        b.delta[c] = b.hi[c] - b.lo[c];
        b.step[c] = (b.n[c] > 1) ? b.delta[c] / (sdp_real)(b.n[c] - 1) : (sdp_real)0;
        b.total *= b.n[c];
    }
}

// the lattice of the state x; `ends(xd, lo, hi)` is the box function at the widened state.  false: the state has none
template <typename Ends>
SDP_DEV bool sdp_look_lattice(const sdp_real *x, const double *steps, SdpBox &box, Ends ends)
{
    double xd[SDP_D], lo[SDP_NU], hi[SDP_NU];
#pragma unroll
    for (int k = 0; k < SDP_D; ++k) xd[k] = (double)x[k];
    ends(xd, lo, hi);
    bool ok = true;
    double total = 1.0;
#pragma unroll
    for (int c = 0; c < SDP_NU; ++c) {
        const double n_interv = (hi[c] - lo[c]) / steps[c];
        const bool single = n_interv < 0.1;
        const double npts = single ? 1.0 : ceil(n_interv) + 1.0;
        ok = ok && fabs(lo[c]) < (double)INFINITY && fabs(hi[c]) < (double)INFINITY && npts < 2147483648.0;
        const double mid = (lo[c] + hi[c]) / 2;
        box.lo[c] = (sdp_real)(single ? mid : lo[c]);
        box.hi[c] = (sdp_real)(single ? mid : hi[c]);
        box.n[c] = ok ? (int)npts : 0;
        total *= npts;
    }
    ok = ok && total < 2147483648.0;
    if (!ok) {
#pragma unroll
        for (int c = 0; c < SDP_NU; ++c) box.n[c] = 0;
    }
    sdp_look_finish_box(box);
    return ok;
}
