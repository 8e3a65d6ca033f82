/*
 * sdp_hip.h -- C ABI of libsdp_hip.so, the MI355X (gfx950) implementation of
 * the stodynprog value-iteration hot path.
 *
 * The reference (pierre-haessig/stodynprog) is a Python library whose only
 * native boundary is one Cython function; this header declares the C entry
 * points a binding (ctypes, cffi, Cython `cdef extern`) uses instead.  Each
 * entry cites the reference interface it replaces (paths relative to the
 * reference checkout).  All functions return 0 on success and a negative
 * SDP_E* code on failure; sdp_last_error() gives the message of the last
 * failure on the calling thread.  No C++ exceptions cross this boundary.
 * Host pointers are owned by the caller for the duration of a call; device
 * memory is owned by the library and tied to the handle that allocated it.
 */
#ifndef SDP_HIP_H
#define SDP_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDP_OK          0
#define SDP_EINVAL     -1   /* bad argument (maps to ValueError / AssertionError) */
#define SDP_EDIM       -2   /* state dimension outside 1..4 (multilinear_cython.pyx:46-47 raises Exception) */
#define SDP_EHIP       -3   /* HIP runtime error (RuntimeError) */
#define SDP_ENOMEM     -4   /* device allocation failed (MemoryError) */
#define SDP_ECOMM      -5   /* RCCL error or librccl not loadable */
#define SDP_EMODULE    -6   /* model code object could not be loaded, or was not built for this problem */

#define SDP_F64 0
#define SDP_F32 1

/*
 * How a problem handle stores its per-node arrays ON THE DEVICE.  Host arrays
 * passed to / returned by this API (value, policy, index, per-node control
 * boxes) are ALWAYS in the reference's order: C order of the state grid, last
 * axis fastest (stodynprog.py:272,478); the library converts on the device.
 *   SDP_LAYOUT_NODES    device order = host order (generic kernels);
 *   SDP_LAYOUT_COLUMNS  axis 0 fastest (numpy.moveaxis(A, 0, -1)): the column
 *                       kernels for storage-separable models read axis-0
 *                       pencils coalesced.  node_begin/node_end and the parts of
 *                       sdp_problem_attach_comm are indices in DEVICE order and
 *                       must then be multiples of orders[0] (whole columns).
 */
#define SDP_LAYOUT_NODES   0
#define SDP_LAYOUT_COLUMNS 1
/* Sweep kernel of a SDP_LAYOUT_NODES handle:
 *   SDP_VARIANT_DIRECT  `sdp_sweep`: one global load per interpolation vertex;
 *   SDP_VARIANT_STAGED  `sdp_sweep_lds`: a workgroup owns a tile of nodes and
 *                       stages the value sub-block its next states reach in LDS
 *                       (csrc/sdp_staged_kernel.h).  Same results, bit for bit.
 * A SDP_VARIANT_DIRECT code object whose `sdp_meta` carries SDP_META_F_LEAD (several controlled
 * state variables next to an exogenous process, csrc/sdp_lead_kernel.h; lanes_per_node must be 1)
 * also exports `sdp_lead_reduce`: the library launches it over the whole grid before every `sdp_sweep`
 * (it needs the whole cost-to-go array on the device: not with attached parts) and owns the arrays it
 * fills.  Same results, bit for bit (reference stodynprog.py:639-691 with any `dims`, :57-81). */
#define SDP_VARIANT_DIRECT 0
#define SDP_VARIANT_STAGED 1

const char *sdp_last_error(void);

/* ---- device ------------------------------------------------------------- */
int sdp_device_count(int *count);
int sdp_set_device(int device);
/* name buffer >= 256 bytes; any out pointer may be NULL */
int sdp_device_info(int device, char *name, int *compute_units, int64_t *hbm_bytes,
                    char *gcn_arch /* >= 64 bytes */);
int sdp_synchronize(void);

/* ---- multilinear interpolation ------------------------------------------- */
/*
 * Replaces  multilinear_interpolation(smin, smax, orders, values, s)
 *   stodynprog/dolointerpolation/multilinear_cython.pyx:17-49
 *   (called from stodynprog/stodynprog.py:285 and dolointerpolation/multilinear.py:87)
 * smin,smax: [d]; orders: [d] int64 ('long[:]'); values: [n_v][S] C-contiguous
 * with S = prod(orders), last axis fastest; s: [d][n_s] C-contiguous;
 * out: [n_v][n_s].  All host pointers.  d must be 1..4 (else SDP_EDIM).
 * Uniform grid, linear extrapolation outside [smin,smax].
 */
int sdp_mlinterp_f64(int d, const double *smin, const double *smax, const int64_t *orders,
                     const double *values, int64_t n_v, const double *s, int64_t n_s,
                     double *out);
int sdp_mlinterp_f32(int d, const float *smin, const float *smax, const int64_t *orders,
                     const float *values, int64_t n_v, const float *s, int64_t n_s,
                     float *out);

/*
 * Interpolator object with device-resident values: replaces a
 * MlinInterpolator / MultilinearInterpolator instance that is set once and
 * evaluated many times (stodynprog.py:269-289, multilinear.py:83-91), e.g. the
 * policy look-ups of a simulation loop.  smin/smax are given as doubles (exact
 * for float32 grids); host_values: [n_v][S] of `dtype`; sdp_interp_eval takes
 * s: [d][n_s] and writes out: [n_v][n_s], both host arrays of `dtype`.
 */
typedef struct sdp_interp sdp_interp;
int sdp_interp_create(int dtype, int d, const double *smin, const double *smax,
                      const int64_t *orders, const void *host_values, int64_t n_v,
                      sdp_interp **out);
int sdp_interp_eval(sdp_interp *h, const void *host_s, int64_t n_s, void *host_out);
int sdp_interp_destroy(sdp_interp *h);

/* ---- value-iteration problem handle ---------------------------------------- */
typedef struct sdp_problem sdp_problem;
typedef struct sdp_comm sdp_comm;

/*
 * Discretised problem, i.e. what DPSolver holds after discretize_state /
 * discretize_perturb / control_steps (stodynprog.py:335-389, 432-463).
 */
typedef struct sdp_problem_desc {
    int32_t dtype;              /* SDP_F64 | SDP_F32: type of every real array below */
    int32_t d;                  /* state variables, 1..4 */
    int32_t nu;                 /* control variables, 1..4 */
    int32_t W;                  /* perturbation points (of the FLAT law when n_perturb >= 2); 0 = deterministic system */
    int64_t orders[4];          /* points per state axis (state_grid lengths) */
    const void *axes[4];        /* state_grid[k]: orders[k] reals (np.linspace values) */
    const void *wgrid;          /* [n_perturb][W] reals, row i = variable i at every point of the law (one variable:
                                 * perturb_grid[0]); NULL if W == 0 */
    const void *proba;          /* [W] reals: the law's probabilities (one variable: perturb_proba[0]) */
    int32_t box_per_node;       /* 0: one box for all nodes, 1: arrays over nodes */
    int32_t lanes_per_node;     /* SDP_LANES the code object was built with */
    int32_t layout;             /* SDP_LAYOUT_NODES | SDP_LAYOUT_COLUMNS (see below) */
    int32_t variant;            /* SDP_VARIANT_DIRECT | SDP_VARIANT_STAGED (node layout only, see below) */
    const void *box_lo;         /* control_grids() lower ends: [nu] or [nu][S] reals */
    const void *box_hi;         /* upper ends */
    const int32_t *box_n;       /* points per control: [nu] or [nu][S] */
    int64_t node_begin;         /* slab of C-order node ids owned by this handle */
    int64_t node_end;           /*   ([0,S) on a single GPU) */
    const char *module_path;    /* gfx950 code object of the traced model (sdp_sweep, sdp_evalpol) */
    int32_t tile[4];            /* SDP_VARIANT_STAGED: node-tile shape the code object was built with */
    int32_t col_seg_nodes;      /* SDP_LAYOUT_COLUMNS with a row window (code object built with SDP_COL_ROWS
                                 * < orders[0]): nodes of a column one workgroup takes at most; 0 = no window */
    int32_t n_perturb;          /* perturbation variables, 0..4; 0 means "1 when W > 0" (the field was `reserved`, must be 0).
                                 * 2..4: the code object is a unit of several variables (csrc/sdp_multiw_kernel.h), the law
                                 * is their product flattened in C order, last variable fastest; node layout, direct
                                 * variant, one GPU */
} sdp_problem_desc;

/* The code object must have been generated for THIS problem: it declares
 *     extern "C" __constant__ int32_t sdp_meta[SDP_META_WORDS]      (csrc/sdp_kernel_args.h)
 * -- real type, d, nu, perturbation or not, layout / kernel variant, the axis-0 length and the
 * perturbation count its column table is sized for, the control lattice of its control table --
 * and sdp_problem_create compares every field with `desc`.  A mismatch, or a code object
 * without `sdp_meta`, is refused with SDP_EMODULE and a message naming the field (the reference
 * raises on a bad shape too, multilinear_cython.pyx:46-47; it never returns stale values). */
int sdp_problem_create(const sdp_problem_desc *desc, sdp_problem **out);
int sdp_problem_destroy(sdp_problem *p);

/* J_next of value_iteration (stodynprog.py:466,498): S reals, C-order. */
int sdp_problem_set_value(sdp_problem *p, const void *host_V);
/* pol of eval_policy (stodynprog.py:693,723): [S][nu] reals (control values). */
int sdp_problem_set_policy(sdp_problem *p, const void *host_pol);

/* Lifted model constants.  A finite-horizon problem whose callables look data
 * up by time index (reference examples/01 Deterministic storage control/
 * det_storage_control.py:89, `P_req = p['P_req_data'][k]`, called from
 * DPSolver.bellman_recursion, stodynprog.py:582) is traced one time step at a
 * time; the constants of the step become the array `sdp_model_prm[n]` of the
 * code object (same `real` type as the problem), so all steps share one kernel.
 * Sets those n values for the launches that follow.  n must equal the count
 * the code object declares (0 when it declares none). */
int sdp_problem_set_params(sdp_problem *p, const void *values, int32_t n);

/*
 * One Bellman backup over the handle's node slab -- DPSolver.value_iteration
 * (stodynprog.py:466-534) fused with _value_at_state_vect (639-691) and the
 * interpolation (multilinear_cython.pyx:51-300).  Reads the value buffer,
 * writes J_k, the optimal control values and their flat lattice indices.
 * With a communicator attached the J_k slabs are all-gathered (RCCL) so that
 * every rank ends with the full J_k.  rel_dp != 0: J_ref = J_k[ref_index]
 * (ref_index: flat C-order index of the reference node, stodynprog.py:384);
 * J_k -= J_ref (stodynprog.py:523-525); *J_ref_out receives J_ref.
 * t_k: time index passed to the model of a non-stationary system.
 */
int sdp_problem_vi_sweep(sdp_problem *p, double t_k, int rel_dp, int64_t ref_index,
                         double *J_ref_out);

/*
 * n_iter fixed-policy backups -- DPSolver.eval_policy (stodynprog.py:693-775).
 * Starts from the value buffer, leaves the result in the J buffer.
 * J_ref_out: [n_iter] reference costs when rel_dp != 0 (may be NULL).
 */
int sdp_problem_eval_policy(sdp_problem *p, int32_t n_iter, int rel_dp, int64_t ref_index,
                            double *J_ref_out);

/*
 * Sweep loops that stop at a tolerance (no reference counterpart: its users judge
 * convergence by eye).  sdp_problem_vi_until runs the loop of sdp_problem_vi_sweep +
 * sdp_problem_swap (J_ref_out[k]: reference cost of sweep k), sdp_problem_eval_policy_until
 * that of sdp_problem_eval_policy (fused relative shift included), at most n_max sweeps,
 * queued back to back.  After sweeps check_every, 2 check_every, ... and after sweep n_max
 * the library reduces the last two cost-to-go arrays a = J^(k), b = J^(k-1) (with rel_dp
 * both shifted, J - J[ref], as the host loop returns them; J^(0) is the starting value):
 *     d = 0 where a == b, else a - b rounded in the problem's real type
 *     stats[2 i] = min d, stats[2 i + 1] = max d     (check i, widened to double; both NaN
 *                                                     if any d is NaN)
 * and stops after the first check with  max d - min d <= tol  (never on NaN).  *n_done:
 * sweeps run; J, policy and J_ref_out[0 .. n_done) are those of a plain call with
 * n_iter = *n_done.  stats: room for ceil(n_max / check_every) checks; J_ref_out: n_max
 * doubles (may be NULL).  tol >= 0, check_every >= 1, else SDP_EINVAL.  With a
 * communicator attached every rank reduces the nodes it computes and the per-rank
 * statistics are all-gathered: every rank holds the same bits and stops at the same sweep
 * (collective: every rank must call it).  A check reads back 24 bytes per rank once.
 */
int sdp_problem_vi_until(sdp_problem *p, int32_t n_max, int rel_dp, int64_t ref_index,
                         int32_t check_every, double tol, int32_t *n_done,
                         double *stats /* [n_checks][2] */, double *J_ref_out /* [n_max] */);
int sdp_problem_eval_policy_until(sdp_problem *p, int32_t n_max, int rel_dp, int64_t ref_index,
                                  int32_t check_every, double tol, int32_t *n_done,
                                  double *stats /* [n_checks][2] */, double *J_ref_out /* [n_max] */);

/*
 * The whole of one DPSolver.value_iteration call with host arrays in and out
 * (stodynprog.py:466-534; the reference takes J_next and returns fresh J_k, pol_k
 * every call): upload of host_V (NULL: keep the device's value buffer), backup,
 * relative-DP shift, download of J_k, of the policy values (host_pol, may be NULL)
 * and of the lattice indices (host_idx, may be NULL), queued back to back with one
 * synchronisation at the end.  Buffers from sdp_host_alloc (page-locked) move at
 * PCIe rate; any other host memory works too, slower.
 */
int sdp_problem_backup_host(sdp_problem *p, const void *host_V, double t_k, int rel_dp,
                            int64_t ref_index, void *host_J, void *host_pol, int32_t *host_idx,
                            double *J_ref_out);
/*
 * on != 0 (the default): on one GPU, grids of 8 MiB and more run the backup of
 * sdp_problem_backup_host in a few phases of the node range and send the finished rows of a
 * phase to the host under the kernel of the next one.  on == 0: one launch, then the downloads.
 * Same arrays either way.
 */
int sdp_problem_set_host_overlap(sdp_problem *p, int on);
int sdp_host_alloc(size_t bytes, void **out);      /* page-locked host memory */
int sdp_host_free(void *ptr);

/*
 * Batched closed-loop simulation without leaving the device -- the loop of the
 * reference's examples (examples/20 Searev storage control/storage_control.py:242-251:
 * `P_sto[k] = P_sto_law(E[k], Speed[k], Accel[k]); x[k+1] = sys.dyn(x[k], P_sto[k], w[k])`,
 * one interpolator call per step).  For B trajectories and T steps:
 *     u[k] = policy(x[k])            every control component interpolated from host_pol
 *                                    ([nu][S] control values on the state grid, C order;
 *                                    same arithmetic as sdp_mlinterp_*)
 *     x[k+1] = dyn(x[k], u[k], w[k]), g[k] = cost(x[k], u[k], w[k])    (the traced model)
 * host_x0 [d][B]; host_w [T][B] (NULL for a deterministic system; [T][n_perturb][B] for a problem of
 * several perturbation variables); outputs host_x
 * [T+1][d][B] (x[0] = x0), host_u [T][nu][B], host_g [T][B] (may be NULL).  t0: time
 * index of step 0 for a non-stationary system.
 */
int sdp_problem_simulate(sdp_problem *p, const void *host_pol, int64_t B, int64_t T,
                         const void *host_x0, const void *host_w, double t0,
                         void *host_x, void *host_u, void *host_g);

/*
 * Monte Carlo evaluation of a policy without leaving the device: B closed-loop trajectories of T
 * steps as above, but the perturbation of every step is DRAWN on the device and only reductions
 * come back.  The draw of trajectory row b at step k (k = 0..T-1, absolute over the whole call):
 *     Philox4x32-10, key = (seed low word, seed high word),
 *                    counter = (id low, id high, k low, k high),  id = traj_offset + b
 *     u = ((r0 >> 5) * 2^26 + (r1 >> 6)) * 2^-53       output words 0 and 1; a double in [0, 1)
 *     j = number of i in [0, n_law - 2] with u >= host_cum[i];   w = host_law_grid[j]
 * host_cum [n_law] doubles: running sum of the law's probabilities (its last entry is not read);
 * host_law_grid [n_law] reals, n_law in 1..4096 (several perturbation variables: [n_perturb][n_law], w = column j,
 * and 8 (n_law - 1) + n_perturb n_law sizeof(real) <= 65536 bytes).  A draw depends on (seed, id, k) alone: B, the
 * launch grid and steps_per_launch (the run is cut into kernel launches of at most that many
 * steps, the state kept on the device between them) do not change a bit of the results.
 * Over the steps k >= n_burn: host_cost_sum [B] reals, acc = acc + g[k] in k order;
 * host_n_outside [B] int64, steps whose x[k] has a component below the first / above the last
 * grid point or NaN; host_occupancy [S] uint64 or NULL, visits of the grid node nearest to x[k]
 * (per axis the interpolation cell + (weight >= 0.5), clamped; C order).  host_x_final [d][B]:
 * the state after step T-1.  host_pol, host_x0, t0: as for the simulation above.  Stochastic
 * systems on one GPU only (SDP_EINVAL otherwise).
 */
int sdp_problem_montecarlo(sdp_problem *p, const void *host_pol, int64_t B, int64_t T, int64_t n_burn,
                           uint64_t seed, uint64_t traj_offset, const void *host_x0,
                           const double *host_cum, int32_t n_law, const void *host_law_grid, double t0,
                           int64_t steps_per_launch, void *host_cost_sum, int64_t *host_n_outside,
                           void *host_x_final, uint64_t *host_occupancy);

/*
 * The same two loops under a TIME-INDEXED policy -- the forward half of a finite-horizon problem, the loop the
 * reference's examples/01 Deterministic storage control ends with (one interpolator of pol[k] and one sys.dyn(k, ..)
 * call per step).  Step k of the call (k = 0..T-1) runs at time index t0 + k and looks its controls up in slice k of
 *     host_pol [n_pol_steps][nu][S]      n_pol_steps == T: the caller hands over the slices of the steps it runs
 * and, when the code object has lifted constants (a model traced for one concrete time index), evaluates the model
 * with row k of
 *     host_prm [T][n_params]             reals; NULL, 0 for a code object without lifted constants
 * (sdp_problem_set_params is not consulted).  The policy is uploaded in chunks of whole steps of at most chunk_bytes
 * (a step larger than that is a chunk of its own) and every chunk is run before the next goes up, with the state --
 * for Monte Carlo also the sums -- in device buffers in between: chunk_bytes and steps_per_launch do not change a bit
 * of the results.  Everything else as for sdp_problem_simulate and sdp_problem_montecarlo; the Philox counter's step
 * is k, the step of the call.  One GPU.  SDP_EMODULE for a code object built before these kernels existed.
 */
int sdp_problem_simulate_h(sdp_problem *p, int64_t n_pol_steps, const void *host_pol, const void *host_prm,
                           int32_t n_params, int64_t chunk_bytes, int64_t B, int64_t T,
                           const void *host_x0, const void *host_w, double t0,
                           void *host_x, void *host_u, void *host_g);
int sdp_problem_montecarlo_h(sdp_problem *p, int64_t n_pol_steps, const void *host_pol, const void *host_prm,
                             int32_t n_params, int64_t chunk_bytes, int64_t B, int64_t T, int64_t n_burn,
                             uint64_t seed, uint64_t traj_offset, const void *host_x0,
                             const double *host_cum, int32_t n_law, const void *host_law_grid, double t0,
                             int64_t steps_per_launch, void *host_cost_sum, int64_t *host_n_outside,
                             void *host_x_final, uint64_t *host_occupancy);

/*
 * One-step lookahead at arbitrary states -- the reference's _value_at_state_vect (stodynprog.py:639-691) for a batch,
 * and the closed loop that applies it.  The handle must be that of a LOOKAHEAD unit (a node-order code object
 * generated with SDP_LOOKAHEAD: kernel sdp_lookahead; with SDP_LOOKAHEAD_BOX also its own box function and kernel
 * sdp_simulate_lookahead); SDP_EMODULE otherwise.  One GPU.  The definition is stodynprog_amd/lookahead.py.
 *
 * sdp_problem_lookahead: at every state b of host_x [d][B], with the cost-to-go host_V [S] (C order),
 *     host_J [B], host_u [nu][B], host_idx [B]   min / argmin over the state's control lattice of
 *                                                 E_w[g(x, u, w) + J_next(f(x, u, w))], control values, flat index
 * The lattice of state b is host_lo, host_hi [nu][B] (reals; the centre twice where n == 1) and host_n [nu][B]
 * (host_n[0][b] == 0: no valid lattice, the results are NaN, NaN, -1) -- or, with host_n NULL, made on the device by
 * the unit's box function from steps [nu], the control step hints (float64), with the same bits.
 *
 * sdp_problem_simulate_lookahead: B closed-loop trajectories of T steps; step k runs at time index t0 + k, looks
 * ahead into slice k of host_V [n_V_steps][S] (n_V_steps == T), or into the one host_V [S] (n_V_steps == 0), and then
 * takes the model's own step at the optimal control.  host_x [T+1][d][B], host_u [T][nu][B], host_g [T][B] as
 * sdp_problem_simulate; host_q [T][B] the minimised expected values.  A time-indexed cost-to-go is uploaded in chunks
 * of whole steps of at most chunk_bytes, the state stays on the device in between: no cut changes a bit.  Needs a
 * unit with its own box function and without lifted constants.
 */
int sdp_problem_lookahead(sdp_problem *p, const void *host_V, int64_t B, const void *host_x,
                          const void *host_lo, const void *host_hi, const int32_t *host_n,
                          const double *steps, double t_k, void *host_J, void *host_u, int32_t *host_idx);
int sdp_problem_simulate_lookahead(sdp_problem *p, int64_t n_V_steps, const void *host_V, int64_t chunk_bytes,
                                   int64_t B, int64_t T, const void *host_x0, const void *host_w,
                                   const double *steps, double t0,
                                   void *host_x, void *host_u, void *host_g, void *host_q);

/*
 * Monte Carlo evaluation under LOOKAHEAD controls: sdp_problem_simulate_lookahead's closed loop with the perturbation
 * of every step drawn on the device and only reductions coming back -- what sdp_problem_montecarlo is to
 * sdp_problem_simulate.  host_V, n_V_steps, chunk_bytes, steps, t0: as sdp_problem_simulate_lookahead; the draw
 * (seed, traj_offset, host_cum, n_law, host_law_grid; the Philox counter's step is k, the step of the call),
 * n_burn, steps_per_launch and the outputs: as sdp_problem_montecarlo.  host_cum / host_law_grid are the law the
 * PLANT draws from; the expectation inside the backup always runs over the law of the handle.  Neither chunk_bytes nor
 * steps_per_launch changes a bit.  Needs a lookahead unit of a stochastic system with its own box function and without
 * lifted constants (SDP_EMODULE for a code object without kernel sdp_montecarlo_lookahead).  One GPU.
 */
int sdp_problem_montecarlo_lookahead(sdp_problem *p, int64_t n_V_steps, const void *host_V, int64_t chunk_bytes,
                                     int64_t B, int64_t T, int64_t n_burn, uint64_t seed, uint64_t traj_offset,
                                     const void *host_x0, const double *host_cum, int32_t n_law,
                                     const void *host_law_grid, const double *steps, double t0,
                                     int64_t steps_per_launch, void *host_cost_sum, int64_t *host_n_outside,
                                     void *host_x_final, uint64_t *host_occupancy);

/* ---- transition operator of a policy: the forward half of the model -------------
 * Under a fixed policy the backup of sdp_problem_eval_policy is (P J)(s) + gbar(s), with
 * (P J)(s) = sum_j P[j] interp(J)(dyn(x_s, pol[s], w_j)).  A sdp_transop holds P^T as a CSR matrix on
 * the device -- W 2^d entries per node, sorted STABLY by target node so that a row keeps the emission
 * order (source s, law point j, vertex v ascending) -- and moves a state distribution: mu' = P^T mu,
 *     out[t]: acc = 0; acc = acc + data[k] * mu[indices[k]]   for k ascending through row t
 * (one rounded multiply and one rounded add per entry; an empty row gives +0).  The definition, entry
 * by entry, is stodynprog_amd/forward.py; the interpolation extrapolates, so weights are negative or
 * above 1 where the model leaves the grid (nothing is clamped: P^T stays the exact adjoint of the
 * backup).  An operator takes nnz (sizeof(real) + 4) + 8 (S + 1) bytes plus two vectors, and about
 * three times that while it is built; nnz < 2^32.  One GPU. */
typedef struct sdp_transop sdp_transop;
/* Entries from the model's code object (kernel sdp_transitions) at the policy host_pol [S][nu]
 * (reals, C order: the layout of sdp_problem_set_policy) and time index t_k, with the problem's law
 * (a deterministic system: one point of weight 1).  The operator does not refer to the problem
 * afterwards.  SDP_EINVAL with a communicator of several ranks. */
int sdp_transop_create(sdp_problem *p, const void *host_pol, double t_k, sdp_transop **out);
/* The same sort and row build on host-given entries in emission order: tgt, src [nnz] node ids in
 * [0, S) -- anything else is refused with SDP_EINVAL before a byte is allocated -- and val [nnz]
 * reals of `dtype`.  For models evaluated on the host, and for any sparse chain on S nodes. */
int sdp_transop_from_coo(int dtype, int64_t S, int64_t nnz, const int32_t *tgt, const int32_t *src,
                         const void *val, sdp_transop **out);
int sdp_transop_destroy(sdp_transop *op);
/* n_steps >= 0 pushes, ping-pong in device memory, no host round trip between them.  host_mu [S]
 * reals replaces the resident vector first; NULL continues from it (SDP_EINVAL if there is none). */
int sdp_transop_push(sdp_transop *op, const void *host_mu_or_null, int32_t n_steps);
/* Pushes from the resident vector until delta = max |mu_{k+1} - mu_k| <= tol, checked after push
 * check_every, 2 check_every, .. and after push n_max (the reduction of the convergence check above:
 * a difference is 0 where the two are equal, NaN never converges; 24 bytes come back per check, the
 * only synchronisations).  *n_done: pushes made; *delta: the last checked value. */
int sdp_transop_push_until(sdp_transop *op, int32_t n_max, int32_t check_every, double tol,
                           int32_t *n_done, double *delta);
int sdp_transop_get(sdp_transop *op, void *host_mu);                 /* S reals: the resident vector */
/* indptr [S+1], indices [nnz] (the sources), data [nnz] reals; any of them may be NULL */
int sdp_transop_get_csr(sdp_transop *op, int64_t *indptr, int32_t *indices, void *data);
/* gbar [S] reals: acc = 0; acc = acc + g_j P[j], j ascending (sdp_transop_create only) */
int sdp_transop_get_mean_cost(sdp_transop *op, void *host_gbar);
/* HIP-event duration of the last call's device work (the build, a push, a push_until), ms */
int sdp_transop_last_kernel_ms(sdp_transop *op, double *ms);
/* Which rows a push gives to a whole wave (its lanes form the products from coalesced loads, one chain adds them in
 * entry order: the same bits as the lane-per-row path): those of min_entries entries or more.  The build sets 8;
 * 0 gives every row to one lane.  A tuning and measuring knob: results do not depend on it. */
int sdp_transop_set_long_rows(sdp_transop *op, int32_t min_entries);
/* .. and of the build's two parts: kernel sdp_transitions, and the device work of sort + gather + row pointers
 * (everything is allocated before the events that bracket it) */
int sdp_transop_build_ms(sdp_transop *op, double *entries_ms, double *sort_ms);

/* ---- the transition operators of the steps of a horizon, and distributions propagated through them --------
 * (stodynprog_amd/forward.py, `chain_entries` and `propagate`, is the definition).  Step k = 0 .. n_steps - 1 is
 * sdp_transop_create under slice k of a time-indexed policy at time index t0 + k, in a unit with lifted constants
 * with row k of a table of them: all steps in ONE launch of kernel sdp_transitions_h (csrc/sdp_trans_horizon_kernel.h)
 * and ONE stable sort by (step, target).  One operator holds n_steps * S < 2^31 rows and fewer than 2^32 entries; a
 * caller cuts a longer horizon into parts and hands the last distribution of one to the next (no cut changes a bit).
 *   host_pol [n_steps][nu][S] reals, control axis first (as sdp_problem_simulate_h takes it)
 *   host_prm [n_steps][n_params] reals, or NULL with n_params = 0 (a unit without lifted constants) */
typedef struct sdp_chainop sdp_chainop;
int sdp_chainop_create(sdp_problem *p, int64_t n_steps, const void *host_pol, const void *host_prm,
                       int32_t n_params, double t0, sdp_chainop **out);
int sdp_chainop_destroy(sdp_chainop *op);
/* host_mu0 [B][S] reals -> host_mu [n_steps + 1][B][S]: mu[0] = mu0, mu[k + 1] = P_k^T mu[k].  1 <= B <= 65535.  The
 * vectors stay on the device; step k is one launch over the rows of block k for all B vectors (the long rows of the
 * block in launches of their own, as in sdp_transop_push), queued without a host synchronisation in between.  Per row
 * acc = 0; acc = acc + data[e] * mu[k][b][source[e]], e ascending: the bits of n_steps solo pushes. */
int sdp_chainop_propagate(sdp_chainop *op, int64_t B, const void *host_mu0, void *host_mu);
/* the CSR of step `step` as sdp_transop_get_csr gives a solo operator's: indptr [S + 1], indices and data [S W 2^d]
 * (any may be NULL) */
int sdp_chainop_get_csr(sdp_chainop *op, int64_t step, int64_t *indptr, int32_t *indices, void *data);
/* gbar [n_steps][S] reals */
int sdp_chainop_get_mean_cost(sdp_chainop *op, void *host_gbar);
/* HIP-event durations, ms: the build's kernel sdp_transitions_h, its sort + gather + row pointers + local sources,
 * and the launches of the last sdp_chainop_propagate */
int sdp_chainop_times(sdp_chainop *op, double *entries_ms, double *sort_ms, double *push_ms);

/* Make the last J_k the next J_next without leaving the device. */
int sdp_problem_swap(sdp_problem *p);

int sdp_problem_get_value(sdp_problem *p, void *host_J);            /* S reals            */
int sdp_problem_get_policy(sdp_problem *p, void *host_pol /* [S][nu] reals or NULL */,
                           int32_t *host_idx /* [S] or NULL */);
/* With a communicator attached this is a collective call: the policy rows of the
 * other ranks' parts are all-gathered first (every rank must call it). */

/* HIP-event duration of the last sweep / eval kernel launch(es), milliseconds. */
int sdp_problem_last_kernel_ms(sdp_problem *p, double *ms);
/* Timed repetition for benchmarks: `reps` sweeps with ping-pong swap between
 * them; returns the total HIP-event time of the whole loop and of the sweep
 * kernels alone. */
int sdp_problem_bench_sweeps(sdp_problem *p, int32_t reps, int rel_dp, int64_t ref_index,
                             double *loop_ms, double *kernel_ms);

/* Diagnostic (tools/clock_probe.py): code objects built with -DSDP_STAMP=1 record
 * s_memtime / s_memrealtime of thread 0 of every workgroup at kernel entry and
 * exit.  enable != 0 allocates the stamp buffer (the launches that follow fill
 * it); host != NULL copies n_words 64-bit words out ([workgroup][4]); enable == 0
 * frees it.  Production code objects never touch the buffer. */
int sdp_problem_debug_stamps(sdp_problem *p, int enable, unsigned long long *host,
                             int64_t n_words);

/* ---- a family of same-shaped problems in one call (csrc/sdp_family_kernel.h) -------- */
/*
 * P problems that share the grid's shape, the number of controls and of perturbation points and one
 * family code object (codegen.family_unit: kernel sdp_family_sweep, lifted constants), and differ in
 * constants, grid ends, law and box table.  Every array of the descriptor is member-major; host arrays
 * are only read during the call.  One launch backs up every listed member; member p of every result has
 * the bits of the sdp_problem calls on problem p alone.  One GPU, node layout.
 */
typedef struct sdp_family sdp_family;
typedef struct sdp_family_desc {
    int32_t dtype;            /* SDP_F64 / SDP_F32 */
    int32_t d;                /* state dimension, 1..4 */
    int32_t nu;               /* control variables, 1..4 */
    int32_t W;                /* perturbation points of every member (0: deterministic) */
    int32_t P;                /* members, >= 1 */
    int32_t n_params;         /* lifted constants per member (SDP_NPARAMS of the code object) */
    int32_t box_per_node;     /* 0: box arrays [P][nu]; 1: [P][nu][S] */
    int32_t lanes_per_node;   /* SDP_LANES of the code object: power of two in 1..64 */
    int64_t orders[4];        /* grid points per state axis, the same for every member */
    const void *axes;         /* [P][sum orders] reals: the members' axes, concatenated */
    const void *wgrid;        /* [P][W] reals (NULL when W == 0) */
    const void *proba;        /* [P][W] reals */
    const void *box_lo;       /* reals */
    const void *box_hi;       /* reals */
    const int32_t *box_n;
    const char *module_path;  /* family code object (.hsaco); its sdp_meta is checked */
} sdp_family_desc;

int sdp_family_create(const sdp_family_desc *desc, sdp_family **out);
int sdp_family_destroy(sdp_family *f);
/* J_next of every member, [P][S] reals in C order; every member is listed again for the sweeps that follow. */
int sdp_family_set_value(sdp_family *f, const void *host_V);
/* The lifted constants, [P][n] reals with n == n_params, for the launches that follow. */
int sdp_family_set_params(sdp_family *f, const void *values, int32_t n);
/* One backup of every member at time index t_k.  rel_dp: J[p] -= J[p][ref_index] afterwards, the
 * subtracted values in J_ref_out[P] (as sdp_problem_vi_sweep does it, per member). */
int sdp_family_vi_sweep(sdp_family *f, double t_k, int rel_dp, int64_t ref_index, double *J_ref_out);
/* n_iter backups, each fed with the result of the one before; J_ref_out [n_iter][P] (rel_dp only). */
int sdp_family_vi_sweeps(sdp_family *f, int32_t n_iter, int rel_dp, int64_t ref_index, double *J_ref_out);
/*
 * At most n_max backups with the convergence check of sdp_problem_vi_until per member, after sweeps
 * check_every, 2 check_every, .. and n_max: one reduction launch for the members still listed and one
 * readback of 24 bytes per such member.  A member whose span dmax - dmin <= tol leaves the list: nothing
 * writes its slices afterwards.  n_done[P]: sweeps every member ran; stats [n_checks][P][2]: dmin, dmax of
 * check c of member p (rows of checks the member did not run are left as they were); J_ref_out [n_max][P].
 */
int sdp_family_vi_until(sdp_family *f, int32_t n_max, int rel_dp, int64_t ref_index, int32_t check_every,
                        double tol, int32_t *n_done, double *stats, double *J_ref_out);
/* Results of every member's last sweep: [P][S] reals; [P][S][nu] reals (or NULL); [P][S] (or NULL). */
int sdp_family_get_value(sdp_family *f, void *host_J);
int sdp_family_get_policy(sdp_family *f, void *host_pol, int32_t *host_idx);
/* HIP-event duration of the launches of the last sweep call (all its sweeps), milliseconds. */
int sdp_family_last_kernel_ms(sdp_family *f, double *ms);

/*
 * Policy evaluation of a family (csrc/sdp_family_policy_kernel.h).  The family's EVALUATION unit
 * (codegen.family_policy_unit: kernels sdp_family_evalpol and sdp_family_evalpol_resident) is loaded beside the
 * sweep unit; its sdp_meta is checked.  Member p of every result has the bits of sdp_problem_eval_policy /
 * sdp_problem_eval_policy_until on problem p alone; a time-dependent system is evaluated at time index 0.
 */
int sdp_family_load_policy_unit(sdp_family *f, const char *module_path);
/* The prescribed policy of every member, [P][S][nu] reals in C order (its buffer is allocated at the first call). */
int sdp_family_set_policy(sdp_family *f, const void *host_pol);
/* The policy the last sweep wrote becomes the prescribed one without a copy: the two buffers swap. */
int sdp_family_take_policy(sdp_family *f);
/* same[P]: 1 where the policy of the last sweep equals the prescribed one value by value (a NaN equals nothing).
 * One launch, P words read back. */
int sdp_family_compare_policy(sdp_family *f, int32_t *same);
/* The members the launches that follow run: n distinct indices.  sdp_family_set_value lists all of them again. */
int sdp_family_set_members(sdp_family *f, const int32_t *members, int32_t n);
/* The two forms of an evaluation: a launch per step, any grid size; or all steps of a member in one workgroup with
 * its values in LDS (a member of more nodes than the unit's two LDS buffers hold is refused with SDP_EINVAL). */
#define SDP_FAMILY_EVAL_STEPS 0
#define SDP_FAMILY_EVAL_RESIDENT 1
/* n_iter steps of the listed members from the values set, under the prescribed policy.  rel_dp: the relative
 * algorithm, the reference cost of every step in J_ref_out [n_iter][P]. */
int sdp_family_eval_policy(sdp_family *f, int32_t n_iter, int rel_dp, int64_t ref_index, int32_t form,
                           double *J_ref_out);
/*
 * At most n_max steps with the check of sdp_problem_eval_policy_until per member (the statistics of the shifted
 * sequence), in the shape of sdp_family_vi_until: n_done[P], stats [n_checks][P][2], J_ref_out [n_max][P]; only
 * the entries of listed members are written.  Steps form: one reduction launch and 24 bytes a listed member read
 * back per checked step, converged members leave the list.  Resident form: the checks run inside the kernel and
 * everything is read back once at the end.
 */
int sdp_family_eval_policy_until(sdp_family *f, int32_t n_max, int rel_dp, int64_t ref_index, int32_t check_every,
                                 double tol, int32_t form, int32_t *n_done, double *stats, double *J_ref_out);

/*
 * Monte Carlo policy evaluation of a family (csrc/sdp_family_mc_kernel.h).  The family's MONTE CARLO unit
 * (codegen.family_mc_unit: kernel sdp_family_montecarlo) is loaded beside the sweep unit; its sdp_meta is checked.
 */
int sdp_family_load_mc_unit(sdp_family *f, const char *module_path);
/*
 * sdp_problem_montecarlo of every member of the handle, together: B trajectories with the ids traj_offset ..
 * traj_offset + B - 1 and T steps per member, member p under its policy host_pol[p] ([P][nu][S] reals), from
 * its start states host_x0[p] ([P][d][B]), with its seed host_seeds[p] and its law (host_cum [P][n_law] float64
 * running sums, host_law_grid [P][n_law] reals; every law has n_law points, 1..4096, the draw table of one member
 * at most 65536 bytes), the constants of sdp_family_set_params.  The sums are zeroed, one launch runs at most
 * steps_per_launch steps (clamped to 2^30) of all members, the state stays on the device in between, and everything
 * is read back once: host_cost_sum [P][B] reals, host_n_outside [P][B], host_x_final [P][d][B] reals,
 * host_occupancy [P][S] or NULL.  Member p of every result has the bits of sdp_problem_montecarlo on problem p
 * alone.  sdp_family_last_kernel_ms covers the call.  SDP_EINVAL for a NULL pointer, a negative size, n_burn
 * outside [0, T], steps_per_launch < 1, a deterministic family, a law that does not fit, or no unit loaded.
 */
int sdp_family_montecarlo(sdp_family *f, const void *host_pol, int64_t B, int64_t T, int64_t n_burn,
                          const uint64_t *host_seeds, uint64_t traj_offset, const void *host_x0,
                          const double *host_cum, int32_t n_law, const void *host_law_grid, double t0,
                          int64_t steps_per_launch, void *host_cost_sum, int64_t *host_n_outside,
                          void *host_x_final, uint64_t *host_occupancy);

/*
 * Transition operators of a family's policies (csrc/sdp_family_trans_kernel.h).  The family's TRANSITION unit
 * (codegen.family_trans_unit: kernel sdp_family_transitions) is loaded beside the sweep unit; its sdp_meta is checked
 * (SDP_META_F_FAMILY_TRANS, the workgroup size and the tile of 256 >> d nodes).
 */
int sdp_family_load_trans_unit(sdp_family *f, const char *module_path);
/*
 * sdp_transop_create of every member of the handle in one launch and one sort: member p under its policy
 * host_pol[p] ([P][S][nu] reals, C order) at time index t_k, with its law (deterministic members: one point of weight
 * 1) and the constants of sdp_family_set_params.  The P operators are ONE block-diagonal sdp_transop on P S rows,
 * member p's node s row p S + s: sdp_transop_push, _get, _get_mean_cost, _get_csr, _build_ms, _last_kernel_ms,
 * _set_long_rows and _destroy serve it as they serve a solo operator, on vectors of [P][S] reals, and member p of every
 * result has the bits of the solo operator of problem p (the sort is stable and members share no row).  The operator
 * does not refer to the family afterwards.  SDP_EINVAL for a NULL pointer, no unit loaded, P S >= 2^31 rows or
 * P S W 2^d >= 2^32 entries.
 */
int sdp_family_transop_create(sdp_family *f, const void *host_pol, double t_k, sdp_transop **out);
/*
 * sdp_transop_push_until with a stop per member, on the operators of a family: every member starts from its slice of
 * the resident vector and stops at its own first checked push with delta[p] = max |mu_{k+1} - mu_k| over its slice
 * <= tol, or at push n_max.  A check is one reduction launch over the members still running and 24 bytes a member
 * back; a member that has stopped is computed no more (both push paths skip its rows) and its slice of the resident
 * vector stays the iterate it stopped on; the loop ends when no member is left.  n_done [P]: pushes each member ran;
 * delta [P]: its last checked value (NaN never converges).  SDP_EINVAL for a solo operator.
 */
int sdp_transop_push_until_members(sdp_transop *op, int32_t n_max, int32_t check_every, double tol,
                                   int32_t *n_done, double *delta);

/*
 * Closed loops of a family over a horizon (csrc/sdp_family_horizon_kernel.h).  The family's HORIZON unit
 * (codegen.family_horizon_unit: kernels sdp_family_simulate and, for a stochastic family, sdp_family_montecarlo_h) is
 * loaded beside the sweep unit; its sdp_meta is checked (SDP_META_F_FAMILY_HORIZON, the two workgroup sizes).
 */
int sdp_family_load_horizon_unit(sdp_family *f, const char *module_path);
/*
 * sdp_problem_simulate_h of every member of the handle, together: B trajectories of T >= 1 steps per member.
 * host_pol is [P][pol_steps][nu][S] reals: a time-indexed policy (pol_timed != 0, pol_steps == T: it goes up a chunk
 * of whole steps of all members at a time, at most chunk_bytes, a larger step a chunk of its own) or one stationary
 * policy per member (pol_timed == 0, pol_steps == 1: uploaded once, read with a step stride of 0).  host_prm is the
 * table of lifted constants [P][T][n_prm] (prm_timed != 0) or [P][1][n_prm] (prm_timed == 0: a model that is symbolic
 * in time, one row per member for every step); n_prm is the family's.  host_x0 [P][d][B], host_w [P][T][B] (NULL: a
 * deterministic family); results host_x [P][T+1][d][B], host_u [P][T][nu][B], host_g [P][T][B].  Member p of every
 * result has the bits of sdp_problem_simulate_h on problem p alone; no cut changes one.  sdp_family_last_kernel_ms
 * covers the call.  SDP_EINVAL for a NULL pointer, a negative size, T < 1, a policy or table of another length,
 * chunk_bytes < 1, missing perturbation sequences, or no unit loaded.
 */
int sdp_family_simulate(sdp_family *f, const void *host_pol, int64_t pol_steps, int32_t pol_timed, const void *host_prm,
                        int32_t n_prm, int32_t prm_timed, int64_t chunk_bytes, int64_t B, int64_t T,
                        const void *host_x0, const void *host_w, double t0, void *host_x, void *host_u, void *host_g);
/*
 * sdp_problem_montecarlo_h of every member of the handle, together: the arguments and results of
 * sdp_family_montecarlo with the policy and the table of sdp_family_simulate.  Launches are cut at the policy's
 * chunks and at steps_per_launch; the states, the sums, n_outside and the occupancy stay on the device in between.
 */
int sdp_family_montecarlo_h(sdp_family *f, const void *host_pol, int64_t pol_steps, int32_t pol_timed,
                            const void *host_prm, int32_t n_prm, int32_t prm_timed, int64_t chunk_bytes, int64_t B,
                            int64_t T, int64_t n_burn, const uint64_t *host_seeds, uint64_t traj_offset,
                            const void *host_x0, const double *host_cum, int32_t n_law, const void *host_law_grid,
                            double t0, int64_t steps_per_launch, void *host_cost_sum, int64_t *host_n_outside,
                            void *host_x_final, uint64_t *host_occupancy);

/*
 * One-step lookahead at arbitrary states for a family (csrc/sdp_family_lookahead_kernel.h).  The family's LOOKAHEAD
 * unit (codegen.family_lookahead_unit: kernels sdp_family_lookahead and, for a stochastic family,
 * sdp_family_montecarlo_lookahead) is loaded beside the sweep unit; its sdp_meta is checked.
 */
int sdp_family_load_lookahead_unit(sdp_family *f, const char *module_path);
/*
 * What the unit's box function reads for every member: box_params [P][n_box] float64, the constants of the traced
 * control_box (n_box must be what the unit was built for), and steps [P][nu] float64, the members' control step
 * hints (NaN is refused).  To be set after every sdp_family_load_lookahead_unit.
 */
int sdp_family_set_lookahead_box(sdp_family *f, const double *box_params, int32_t n_box, const double *steps);
/*
 * sdp_problem_lookahead of every member of the handle in one launch, the lattice made on the device: member p at
 * its B states host_x[p] ([P][d][B] reals) with the cost-to-go of sdp_family_set_value, the constants of
 * sdp_family_set_params and the box of sdp_family_set_lookahead_box.  host_J [P][B] reals, host_u [P][nu][B] reals,
 * host_idx [P][B]; a state without a valid lattice gives NaN, NaN, -1.  Member p has the bits of
 * sdp_problem_lookahead on problem p alone.  SDP_EINVAL for a NULL pointer, a negative size, no unit loaded, no box
 * set, or values that are not those of sdp_family_set_value.
 */
int sdp_family_lookahead(sdp_family *f, int64_t B, const void *host_x, double t_k, void *host_J, void *host_u,
                         int32_t *host_idx);
/*
 * sdp_problem_montecarlo_lookahead of every member of the handle, together, with one cost-to-go per member (the
 * value array of sdp_family_set_value) for every step: the arguments and results of sdp_family_montecarlo without
 * the policy.  The law the plant draws from is the caller's; the expectation inside the backup runs over the
 * member's own law.  n_outside and the occupancy are zeroed before the first launch; sdp_family_last_kernel_ms
 * covers the call.
 */
int sdp_family_montecarlo_lookahead(sdp_family *f, int64_t B, int64_t T, int64_t n_burn, const uint64_t *host_seeds,
                                    uint64_t traj_offset, const void *host_x0, const double *host_cum, int32_t n_law,
                                    const void *host_law_grid, double t0, int64_t steps_per_launch,
                                    void *host_cost_sum, int64_t *host_n_outside, void *host_x_final,
                                    uint64_t *host_occupancy);

/*
 * Closed loops of a family under lookahead controls over a horizon (csrc/sdp_family_lookahead_horizon_kernel.h).  The
 * family's unit (codegen.family_lookahead_horizon_unit: kernels sdp_family_simulate_lookahead and, for a stochastic
 * family, sdp_family_montecarlo_lookahead_h) is loaded beside the sweep unit; its sdp_meta is checked
 * (SDP_META_F_FAMILY_LOOKAHEAD_HORIZON, the workgroup size, the lanes of a state).  The lanes and the number of box
 * constants are shared with the lookahead unit of the handle: loading a unit that differs in either drops the other.
 * sdp_family_set_lookahead_box is to be called after every load, as for the lookahead unit.
 */
int sdp_family_load_lookahead_horizon_unit(sdp_family *f, const char *module_path);
/*
 * sdp_problem_simulate_lookahead of every member of the handle, together, every lattice made on the device: B
 * trajectories of T >= 1 steps per member.  host_V is [P][V_steps][S] reals: a time-indexed cost-to-go (V_timed != 0,
 * V_steps == T, step k looks ahead into slice k: it goes up a chunk of whole steps of all members at a time, at most
 * chunk_bytes, a larger step a chunk of its own) or one cost-to-go per member (V_timed == 0, V_steps == 1: uploaded
 * once, read with a step stride of 0); the handle's value array is not read.  host_prm is the table of lifted constants
 * [P][T][n_prm] (prm_timed != 0) or [P][1][n_prm] (prm_timed == 0), as in sdp_family_simulate; the box is that of
 * sdp_family_set_lookahead_box, at the time index t0 + k.  host_x0 [P][d][B], host_w [P][T][B] (NULL: a deterministic
 * family); results host_x [P][T+1][d][B], host_u [P][T][nu][B], host_g and host_q [P][T][B] (q: the minimised expected
 * value).  A state without a valid lattice gives NaN controls and q, and the trajectory goes on as the model maps them.
 * Member p of every result has the bits of sdp_problem_simulate_lookahead on problem p alone; no cut changes one.
 * sdp_family_last_kernel_ms covers the call.  SDP_EINVAL for a NULL pointer, a negative size, T < 1, a cost-to-go or
 * table of another length, chunk_bytes < 1, missing perturbation sequences, no unit loaded, or no box set.
 */
int sdp_family_simulate_lookahead(sdp_family *f, const void *host_V, int64_t V_steps, int32_t V_timed,
                                  const void *host_prm, int32_t n_prm, int32_t prm_timed, int64_t chunk_bytes, int64_t B,
                                  int64_t T, const void *host_x0, const void *host_w, double t0, void *host_x,
                                  void *host_u, void *host_g, void *host_q);
/*
 * sdp_problem_montecarlo_lookahead of every member of the handle, together: the arguments and results of
 * sdp_family_montecarlo_lookahead with the cost-to-go and the table of sdp_family_simulate_lookahead.  Launches are cut
 * at the cost-to-go's chunks and at steps_per_launch; the states, the sums, n_outside and the occupancy stay on the
 * device in between.
 */
int sdp_family_montecarlo_lookahead_h(sdp_family *f, const void *host_V, int64_t V_steps, int32_t V_timed,
                                      const void *host_prm, int32_t n_prm, int32_t prm_timed, int64_t chunk_bytes,
                                      int64_t B, int64_t T, int64_t n_burn, const uint64_t *host_seeds,
                                      uint64_t traj_offset, const void *host_x0, const double *host_cum, int32_t n_law,
                                      const void *host_law_grid, double t0, int64_t steps_per_launch,
                                      void *host_cost_sum, int64_t *host_n_outside, void *host_x_final,
                                      uint64_t *host_occupancy);

/* ---- tabulated backup (models that cannot be traced into device code) ------- */
/*
 * Replaces the numeric part of DPSolver._value_at_state_vect
 * (stodynprog.py:677-690) for a batch of nodes whose dyn/cost callbacks were
 * evaluated on the host exactly as stodynprog.py:674,676 does:
 *   cell  = g[cell] + interp(V, x_next[:, cell])          (stodynprog.py:677)
 *   J[c]  = sum_w cell(c,w) * proba[w]  (W == 0: no expectation; 679-683)
 *   idx   = first-occurrence argmin over the node's controls (686)
 * Node n owns cells [cell_off[n], cell_off[n+1]), laid out [control][w].
 * The value array stays on the device between calls.
 */
typedef struct sdp_tab sdp_tab;
int sdp_tab_create(int d, const double *smin, const double *smax, const int64_t *orders,
                   const double *host_V, sdp_tab **out);
int sdp_tab_destroy(sdp_tab *t);
int sdp_tab_backup(sdp_tab *t, int64_t n_nodes, const int64_t *cell_off, int64_t W,
                   const double *proba, const double *x_next /* [d][n_cells] */,
                   const double *g /* [n_cells] */, double *J_out /* [n_nodes] */,
                   int64_t *idx_out /* [n_nodes] */);

/* ---- multi-GPU: one process per GPU, RCCL over xGMI ----------------------------
 * librccl.so is dlopen()ed on first use.  The product library binds librccl and nothing
 * else.  A TEST build of the same source (-DSDP_TEST_HOOKS, made by the test-suite into a
 * file of its own; sdp_test_hooks() returns 1 there, 0 in the product) additionally honours
 * the environment variable SDP_RCCL_LIBRARY: the nccl* entry points are then taken from
 * that shared object (tests/mock_rccl.cpp: a host-staged stand-in that lets several ranks
 * share the ONE GPU of the test box, which RCCL itself refuses).  sdp_comm_library()
 * reports the library the nccl* symbols came from. */
int sdp_test_hooks(void);
int sdp_comm_unique_id(char id[128]);                       /* rank 0 */
int sdp_comm_create(int rank, int nranks, const char id[128], sdp_comm **out);
int sdp_comm_destroy(sdp_comm *c);
const char *sdp_comm_library(void);      /* path/name the nccl* symbols came from, "" if not loaded */
/*
 * Shard the handle's backups over the ranks of `c`.  The node range (device
 * order) is cut into n_phases contiguous phases and every phase into one part
 * per rank: part_bounds[ph*(nranks+1) + r] .. [.. + r + 1] are rank r's nodes of
 * phase ph (whole columns in SDP_LAYOUT_COLUMNS).  Each backup then runs phase by
 * phase; the RCCL all-gather of a phase overlaps the kernel of the next one.
 * The handle must have been created with node range [0, S).
 */
int sdp_problem_attach_comm(sdp_problem *p, sdp_comm *c, int32_t n_phases,
                            const int64_t *part_bounds /* [n_phases][nranks+1] */);
/*
 * Alternative exchange for the sharded backups: every rank maps the other ranks' value / J
 * buffers (HIP IPC) and, phase by phase, WRITES its rows into them with device-to-device
 * copies on one stream per peer -- copy engines over xGMI, no compute units, all links of the
 * fully connected node at once -- instead of an RCCL all-gather per phase.  The writes are
 * one-sided, so two 1-word all-reduces bracket them: one before the first write of an API call
 * (every peer has returned from its previous call, i.e. finished reading its J), one at the end
 * of every backup (all rows have landed everywhere).  Same results.  Collective (all ranks
 * call it, after sdp_problem_attach_comm); on failure the handle keeps the RCCL exchange.
 */
int sdp_problem_enable_peer_exchange(sdp_problem *p);
/*
 * Unmaps the peers' buffers again (the RCCL exchange is back in place).  Local, but when problems are torn down
 * the order matters across the ranks: every rank unmaps, THEN (after a barrier of the caller's) the buffers are
 * freed by sdp_problem_destroy -- memory a peer process still maps must not be freed under it.
 */
int sdp_problem_disable_peer_exchange(sdp_problem *p);
/*
 * Sparse peer exchange (after sdp_problem_enable_peer_exchange): a backup sends a peer only the
 * rows of J that peer READS in its own backups -- for a column q of need_off, the sorted,
 * disjoint node ranges ranges[2k], ranges[2k+1], k in [need_off[q], need_off[q+1]) (whole columns
 * in the column layout; the relative-DP reference node must be in every list).  The host
 * computes them from the model: the cells the trailing next states of a rank's columns fall in.
 * A rank's J is then complete only there; sdp_problem_get_value completes it first (every rank
 * sends all its rows: collective), sdp_problem_backup_host sends all rows to begin with.
 * NULL, NULL switches back to sending everything.
 */
int sdp_problem_set_peer_needs(sdp_problem *p, const int64_t *need_off /* [nranks+1] */,
                               const int64_t *ranges /* [need_off[nranks]][2] */);
/* Sparse peer exchange: make the last backup's J complete on every rank (collective; a no-op
 * otherwise) -- what sdp_problem_get_value does before it downloads. */
int sdp_problem_complete_value(sdp_problem *p);
/*
 * Direct exchange (after sdp_problem_enable_peer_exchange; at most 8 ranks, the GPUs of one node):
 * the backup kernel that computes J[node] also STORES it into the mapped J buffer of every other rank
 * (with need lists set: of the ranks that read the node's column) -- stores over xGMI issued by the
 * kernel itself, spread over the whole sweep, instead of copies after each phase.  Nothing is left to
 * move when the kernel ends: a backup costs ONE launch and ONE 1-word all-reduce (the ranks meet
 * before anybody reads J or overwrites V).  Same results.  The reference has no counterpart (its only
 * parallel attempt is the commented-out Pool.imap over the nodes, stodynprog.py:503-509).
 */
int sdp_problem_set_direct_exchange(sdp_problem *p, int on);
/*
 * Send / receive exchange (an alternative to sdp_problem_enable_peer_exchange; call it BEFORE sdp_problem_set_peer_needs):
 * the sparse exchange through the collective library alone.  After each phase's kernel a rank ncclSends every other
 * rank the bounding range of the rows of that phase the other rank reads, and ncclRecvs its own -- one grouped
 * send / receive per pair of ranks and phase, no buffer of another process mapped, no store into one.  A rank's J is
 * complete where it reads; sdp_problem_complete_value / sdp_problem_get_value run the all-gather of every phase.
 * Without need lists it is the RCCL all-gather.  (The reference's counterpart: none; its loop over the nodes is
 * serial, stodynprog.py:511-515.)
 */
int sdp_problem_set_sendrecv_exchange(sdp_problem *p, int on);
/*
 * Reduced-array sweep (several controlled state variables, csrc/sdp_lead_kernel.h) on a sharded
 * problem: rows of the FIRST state axis the controls of a node reach on either side.  A rank then
 * reduces its own rows plus that many instead of the whole grid.  A guess is enough: a node whose
 * controls reach further is noticed by the kernel and evaluated from the value array itself (time,
 * not correctness).  rows < 0 (default): every rank reduces everything.
 */
int sdp_problem_set_lead_halo(sdp_problem *p, int64_t rows);
int sdp_comm_allreduce_max(sdp_comm *c, double *inout);    /* host scalar, for timing */
int sdp_comm_barrier(sdp_comm *c);

#ifdef __cplusplus
}
#endif
#endif /* SDP_HIP_H */
