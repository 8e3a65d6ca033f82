// sdp_kernel_args.h -- plain-old-data argument blocks shared by the host
// library (sdp_hip.hip) and the device kernels (built-in and generated-model
// code objects).  Passed by value as the single kernel argument.
#pragma once
#include <stdint.h>

#define SDP_MAXD 4   // multilinear_cython.pyx:33-47 dispatches d = 1..4 only

// Every model code object carries `extern "C" __constant__ int32_t sdp_meta[SDP_META_WORDS]`: what it
// was generated for.  sdp_problem_create reads it and refuses (SDP_EMODULE) a problem it does not
// match -- compiled-in table sizes, dtype, dimensions -- instead of launching a kernel that would
// return stale results (the kernels trap on such a launch: sdp_trap_unless).
#define SDP_META_WORDS 16
#define SDP_META_MAGIC 0x33504453      // "SDP3"
enum {
    SDP_META_MAGIC_AT = 0, SDP_META_REAL_BYTES, SDP_META_D, SDP_META_NU, SDP_META_HAS_W,
    SDP_META_LAYOUT,        // 0 node order, 1 columns (axis 0 fastest)
    SDP_META_COL_N0,        // points of axis 0 the column table was sized for (0: node-order unit)
    SDP_META_COL_W,         // perturbation points of the column table (>= 1)
    SDP_META_FLAGS,         // SDP_META_F_*
    SDP_META_UTAB,          // tabulated values per control (0: none)
    SDP_META_UTAB_N,        // controls the control table has room for (the lattice may be shorter)
    SDP_META_THREADS,       // workgroup size of the sweep kernel (column / staged units)
    SDP_META_COL_ROWS,      // rows of axis 0 the table holds (< COL_N0: row window)
    SDP_META_LEAD_AXES,     // SDP_META_F_LEAD units: controlled state variables (the plane-major arrays' "lead" axes)
    SDP_META_LEAD_PERM,     // ... and which state variable logical axis j is (nibble j; stocks first)
    SDP_META_NW             // perturbation variables the model entry takes as a vector (sdp_multiw_kernel.h: 2..4); 0: at most
                            // one, told by SDP_META_HAS_W (every unit of one variable)
};
enum {
    SDP_META_F_FILTER = 1, SDP_META_F_WINDOW = 2, SDP_META_F_TRAIL_HAS_U = 4, SDP_META_F_STAGED = 8,
    SDP_META_F_WPAIR = 16, SDP_META_F_LEAN = 32,
    SDP_META_F_CLAIMS = 64, // the sweep kernel's workgroups claim their units (persistent: a bounded grid)
    SDP_META_F_SHIFT = 128, // certified filter on the shifted lattice (a perturbation that reaches x0')
    SDP_META_F_LEAD = 256,  // node-order sweep with the filter on an array reduced over w (sdp_lead_kernel.h):
                            // the code object also exports sdp_lead_reduce, launched before every sweep
    SDP_META_F_PEER_STORES = 512,  // the backup kernels store J through sdp_store_J (SdpSweepArgs.peer_J: direct exchange)
    SDP_META_F_FAMILY = 1024,      // a family unit (sdp_family_kernel.h): sdp_family_sweep and nothing else
    SDP_META_F_FAMILY_POLICY = 2048,   // a family evaluation unit (sdp_family_policy_kernel.h): sdp_family_evalpol and
                            // sdp_family_evalpol_resident; SDP_META_THREADS is the resident kernel's workgroup size and
                            // SDP_META_COL_ROWS the nodes of a member its two LDS buffers hold
    SDP_META_F_FAMILY_MC = 4096,       // a family Monte Carlo unit (sdp_family_mc_kernel.h): sdp_family_montecarlo and nothing
                            // else; SDP_META_THREADS is its workgroup size, the trajectories of a tile
    SDP_META_F_FAMILY_LOOKAHEAD = 8192 // a family lookahead unit (sdp_family_lookahead_kernel.h): sdp_family_lookahead and
                            // sdp_family_montecarlo_lookahead; SDP_META_THREADS is their workgroup size, SDP_META_COL_ROWS the
                            // lanes of a state (SDP_LANES) and SDP_META_UTAB the constants of the box function per member
    , SDP_META_F_FAMILY_HORIZON = 16384 // a family horizon unit (sdp_family_horizon_kernel.h): sdp_family_simulate and, for a
                            // stochastic family, sdp_family_montecarlo_h; SDP_META_THREADS is the Monte Carlo kernel's
                            // workgroup size and SDP_META_COL_ROWS that of sdp_family_simulate
    , SDP_META_F_FAMILY_TRANS = 32768   // a family transition unit (sdp_family_trans_kernel.h): sdp_family_transitions and
                            // nothing else; SDP_META_THREADS is its workgroup size and SDP_META_COL_ROWS the nodes of a tile
    , SDP_META_F_FAMILY_LOOKAHEAD_HORIZON = 65536   // a family lookahead unit over a horizon (sdp_family_lookahead_horizon_kernel.h):
                            // sdp_family_simulate_lookahead and, for a stochastic family, sdp_family_montecarlo_lookahead_h;
                            // SDP_META_THREADS, SDP_META_COL_ROWS and SDP_META_UTAB as in a family lookahead unit
};
#define SDP_MAX_PEERS 8     // ranks of a direct exchange: the GPUs of one node
#define SDP_MAXU 4   // control variables per system

// One Bellman backup over a contiguous range of state nodes
// (reference stodynprog.py:466-534 + 639-691).
struct SdpSweepArgs {
    const void *V;         // [S] cost-to-go J_next, C-order, last axis fastest
    void *J;               // [S] output J_k (only nodes in [node_begin,node_end) written)
    void *pol;             // [S*nu] output optimal control VALUES (may be null)
    int32_t *idx;          // [S] output flat C-order index into the control lattice (may be null)
    const void *axes;      // concatenated state-grid axes (reals); axis k at axis_off[k]
    const void *wgrid;     // [W] perturbation grid (null when W == 0); several variables: [m][W], row i = variable i on the flat law
    const void *proba;     // [W] perturbation weights
    const void *box_lo;    // control box lower ends: [nu] or [nu][S] (per node)
    const void *box_hi;    // control box upper ends
    const int32_t *box_n;  // number of control points: [nu] or [nu][S]
    const void *pol_in;    // [S*nu] prescribed policy (eval_policy kernel only)
    int64_t node_begin;    // first node of this launch (flat C-order id)
    int64_t node_end;      // one past the last node
    int64_t S;             // total number of state nodes
    double t_k;            // time index for non-stationary systems
    int32_t orders[SDP_MAXD];
    int32_t axis_off[SDP_MAXD];
    int32_t W;             // perturbation points (0: deterministic system)
    int32_t box_per_node;  // 0: constant box, 1: per-node arrays
    // ---- column layout only (sdp_column_kernel.h) ----------------------------
    // Arrays over nodes (V, J, pol, idx, box_*, pol_in) are then stored with the
    // LEADING state axis fastest: element (c, i) at c*n_lead + i, c = C-order
    // index over axes 1..d-1 ("column"), i = index along axis 0.
    int64_t col_begin;     // first column of this launch
    int64_t col_end;       // one past the last column
    int32_t n_lead;        // orders[0]
    int32_t col_splits;    // workgroups sharing one column (each redoes the table)
    // ---- policy-evaluation kernels only: fused relative-DP shift ------------------
    int64_t shift_index;   // >= 0: every V read is V[.] - V[shift_index] (device order); -1: none
    double *ref_out;       // if set, thread 0 of workgroup 0 stores V[shift_index] there (J_ref of the previous step)
    // ---- diagnostic builds only (SDP_STAMP code objects; null in production) ----
    // [gridDim.x][4] words: s_memtime / s_memrealtime of thread 0 at kernel entry and exit
    // (in-kernel clock = d memtime / d memrealtime x 100 MHz, MI355X_MICROARCH.md DVFS item 6)
    unsigned long long *stamps;
    // ---- filtered column kernel: units handed out in order (sdp_column_kernel.h) ----
    // claim[32 * k], k = 0..7: next unit of XCD k's share (relative); claim[256]: workgroups that
    // have finished (the last one zeroes everything for the next launch).  Zero before the first launch.
    unsigned int *claim;
    // ---- several controlled state variables (sdp_lead_kernel.h): the array reduced over w, in node order ----
    void *aux_a;           // [S] A = sum_w p_w inner_w, plane-major, written by sdp_lead_reduce, read by sdp_sweep
    void *aux_v;           // [S] copy of V, plane-major (the second pass reads it)
    void *aux_e;           // [nodes per block of trailing coordinates] bound factor of the trailing cells
    unsigned long long *aux_vmax;   // bits of max |V| as a double (zero before sdp_lead_reduce)
    int64_t aux_begin;     // plane-major arrays: lead indices [aux_begin, aux_end) hold valid values (the part of the
    int64_t aux_end;       //   grid sdp_lead_reduce was run on); a node whose controls reach outside takes the long way on V
    // ---- direct exchange (several GPUs, sdp_problem_set_direct_exchange): the kernel that computes J[node] also
    // stores it into the J buffers of the other ranks, mapped into this process (HIP IPC; xGMI stores) ----
    void *peer_J[SDP_MAX_PEERS];        // null: no store (this rank itself, ranks beyond the communicator)
    const unsigned char *peer_mask;     // column layout: [columns] bit q set = rank q reads the column; null: every peer gets every node
    int32_t n_peer;                     // 0: single GPU or another exchange -- no peer stores at all
    int32_t pad_;
    void *reserve_;                     // not used (zero): the implicit kernel arguments behind the struct keep their offsets
};

// One Bellman backup of a FAMILY of same-shaped problems (sdp_family_kernel.h, kernel `sdp_family_sweep`): the
// backup of SdpSweepArgs with a member index in front of every array.  Members share the grid's shape, the number
// of controls and of perturbation points and the model's structure; each has its own constants, grid ends, law
// and box table.  A launch runs the members listed in `members`, whole.
struct SdpFamilyArgs {
    const void *V;         // [P][S] cost-to-go J_next of every member, C order
    void *J;               // [P][S] output J_k (only the slices of the listed members are written)
    void *pol;             // [P][S][nu] output optimal control VALUES (may be null)
    int32_t *idx;          // [P][S] output flat C-order index into the member's control lattice (may be null)
    const void *axes;      // [P][n_axes] concatenated state-grid axes of every member; axis k at axis_off[k]
    const void *wgrid;     // [P][W] perturbation grids (null when W == 0)
    const void *proba;     // [P][W] perturbation weights
    const void *prm;       // [P][SDP_NPARAMS] lifted constants, row p for member p (sdp_model_cell_at)
    const void *box_lo;    // control box lower ends: [P][nu] or [P][nu][S] (per node)
    const void *box_hi;    // control box upper ends
    const int32_t *box_n;  // number of control points: [P][nu] or [P][nu][S]
    const int32_t *members;// [n_active] the members this launch runs (distinct, each < P)
    int64_t S;             // state nodes of one member
    double t_k;            // time index for non-stationary systems
    int32_t orders[SDP_MAXD];
    int32_t axis_off[SDP_MAXD];
    int32_t n_axes;        // sum of orders: reals per row of `axes`
    int32_t W;             // perturbation points (0: deterministic systems)
    int32_t box_per_node;  // 0: one box per member, 1: per-node arrays
    int32_t n_active;      // members listed (>= 1)
};

// Fixed-policy backups of a family (sdp_family_policy_kernel.h).  `f` is the block of the sweep with `f.pol` the
// PRESCRIBED policy [P][S][nu] (read, not written) and the box arrays and `f.idx` unused (null).
// Kernel `sdp_family_evalpol` runs one step of the listed members, f.V -> f.J: with `shift` every vertex of member p
// is read as V - V[p][ref_index] (the relative shift of the previous step, SdpLerp<.., SHIFT>) and that value is
// stored in refs[slot][p].
// Kernel `sdp_family_evalpol_resident` runs ALL steps of a listed member in one workgroup, the values in LDS: it
// starts from f.V, writes the result (shifted once more with rel_dp) to f.J, the reference cost of step k to
// refs[k][p], the steps run to n_done[p] and, with check_every > 0, dmin / dmax of every check the member ran to
// stats[check][p][0..1] (it stops at the first check with dmax - dmin <= tol; a NaN never converges).
struct SdpFamilyEvalArgs {
    SdpFamilyArgs f;
    int64_t ref_index;     // node of the relative shift (only read with shift / rel_dp)
    double *refs;          // [rows][P] reference costs (may be null without shift / rel_dp)
    int32_t P;             // members of the family: the row length of refs, n_done and stats
    int32_t shift;         // evalpol: 1 = read V - V[ref_index] and store V[ref_index] to refs[slot]
    int32_t slot;
    // ---- resident kernel only ----
    int32_t rel_dp;
    int32_t n_iter;        // steps (at most, with a check)
    int32_t check_every;   // 0: no check; else after steps c, 2c, .. and after step n_iter
    double tol;
    int32_t *n_done;       // [P]
    double *stats;         // [checks][P][2] (null without a check)
};

// Monte Carlo policy evaluation of a family (sdp_family_mc_kernel.h, kernel `sdp_family_montecarlo`): SdpMcArgs with
// a member index in front of every array.  Every member runs the same B trajectory ids over the same steps, each
// with its own policy, constants, grid ends, seed and law (all laws have n_law points).  A launch runs the steps
// [step_begin, step_end) of all P members and leaves the states and the sums in the buffers.
struct SdpFamilyMcArgs {
    const void *pol;       // [P][nu][S] policies (control VALUES on the state grid), control axis first
    const void *axes;      // [P][n_axes] concatenated state-grid axes of every member; axis k at axis_off[k]
    const void *prm;       // [P][SDP_NPARAMS] lifted constants, row p for member p (sdp_model_cell_at)
    const double *cum;     // [P][n_law] float64 running sums of the laws' probabilities (the last entry is not read)
    const void *law_grid;  // [P][n_law] perturbation values (reals)
    const uint64_t *seed;  // [P] Philox keys
    void *x;               // [P][d][B] states: x at step_begin in, x at step_end out
    void *acc;             // [P][B] running cost sums (reals)
    long long *n_outside;  // [P][B] steps k >= n_burn whose x_k lies outside the member's state grid or is NaN
    unsigned long long *occupancy;   // [P][S] visits of the node nearest to x_k, k >= n_burn (null: not counted)
    int64_t B;             // trajectories of one member
    int64_t S;             // state nodes of one member
    uint64_t traj_offset;  // id of row 0 (Philox counter words 0 and 1 hold traj_offset + row)
    int64_t step_begin;    // absolute step index (Philox counter words 2 and 3) of this launch's first step
    int64_t step_end;      // one past its last step
    int64_t n_burn;        // steps before this one advance the state only
    double t0;             // time index of step 0 (non-stationary systems)
    int32_t n_law;         // points of every law (>= 1)
    int32_t n_axes;        // sum of orders: reals per row of `axes`
    int32_t P;             // members (>= 1): all of them run
    int32_t pad_;
    int32_t orders[SDP_MAXD];
    int32_t axis_off[SDP_MAXD];
};

// One-step lookahead at arbitrary states for a family (sdp_family_lookahead_kernel.h, kernel `sdp_family_lookahead`):
// SdpLookArgs with a member index in front of every array and the lattice always made on the device, by the unit's
// `sdp_model_box_at` on the member's row of box constants.  `f` is the block of the sweep with `f.V` the cost-to-go
// J_next [P][S]; its box arrays, `f.J`, `f.pol`, `f.idx` and `f.members` are unused (null) and `f.n_active` is P: all
// members run, each on its own B states.
struct SdpFamilyLookArgs {
    SdpFamilyArgs f;
    const double *bprm;    // [P][SDP_NBOXPARAMS] constants of the box function, row p for member p (float64 whatever the reals)
    const double *steps;   // [P][nu] control step hints (DPSolver.control_steps of every member)
    const void *x;         // [P][d][B] states
    void *J;               // [P][B] minimised expected value
    int32_t *idx;          // [P][B] flat C-order index of the optimal control in the state's lattice
    void *u;               // [P][nu][B] optimal control VALUES
    int64_t B;             // states of one member
};

// Monte Carlo evaluation under lookahead controls for a family (kernel `sdp_family_montecarlo_lookahead`): SdpLookMcArgs
// with a member index in front of every array, one cost-to-go per member for every step.  The law the backup sums
// over (f.wgrid, f.proba) is the member's own; the law the plant draws from (cum, law_grid) is the caller's.
struct SdpFamilyLookMcArgs {
    SdpFamilyArgs f;       // as SdpFamilyLookArgs (f.t_k is not read: the time index of step k is t0 + k)
    const double *bprm;    // [P][SDP_NBOXPARAMS]
    const double *steps;   // [P][nu]
    const double *cum;     // [P][n_law] float64 running sums of the drawn laws' probabilities (the last entry is not read)
    const void *law_grid;  // [P][n_law] drawn perturbation values (reals)
    const uint64_t *seed;  // [P] Philox keys
    void *x;               // [P][d][B] states: x at step_begin in, x at step_end out
    void *acc;             // [P][B] running cost sums (reals)
    long long *n_outside;  // [P][B] steps k >= n_burn whose x_k lies outside the member's state grid or is NaN
    unsigned long long *occupancy;   // [P][S] visits of the node nearest to x_k, k >= n_burn (null: not counted)
    int64_t B;             // trajectories of one member
    uint64_t traj_offset;  // id of row 0 (Philox counter words 0 and 1 hold traj_offset + row)
    int64_t step_begin;    // step of the call (Philox counter words 2 and 3) of this launch's first step
    int64_t step_end;      // one past its last step
    int64_t n_burn;        // steps before this one advance the state only
    double t0;             // time index of step 0 of the call
    int32_t n_law;         // points of every drawn law (>= 1)
    int32_t pad_;
};

// Closed loops of a family over a horizon (sdp_family_horizon_kernel.h): SdpSimHArgs and SdpMcHArgs with a member index
// in front of every array.  The policy and the table of constants are addressed by two strides each, in reals: member p
// at step k of the call reads the policy slice pol + p * pol_member_stride + (k - chunk_first) * pol_step_stride and the
// row prm + p * prm_member_stride + k * prm_step_stride.  A step stride of 0 is one slice (a stationary policy) or one
// row (a model that is symbolic in time) for every step.
struct SdpFamilySimHArgs {
    const void *pol;       // [P][steps of this launch's chunk, or 1][nu][S]
    const void *prm;       // [P][steps of the call, or 1][SDP_NPARAMS]
    const void *axes;      // [P][n_axes] concatenated state-grid axes of every member; axis k at axis_off[k]
    const void *w;         // [P][T][B] perturbation sequences of the whole call (null: deterministic members)
    void *x;               // [P][T+1][d][B] states of the whole call: row step_begin read, rows step_begin + 1 .. step_end written
    void *u;               // [P][T][nu][B] controls applied
    void *g;               // [P][T][B] instantaneous costs
    int64_t B;             // trajectories of one member
    int64_t S;             // state nodes of one member
    int64_t T;             // steps of the whole call
    int64_t pol_member_stride, pol_step_stride;
    int64_t prm_member_stride, prm_step_stride;
    int64_t step_begin;    // first step of this launch (step of the call)
    int64_t step_end;      // one past its last step
    int64_t chunk_first;   // step of the call whose policy slice is the member's first on the device
    double t0;             // time index of step 0 of the call
    int32_t n_axes;        // sum of orders: reals per row of `axes`
    int32_t P;             // members (>= 1): all of them run
    int32_t orders[SDP_MAXD];
    int32_t axis_off[SDP_MAXD];
};

struct SdpFamilyMcHArgs {
    const void *pol;       // as SdpFamilySimHArgs
    const void *prm;
    const void *axes;
    const double *cum;     // as SdpFamilyMcArgs from here on
    const void *law_grid;
    const uint64_t *seed;
    void *x;
    void *acc;
    long long *n_outside;
    unsigned long long *occupancy;
    int64_t B;
    int64_t S;
    int64_t pol_member_stride, pol_step_stride;
    int64_t prm_member_stride, prm_step_stride;
    uint64_t traj_offset;
    int64_t step_begin;
    int64_t step_end;
    int64_t n_burn;
    int64_t chunk_first;   // step of the call whose policy slice is the member's first on the device
    double t0;
    int32_t n_law;
    int32_t n_axes;
    int32_t P;
    int32_t pad_;
    int32_t orders[SDP_MAXD];
    int32_t axis_off[SDP_MAXD];
};

// Closed loops of a family under lookahead controls over a horizon (sdp_family_lookahead_horizon_kernel.h): SdpLookSimArgs
// and SdpLookMcArgs with a member index in front of every array.  `f` is the block of SdpFamilyLookArgs, but `f.V` and
// `f.prm` are the bases of two tables addressed by two strides each, in reals, as in SdpFamilySimHArgs: member p at step k
// of the call looks ahead into the cost-to-go V + p * V_member_stride + (k - chunk_first) * V_step_stride and runs on the
// row prm + p * prm_member_stride + k * prm_step_stride.  A step stride of 0 is one slice (one cost-to-go for every step)
// or one row (a model that is symbolic in time) for every step.  `f.t_k` is not read: the time index of step k is t0 + k.
struct SdpFamilyLookSimArgs {
    SdpFamilyArgs f;       // f.V [P][steps of this launch's chunk, or 1][S]; f.prm [P][steps of the call, or 1][SDP_NPARAMS]
    const double *bprm;    // [P][SDP_NBOXPARAMS] constants of the box function, row p for member p
    const double *steps;   // [P][nu] control step hints
    const void *w;         // [P][T][B] perturbation sequences of the whole call (null: deterministic members)
    void *x;               // [P][T+1][d][B] states of the whole call: row step_begin read, rows step_begin + 1 .. step_end written
    void *u;               // [P][T][nu][B] controls applied
    void *g;               // [P][T][B] instantaneous costs
    void *q;               // [P][T][B] minimised expected values
    int64_t B;             // trajectories of one member
    int64_t T;             // steps of the whole call
    int64_t V_member_stride, V_step_stride;
    int64_t prm_member_stride, prm_step_stride;
    int64_t step_begin;    // first step of this launch (step of the call)
    int64_t step_end;      // one past its last step
    int64_t chunk_first;   // step of the call whose cost-to-go slice is the member's first on the device
    double t0;             // time index of step 0 of the call
};

struct SdpFamilyLookMcHArgs {
    SdpFamilyArgs f;       // as SdpFamilyLookSimArgs
    const double *bprm;    // as SdpFamilyLookMcArgs from here on
    const double *steps;
    const double *cum;
    const void *law_grid;
    const uint64_t *seed;
    void *x;
    void *acc;
    long long *n_outside;
    unsigned long long *occupancy;
    int64_t B;
    uint64_t traj_offset;
    int64_t step_begin;
    int64_t step_end;
    int64_t n_burn;
    double t0;
    int64_t V_member_stride, V_step_stride;
    int64_t prm_member_stride, prm_step_stride;
    int64_t chunk_first;   // step of the call whose cost-to-go slice is the member's first on the device
    int32_t n_law;
    int32_t pad_;
};

// Batched closed-loop simulation (the user loop of the reference's examples, e.g.
// examples/20 Searev storage control/storage_control.py:242-251): per step the
// policy is looked up by multilinear interpolation and the dynamics advance.
struct SdpSimArgs {
    const void *pol;       // [nu][S] policy (control VALUES on the state grid), C order
    const void *axes;      // concatenated state-grid axes, like SdpSweepArgs
    const void *x0;        // [d][B] start states
    const void *w;         // [T][B] perturbation sequences (null: deterministic system); several variables: [T][m][B]
    void *x;               // [T+1][d][B] states (x[0] = x0)
    void *u;               // [T][nu][B] controls applied
    void *g;               // [T][B] instantaneous costs (may be null)
    int64_t B;             // trajectories
    int64_t T;             // steps
    int64_t S;             // state nodes
    double t0;             // time index of step 0 (non-stationary systems)
    int32_t orders[SDP_MAXD];
    int32_t axis_off[SDP_MAXD];
};

// Monte Carlo policy evaluation (sdp_mc_kernel.h): the same closed loop with the perturbation drawn on
// the device (Philox4x32-10 keyed by the seed, counter = trajectory id and absolute step) and reduced
// per trajectory; one launch runs the steps [step_begin, step_end) and leaves the state in the buffers.
struct SdpMcArgs {
    const void *pol;       // [nu][S] policy, like SdpSimArgs
    const void *axes;      // concatenated state-grid axes
    const double *cum;     // [n_law] float64 running sum of the law's probabilities (the last entry is not read)
    const void *law_grid;  // [n_law] perturbation values (reals); several variables: [m][n_law]
    void *x;               // [d][B] states: x at step_begin in, x at step_end out
    void *acc;             // [B] running cost sums (reals)
    long long *n_outside;  // [B] steps k >= n_burn whose x_k lies outside the state grid or is NaN
    unsigned long long *occupancy;   // [S] visits of the node nearest to x_k, k >= n_burn (null: not counted)
    int64_t B;             // trajectories
    int64_t S;             // state nodes
    uint64_t seed;         // Philox key
    uint64_t traj_offset;  // id of row 0 (Philox counter words 0 and 1 hold traj_offset + row)
    int64_t step_begin;    // absolute step index (Philox counter words 2 and 3) of this launch's first step
    int64_t step_end;      // one past its last step
    int64_t n_burn;        // steps before this one advance the state only
    double t0;             // time index of step 0 (non-stationary systems)
    int32_t n_law;         // points of the law (>= 1)
    int32_t pad_;
    int32_t orders[SDP_MAXD];
    int32_t axis_off[SDP_MAXD];
};

// The same two loops under a TIME-INDEXED policy (sdp_horizon_kernel.h: kernels `sdp_simulate_h` and
// `sdp_montecarlo_h`): step k of the call looks its controls up in slice k of the policy and, in a unit with
// lifted constants, evaluates the model with row k of a table of them.  A launch runs the steps
// [step_begin, step_end) of the call with the policy slices of a chunk [chunk_first, ..) on the device.
struct SdpSimHArgs {
    const void *pol;       // [steps of this launch's chunk][nu][S]: step k reads slice k - chunk_first
    const void *prm;       // [steps of the call][SDP_NPARAMS] lifted constants, row k for step k (null: none)
    const void *axes;      // concatenated state-grid axes, like SdpSweepArgs
    const void *w;         // [T][B] perturbation sequences of the whole call (null: deterministic); several variables: [T][m][B]
    void *x;               // [T+1][d][B] states of the whole call: row step_begin read (row 0 = x0, put there by the host), rows step_begin + 1 .. step_end written
    void *u;               // [T][nu][B] controls applied
    void *g;               // [T][B] instantaneous costs (may be null)
    int64_t B;             // trajectories
    int64_t S;             // state nodes
    int64_t step_begin;    // first step of this launch (step of the call)
    int64_t step_end;      // one past its last step
    int64_t chunk_first;   // step of the call whose policy slice is pol[0]
    double t0;             // time index of step 0 of the call
    int32_t orders[SDP_MAXD];
    int32_t axis_off[SDP_MAXD];
};

struct SdpMcHArgs {
    const void *pol;       // [steps of this launch's chunk][nu][S], like SdpSimHArgs
    const void *prm;       // [steps of the call][SDP_NPARAMS], like SdpSimHArgs (null: none)
    const void *axes;      // concatenated state-grid axes
    const double *cum;     // as SdpMcArgs from here on
    const void *law_grid;
    void *x;
    void *acc;
    long long *n_outside;
    unsigned long long *occupancy;
    int64_t B;
    int64_t S;
    uint64_t seed;
    uint64_t traj_offset;
    int64_t step_begin;
    int64_t step_end;
    int64_t n_burn;
    int64_t chunk_first;   // step of the call whose policy slice is pol[0]
    double t0;
    int32_t n_law;
    int32_t pad_;
    int32_t orders[SDP_MAXD];
    int32_t axis_off[SDP_MAXD];
};

// Entries of the transition operator of a policy (sdp_trans_kernel.h): per node s (flat C-order id), point j of
// the flat law and vertex v of the interpolation cell of the next state, the target node and the weight at
// position (s W + j) 2^d + v, and the mean cost of every node.
struct SdpTransArgs {
    const void *pol;       // [S][nu] policy (control VALUES at the nodes), C order whatever the unit's layout
    const void *axes;      // concatenated state-grid axes, like SdpSweepArgs
    const void *wtab;      // [W] perturbation values; several variables: [m][W]; not read by a deterministic unit
    const void *proba;     // [W] weights of the flat law (a deterministic system: the one weight 1)
    int32_t *tgt;          // [S W 2^d] target nodes, flat C-order ids
    void *val;             // [S W 2^d] weights (reals)
    void *gbar;            // [S] mean cost of one step under the policy (reals)
    int64_t S;             // state nodes
    double t_k;            // time index (non-stationary systems)
    int32_t W;             // points of the flat law (>= 1)
    int32_t pad_;
    int32_t orders[SDP_MAXD];
    int32_t axis_off[SDP_MAXD];
};

// Entries of the transition operators of the steps of a horizon (sdp_trans_horizon_kernel.h, kernel `sdp_transitions_h`):
// SdpTransArgs with a step index in front of every array.  Step k of the call reads slice k - chunk_first of the policy
// and, in a unit with lifted constants, row k of a table of them; its time index is t0 + k.  The operators form ONE
// block-diagonal operator: node s of step k is row (k - step_begin) S + s.
struct SdpTransHArgs {
    const void *pol;       // [steps of this launch's chunk][nu][S], control axis first: step k reads slice k - chunk_first
    const void *prm;       // [steps of the call][SDP_NPARAMS] lifted constants, row k for step k (null: none)
    const void *axes;      // concatenated state-grid axes, like SdpSweepArgs
    const void *wtab;      // as SdpTransArgs
    const void *proba;
    int32_t *tgt;          // [step_end - step_begin][S W 2^d] target rows, (k - step_begin) S + node
    void *val;             // [step_end - step_begin][S W 2^d] weights (reals)
    void *gbar;            // [step_end - step_begin][S] mean cost of step k under its policy slice (reals)
    int64_t S;             // state nodes
    int64_t step_begin;    // first step of this launch (step of the call)
    int64_t step_end;      // one past its last step
    int64_t chunk_first;   // step of the call whose policy slice is pol[0]
    double t0;             // time index of step 0 of the call
    int32_t W;             // points of the flat law (>= 1)
    int32_t pad_;
    int32_t orders[SDP_MAXD];
    int32_t axis_off[SDP_MAXD];
};

// Entries of the transition operators of a family's policies (sdp_family_trans_kernel.h, kernel
// `sdp_family_transitions`): SdpTransArgs with a member index in front of every array.  `f` is the block of the sweep
// with `f.pol` the PRESCRIBED policies [P][S][nu] (read, not written); `f.V`, `f.J`, `f.idx`, the box arrays and
// `f.members` are unused (null) and `f.n_active` is P: all members run.  A deterministic family has f.W = 0 and
// `f.proba` the one weight 1, which every member reads.  The operators form ONE block-diagonal operator: member p's
// node s is row p S + s.
struct SdpFamilyTransArgs {
    SdpFamilyArgs f;
    int32_t *tgt;          // [P][S W 2^d] target rows, p S + node
    void *val;             // [P][S W 2^d] weights (reals)
    void *gbar;            // [P][S] mean cost of one step under the member's policy (reals)
    int32_t W;             // points of every member's flat law (>= 1: f.W, or 1 for a deterministic family)
    int32_t pad_;
};

// One-step lookahead at arbitrary states (sdp_lookahead_kernel.h, kernel `sdp_lookahead` of a lookahead unit): the
// backup of SdpSweepArgs with the node replaced by state b of a batch, its control lattice made by the host.
struct SdpLookArgs {
    const void *V;         // [S] cost-to-go J_next, C order
    const void *axes;      // concatenated state-grid axes, like SdpSweepArgs
    const void *wgrid;     // [W] perturbation grid (null when W == 0); several variables: [m][W]
    const void *proba;     // [W] perturbation weights
    const void *x;         // [d][B] states
    const void *box_lo;    // [nu][B] control lattice of every state: lower ends (the centre where n == 1)
    const void *box_hi;    // [nu][B] upper ends
    const int32_t *box_n;  // [nu][B] points; n[0][b] == 0: state b has no valid lattice (J and u NaN, idx -1).  Null: the unit's
                           //   own box function (SDP_LOOKAHEAD_BOX) and `steps` make the lattice on the device
    void *J;               // [B] minimised expected value
    int32_t *idx;          // [B] flat C-order index of the optimal control in the state's lattice
    void *u;               // [nu][B] optimal control VALUES
    int64_t B;             // states
    int64_t S;             // state nodes
    double t_k;            // time index for non-stationary systems
    double steps[SDP_MAXU];// control step hints (DPSolver.control_steps): read with a device-made lattice only
    int32_t orders[SDP_MAXD];
    int32_t axis_off[SDP_MAXD];
    int32_t W;             // perturbation points (0: deterministic system)
    int32_t pad_;
};

// The closed loop under lookahead controls (kernel `sdp_simulate_lookahead`, units with SDP_LOOKAHEAD_BOX): per
// step the backup at the carried state, then the model's own step at the optimal control.  A launch runs the steps
// [step_begin, step_end) of the call with the cost-to-go slices of a chunk [chunk_first, ..) on the device.
struct SdpLookSimArgs {
    const void *V;         // [S] one cost-to-go for every step (V_stride == 0), or [steps of the chunk][S]: step k reads slice k - chunk_first
    const void *axes;      // concatenated state-grid axes, like SdpSweepArgs
    const void *wgrid;     // the law the backup sums over, as SdpLookArgs
    const void *proba;
    const void *w;         // [T][B] perturbation sequences of the whole call (null: deterministic); several variables: [T][m][B]
    void *x;               // [T+1][d][B] states of the whole call: row step_begin read, rows step_begin + 1 .. step_end written
    void *u;               // [T][nu][B] controls applied
    void *g;               // [T][B] instantaneous costs
    void *q;               // [T][B] minimised expected values
    int64_t B;             // trajectories
    int64_t S;             // state nodes
    int64_t V_stride;      // 0, or S (a time-indexed cost-to-go)
    int64_t step_begin;    // first step of this launch (step of the call)
    int64_t step_end;      // one past its last step
    int64_t chunk_first;   // step of the call whose cost-to-go slice is V[0]
    double t0;             // time index of step 0 of the call
    double steps[SDP_MAXU];// control step hints
    int32_t orders[SDP_MAXD];
    int32_t axis_off[SDP_MAXD];
    int32_t W;
    int32_t pad_;
};

// Monte Carlo evaluation under lookahead controls (kernel `sdp_montecarlo_lookahead`, units with SDP_LOOKAHEAD_BOX
// of a stochastic system): the closed loop of SdpLookSimArgs with the perturbation of every step DRAWN as
// `sdp_montecarlo` draws it and only the reductions of SdpMcArgs kept.  The law the backup sums over (wgrid, proba)
// is the solver's own; the law the plant draws from (cum, law_grid) is the caller's.
struct SdpLookMcArgs {
    const void *V;         // [S] one cost-to-go for every step (V_stride == 0), or [steps of the chunk][S]: step k reads slice k - chunk_first
    const void *axes;      // concatenated state-grid axes, like SdpSweepArgs
    const void *wgrid;     // the law the backup sums over, as SdpLookArgs
    const void *proba;
    const double *cum;     // [n_law] float64 running sum of the drawn law's probabilities (the last entry is not read)
    const void *law_grid;  // [n_law] drawn perturbation values (reals); several variables: [m][n_law]
    void *x;               // [d][B] states: x at step_begin in, x at step_end out
    void *acc;             // [B] running cost sums (reals)
    long long *n_outside;  // [B] steps k >= n_burn whose x_k lies outside the state grid or is NaN
    unsigned long long *occupancy;   // [S] visits of the node nearest to x_k, k >= n_burn (null: not counted)
    int64_t B;             // trajectories
    int64_t S;             // state nodes
    int64_t V_stride;      // 0, or S (a time-indexed cost-to-go)
    uint64_t seed;         // Philox key
    uint64_t traj_offset;  // id of row 0 (Philox counter words 0 and 1 hold traj_offset + row)
    int64_t step_begin;    // step of the call (Philox counter words 2 and 3) of this launch's first step
    int64_t step_end;      // one past its last step
    int64_t n_burn;        // steps before this one advance the state only
    int64_t chunk_first;   // step of the call whose cost-to-go slice is V[0]
    double t0;             // time index of step 0 of the call
    double steps[SDP_MAXU];// control step hints
    int32_t orders[SDP_MAXD];
    int32_t axis_off[SDP_MAXD];
    int32_t W;             // points of the law the backup sums over
    int32_t n_law;         // points of the drawn law (>= 1)
};

// Stand-alone multilinear interpolation (multilinear_cython.pyx:17-49).
struct SdpInterpArgs {
    const void *values;    // [n_v][S]
    const void *s;         // [d][n_s] query coordinates
    void *out;             // [n_v][n_s]
    int64_t n_s;
    int64_t S;
    int32_t n_v;
    int32_t d;
    int32_t orders[SDP_MAXD];
    double smin[SDP_MAXD]; // converted to the kernel's real type on device
    double smax[SDP_MAXD];
};

// Tabulated backup: the model callbacks were evaluated on the host
// (stodynprog.py:674,676); the device does gather + expectation + argmin.
struct SdpTabArgs {
    const void *V;          // [S]
    const void *x_next;     // [d][n_cells]
    const void *g;          // [n_cells]
    const int64_t *cell_off;// [n_nodes+1] first cell of each node
    const void *proba;      // [W]
    void *J;                // [n_nodes]
    int32_t *idx;           // [n_nodes]
    int64_t n_nodes;
    int64_t n_cells;
    int32_t W;
    int32_t d;
    int32_t orders[SDP_MAXD];
    double smin[SDP_MAXD];
    double smax[SDP_MAXD];
};
