// sdp_hip.hip -- libsdp_hip.so: C ABI (include/sdp_hip.h) + built-in gfx950
// kernels (stand-alone multilinear interpolation, tabulated backup,
// relative-DP shift) + launch of the generated-model code objects + RCCL glue.
// Plain HIP runtime; no PyTorch, no CUDA compatibility layer.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <unistd.h>
#include <string.h>
#include <memory>
#include <mutex>
#include <string>
#include <vector>
#include <algorithm>
#include <utility>

#include <rocprim/rocprim.hpp>

#include "../../include/sdp_hip.h"
#include "sdp_device.h"

// ---------------------------------------------------------------------------
// error plumbing
// ---------------------------------------------------------------------------
static thread_local char g_err[1024] = "";

static int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                  \
    do {                                                                               \
        hipError_t e__ = (expr);                                                       \
        if (e__ != hipSuccess)                                                         \
            return fail(e__ == hipErrorOutOfMemory ? SDP_ENOMEM : SDP_EHIP,            \
                        "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__),        \
                        __FILE__, __LINE__);                                           \
    } while (0)

extern "C" const char *sdp_last_error(void) { return g_err; }

static size_t real_size(int dtype) { return dtype == SDP_F32 ? 4 : 8; }

// ---------------------------------------------------------------------------
// device
// ---------------------------------------------------------------------------
extern "C" int sdp_device_count(int *count)
{
    if (!count) return fail(SDP_EINVAL, "count is NULL");
    hipError_t e = hipGetDeviceCount(count);
    if (e != hipSuccess) { *count = 0; return fail(SDP_EHIP, "hipGetDeviceCount: %s", hipGetErrorString(e)); }
    return SDP_OK;
}

extern "C" int sdp_set_device(int device)
{
    HIP_TRY(hipSetDevice(device));
    return SDP_OK;
}

extern "C" int sdp_device_info(int device, char *name, int *compute_units, int64_t *hbm_bytes,
                               char *gcn_arch)
{
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (name) { strncpy(name, prop.name, 255); name[255] = 0; }
    if (compute_units) *compute_units = prop.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = (int64_t)prop.totalGlobalMem;
    if (gcn_arch) { strncpy(gcn_arch, prop.gcnArchName, 63); gcn_arch[63] = 0; }
    return SDP_OK;
}

extern "C" int sdp_synchronize(void)
{
    HIP_TRY(hipDeviceSynchronize());
    return SDP_OK;
}

static int device_cus()
{
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess)
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    return cus > 0 ? cus : 256;
}

// ---------------------------------------------------------------------------
// built-in kernel: stand-alone multilinear interpolation
// (multilinear_cython.pyx:17-49 dispatcher, 51-300 point kernels).
// One lane per query point: the d coordinate rows s[k][i] are read coalesced,
// the 2^d vertex gathers go through L1/L2, the value rows are looped in-lane
// so the cell location is computed once per point.
// ---------------------------------------------------------------------------
template <typename real, int D>
__global__ void __launch_bounds__(256) k_mlinterp(SdpInterpArgs a)
{
    SdpGrid<real, D> grid;
    real smin[D], smax[D];
#pragma unroll
    for (int k = 0; k < D; ++k) { smin[k] = (real)a.smin[k]; smax[k] = (real)a.smax[k]; }
    sdp_make_grid<real, D>(grid, a.orders, smin, smax);
    const real *__restrict__ s = (const real *)a.s;
    const real *__restrict__ values = (const real *)a.values;
    real *__restrict__ out = (real *)a.out;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n_s; i += stride) {
        SdpCell<real, D, double> c;
#pragma unroll
        for (int k = 0; k < D; ++k) sdp_locate_axis<real, D, double>(grid, k, s[k * a.n_s + i], c);
        for (int v = 0; v < a.n_v; ++v)
            out[v * a.n_s + i] = (real)SdpLerp<real, D, double, 0>::eval(values + v * a.S, grid, c, 0);
    }
}

template <typename real>
static int launch_mlinterp(const SdpInterpArgs &a, hipStream_t stream)
{
    if (a.n_s == 0 || a.n_v == 0) return SDP_OK;
    int64_t blocks = (a.n_s + 255) / 256;
    const int64_t cap = (int64_t)device_cus() * 16;
    if (blocks > cap) blocks = cap;
    dim3 g((unsigned)blocks), b(256);
    switch (a.d) {
    case 1: hipLaunchKernelGGL((k_mlinterp<real, 1>), g, b, 0, stream, a); break;
    case 2: hipLaunchKernelGGL((k_mlinterp<real, 2>), g, b, 0, stream, a); break;
    case 3: hipLaunchKernelGGL((k_mlinterp<real, 3>), g, b, 0, stream, a); break;
    case 4: hipLaunchKernelGGL((k_mlinterp<real, 4>), g, b, 0, stream, a); break;
    default: return fail(SDP_EDIM, "Can't interpolate in dimension strictly greater than 5");
    }
    HIP_TRY(hipGetLastError());
    return SDP_OK;
}

// Buffers that were exported to other processes (hipIpcGetMemHandle) are not handed back to the allocator when their
// problem goes: a later allocation at the same address gets an IPC handle the peers may still hold a stale mapping for
// -- seen as `hipIpcGetMemHandle: invalid argument`, and as GPU page faults in a peer's stores a few plans later,
// roughly once in seven runs of bench.py's exchange tuning (nine problems with mappings, one after the other) even
// with "every rank unmaps, barrier, then free" (tools/ubench/ipc_reexport.hip is the two-process probe of that
// sequence; DESIGN section 5 has what it showed).  They rest here instead, and the NEXT problem that needs a buffer of
// that size on that device takes one back (the same live allocation exports to the same handle: nothing stale about
// it), so a process that re-plans with one grid holds two such buffers however often it re-plans.  Bounded: beyond
// PARK_CAP_BYTES the oldest are freed; an allocation that fails for lack of memory frees all of them and tries again.
struct Parked { void *p; size_t bytes; int device; };
static std::mutex g_park_mu;
static std::vector<Parked> g_parked;
static size_t g_parked_bytes = 0;
static const size_t PARK_CAP_BYTES = (size_t)4 << 30;

static int current_device()
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); dev = 0; }
    return dev;
}

// free every parked buffer of the current device (all of them with any_device); returns the bytes released
static size_t drain_parked(bool any_device = false)
{
    std::lock_guard<std::mutex> lock(g_park_mu);
    const int dev = current_device();
    size_t freed = 0;
    std::vector<Parked> keep;
    for (auto &q : g_parked) {
        if (any_device || q.device == dev) { (void)hipFree(q.p); freed += q.bytes; }
        else keep.push_back(q);
    }
    g_parked.swap(keep);
    g_parked_bytes -= freed;
    return freed;
}

struct DevBuf {
    void *p = nullptr;
    bool ever_exported = false;            // handed to another process once (this allocation): park it, never free it early
    ~DevBuf() { if (p) (void)hipFree(p); }
    int alloc(size_t bytes)
    {
        if (p) { (void)hipFree(p); p = nullptr; }
        ever_exported = false;
        if (bytes == 0) bytes = 8;
        hipError_t e = hipMalloc(&p, bytes);
        if (e == hipErrorOutOfMemory && drain_parked() > 0) {          // (parked buffers are the first to go)
            (void)hipGetLastError();
            e = hipMalloc(&p, bytes);
        }
        if (e != hipSuccess) { p = nullptr; (void)hipGetLastError(); return fail(SDP_ENOMEM, "hipMalloc(%zu bytes): %s", bytes, hipGetErrorString(e)); }
        return SDP_OK;
    }
    // a buffer that may be exported later (V, J of a problem): a parked one of this size if there is one.
    // Never less than EXPORT_MIN_BYTES: the runtime carves small allocations out of shared 2 MiB blocks, and
    // a HIP IPC handle of such a fragment shares the whole BLOCK with the other process -- V, J and whatever
    // else lives there, mapped once per handle.  A buffer of its own block is exported alone.
    static constexpr size_t EXPORT_MIN_BYTES = (size_t)4 << 20;
    int alloc_exportable(size_t bytes)
    {
        if (bytes < EXPORT_MIN_BYTES) bytes = EXPORT_MIN_BYTES;
        if (p) { (void)hipFree(p); p = nullptr; }
        {
            std::lock_guard<std::mutex> lock(g_park_mu);
            const int dev = current_device();
            for (size_t k = 0; k < g_parked.size(); ++k)
                if (g_parked[k].bytes == bytes && g_parked[k].device == dev) {
                    p = g_parked[k].p;
                    ever_exported = true;
                    g_parked_bytes -= bytes;
                    g_parked.erase(g_parked.begin() + (long)k);
                    return SDP_OK;
                }
        }
        return alloc(bytes);
    }
};

// Mappings of other processes' buffers (hipIpcOpenMemHandle), ONE per remote allocation and process, counted.
// Problems come and go in an order the ranks do not share (a Python object waiting for its garbage collector keeps
// its mappings for a while), and a rank that re-plans takes its parked buffers back and exports them again: a second
// problem here then maps what a first one still holds.  A second hipIpcOpenMemHandle of the same handle and the
// first problem's hipIpcCloseMemHandle of it are exactly what corrupted things in round 5's first runs (the same
// remote buffer at one address twice: the close of the old mapping took the new one with it -- wrong J, GPU page
// faults, and `hipIpcGetMemHandle: invalid argument` once the runtime's own table of allocations was off).  So the
// library opens a handle once, hands the same address to whoever asks again, and closes it with its last user.
struct IpcMap { hipIpcMemHandle_t h; void *ptr; int refs; };
static std::mutex g_ipc_mu;
static std::vector<IpcMap> g_ipc_maps;

static void ipc_trace(const char *what, const void *ptr, const hipIpcMemHandle_t *h, int refs)
{
#ifdef SDP_TEST_HOOKS
    static const int on = getenv("SDP_IPC_TRACE") != nullptr;
    if (!on) return;
    unsigned long long sig = 0;
    if (h) for (size_t k = 0; k < sizeof(*h); ++k) sig = sig * 1099511628211ull + ((const unsigned char *)h)[k];
    fprintf(stderr, "[ipc %d] %s ptr %p handle %016llx refs %d\n", (int)getpid(), what, ptr, sig, refs);
#else
    (void)what; (void)ptr; (void)h; (void)refs;
#endif
}

static hipError_t ipc_open(void **out, const hipIpcMemHandle_t &h)
{
    std::lock_guard<std::mutex> lock(g_ipc_mu);
    for (auto &m : g_ipc_maps)
        if (memcmp(&m.h, &h, sizeof(h)) == 0) {
            ++m.refs;
            *out = m.ptr;
            ipc_trace("reuse", m.ptr, &h, m.refs);
            return hipSuccess;
        }
    void *q = nullptr;
    hipError_t e = hipIpcOpenMemHandle(&q, h, hipIpcMemLazyEnablePeerAccess);
    if (e != hipSuccess) { *out = nullptr; ipc_trace("open FAILED", nullptr, &h, 0); return e; }
    g_ipc_maps.push_back({h, q, 1});
    *out = q;
    ipc_trace("open", q, &h, 1);
    return hipSuccess;
}

static void ipc_close(void *ptr)
{
    if (!ptr) return;
    std::lock_guard<std::mutex> lock(g_ipc_mu);
    for (size_t k = 0; k < g_ipc_maps.size(); ++k)
        if (g_ipc_maps[k].ptr == ptr) {
            if (--g_ipc_maps[k].refs > 0) { ipc_trace("release", ptr, &g_ipc_maps[k].h, g_ipc_maps[k].refs); return; }
            ipc_trace("close", ptr, &g_ipc_maps[k].h, 0);
            (void)hipIpcCloseMemHandle(ptr);
            g_ipc_maps.erase(g_ipc_maps.begin() + (long)k);
            return;
        }
    ipc_trace("close of an unknown mapping", ptr, nullptr, 0);
}

static void park_exported(DevBuf &b, size_t bytes)
{
    if (!b.p || !b.ever_exported) return;                  // (never exported: its destructor frees it)
    if (bytes < DevBuf::EXPORT_MIN_BYTES) bytes = DevBuf::EXPORT_MIN_BYTES;
    std::lock_guard<std::mutex> lock(g_park_mu);
    g_parked.push_back({b.p, bytes, current_device()});
    g_parked_bytes += bytes;
    b.p = nullptr;
    size_t k = 0;
    while (k + 1 < g_parked.size() && g_parked_bytes > PARK_CAP_BYTES) {     // (the newest stays)
        (void)hipFree(g_parked[k].p);
        g_parked_bytes -= g_parked[k].bytes;
        ++k;
    }
    g_parked.erase(g_parked.begin(), g_parked.begin() + (long)k);
}

static int upload(DevBuf &b, const void *host, size_t bytes)
{
    int rc = b.alloc(bytes);
    if (rc) return rc;
    if (bytes) HIP_TRY(hipMemcpy(b.p, host, bytes, hipMemcpyHostToDevice));
    return SDP_OK;
}

template <typename real>
static int mlinterp_host(int d, const real *smin, const real *smax, const int64_t *orders,
                         const real *values, int64_t n_v, const real *s, int64_t n_s, real *out)
{
    if (d < 1 || d > SDP_MAXD)                                    // pyx:46-47
        return fail(SDP_EDIM, "Can't interpolate in dimension strictly greater than 5");
    if (!smin || !smax || !orders || (!values && n_v) || (!s && n_s) || (!out && n_v && n_s))
        return fail(SDP_EINVAL, "NULL argument");
    if (n_v < 0 || n_s < 0) return fail(SDP_EINVAL, "negative size");
    SdpInterpArgs a;
    memset(&a, 0, sizeof(a));
    int64_t S = 1;
    for (int k = 0; k < d; ++k) {
        if (orders[k] < 2) return fail(SDP_EINVAL, "orders[%d] = %lld: need at least 2 points per axis", k, (long long)orders[k]);
        a.orders[k] = (int32_t)orders[k];
        a.smin[k] = (double)smin[k];
        a.smax[k] = (double)smax[k];
        S *= orders[k];
        if (S >= (int64_t)1 << 31) return fail(SDP_EINVAL, "grid too large: 32-bit vertex indices (pyx:164-165)");
    }
    if (n_v == 0 || n_s == 0) return SDP_OK;
    DevBuf dv, ds, dout;
    int rc;
    if ((rc = dv.alloc(sizeof(real) * S * n_v))) return rc;
    if ((rc = ds.alloc(sizeof(real) * d * n_s))) return rc;
    if ((rc = dout.alloc(sizeof(real) * n_v * n_s))) return rc;
    HIP_TRY(hipMemcpy(dv.p, values, sizeof(real) * S * n_v, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(ds.p, s, sizeof(real) * d * n_s, hipMemcpyHostToDevice));
    a.values = dv.p; a.s = ds.p; a.out = dout.p;
    a.n_s = n_s; a.S = S; a.n_v = (int32_t)n_v; a.d = d;
    if ((rc = launch_mlinterp<real>(a, 0))) return rc;
    HIP_TRY(hipMemcpy(out, dout.p, sizeof(real) * n_v * n_s, hipMemcpyDeviceToHost));
    return SDP_OK;
}

extern "C" int sdp_mlinterp_f64(int d, const double *smin, const double *smax,
                                const int64_t *orders, const double *values, int64_t n_v,
                                const double *s, int64_t n_s, double *out)
{
    return mlinterp_host<double>(d, smin, smax, orders, values, n_v, s, n_s, out);
}

extern "C" int sdp_mlinterp_f32(int d, const float *smin, const float *smax,
                                const int64_t *orders, const float *values, int64_t n_v,
                                const float *s, int64_t n_s, float *out)
{
    return mlinterp_host<float>(d, smin, smax, orders, values, n_v, s, n_s, out);
}

// ---------------------------------------------------------------------------
// interpolator handle: the value rows stay on the device between evaluations
// (MlinInterpolator.set_values once, __call__ many times -- e.g. the policy
// look-ups of a simulation loop, reference storage_control.py:242-251)
// ---------------------------------------------------------------------------
struct sdp_interp {
    int dtype = SDP_F64, d = 0;
    int64_t S = 0, n_v = 0;
    int32_t orders[SDP_MAXD] = {0, 0, 0, 0};
    double smin[SDP_MAXD], smax[SDP_MAXD];
    DevBuf values, pts, out;
    size_t pts_bytes = 0, out_bytes = 0;
};

extern "C" int sdp_interp_create(int dtype, int d, const double *smin, const double *smax,
                                 const int64_t *orders, const void *host_values, int64_t n_v,
                                 sdp_interp **out)
{
    if (dtype != SDP_F64 && dtype != SDP_F32) return fail(SDP_EINVAL, "dtype must be SDP_F64 or SDP_F32");
    if (d < 1 || d > SDP_MAXD) return fail(SDP_EDIM, "Can't interpolate in dimension strictly greater than 5");
    if (!smin || !smax || !orders || !host_values || !out || n_v < 1) return fail(SDP_EINVAL, "bad argument");
    std::unique_ptr<sdp_interp> h(new sdp_interp());
    h->dtype = dtype; h->d = d; h->n_v = n_v;
    int64_t S = 1;
    for (int k = 0; k < d; ++k) {
        if (orders[k] < 2) return fail(SDP_EINVAL, "orders[%d] = %lld: need at least 2 points per axis", k, (long long)orders[k]);
        h->orders[k] = (int32_t)orders[k]; h->smin[k] = smin[k]; h->smax[k] = smax[k];
        S *= orders[k];
        if (S >= (int64_t)1 << 31) return fail(SDP_EINVAL, "grid too large: 32-bit vertex indices (pyx:164-165)");
    }
    h->S = S;
    int rc = upload(h->values, host_values, (size_t)S * n_v * real_size(dtype));
    if (rc) return rc;
    *out = h.release();
    return SDP_OK;
}

extern "C" int sdp_interp_destroy(sdp_interp *h)
{
    delete h;
    return SDP_OK;
}

extern "C" int sdp_interp_eval(sdp_interp *h, const void *host_s, int64_t n_s, void *host_out)
{
    if (!h || n_s < 0 || (n_s && (!host_s || !host_out))) return fail(SDP_EINVAL, "bad argument");
    if (n_s == 0) return SDP_OK;
    const size_t rs = real_size(h->dtype);
    const size_t pb = (size_t)h->d * n_s * rs, ob = (size_t)h->n_v * n_s * rs;
    int rc;
    if (h->pts_bytes < pb) { if ((rc = h->pts.alloc(pb))) return rc; h->pts_bytes = pb; }
    if (h->out_bytes < ob) { if ((rc = h->out.alloc(ob))) return rc; h->out_bytes = ob; }
    HIP_TRY(hipMemcpy(h->pts.p, host_s, pb, hipMemcpyHostToDevice));
    SdpInterpArgs a;
    memset(&a, 0, sizeof(a));
    for (int k = 0; k < h->d; ++k) { a.orders[k] = h->orders[k]; a.smin[k] = h->smin[k]; a.smax[k] = h->smax[k]; }
    a.values = h->values.p; a.s = h->pts.p; a.out = h->out.p;
    a.n_s = n_s; a.S = h->S; a.n_v = (int32_t)h->n_v; a.d = h->d;
    rc = h->dtype == SDP_F32 ? launch_mlinterp<float>(a, 0) : launch_mlinterp<double>(a, 0);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(host_out, h->out.p, ob, hipMemcpyDeviceToHost));
    return SDP_OK;
}

// ---------------------------------------------------------------------------
// built-in kernels: relative-DP shift (stodynprog.py:523-525, 760-762)
// ---------------------------------------------------------------------------
template <typename real>
__global__ void k_pick_ref(const real *__restrict__ J, int64_t ref, double *__restrict__ out)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) *out = (double)J[ref];
}

template <typename real>
__global__ void __launch_bounds__(256) k_shift(real *__restrict__ J, int64_t n,
                                               const double *__restrict__ ref)
{
    const real r = (real)*ref;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        J[i] = J[i] - r;
}

// ---------------------------------------------------------------------------
// built-in kernel: convergence statistics of two consecutive cost-to-go arrays
// (stodynprog_amd/convergence.py: diff_stats is the definition).  Per node
//     a = J[i] (- J[ra]),  b = V[i] (- V[rb])     (ra / rb < 0: no shift; else each rounded once in `real`)
//     d = 0 where a == b, else a - b rounded in `real`
// and dmin / dmax of d over a list of node ranges, NaN flagged apart.  Min and max do not depend on the
// order, so any grid, split or rank count gives the same bits.  Accumulated as order-preserving 64-bit
// keys of the doubles: acc[0] = max of ~key(dmin), acc[1] = max of key(dmax), acc[2] = NaN seen; all three
// start at 0 (one stream-ordered memset), and 0 is the identity of every one of them.
// ---------------------------------------------------------------------------
#define SDP_STAT_RANGES 8
struct SdpStatRanges {
    int64_t b[SDP_STAT_RANGES], e[SDP_STAT_RANGES];
    int n;
};

__device__ __host__ inline unsigned long long sdp_order_key(double x)
{
    unsigned long long u;
    memcpy(&u, &x, 8);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

static double sdp_key_value(unsigned long long k)
{
    const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    double x;
    memcpy(&x, &u, 8);
    return x;
}

// (branch-free: d is NaN exactly where a or b is, and a NaN d leaves mn / mx as they are)
template <typename real>
__device__ inline void stat_node(real a, real b, real &mn, real &mx, int &nan)
{
    const real d = a == b ? real(0) : a - b;
    nan |= d != d;
    mn = d < mn ? d : mn;
    mx = d > mx ? d : mx;
}

template <typename real>
__global__ void __launch_bounds__(256) k_diff_stats(const real *__restrict__ J, const real *__restrict__ V,
                                                    int64_t ra, int64_t rb, SdpStatRanges r,
                                                    unsigned long long *__restrict__ acc)
{
    constexpr int VEC = 16 / sizeof(real);                 // 16-byte loads: 2 doubles or 4 floats
    struct alignas(16) Pack { real v[VEC]; };
    const real ja = ra >= 0 ? J[ra] : real(0), vb = rb >= 0 ? V[rb] : real(0);
    real mn = real(INFINITY), mx = real(-INFINITY);
    int nan = 0;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (int64_t)gridDim.x * blockDim.x;
    for (int k = 0; k < r.n; ++k) {
        const int64_t b = r.b[k], e = r.e[k];
        int64_t vb0 = (b + VEC - 1) / VEC * VEC;           // J and V share their alignment (same element index)
        if (vb0 > e) vb0 = e;
        const int64_t ve = vb0 + (e - vb0) / VEC * VEC;
        for (int64_t i = b + tid; i < vb0; i += nth) {      // head and tail: fewer than VEC nodes each
            const real a = ra >= 0 ? J[i] - ja : J[i], c = rb >= 0 ? V[i] - vb : V[i];
            stat_node(a, c, mn, mx, nan);
        }
        for (int64_t i = ve + tid; i < e; i += nth) {
            const real a = ra >= 0 ? J[i] - ja : J[i], c = rb >= 0 ? V[i] - vb : V[i];
            stat_node(a, c, mn, mx, nan);
        }
        // four 16-byte loads of each array in flight per lane, then the arithmetic
        constexpr int UNROLL = 4;
        const int64_t step = nth * VEC;
        int64_t i = vb0 + tid * VEC;
        for (; i + (UNROLL - 1) * step < ve; i += UNROLL * step) {
            Pack pa[UNROLL], pc[UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                pa[u] = *(const Pack *)(J + i + u * step);
                pc[u] = *(const Pack *)(V + i + u * step);
            }
#pragma unroll
            for (int u = 0; u < UNROLL; ++u)
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    const real a = ra >= 0 ? pa[u].v[j] - ja : pa[u].v[j];
                    const real c = rb >= 0 ? pc[u].v[j] - vb : pc[u].v[j];
                    stat_node(a, c, mn, mx, nan);
                }
        }
        for (; i < ve; i += step) {
            const Pack pa = *(const Pack *)(J + i), pc = *(const Pack *)(V + i);
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                const real a = ra >= 0 ? pa.v[j] - ja : pa.v[j], c = rb >= 0 ? pc.v[j] - vb : pc.v[j];
                stat_node(a, c, mn, mx, nan);
            }
        }
    }
    // wavefront, then block (four wavefronts through LDS), then one atomic per word and block
    for (int off = warpSize / 2; off > 0; off >>= 1) {
        const real omn = __shfl_xor(mn, off), omx = __shfl_xor(mx, off);
        mn = omn < mn ? omn : mn;
        mx = omx > mx ? omx : mx;
        nan |= __shfl_xor(nan, off);
    }
    __shared__ real s_mn[4], s_mx[4];
    __shared__ int s_nan[4];
    const int wave = threadIdx.x / warpSize;
    if (threadIdx.x % warpSize == 0) { s_mn[wave] = mn; s_mx[wave] = mx; s_nan[wave] = nan; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int waves = (blockDim.x + warpSize - 1) / warpSize;
        for (int w = 1; w < waves; ++w) {
            mn = s_mn[w] < mn ? s_mn[w] : mn;
            mx = s_mx[w] > mx ? s_mx[w] : mx;
            nan |= s_nan[w];
        }
        atomicMax(acc + 0, ~sdp_order_key((double)mn));
        atomicMax(acc + 1, sdp_order_key((double)mx));
        if (nan) atomicMax(acc + 2, 1ull);
    }
}

// ---------------------------------------------------------------------------
// built-in kernels: tabulated backup (stodynprog.py:677-690)
//   k_tab_cells : one lane per lattice cell, coalesced x_next / g reads,
//                 jc = g + interp(V, x_next)
//   k_tab_reduce: one wavefront per node, lanes stride over controls, in-lane
//                 sequential expectation over w, butterfly first-index argmin
// ---------------------------------------------------------------------------
template <int D>
__global__ void __launch_bounds__(256) k_tab_cells(SdpTabArgs a, double *__restrict__ jc)
{
    SdpGrid<double, D> grid;
    double smin[D], smax[D];
#pragma unroll
    for (int k = 0; k < D; ++k) { smin[k] = a.smin[k]; smax[k] = a.smax[k]; }
    sdp_make_grid<double, D>(grid, a.orders, smin, smax);
    const double *__restrict__ xn = (const double *)a.x_next;
    const double *__restrict__ g = (const double *)a.g;
    const double *__restrict__ V = (const double *)a.V;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n_cells; i += stride) {
        double pt[D];
#pragma unroll
        for (int k = 0; k < D; ++k) pt[k] = xn[k * a.n_cells + i];
        jc[i] = g[i] + sdp_interp_point<double, D>(V, grid, pt);
    }
}

__global__ void __launch_bounds__(256) k_tab_reduce(SdpTabArgs a, const double *__restrict__ jc,
                                                    int64_t *__restrict__ idx_out)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const double *__restrict__ proba = (const double *)a.proba;
    const int W = a.W > 0 ? a.W : 1;
    for (int64_t n = wave; n < a.n_nodes; n += n_waves) {
        const int64_t off = a.cell_off[n];
        const int U = (int)((a.cell_off[n + 1] - off) / W);
        double best = INFINITY;
        int ibest = INT_MAX;
        for (int c = lane; c < U; c += 64) {
            double acc;
            if (a.W > 0) {
                acc = 0.0;
                for (int w = 0; w < W; ++w) acc = acc + jc[off + (int64_t)c * W + w] * proba[w];
            } else {
                acc = jc[off + c];
            }
            if (ibest == INT_MAX || sdp_better_seq(acc, best)) { best = acc; ibest = c; }
        }
        sdp_seg_argmin<double, 64>(best, ibest);
        if (lane == 0) { ((double *)a.J)[n] = best; idx_out[n] = ibest; }
    }
}

struct sdp_tab {
    int d = 0;
    int64_t S = 0;
    int32_t orders[SDP_MAXD] = {0, 0, 0, 0};
    double smin[SDP_MAXD], smax[SDP_MAXD];
    DevBuf V;
    // per-call buffers, kept and grown: x_next, g, cell_off, proba, jc, J, idx
    DevBuf buf[7];
    size_t cap[7] = {0, 0, 0, 0, 0, 0, 0};
    int reserve(int k, size_t bytes)
    {
        if (cap[k] >= bytes) return SDP_OK;
        int rc = buf[k].alloc(bytes + bytes / 4);
        cap[k] = rc ? 0 : bytes + bytes / 4;
        return rc;
    }
    int put(int k, const void *host, size_t bytes)
    {
        int rc = reserve(k, bytes);
        if (rc) return rc;
        if (bytes) HIP_TRY(hipMemcpy(buf[k].p, host, bytes, hipMemcpyHostToDevice));
        return SDP_OK;
    }
};

extern "C" int sdp_tab_create(int d, const double *smin, const double *smax,
                              const int64_t *orders, const double *host_V, sdp_tab **out)
{
    if (d < 1 || d > SDP_MAXD) return fail(SDP_EDIM, "Can't interpolate in dimension strictly greater than 5");
    if (!smin || !smax || !orders || !host_V || !out) return fail(SDP_EINVAL, "NULL argument");
    std::unique_ptr<sdp_tab> t(new sdp_tab());
    t->d = d;
    int64_t S = 1;
    for (int k = 0; k < d; ++k) {
        if (orders[k] < 2) return fail(SDP_EINVAL, "state axis %d has %lld points: at least 2 needed", k, (long long)orders[k]);
        t->orders[k] = (int32_t)orders[k]; t->smin[k] = smin[k]; t->smax[k] = smax[k];
        S *= orders[k];
        if (S >= (int64_t)1 << 31) return fail(SDP_EINVAL, "state grid too large");
    }
    t->S = S;
    int rc = upload(t->V, host_V, S * 8);
    if (rc) return rc;
    *out = t.release();
    return SDP_OK;
}

extern "C" int sdp_tab_destroy(sdp_tab *t)
{
    delete t;
    return SDP_OK;
}

extern "C" int sdp_tab_backup(sdp_tab *t, int64_t n_nodes, const int64_t *cell_off, int64_t W,
                              const double *proba, const double *x_next, const double *g,
                              double *J_out, int64_t *idx_out)
{
    if (!t || !cell_off || !J_out || !idx_out) return fail(SDP_EINVAL, "NULL argument");
    if (n_nodes < 0 || W < 0) return fail(SDP_EINVAL, "negative size");
    if (n_nodes == 0) return SDP_OK;
    const int64_t n_cells = cell_off[n_nodes];
    if (n_cells <= 0 || !x_next || !g) return fail(SDP_EINVAL, "empty lattice");
    if (W > 0 && !proba) return fail(SDP_EINVAL, "perturbation weights missing");
    // the handle keeps its device buffers from call to call (a caller that backs nodes
    // up one at a time -- DPSolver._value_at_state_vect -- allocates nothing here)
    DevBuf &dx = t->buf[0], &dg = t->buf[1], &doff = t->buf[2], &dp = t->buf[3], &djc = t->buf[4],
           &dJ = t->buf[5], &didx = t->buf[6];
    int rc;
    if ((rc = t->put(0, x_next, (size_t)t->d * n_cells * 8))) return rc;
    if ((rc = t->put(1, g, (size_t)n_cells * 8))) return rc;
    if ((rc = t->put(2, cell_off, (size_t)(n_nodes + 1) * 8))) return rc;
    if (W > 0 && (rc = t->put(3, proba, (size_t)W * 8))) return rc;
    if ((rc = t->reserve(4, (size_t)n_cells * 8))) return rc;
    if ((rc = t->reserve(5, (size_t)n_nodes * 8))) return rc;
    if ((rc = t->reserve(6, (size_t)n_nodes * 8))) return rc;
    SdpTabArgs a;
    memset(&a, 0, sizeof(a));
    a.V = t->V.p; a.x_next = dx.p; a.g = dg.p; a.cell_off = (const int64_t *)doff.p;
    a.proba = dp.p; a.J = dJ.p; a.n_nodes = n_nodes; a.n_cells = n_cells;
    a.W = (int32_t)W; a.d = t->d;
    for (int k = 0; k < t->d; ++k) { a.orders[k] = t->orders[k]; a.smin[k] = t->smin[k]; a.smax[k] = t->smax[k]; }
    const int cus = device_cus();
    int64_t blocks = (n_cells + 255) / 256;
    if (blocks > (int64_t)cus * 16) blocks = (int64_t)cus * 16;
    dim3 gc((unsigned)blocks), b(256);
    switch (t->d) {
    case 1: hipLaunchKernelGGL(k_tab_cells<1>, gc, b, 0, 0, a, (double *)djc.p); break;
    case 2: hipLaunchKernelGGL(k_tab_cells<2>, gc, b, 0, 0, a, (double *)djc.p); break;
    case 3: hipLaunchKernelGGL(k_tab_cells<3>, gc, b, 0, 0, a, (double *)djc.p); break;
    default: hipLaunchKernelGGL(k_tab_cells<4>, gc, b, 0, 0, a, (double *)djc.p); break;
    }
    HIP_TRY(hipGetLastError());
    int64_t rblocks = (n_nodes + 3) / 4;
    if (rblocks > (int64_t)cus * 8) rblocks = (int64_t)cus * 8;
    hipLaunchKernelGGL(k_tab_reduce, dim3((unsigned)rblocks), b, 0, 0, a, (const double *)djc.p, (int64_t *)didx.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(J_out, dJ.p, (size_t)n_nodes * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(idx_out, didx.p, (size_t)n_nodes * 8, hipMemcpyDeviceToHost));
    return SDP_OK;
}

// ---------------------------------------------------------------------------
// built-in kernel: layout conversion at the API boundary.  Host arrays are
// always in the reference's C order (last state axis fastest); a handle in
// SDP_LAYOUT_COLUMNS keeps its per-node arrays with axis 0 fastest.  Both
// directions are the transpose of an [R][C] matrix of elements of WORDS 32-bit
// words, done through a 32x33 LDS tile so reads and writes are both coalesced.
// ---------------------------------------------------------------------------
template <int WORDS>
__global__ void __launch_bounds__(256) k_transpose(const uint32_t *__restrict__ in,
                                                   uint32_t *__restrict__ out, int64_t R, int64_t C)
{
    __shared__ uint32_t tile[WORDS][32][33];
    const int64_t tiles_c = (C + 31) / 32, tiles_r = (R + 31) / 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;      // 32 x 8 threads
    for (int64_t t = blockIdx.x; t < tiles_r * tiles_c; t += gridDim.x) {
        const int64_t r0 = (t / tiles_c) * 32, c0 = (t % tiles_c) * 32;
        __syncthreads();
        for (int j = ty; j < 32; j += 8) {
            const int64_t r = r0 + j, c = c0 + tx;
            if (r < R && c < C)
#pragma unroll
                for (int k = 0; k < WORDS; ++k) tile[k][j][tx] = in[(r * C + c) * WORDS + k];
        }
        __syncthreads();
        for (int j = ty; j < 32; j += 8) {
            const int64_t c = c0 + j, r = r0 + tx;
            if (r < R && c < C)
#pragma unroll
                for (int k = 0; k < WORDS; ++k) out[(c * R + r) * WORDS + k] = tile[k][tx][j];
        }
    }
}

static int launch_transpose(const void *in, void *out, int64_t R, int64_t C, int words,
                            hipStream_t stream)
{
    if (R == 0 || C == 0) return SDP_OK;
    int64_t tiles = ((R + 31) / 32) * ((C + 31) / 32);
    unsigned blocks = (unsigned)(tiles < 65536 ? tiles : 65536);
    const uint32_t *i = (const uint32_t *)in;
    uint32_t *o = (uint32_t *)out;
    switch (words) {
    case 1: hipLaunchKernelGGL(k_transpose<1>, dim3(blocks), dim3(256), 0, stream, i, o, R, C); break;
    case 2: hipLaunchKernelGGL(k_transpose<2>, dim3(blocks), dim3(256), 0, stream, i, o, R, C); break;
    case 3: hipLaunchKernelGGL(k_transpose<3>, dim3(blocks), dim3(256), 0, stream, i, o, R, C); break;
    case 4: hipLaunchKernelGGL(k_transpose<4>, dim3(blocks), dim3(256), 0, stream, i, o, R, C); break;
    case 6: hipLaunchKernelGGL(k_transpose<6>, dim3(blocks), dim3(256), 0, stream, i, o, R, C); break;
    case 8: hipLaunchKernelGGL(k_transpose<8>, dim3(blocks), dim3(256), 0, stream, i, o, R, C); break;
    default: return fail(SDP_EINVAL, "unsupported element size for the layout conversion");
    }
    HIP_TRY(hipGetLastError());
    return SDP_OK;
}

// ---------------------------------------------------------------------------
// RCCL, loaded lazily so single-GPU use never needs librccl
// ---------------------------------------------------------------------------
typedef struct { char internal[128]; } nccl_uid;
typedef void *nccl_comm_t;
enum { NCCL_INT8 = 0, NCCL_INT32 = 2, NCCL_FLOAT32 = 7, NCCL_FLOAT64 = 8, NCCL_MAX = 2 };

struct RcclApi {
    void *h = nullptr;
    int (*GetUniqueId)(nccl_uid *) = nullptr;
    int (*CommInitRank)(nccl_comm_t *, int, nccl_uid, int) = nullptr;
    int (*CommDestroy)(nccl_comm_t) = nullptr;
    int (*AllGather)(const void *, void *, size_t, int, nccl_comm_t, hipStream_t) = nullptr;
    int (*AllReduce)(const void *, void *, size_t, int, int, nccl_comm_t, hipStream_t) = nullptr;
    // point-to-point, grouped: the sparse exchange that needs nothing but the collective library (sendrecv_phase)
    int (*Send)(const void *, size_t, int, int, nccl_comm_t, hipStream_t) = nullptr;
    int (*Recv)(void *, size_t, int, int, nccl_comm_t, hipStream_t) = nullptr;
    int (*GroupStart)(void) = nullptr;
    int (*GroupEnd)(void) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
};
static RcclApi g_rccl;
static std::string g_rccl_name;

extern "C" const char *sdp_comm_library(void) { return g_rccl_name.c_str(); }
extern "C" int sdp_test_hooks(void)
{
#ifdef SDP_TEST_HOOKS
    return 1;
#else
    return 0;
#endif
}

static int rccl_load()
{
    if (g_rccl.h) return SDP_OK;
#ifdef SDP_TEST_HOOKS
    // TEST BUILD ONLY (-DSDP_TEST_HOOKS, never the product library): SDP_RCCL_LIBRARY names another
    // library with the same nccl* entry points (the tests load a host-staged stand-in to run
    // several ranks on the one GPU of the test box)
    const char *override_path = getenv("SDP_RCCL_LIBRARY");
#else
    const char *override_path = nullptr;
#endif
    const char *names[] = {override_path && *override_path ? override_path : "librccl.so",
                           "librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"};
    void *h = nullptr;
    for (const char *n : names) {
        h = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
        if (h) g_rccl_name = n;
        if (h || (override_path && *override_path)) break;     // an explicit path must load
    }
    if (!h) return fail(SDP_ECOMM, "cannot load librccl.so: %s", dlerror());
#define SYM(field, name)                                                         \
    *(void **)(&g_rccl.field) = dlsym(h, name);                                  \
    if (!g_rccl.field) return fail(SDP_ECOMM, "librccl: missing symbol %s", name)
    SYM(GetUniqueId, "ncclGetUniqueId");
    SYM(CommInitRank, "ncclCommInitRank");
    SYM(CommDestroy, "ncclCommDestroy");
    SYM(AllGather, "ncclAllGather");
    SYM(AllReduce, "ncclAllReduce");
    SYM(Send, "ncclSend");
    SYM(Recv, "ncclRecv");
    SYM(GroupStart, "ncclGroupStart");
    SYM(GroupEnd, "ncclGroupEnd");
    SYM(GetErrorString, "ncclGetErrorString");
#undef SYM
    g_rccl.h = h;
    return SDP_OK;
}

#define NCCL_TRY(expr)                                                                 \
    do {                                                                               \
        int r__ = (expr);                                                              \
        if (r__ != 0) return fail(SDP_ECOMM, "%s failed: %s", #expr, g_rccl.GetErrorString(r__)); \
    } while (0)

struct sdp_comm {
    nccl_comm_t comm = nullptr;
    int rank = 0, nranks = 1;
    hipStream_t stream = nullptr;
    double *d_scalar = nullptr;
};

extern "C" int sdp_comm_unique_id(char id[128])
{
    int rc = rccl_load();
    if (rc) return rc;
    nccl_uid uid;
    NCCL_TRY(g_rccl.GetUniqueId(&uid));
    memcpy(id, uid.internal, 128);
    return SDP_OK;
}

extern "C" int sdp_comm_create(int rank, int nranks, const char id[128], sdp_comm **out)
{
    if (!out || !id || nranks < 1 || rank < 0 || rank >= nranks) return fail(SDP_EINVAL, "bad communicator arguments");
    int rc = rccl_load();
    if (rc) return rc;
    sdp_comm *c = new sdp_comm();
    c->rank = rank; c->nranks = nranks;
    nccl_uid uid;
    memcpy(uid.internal, id, 128);
    int r = g_rccl.CommInitRank(&c->comm, nranks, uid, rank);
    if (r != 0) { delete c; return fail(SDP_ECOMM, "ncclCommInitRank: %s", g_rccl.GetErrorString(r)); }
    int prio_lo = 0, prio_hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);   // numerically lowest = highest priority
    if (hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, prio_hi) != hipSuccess ||
        hipMalloc((void **)&c->d_scalar, 8) != hipSuccess) {
        delete c; return fail(SDP_EHIP, "communicator stream/scratch allocation failed");
    }
    *out = c;
    return SDP_OK;
}

extern "C" int sdp_comm_destroy(sdp_comm *c)
{
    if (!c) return SDP_OK;
    if (c->comm) g_rccl.CommDestroy(c->comm);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    if (c->d_scalar) (void)hipFree(c->d_scalar);
    delete c;
    return SDP_OK;
}

extern "C" int sdp_comm_allreduce_max(sdp_comm *c, double *inout)
{
    if (!c || !inout) return fail(SDP_EINVAL, "NULL argument");
    HIP_TRY(hipMemcpyAsync(c->d_scalar, inout, 8, hipMemcpyHostToDevice, c->stream));
    NCCL_TRY(g_rccl.AllReduce(c->d_scalar, c->d_scalar, 1, NCCL_FLOAT64, NCCL_MAX, c->comm, c->stream));
    HIP_TRY(hipMemcpyAsync(inout, c->d_scalar, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SDP_OK;
}

extern "C" int sdp_comm_barrier(sdp_comm *c)
{
    double v = 0;
    return sdp_comm_allreduce_max(c, &v);
}

// ---------------------------------------------------------------------------
// problem handle
// ---------------------------------------------------------------------------
struct sdp_problem {
    int dtype = SDP_F64, d = 0, nu = 0, W = 0, lanes = 64, box_per_node = 0, layout = 0, variant = 0;
    int stg_threads = 0, col_seg = 0;
    int n_perturb = 0;                 // perturbation variables (sdp_problem_desc.n_perturb; >= 2: the flat law of several)
    int64_t stg_tiles = 0;
    int64_t S = 0, node_begin = 0, node_end = 0;
    int32_t orders[SDP_MAXD] = {0, 0, 0, 0};
    int32_t axis_off[SDP_MAXD] = {0, 0, 0, 0};
    DevBuf axes, wgrid, proba, box_lo, box_hi, box_n, V, J, pol, idx, pol_in, refs, scratch, stamps, claim;
    DevBuf stats, stats_all;               // convergence check: this rank's 3 key words, every rank's (diff_stats)
    hipEvent_t ev_stats = nullptr;         // .. the statistics are ready for the all-gather
    DevBuf gstage;                         // gather buffer of phases with uneven parts (gather_phase_of)
    size_t gstage_bytes = 0;
    DevBuf stage[3];                       // layout-conversion buffers of the fused host call (J, pol, idx)
    size_t stage_bytes[3] = {0, 0, 0};
    // peer-write exchange (sdp_problem_enable_peer_exchange): the other ranks' value / J buffers
    // mapped into this process, one copy stream per peer
    bool peer_exchange = false;
    std::vector<void *> peer_V, peer_J;    // [nranks] (own entry: the local buffer)
    std::vector<hipStream_t> peer_stream;  // [nranks] (own entry unused)
    std::vector<hipEvent_t> peer_done;     // [nranks]
    int *d_flag = nullptr;                 // word for the rendezvous all-reduces
    hipEvent_t ev_enter = nullptr, ev_fence = nullptr;
    bool peer_fence = true;                // next backup is the first of an API call: see open_pushes
    hipStream_t copy_stream = nullptr;     // downloads of finished phases, under the next phase's kernel
    hipEvent_t ev_host[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev_copy = nullptr;
    int host_overlap = 1;                  // sdp_problem_set_host_overlap
    int64_t stamp_words = 0;
    size_t scratch_bytes = 0;
    hipModule_t mod = nullptr;
    hipFunction_t f_sweep = nullptr, f_evalpol = nullptr, f_simulate = nullptr, f_montecarlo = nullptr, f_transitions = nullptr;
    hipFunction_t f_simulate_h = nullptr, f_montecarlo_h = nullptr;      // the loops under a time-indexed policy (sdp_horizon_kernel.h)
    hipFunction_t f_transitions_h = nullptr;                             // the operators of the steps of a horizon (sdp_trans_horizon_kernel.h)
    hipFunction_t f_lookahead = nullptr, f_simulate_lookahead = nullptr; // lookahead units only (sdp_lookahead_kernel.h); the second: units with their own box function
    hipFunction_t f_montecarlo_lookahead = nullptr;                      // .. and, of those, the units of a stochastic system
    // several controlled state variables (csrc/sdp_lead_kernel.h): the kernel that reduces V over w, launched
    // before every sweep, and its outputs (A[S] and a copy of V, both plane-major; E[nodes per trailing block];
    // bits of max |V|)
    hipFunction_t f_lead_reduce = nullptr;
    DevBuf lead_a, lead_v, lead_e, lead_vmax;
    hipDeviceptr_t prm_dev = nullptr;     // `sdp_model_prm` of the code object (lifted model constants)
    size_t prm_bytes = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr, ev3 = nullptr;
    double last_kernel_ms = 0;
    sdp_comm *comm = nullptr;
    std::vector<int64_t> parts;            // [n_phases][nranks+1] node bounds (device order)
    std::vector<hipEvent_t> ev_phase;
    hipEvent_t ev_comm = nullptr;
    int n_phases = 0;
    bool comm_pending = false;
    // sparse peer exchange (sdp_problem_set_peer_needs): need[q] = sorted, disjoint node ranges of J
    // that rank q reads in a backup; J / V are then complete on a rank only there
    std::vector<std::vector<std::pair<int64_t, int64_t>>> need;
    bool sparse = false, J_partial = false, V_partial = false;
    // direct exchange (sdp_problem_set_direct_exchange): the backup kernels themselves store J into the
    // peers' mapped buffers (SdpSweepArgs.peer_J); sparse: per column the ranks that read it
    bool direct = false, mask_valid = false, send_everything = false;
    bool sendrecv = false;                 // sparse exchange by grouped ncclSend / ncclRecv (no mapped buffers): sdp_problem_set_sendrecv_exchange
    DevBuf peer_mask;
    // reduced-array sweep (csrc/sdp_lead_kernel.h), sharded: rows of the first stock the controls of a node
    // reach on either side (a guess of the host: too small costs time, not correctness); < 0: reduce everything
    int64_t lead_halo = -1;
    // what the plane-major arrays currently hold: the value buffer they were reduced from, its generation
    // (bumped whenever the contents of V change), and the lead indices covered
    const void *red_V = nullptr;
    uint64_t red_gen = 0, V_gen = 1;
    int red_parity = 0;                    // line kernel: which of the two slots of lead_vmax the last reduction used
    int64_t red_begin = 0, red_end = 0;
    double red_t = 0;
    int cus = 256;
    int refs_cap = 0;
    int col_threads = 512;
    int col_occupancy = 8;                 // workgroups of sdp_sweep_col a CU holds at once
    int32_t meta[SDP_META_WORDS] = {0};    // `sdp_meta` of the code object
    int peer_me = -1;                      // this rank, as of sdp_problem_enable_peer_exchange
    void release_peers()
    {
        // (the rank is the one recorded when the mappings were made: the communicator is not
        // owned by the problem and may already be gone)
        const int me = peer_me;
        for (size_t r = 0; r < peer_V.size(); ++r) {
            if ((int)r == me) continue;
            ipc_close(peer_V[r]);
            ipc_close(peer_J[r]);
        }
        peer_V.clear(); peer_J.clear();
        for (auto &st : peer_stream) if (st) (void)hipStreamDestroy(st);
        for (auto &e : peer_done) if (e) (void)hipEventDestroy(e);
        peer_stream.clear(); peer_done.clear();
        if (d_flag) { (void)hipFree(d_flag); d_flag = nullptr; }
        if (ev_enter) { (void)hipEventDestroy(ev_enter); ev_enter = nullptr; }
        if (ev_fence) { (void)hipEventDestroy(ev_fence); ev_fence = nullptr; }
        peer_exchange = false;
        direct = false;
        peer_me = -1;
    }
    ~sdp_problem()
    {
        {
            const size_t bytes = (size_t)S * (dtype == SDP_F64 ? 8 : 4);
            park_exported(V, bytes);                       // (no-ops for buffers that never left this process)
            park_exported(J, bytes);
        }
        if (mod) (void)hipModuleUnload(mod);
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (ev2) (void)hipEventDestroy(ev2);
        if (ev3) (void)hipEventDestroy(ev3);
        if (ev_comm) (void)hipEventDestroy(ev_comm);
        if (ev_stats) (void)hipEventDestroy(ev_stats);
        release_peers();
        if (ev_copy) (void)hipEventDestroy(ev_copy);
        for (auto &e : ev_host) if (e) (void)hipEventDestroy(e);
        if (copy_stream) (void)hipStreamDestroy(copy_stream);
        for (auto &e : ev_phase) if (e) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

static int64_t lead_trailing_nodes(const sdp_problem *p);

extern "C" int sdp_problem_create(const sdp_problem_desc *desc, sdp_problem **out)
{
    if (!desc || !out) return fail(SDP_EINVAL, "NULL argument");
    if (desc->dtype != SDP_F64 && desc->dtype != SDP_F32) return fail(SDP_EINVAL, "dtype must be SDP_F64 or SDP_F32");
    if (desc->d < 1 || desc->d > SDP_MAXD)
        return fail(SDP_EDIM, "state dimension %d: multilinear interpolation supports 1..4", desc->d);
    if (desc->nu < 1 || desc->nu > SDP_MAXU) return fail(SDP_EINVAL, "number of controls %d outside 1..%d", desc->nu, SDP_MAXU);
    if (desc->W < 0) return fail(SDP_EINVAL, "negative perturbation count");
    if (desc->n_perturb < 0 || desc->n_perturb > 4) return fail(SDP_EINVAL, "%d perturbation variables: at most 4", (int)desc->n_perturb);
    if (desc->n_perturb > 0 && desc->W < 1) return fail(SDP_EINVAL, "%d perturbation variables but no point of their law", (int)desc->n_perturb);
    if (!desc->module_path) return fail(SDP_EMODULE, "no model code object given");
    if (!desc->box_lo || !desc->box_hi || !desc->box_n) return fail(SDP_EINVAL, "control box arrays missing");
    sdp_problem *p = new sdp_problem();
    std::unique_ptr<sdp_problem> guard(p);
    p->dtype = desc->dtype; p->d = desc->d; p->nu = desc->nu; p->W = desc->W;
    p->n_perturb = desc->n_perturb > 0 ? desc->n_perturb : (desc->W > 0 ? 1 : 0);       // (0: "1 when W > 0")
    p->lanes = desc->lanes_per_node; p->box_per_node = desc->box_per_node;
    if (p->lanes < 1 || p->lanes > 64 || (p->lanes & (p->lanes - 1))) return fail(SDP_EINVAL, "lanes_per_node must be a power of two in 1..64");
    const size_t rs = real_size(p->dtype);
    int64_t S = 1, total = 0;
    for (int k = 0; k < p->d; ++k) {
        if (desc->orders[k] < 2) return fail(SDP_EINVAL, "state axis %d has %lld points: at least 2 needed to interpolate", k, (long long)desc->orders[k]);
        if (!desc->axes[k]) return fail(SDP_EINVAL, "state axis %d missing", k);
        p->orders[k] = (int32_t)desc->orders[k];
        p->axis_off[k] = (int32_t)total;
        total += desc->orders[k];
        S *= desc->orders[k];
        if (S >= (int64_t)1 << 31) return fail(SDP_EINVAL, "state grid too large: 32-bit vertex indices (pyx:164-165)");
    }
    p->S = S;
    p->node_begin = desc->node_begin;
    p->node_end = desc->node_end;
    if (p->node_begin < 0 || p->node_end > S || p->node_begin > p->node_end) return fail(SDP_EINVAL, "node slab [%lld,%lld) outside [0,%lld)", (long long)p->node_begin, (long long)p->node_end, (long long)S);
    p->cus = device_cus();

    // concatenated axes
    std::vector<char> ax(total * rs);
    for (int k = 0; k < p->d; ++k)
        memcpy(ax.data() + (size_t)p->axis_off[k] * rs, desc->axes[k], (size_t)desc->orders[k] * rs);
    int rc;
    if ((rc = upload(p->axes, ax.data(), ax.size()))) return rc;
    if (p->W > 0) {
        if (!desc->wgrid || !desc->proba) return fail(SDP_EINVAL, "perturbation grid/weights missing");
        if ((rc = upload(p->wgrid, desc->wgrid, (size_t)p->n_perturb * p->W * rs))) return rc;        // [n_perturb][W]
        if ((rc = upload(p->proba, desc->proba, p->W * rs))) return rc;
    }
    const size_t nbox = (size_t)p->nu * (p->box_per_node ? (size_t)S : 1);
    if (p->box_per_node && desc->layout == SDP_LAYOUT_COLUMNS) {
        // [nu][N0][P] (reference order) -> [nu][P][N0] (axis 0 fastest)
        const int64_t n0 = desc->orders[0], P = S / n0;
        auto reorder = [&](const void *src, size_t es, DevBuf &dst) -> int {
            std::vector<char> tmp(nbox * es);
            for (int c = 0; c < p->nu; ++c)
                for (int64_t i = 0; i < n0; ++i)
                    for (int64_t q = 0; q < P; ++q)
                        memcpy(tmp.data() + ((size_t)c * S + q * n0 + i) * es,
                               (const char *)src + ((size_t)c * S + i * P + q) * es, es);
            return upload(dst, tmp.data(), tmp.size());
        };
        if ((rc = reorder(desc->box_lo, rs, p->box_lo))) return rc;
        if ((rc = reorder(desc->box_hi, rs, p->box_hi))) return rc;
        if ((rc = reorder(desc->box_n, 4, p->box_n))) return rc;
    } else {
        if ((rc = upload(p->box_lo, desc->box_lo, nbox * rs))) return rc;
        if ((rc = upload(p->box_hi, desc->box_hi, nbox * rs))) return rc;
        if ((rc = upload(p->box_n, desc->box_n, nbox * 4))) return rc;
    }
    if ((rc = p->V.alloc_exportable(S * rs))) return rc;       // (a parked, once-exported buffer of this size if there is one)
    if ((rc = p->J.alloc_exportable(S * rs))) return rc;
    if ((rc = p->pol.alloc((size_t)S * p->nu * rs))) return rc;
    if ((rc = p->idx.alloc(S * 4))) return rc;
    HIP_TRY(hipMemset(p->V.p, 0, S * rs));
    HIP_TRY(hipMemset(p->J.p, 0, S * rs));
    HIP_TRY(hipMemset(p->pol.p, 0, (size_t)S * p->nu * rs));
    HIP_TRY(hipMemset(p->idx.p, 0, S * 4));

    hipError_t e = hipModuleLoad(&p->mod, desc->module_path);
    if (e != hipSuccess) { p->mod = nullptr; return fail(SDP_EMODULE, "hipModuleLoad(%s): %s", desc->module_path, hipGetErrorString(e)); }
    p->layout = desc->layout;
    if (p->layout != SDP_LAYOUT_NODES && p->layout != SDP_LAYOUT_COLUMNS) return fail(SDP_EINVAL, "unknown layout %d", p->layout);
    if (p->layout == SDP_LAYOUT_COLUMNS) {
        if (p->d < 2) return fail(SDP_EINVAL, "column layout needs at least two state axes");
        if (p->node_begin % p->orders[0] || p->node_end % p->orders[0])
            return fail(SDP_EINVAL, "column layout: the node slab must consist of whole columns");
    }
    p->variant = desc->variant;
    p->col_seg = desc->col_seg_nodes > 0 ? desc->col_seg_nodes : 0;
    if (p->variant != SDP_VARIANT_DIRECT && p->variant != SDP_VARIANT_STAGED) return fail(SDP_EINVAL, "unknown kernel variant %d", p->variant);
    if (p->variant == SDP_VARIANT_STAGED) {
        if (p->layout != SDP_LAYOUT_NODES) return fail(SDP_EINVAL, "the staged kernel works on the node layout");
        p->stg_tiles = 1;
        for (int k = 0; k < p->d; ++k) {
            if (desc->tile[k] < 1) return fail(SDP_EINVAL, "staged kernel: tile[%d] = %d", k, (int)desc->tile[k]);
            p->stg_tiles *= (p->orders[k] + desc->tile[k] - 1) / desc->tile[k];
        }
    }
    // what the code object was generated for must be THIS problem: the kernels carry table
    // sizes, dimensions and the real type as compile-time constants
    {
        hipDeviceptr_t mptr = nullptr;
        size_t mbytes = 0;
        if (hipModuleGetGlobal(&mptr, &mbytes, p->mod, "sdp_meta") != hipSuccess || mbytes != sizeof(p->meta)) {
            (void)hipGetLastError();
            return fail(SDP_EMODULE, "code object %s does not declare `sdp_meta` (%d words, sdp_kernel_args.h): "
                        "cannot check that it was built for this problem", desc->module_path, SDP_META_WORDS);
        }
        HIP_TRY(hipMemcpyDtoH(p->meta, mptr, sizeof(p->meta)));
        const int32_t *m = p->meta;
        const int64_t controls = [&] {
            if (p->box_per_node) return (int64_t)-1;
            int64_t t = 1;
            for (int c = 0; c < p->nu; ++c) t *= ((const int32_t *)desc->box_n)[c];
            return t;
        }();
        const char *what = nullptr;
        char detail[160] = "";
#define META_CHECK(cond, ...) if (!what && !(cond)) { what = #cond; snprintf(detail, sizeof(detail), __VA_ARGS__); }
        META_CHECK(m[SDP_META_MAGIC_AT] == SDP_META_MAGIC, "bad magic 0x%x", (unsigned)m[SDP_META_MAGIC_AT]);
        META_CHECK(m[SDP_META_REAL_BYTES] == (int)rs, "built for %d-byte reals, the problem has %d-byte reals", m[SDP_META_REAL_BYTES], (int)rs);
        META_CHECK(m[SDP_META_D] == p->d, "built for %d state variables, the problem has %d", m[SDP_META_D], p->d);
        META_CHECK(m[SDP_META_NU] == p->nu, "built for %d controls, the problem has %d", m[SDP_META_NU], p->nu);
        META_CHECK((m[SDP_META_HAS_W] != 0) == (p->W > 0), "built %s a perturbation, the problem has W = %d", m[SDP_META_HAS_W] ? "with" : "without", p->W);
        // (every unit also carries the node-order kernels sdp_sweep / sdp_evalpol: a column or staged unit
        // may serve a node-layout, direct-variant problem; the reverse is what must be refused)
        META_CHECK((m[SDP_META_NW] ? m[SDP_META_NW] : (m[SDP_META_HAS_W] ? 1 : 0)) == p->n_perturb, "built for %d perturbation variable(s), the problem has %d", m[SDP_META_NW] ? m[SDP_META_NW] : (m[SDP_META_HAS_W] ? 1 : 0), p->n_perturb);
        META_CHECK(p->n_perturb < 2 || (p->layout == SDP_LAYOUT_NODES && p->variant == SDP_VARIANT_DIRECT), "several perturbation variables run the node layout's direct kernels only");
        META_CHECK(p->layout != SDP_LAYOUT_COLUMNS || m[SDP_META_LAYOUT] == SDP_LAYOUT_COLUMNS, "the column layout was asked of a code object without column kernels");
        META_CHECK(p->variant != SDP_VARIANT_STAGED || (m[SDP_META_FLAGS] & SDP_META_F_STAGED), "the staged-tile variant was asked of a code object without sdp_sweep_lds");
        if (p->layout == SDP_LAYOUT_COLUMNS) {
            META_CHECK(m[SDP_META_COL_N0] == p->orders[0], "column table built for %d points along axis 0, the grid has %d", m[SDP_META_COL_N0], p->orders[0]);
            META_CHECK(m[SDP_META_COL_W] == (p->W > 0 ? p->W : 1), "column table built for %d perturbation points, the problem has %d", m[SDP_META_COL_W], p->W);
            META_CHECK(((m[SDP_META_FLAGS] & SDP_META_F_WINDOW) != 0) == (p->col_seg > 0) || (m[SDP_META_FLAGS] & SDP_META_F_TRAIL_HAS_U), "row-window kernel %s but col_seg_nodes = %d", (m[SDP_META_FLAGS] & SDP_META_F_WINDOW) ? "present" : "absent", p->col_seg);
            META_CHECK(m[SDP_META_UTAB] == 0 || (controls >= 1 && controls <= m[SDP_META_UTAB_N]), "control table built for one lattice of at most %d controls at every node, the problem has %s%lld", m[SDP_META_UTAB_N], controls < 0 ? "per-node boxes " : "", (long long)controls);
        }
#undef META_CHECK
        if (what)
            return fail(SDP_EMODULE, "code object %s was not built for this problem: %s", desc->module_path, detail);
    }
    const char *k_sweep = p->layout == SDP_LAYOUT_COLUMNS ? "sdp_sweep_col"
                          : (p->variant == SDP_VARIANT_STAGED ? "sdp_sweep_lds" : "sdp_sweep");
    const char *k_eval = p->layout == SDP_LAYOUT_COLUMNS ? "sdp_evalpol_col" : "sdp_evalpol";
    e = hipModuleGetFunction(&p->f_sweep, p->mod, k_sweep);
    if (e != hipSuccess) return fail(SDP_EMODULE, "code object %s has no %s kernel: %s", desc->module_path, k_sweep, hipGetErrorString(e));
    if (p->layout == SDP_LAYOUT_COLUMNS) {
        // the workgroup size the column kernels were compiled for (__launch_bounds__)
        int mt = 0;
        if (hipFuncGetAttribute(&mt, HIP_FUNC_ATTRIBUTE_MAX_THREADS_PER_BLOCK, p->f_sweep) == hipSuccess && mt >= 64)
            p->col_threads = mt > 1024 ? 1024 : mt;
        {
            int occ = 0;
            if (hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&occ, p->f_sweep, p->col_threads, 0) == hipSuccess && occ >= 1)
                p->col_occupancy = occ > 16 ? 16 : occ;
            else
                (void)hipGetLastError();
        }
        // unit counters of the filtered column kernel (SdpSweepArgs.claim): zero once, the kernel
        // leaves them zero
        int rc = p->claim.alloc(4 * (8 * 32 + 32));
        if (rc) return rc;
        HIP_TRY(hipMemset(p->claim.p, 0, 4 * (8 * 32 + 32)));
    }
    if (p->layout != SDP_LAYOUT_COLUMNS && p->variant != SDP_VARIANT_STAGED && (p->meta[SDP_META_FLAGS] & SDP_META_F_LEAD)) {
        e = hipModuleGetFunction(&p->f_lead_reduce, p->mod, "sdp_lead_reduce");
        if (e != hipSuccess) return fail(SDP_EMODULE, "code object %s has no sdp_lead_reduce kernel: %s", desc->module_path, hipGetErrorString(e));
        // (one state variable, sdp_line_kernel.h: the filter on the shifted lattice -- several lanes per node, and aux_a holds
        // (A', B', C') triplets for the positions of a lattice of 2 S + 64 rows at most; no copy of V)
        const bool line = p->d == 1 && (p->meta[SDP_META_FLAGS] & SDP_META_F_SHIFT);
        if (line && p->meta[SDP_META_COL_W] != p->W)
            return fail(SDP_EMODULE, "code object %s was built for %d perturbation points, the problem has %d", desc->module_path, p->meta[SDP_META_COL_W], p->W);
        if (!line && p->lanes != 1) return fail(SDP_EINVAL, "the reduced-array sweep takes one lane per node (lanes = %d)", p->lanes);
        int rc = p->lead_a.alloc(line ? (size_t)(2 * p->S + 64) * 24 : (size_t)p->S * 8);   // (the reduced array: 8-byte sums whatever the reals are, sdp_lead_kernel.h)
        if (!rc) rc = p->lead_v.alloc(line ? 8 : (size_t)p->S * rs);
        if (!rc) rc = p->lead_e.alloc((size_t)lead_trailing_nodes(p) * rs);            // (a value per trailing index)
        if (!rc) rc = p->lead_vmax.alloc(32);        // (the line kernel: two slots of two words, used in turn)
        if (!rc) HIP_TRY(hipMemset(p->lead_vmax.p, 0, 32));
        if (rc) return rc;
    }
    if (p->variant == SDP_VARIANT_STAGED) {
        int mt = 0;
        if (hipFuncGetAttribute(&mt, HIP_FUNC_ATTRIBUTE_MAX_THREADS_PER_BLOCK, p->f_sweep) != hipSuccess || mt < 64)
            return fail(SDP_EMODULE, "cannot read the workgroup size of sdp_sweep_lds");
        p->stg_threads = mt;
        int64_t tile_nodes = 1;
        for (int k = 0; k < p->d; ++k) tile_nodes *= desc->tile[k];
        if (tile_nodes != mt) return fail(SDP_EINVAL, "staged kernel: tile of %lld nodes but workgroups of %d threads", (long long)tile_nodes, mt);
    }
    e = hipModuleGetFunction(&p->f_evalpol, p->mod, k_eval);
    if (e != hipSuccess) return fail(SDP_EMODULE, "code object %s has no %s kernel: %s", desc->module_path, k_eval, hipGetErrorString(e));
    if (hipModuleGetFunction(&p->f_simulate, p->mod, "sdp_simulate") != hipSuccess) {
        (void)hipGetLastError();
        p->f_simulate = nullptr;
    }
    if (hipModuleGetFunction(&p->f_montecarlo, p->mod, "sdp_montecarlo") != hipSuccess) {
        (void)hipGetLastError();
        p->f_montecarlo = nullptr;
    }
    if (hipModuleGetFunction(&p->f_simulate_h, p->mod, "sdp_simulate_h") != hipSuccess) {
        (void)hipGetLastError();
        p->f_simulate_h = nullptr;
    }
    if (hipModuleGetFunction(&p->f_montecarlo_h, p->mod, "sdp_montecarlo_h") != hipSuccess) {
        (void)hipGetLastError();
        p->f_montecarlo_h = nullptr;
    }
    if (hipModuleGetFunction(&p->f_lookahead, p->mod, "sdp_lookahead") != hipSuccess) {
        (void)hipGetLastError();
        p->f_lookahead = nullptr;
    }
    if (hipModuleGetFunction(&p->f_simulate_lookahead, p->mod, "sdp_simulate_lookahead") != hipSuccess) {
        (void)hipGetLastError();
        p->f_simulate_lookahead = nullptr;
    }
    if (hipModuleGetFunction(&p->f_montecarlo_lookahead, p->mod, "sdp_montecarlo_lookahead") != hipSuccess) {
        (void)hipGetLastError();
        p->f_montecarlo_lookahead = nullptr;
    }
    if (hipModuleGetFunction(&p->f_transitions, p->mod, "sdp_transitions") != hipSuccess) {
        (void)hipGetLastError();
        p->f_transitions = nullptr;
    }
    if (hipModuleGetFunction(&p->f_transitions_h, p->mod, "sdp_transitions_h") != hipSuccess) {
        (void)hipGetLastError();
        p->f_transitions_h = nullptr;
    }
    // lifted model constants (codegen: `__constant__ sdp_real sdp_model_prm[]`), if any
    if (hipModuleGetGlobal(&p->prm_dev, &p->prm_bytes, p->mod, "sdp_model_prm") != hipSuccess) {
        (void)hipGetLastError();
        p->prm_dev = nullptr;
        p->prm_bytes = 0;
    }
    HIP_TRY(hipStreamCreate(&p->stream));
    HIP_TRY(hipEventCreate(&p->ev0));
    HIP_TRY(hipEventCreate(&p->ev1));
    HIP_TRY(hipEventCreate(&p->ev2));
    HIP_TRY(hipEventCreate(&p->ev3));
    guard.release();
    *out = p;
    return SDP_OK;
}

extern "C" int sdp_problem_set_params(sdp_problem *p, const void *values, int32_t n)
{
    if (!p || n < 0 || (n > 0 && !values)) return fail(SDP_EINVAL, "sdp_problem_set_params: bad arguments");
    const size_t bytes = (size_t)n * real_size(p->dtype);
    if (bytes != p->prm_bytes)
        return fail(SDP_EINVAL, "sdp_problem_set_params: the code object declares %zu parameter(s), %d given",
                    p->prm_bytes / real_size(p->dtype), (int)n);
    if (!bytes) return SDP_OK;
    // on the problem's stream: ordered after the launches that still read the old values
    HIP_TRY(hipMemcpyAsync(p->prm_dev, values, bytes, hipMemcpyHostToDevice, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));        // `values` may be reused by the caller
    p->red_V = nullptr;                               // (the reduced array was made with the old constants)
    return SDP_OK;
}

extern "C" int sdp_problem_destroy(sdp_problem *p)
{
    if (p) { (void)hipDeviceSynchronize(); delete p; }
    return SDP_OK;
}

static int ensure_scratch(sdp_problem *p, size_t bytes)
{
    if (p->scratch_bytes >= bytes) return SDP_OK;
    int rc = p->scratch.alloc(bytes);
    if (rc) { p->scratch_bytes = 0; return rc; }
    p->scratch_bytes = bytes;
    return SDP_OK;
}

// host (reference C order) -> device buffer in the handle's layout
static int upload_nodes(sdp_problem *p, void *dev, const void *host, size_t elem_bytes)
{
    const size_t bytes = (size_t)p->S * elem_bytes;
    if (p->layout != SDP_LAYOUT_COLUMNS) {
        HIP_TRY(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, p->stream));
    } else {
        int rc = ensure_scratch(p, bytes);
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(p->scratch.p, host, bytes, hipMemcpyHostToDevice, p->stream));
        // [N0][P] -> [P][N0]
        if ((rc = launch_transpose(p->scratch.p, dev, p->orders[0], p->S / p->orders[0],
                                   (int)(elem_bytes / 4), p->stream))) return rc;
    }
    HIP_TRY(hipStreamSynchronize(p->stream));
    return SDP_OK;
}

// device buffer in the handle's layout -> host (reference C order)
static int download_nodes(sdp_problem *p, void *host, const void *dev, size_t elem_bytes)
{
    const size_t bytes = (size_t)p->S * elem_bytes;
    if (p->layout != SDP_LAYOUT_COLUMNS) {
        HIP_TRY(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, p->stream));
    } else {
        int rc = ensure_scratch(p, bytes);
        if (rc) return rc;
        // [P][N0] -> [N0][P]
        if ((rc = launch_transpose(dev, p->scratch.p, p->S / p->orders[0], p->orders[0],
                                   (int)(elem_bytes / 4), p->stream))) return rc;
        HIP_TRY(hipMemcpyAsync(host, p->scratch.p, bytes, hipMemcpyDeviceToHost, p->stream));
    }
    HIP_TRY(hipStreamSynchronize(p->stream));
    return SDP_OK;
}

extern "C" int sdp_problem_set_value(sdp_problem *p, const void *host_V)
{
    if (!p || !host_V) return fail(SDP_EINVAL, "NULL argument");
    p->V_partial = false;
    ++p->V_gen;                              // (whatever was derived from the old contents is stale)
    return upload_nodes(p, p->V.p, host_V, real_size(p->dtype));
}

extern "C" int sdp_problem_set_policy(sdp_problem *p, const void *host_pol)
{
    if (!p || !host_pol) return fail(SDP_EINVAL, "NULL argument");
    const size_t bytes = (size_t)p->S * p->nu * real_size(p->dtype);
    int rc;
    if (!p->pol_in.p && (rc = p->pol_in.alloc(bytes))) return rc;
    return upload_nodes(p, p->pol_in.p, host_pol, (size_t)p->nu * real_size(p->dtype));
}

static void fill_args(const sdp_problem *p, SdpSweepArgs &a, double t_k, int64_t nb, int64_t ne)
{
    memset(&a, 0, sizeof(a));
    a.V = p->V.p; a.J = p->J.p; a.pol = p->pol.p; a.idx = (int32_t *)p->idx.p;
    a.axes = p->axes.p; a.wgrid = p->wgrid.p; a.proba = p->proba.p;
    a.box_lo = p->box_lo.p; a.box_hi = p->box_hi.p; a.box_n = (const int32_t *)p->box_n.p;
    a.pol_in = p->pol_in.p;
    a.node_begin = nb; a.node_end = ne; a.S = p->S; a.t_k = t_k;
    for (int k = 0; k < SDP_MAXD; ++k) { a.orders[k] = p->orders[k]; a.axis_off[k] = p->axis_off[k]; }
    a.W = p->W; a.box_per_node = p->box_per_node;
    a.shift_index = -1; a.ref_out = nullptr;
    a.stamps = (unsigned long long *)p->stamps.p;
    a.claim = (unsigned int *)p->claim.p;
    a.aux_a = p->lead_a.p; a.aux_v = p->lead_v.p; a.aux_e = p->lead_e.p; a.aux_vmax = (unsigned long long *)p->lead_vmax.p;
    a.aux_begin = p->red_begin; a.aux_end = p->red_end;
    if (p->direct && p->comm && p->comm->nranks > 1 && p->peer_exchange) {
        const int n = p->comm->nranks;
        a.n_peer = n;
        for (int q = 0; q < n && q < SDP_MAX_PEERS; ++q) a.peer_J[q] = q == p->comm->rank ? nullptr : p->peer_J[(size_t)q];
        a.peer_mask = p->send_everything ? nullptr : (const unsigned char *)(p->sparse ? p->peer_mask.p : nullptr);
    }
    if (p->layout == SDP_LAYOUT_COLUMNS) {
        a.n_lead = p->orders[0];
        a.col_begin = nb / p->orders[0];
        a.col_end = ne / p->orders[0];
        a.col_splits = 1;
    }
}

static int launch_module(hipFunction_t f, SdpSweepArgs &a, unsigned blocks, unsigned threads,
                         hipStream_t stream)
{
    size_t size = sizeof(a);
    void *extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a, HIP_LAUNCH_PARAM_BUFFER_SIZE, &size,
                     HIP_LAUNCH_PARAM_END};
    HIP_TRY(hipModuleLaunchKernel(f, blocks, 1, 1, threads, 1, 1, 0, stream, nullptr, extra));
    return SDP_OK;
}

// Column kernels: a unit of work is (column, split).  Splitting a column over
// several workgroups repeats its table build, so split only as far as needed
// to give every CU a few workgroups; `min_nodes` nodes per split at least.
static unsigned column_grid(const sdp_problem *p, SdpSweepArgs &a, int min_nodes, bool sweep_kernel)
{
    const int64_t cols = a.col_end - a.col_begin;
    const int n0 = p->orders[0];
    int64_t want = (int64_t)p->cus * 4;
    int splits = (int)((want + cols - 1) / cols);
    int max_splits = n0 / (min_nodes > 0 ? min_nodes : 1);
    if (max_splits < 1) max_splits = 1;
    if (splits > max_splits) splits = max_splits;
    if (splits < 1) splits = 1;
    // row window: a workgroup's table covers the rows reachable from col_seg nodes
    if (p->col_seg > 0 && splits < (n0 + p->col_seg - 1) / p->col_seg) splits = (n0 + p->col_seg - 1) / p->col_seg;
    a.col_splits = splits;
    int64_t units = cols * splits;
    // Single GPU: a bounded grid whose workgroups stride over the units.  With
    // a communicator: one workgroup per unit, so CUs are handed back all the
    // time and the RCCL kernels of the previous phase's all-gather (on their
    // own, higher-priority stream) get scheduled beside the sweep instead of
    // behind it.
    // (kernels whose workgroups CLAIM their units are persistent whatever the grid: a workgroup per
    // unit would only add thousands of workgroups that start, find nothing left and leave)
    // Their grid is what the chip holds at once (occupancy of the kernel: LDS, registers, wave slots).
    // (sdp_evalpol_col strides over the units: it takes the bounded grid of the other kernels)
    const bool claims = sweep_kernel && (p->meta[SDP_META_FLAGS] & SDP_META_F_CLAIMS) != 0;
    int64_t blocks = (p->comm && p->comm->nranks > 1 && !claims) ? units
                     : (int64_t)p->cus * (claims ? p->col_occupancy : 8);
    if (blocks > units) blocks = units;
    blocks = ((blocks + 7) / 8) * 8;
    if (blocks < 8) blocks = 8;
    return (unsigned)blocks;
}

// workgroups for the sweep: a multiple of 8 (one share per XCD), enough to
// fill every CU several times over, never more than there are node tiles
static unsigned sweep_blocks(const sdp_problem *p, int64_t nodes)
{
    // (with a communicator the bounded grid is kept: the generic kernel leaves
    // most of the LDS and half of the wave slots free for the RCCL kernels)
    // (the line kernel, one state variable on the shifted lattice: a workgroup's four waves share a tile of 64 / lanes nodes)
    const bool line = p->d == 1 && (p->meta[SDP_META_FLAGS] & SDP_META_F_LEAD) && (p->meta[SDP_META_FLAGS] & SDP_META_F_SHIFT);
    const int64_t tile = (64 / p->lanes) * (line ? 1 : 4);
    int64_t tiles = (nodes + tile - 1) / tile;
    int64_t blocks = (int64_t)p->cus * 8;
    if (blocks > tiles) blocks = tiles;
    blocks = ((blocks + 7) / 8) * 8;
    if (blocks < 8) blocks = 8;
    return (unsigned)blocks;
}

// reduced-array sweep: nodes per block of trailing coordinates, and the lead indices [lb, le) whose reduced
// values a launch over the nodes [nb, ne) may read
static int64_t lead_trailing_nodes(const sdp_problem *p)
{
    int64_t ts = 1;
    for (int k = p->meta[SDP_META_LEAD_AXES]; k < p->d; ++k) ts *= p->orders[(p->meta[SDP_META_LEAD_PERM] >> (4 * k)) & 15];
    return ts;
}
static bool lead_permuted(const sdp_problem *p)
{
    for (int k = 0; k < p->d; ++k)
        if (((p->meta[SDP_META_LEAD_PERM] >> (4 * k)) & 15) != k) return true;
    return false;
}
static void lead_reduce_range(const sdp_problem *p, int64_t nb, int64_t ne, int64_t &lb, int64_t &le)
{
    const int64_t ts = lead_trailing_nodes(p), ls = p->S / ts;
    lb = 0; le = ls;
    // (stocks not listed first: a slab of nodes is no range of lead indices -- everything is reduced)
    if (p->lead_halo < 0 || !p->comm || p->comm->nranks < 2 || lead_permuted(p)) return;
    // this rank's nodes over all phases of the backup (one contiguous slab with dist.slab_partition)
    int64_t lo = nb, hi = ne;
    const int n = p->comm->nranks, me = p->comm->rank;
    for (int ph = 0; ph < p->n_phases; ++ph) {
        const int64_t *b = p->parts.data() + (size_t)ph * (n + 1);
        if (b[me + 1] > b[me]) { lo = b[me] < lo ? b[me] : lo; hi = b[me + 1] > hi ? b[me + 1] : hi; }
    }
    const int64_t row = ls / p->orders[0];                  // lead indices per row of the first stock
    lb = lo / ts - (p->lead_halo + 1) * row;
    le = (hi + ts - 1) / ts + (p->lead_halo + 2) * row;
    if (lb < 0) lb = 0;
    if (le > ls) le = ls;
}

static int launch_sweep(sdp_problem *p, double t_k, int64_t nb, int64_t ne)
{
    if (ne <= nb) return SDP_OK;
    SdpSweepArgs a;
    fill_args(p, a, t_k, nb, ne);
    if (p->layout == SDP_LAYOUT_COLUMNS) {
        // 512-thread workgroups: 8 waves share one LDS table, one lane per node
        const unsigned threads = (unsigned)p->col_threads;   // SDP_COL_THREADS of the code object
        const unsigned blocks = column_grid(p, a, 64, true);
        return launch_module(p->f_sweep, a, blocks, threads, p->stream);
    }
    if (p->variant == SDP_VARIANT_STAGED) {
        // bounded grid of tile-walking workgroups (LDS admits two per CU; a few per slot
        // even out tiles of different cost), a multiple of 8 for the XCD-contiguous walk
        int64_t blocks = (int64_t)p->cus * 4;
        if (blocks > p->stg_tiles) blocks = p->stg_tiles;
        blocks = ((blocks + 7) / 8) * 8;
        return launch_module(p->f_sweep, a, (unsigned)blocks, (unsigned)p->stg_threads, p->stream);
    }
    if (p->f_lead_reduce) {
        // The array reduced over w (every node's first pass reads it at the nodes its controls reach): from
        // the whole of V on one GPU; sharded, from this rank's rows of the first stock plus `lead_halo` rows
        // on either side -- once per value array, however many launches (phases) the backup takes.
        if (p->V_partial) return fail(SDP_EINVAL, "the reduced-array sweep needs the whole cost-to-go array on this device");
        int64_t lb, le;
        lead_reduce_range(p, nb, ne, lb, le);
        if (!(p->red_V == p->V.p && p->red_gen == p->V_gen && p->red_t == t_k && p->red_begin <= lb && le <= p->red_end)) {
            const bool line = p->d == 1 && (p->meta[SDP_META_FLAGS] & SDP_META_F_SHIFT);
            // (the line kernel keeps its maximum in one of two slots and clears the other for the next reduction itself:
            // no fill launch between the kernels of a sweep that takes tens of microseconds)
            if (line) p->red_parity ^= 1;
            else HIP_TRY(hipMemsetAsync(p->lead_vmax.p, 0, 16, p->stream));
            const int64_t ts = lead_trailing_nodes(p);
            SdpSweepArgs r = a;
            if (line) {
                r.aux_vmax = (unsigned long long *)p->lead_vmax.p + 2 * p->red_parity;
                r.aux_e = (unsigned long long *)p->lead_vmax.p + 2 * (p->red_parity ^ 1);
            }
            r.n_peer = 0;
            r.node_begin = lb * ts; r.node_end = le * ts;
            r.aux_begin = lb; r.aux_end = le;
            int rc = launch_module(p->f_lead_reduce, r, sweep_blocks(p, r.node_end - r.node_begin), 256, p->stream);
            if (rc) return rc;
            p->red_V = p->V.p; p->red_gen = p->V_gen; p->red_t = t_k; p->red_begin = lb; p->red_end = le;
        }
        a.aux_begin = p->red_begin; a.aux_end = p->red_end;
        if (p->d == 1 && (p->meta[SDP_META_FLAGS] & SDP_META_F_SHIFT)) a.aux_vmax = (unsigned long long *)p->lead_vmax.p + 2 * p->red_parity;
    }
    return launch_module(p->f_sweep, a, sweep_blocks(p, ne - nb), 256, p->stream);
}

static int launch_evalpol(sdp_problem *p, double t_k, int64_t nb, int64_t ne,
                          int64_t shift_index, double *ref_out)
{
    if (ne <= nb) return SDP_OK;
    SdpSweepArgs a;
    fill_args(p, a, t_k, nb, ne);
    a.shift_index = shift_index;
    a.ref_out = ref_out;
    if (p->layout == SDP_LAYOUT_COLUMNS) {
        const unsigned blocks = column_grid(p, a, 64, false);      // one lane per node
        const int per_split = (p->orders[0] + a.col_splits - 1) / a.col_splits;
        unsigned threads = (unsigned)((per_split + 63) / 64) * 64;
        if (threads > (unsigned)p->col_threads) threads = (unsigned)p->col_threads;
        return launch_module(p->f_evalpol, a, blocks, threads, p->stream);
    }
    const int64_t nodes = ne - nb;
    int64_t blocks = (nodes + 255) / 256;
    if (blocks > (int64_t)p->cus * 16) blocks = (int64_t)p->cus * 16;
    return launch_module(p->f_evalpol, a, (unsigned)blocks, 256, p->stream);
}

// Exchange of one phase of a per-node array (in place) on the communicator's
// stream: rank r owns nodes [b[r], b[r+1]) of the phase, elem_bytes bytes per
// node.  Equal parts: one in-place ncclAllGather.  Uneven parts (a column count
// that is no multiple of ranks x phases -- Searev's 61 x 61 columns on 8 GPUs --, tapered
// plans): every part padded to the longest one in a gather buffer, ONE
// ncclAllGather there, and the parts copied to their places ("pad, or
// use grouped ncclBroadcast" -- round 4 used the grouped broadcasts, one per rank
// and phase; with 8 ranks a tapered plan stalled in 3 of 12 full-size runs under the
// stand-in, cause not found: the path is gone).  Moved as raw bytes, so it serves J,
// the policy and the index.
static int gather_phase_of(sdp_problem *p, int phase, void *buffer, size_t elem_bytes)
{
    const int n = p->comm->nranks, me = p->comm->rank;
    const int64_t *b = p->parts.data() + (size_t)phase * (n + 1);
    bool even = true;
    const int64_t len0 = b[1] - b[0];
    int64_t longest = 0;
    for (int r = 0; r < n; ++r) {
        even = even && (b[r + 1] - b[r] == len0);
        longest = std::max(longest, b[r + 1] - b[r]);
    }
    if (b[n] == b[0]) return SDP_OK;
    char *base = (char *)buffer;
    hipStream_t cs = p->comm->stream;
    if (even) {
        NCCL_TRY(g_rccl.AllGather(base + b[me] * elem_bytes, base + b[0] * elem_bytes,
                                  (size_t)len0 * elem_bytes, NCCL_INT8, p->comm->comm, cs));
        return SDP_OK;
    }
    const size_t slot = (size_t)longest * elem_bytes;
    if (p->gstage_bytes < slot * (size_t)n) {
        // (sdp_problem_attach_comm sizes the buffer for the J exchange of every phase; only the policy
        // gather -- on request, nothing in flight -- can come here.  hipFree waits for the device.)
        int rc = p->gstage.alloc(slot * (size_t)n);
        if (rc) { p->gstage_bytes = 0; return rc; }
        p->gstage_bytes = slot * (size_t)n;
    }
    char *g = (char *)p->gstage.p;
    const size_t mine = (size_t)(b[me + 1] - b[me]) * elem_bytes;
    if (mine) HIP_TRY(hipMemcpyAsync(g + (size_t)me * slot, base + b[me] * elem_bytes, mine, hipMemcpyDeviceToDevice, cs));
    NCCL_TRY(g_rccl.AllGather(g + (size_t)me * slot, g, slot, NCCL_INT8, p->comm->comm, cs));
    for (int r = 0; r < n; ++r) {
        const size_t cnt = (size_t)(b[r + 1] - b[r]) * elem_bytes;
        if (r == me || cnt == 0) continue;
        HIP_TRY(hipMemcpyAsync(base + b[r] * elem_bytes, g + (size_t)r * slot, cnt, hipMemcpyDeviceToDevice, cs));
    }
    return SDP_OK;
}

// Peer-write form of the exchange of one phase of J: this rank's rows of the phase go straight
// into every other rank's J buffer (mapped through HIP IPC) as device-to-device copies on one
// stream per peer -- copy engines over xGMI, no compute units, all links at once -- ordered
// behind the phase's kernel by `after`.
static int push_phase(sdp_problem *p, int phase, hipEvent_t after, bool everything)
{
    const int n = p->comm->nranks, me = p->comm->rank;
    const int64_t *b = p->parts.data() + (size_t)phase * (n + 1);
    const size_t rs = real_size(p->dtype);
    const int64_t lo = b[me], hi = b[me + 1];
    if (hi <= lo) return SDP_OK;
    for (int k = 1; k < n; ++k) {
        const int q = (me + k) % n;                       // start with a different peer on every rank
        if (!p->sparse || everything) {
            HIP_TRY(hipStreamWaitEvent(p->peer_stream[q], after, 0));
            HIP_TRY(hipMemcpyAsync((char *)p->peer_J[q] + (size_t)lo * rs, (const char *)p->J.p + (size_t)lo * rs,
                                   (size_t)(hi - lo) * rs, hipMemcpyDeviceToDevice, p->peer_stream[q]));
            continue;
        }
        // only the rows the peer reads (sdp_problem_set_peer_needs)
        const auto &iv = p->need[q];
        auto it = std::lower_bound(iv.begin(), iv.end(), lo,
                                   [](const std::pair<int64_t, int64_t> &r, int64_t v) { return r.second <= v; });
        bool waited = false;
        for (; it != iv.end() && it->first < hi; ++it) {
            const int64_t s0 = it->first > lo ? it->first : lo, s1 = it->second < hi ? it->second : hi;
            if (s1 <= s0) continue;
            if (!waited) { HIP_TRY(hipStreamWaitEvent(p->peer_stream[q], after, 0)); waited = true; }
            HIP_TRY(hipMemcpyAsync((char *)p->peer_J[q] + (size_t)s0 * rs, (const char *)p->J.p + (size_t)s0 * rs,
                                   (size_t)(s1 - s0) * rs, hipMemcpyDeviceToDevice, p->peer_stream[q]));
        }
    }
    return SDP_OK;
}

// Start of the first peer-write backup of an API call.  Writes into a peer's J are one-sided:
// nothing in them waits for the peer, which may still be reading that buffer on behalf of its
// PREVIOUS call (relative-DP shift, download to the host) when a faster rank starts the next
// one.  So the first pushes of a call wait behind a tiny all-reduce that every rank joins only
// once its previous call has returned.  It runs on the communicator stream under the first
// phase's kernel.  Inside a chain of backups the end-of-backup rendezvous is enough (pushes of
// step k+1 go to the buffer step k only read, and every rank's step-k kernels precede it).
static int open_pushes(sdp_problem *p)
{
    const int n = p->comm->nranks, me = p->comm->rank;
    hipStream_t cs = p->comm->stream;
    HIP_TRY(hipEventRecord(p->ev_enter, p->stream));
    HIP_TRY(hipStreamWaitEvent(cs, p->ev_enter, 0));
    NCCL_TRY(g_rccl.AllReduce(p->d_flag, p->d_flag, 1, NCCL_INT32, NCCL_MAX, p->comm->comm, cs));
    HIP_TRY(hipEventRecord(p->ev_fence, cs));
    for (int q = 0; q < n; ++q)
        if (q != me) HIP_TRY(hipStreamWaitEvent(p->peer_stream[q], p->ev_fence, 0));
    // direct exchange: the kernels themselves write into the peers
    if (p->direct) HIP_TRY(hipStreamWaitEvent(p->stream, p->ev_fence, 0));
    p->peer_fence = false;
    return SDP_OK;
}

// End of a peer-write backup: when the tiny all-reduce below completes on this rank, every
// rank has passed its own copies (stream order), so all rows have landed everywhere.
static int finish_pushes(sdp_problem *p, hipEvent_t last_kernel)
{
    const int n = p->comm->nranks, me = p->comm->rank;
    hipStream_t cs = p->comm->stream;
    // The rendezvous must also say "this rank has finished READING V": once it completes, a peer may
    // start the next step and write rows into this rank's next J buffer -- the buffer this step's
    // kernels read as V.  With the dense exchange every phase's pushes wait for that phase's kernel,
    // so the copy streams carry the order; with the sparse one a rank whose last phases send nothing
    // would join the rendezvous with kernels still running.
    if (last_kernel) HIP_TRY(hipStreamWaitEvent(cs, last_kernel, 0));
    for (int q = 0; q < n; ++q) {
        if (q == me) continue;
        HIP_TRY(hipEventRecord(p->peer_done[q], p->peer_stream[q]));
        HIP_TRY(hipStreamWaitEvent(cs, p->peer_done[q], 0));
    }
    NCCL_TRY(g_rccl.AllReduce(p->d_flag, p->d_flag, 1, NCCL_INT32, NCCL_MAX, p->comm->comm, cs));
    return SDP_OK;
}

// direct sparse exchange: per column of the column layout, the ranks that read it (need lists of
// sdp_problem_set_peer_needs) as a bit mask the kernel looks up when it stores J
static int build_peer_mask(sdp_problem *p)
{
    if (p->mask_valid) return SDP_OK;
    if (p->layout != SDP_LAYOUT_COLUMNS) return fail(SDP_EINVAL, "the sparse direct exchange works on whole columns (column layout)");
    const int64_t n0 = p->orders[0], cols = p->S / n0;
    std::vector<unsigned char> mask((size_t)cols, 0);
    const int n = p->comm->nranks, me = p->comm->rank;
    for (int q = 0; q < n && q < SDP_MAX_PEERS; ++q) {
        if (q == me) continue;
        for (const auto &iv : p->need[(size_t)q])
            for (int64_t c = iv.first / n0; c < iv.second / n0; ++c) mask[(size_t)c] |= (unsigned char)(1u << q);
    }
    int rc = p->peer_mask.alloc((size_t)cols);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(p->peer_mask.p, mask.data(), (size_t)cols, hipMemcpyHostToDevice));
    p->mask_valid = true;
    return SDP_OK;
}

// Sparse exchange of one phase of J through the collective library alone (the path to a sparse
// exchange that rests on RCCL, not on stores into HIP-IPC mappings).  A rank reads the cost-to-go array only where the
// trailing next states of its columns fall (need lists: sdp_problem_set_peer_needs); rank q therefore gets, of this
// rank's rows of the phase, the BOUNDING range of what it reads there -- one ncclSend / ncclRecv per pair of ranks
// and phase inside one group (the need lists of a contracting exogenous process are runs of whole rows of the second
// axis: the bounding range is little more than their union; for anything else it is at worst the dense exchange).
// Both sides work the range out from the same lists and partition, so the counts match by construction.  Two-sided:
// nothing lands in a rank's J before that rank has posted its receive, which it does behind the phase's own kernel
// on the communicator stream -- no rendezvous beside the sends and receives themselves.
static void bounding_need(const std::vector<std::pair<int64_t, int64_t>> &iv, int64_t lo, int64_t hi, int64_t &s0, int64_t &s1)
{
    s0 = s1 = 0;
    if (hi <= lo) return;
    auto it = std::lower_bound(iv.begin(), iv.end(), lo,
                               [](const std::pair<int64_t, int64_t> &r, int64_t v) { return r.second <= v; });
    if (it == iv.end() || it->first >= hi) return;
    s0 = it->first > lo ? it->first : lo;
    auto last = std::lower_bound(iv.begin(), iv.end(), hi,
                                 [](const std::pair<int64_t, int64_t> &r, int64_t v) { return r.first < v; });
    --last;                                                // the last range that starts below hi
    s1 = last->second < hi ? last->second : hi;
}
// (slab partitions -- dist.slab_partition: nranks x G phases in node order, phase r G + g owned by rank r alone -- are
// exchanged G times a backup, not nranks x G times: when this rank's g-th phase is done it sends its rows of that phase
// and receives every peer's rows of THEIR g-th phase in one group; the phases it does not own pass)
static bool slab_phases(const sdp_problem *p, int &per_rank)
{
    const int n = p->comm->nranks;
    per_rank = 0;
    if (p->n_phases % n) return false;
    const int g = p->n_phases / n;
    for (int ph = 0; ph < p->n_phases; ++ph) {
        const int64_t *b = p->parts.data() + (size_t)ph * (n + 1);
        for (int r = 0; r < n; ++r)
            if (b[r + 1] > b[r] && r != ph / g) return false;
    }
    per_rank = g;
    return true;
}
static int sendrecv_phase(sdp_problem *p, int phase)
{
    const int n = p->comm->nranks, me = p->comm->rank;
    int per = 0;
    const bool slab = slab_phases(p, per);
    if (slab && phase / per != me) return SDP_OK;
    const int g = slab ? phase % per : 0;
    const int64_t *b = p->parts.data() + (size_t)phase * (n + 1);
    const size_t rs = real_size(p->dtype);
    hipStream_t cs = p->comm->stream;
    char *J = (char *)p->J.p;
    NCCL_TRY(g_rccl.GroupStart());
    for (int k = 1; k < n; ++k) {
        const int to = (me + k) % n, from = (me - k + n) % n;
        const int64_t *bf = slab ? p->parts.data() + (size_t)(from * per + g) * (n + 1) : b;
        int64_t s0, s1;
        bounding_need(p->need[(size_t)to], b[me], b[me + 1], s0, s1);
        if (s1 > s0) NCCL_TRY(g_rccl.Send(J + (size_t)s0 * rs, (size_t)(s1 - s0) * rs, NCCL_INT8, to, p->comm->comm, cs));
        bounding_need(p->need[(size_t)me], bf[from], bf[from + 1], s0, s1);
        if (s1 > s0) NCCL_TRY(g_rccl.Recv(J + (size_t)s0 * rs, (size_t)(s1 - s0) * rs, NCCL_INT8, from, p->comm->comm, cs));
    }
    NCCL_TRY(g_rccl.GroupEnd());
    return SDP_OK;
}

static int gather_phase(sdp_problem *p, int phase)
{
    return gather_phase_of(p, phase, p->J.p, real_size(p->dtype));
}

// One backup (Bellman sweep or fixed-policy evaluation) over the nodes this
// handle owns, V -> J.  Single GPU: one launch.  With a communicator the node
// range is cut into phases, every phase is shared out over the ranks, and the
// all-gather of phase k (communicator stream) overlaps the kernel of phase k+1
// (problem stream); the problem stream then waits for the last gather, so
// whatever follows (relative-DP shift, next sweep) sees the complete J.
static int run_backup(sdp_problem *p, bool evalpol, double t_k, int64_t shift_index = -1,
                      double *ref_out = nullptr, bool everything = false)
{
    int rc;
    if (!p->comm) {
        return evalpol ? launch_evalpol(p, t_k, p->node_begin, p->node_end, shift_index, ref_out)
                       : launch_sweep(p, t_k, p->node_begin, p->node_end);
    }
    const int n = p->comm->nranks, rank = p->comm->rank;
    if (n > 1 && p->peer_exchange && p->peer_fence && (rc = open_pushes(p))) return rc;
    const bool direct = n > 1 && p->peer_exchange && p->direct;
    if (direct && p->sparse && !everything && (rc = build_peer_mask(p))) return rc;
    p->send_everything = everything;
    for (int ph = 0; ph < p->n_phases; ++ph) {
        const int64_t *b = p->parts.data() + (size_t)ph * (n + 1);
        rc = evalpol ? launch_evalpol(p, t_k, b[rank], b[rank + 1], shift_index, ref_out)
                     : launch_sweep(p, t_k, b[rank], b[rank + 1]);
        if (rc) return rc;
        if (n > 1) {
            HIP_TRY(hipEventRecord(p->ev_phase[ph], p->stream));
            if (direct) {
                // (the kernel has stored its rows into the peers that read them: nothing to copy)
            } else if (p->peer_exchange) {
                if ((rc = push_phase(p, ph, p->ev_phase[ph], everything))) return rc;
            } else if (p->sendrecv && p->sparse && !everything) {
                HIP_TRY(hipStreamWaitEvent(p->comm->stream, p->ev_phase[ph], 0));
                if ((rc = sendrecv_phase(p, ph))) return rc;
            } else {
                HIP_TRY(hipStreamWaitEvent(p->comm->stream, p->ev_phase[ph], 0));
                if ((rc = gather_phase(p, ph))) return rc;
            }
        }
    }
    if (n > 1) {
        if (p->peer_exchange && (rc = finish_pushes(p, p->n_phases ? p->ev_phase[p->n_phases - 1] : nullptr))) return rc;
        HIP_TRY(hipEventRecord(p->ev_comm, p->comm->stream));
        p->comm_pending = true;
        p->J_partial = (p->peer_exchange || p->sendrecv) && p->sparse && !everything;
    }
    return SDP_OK;
}

// make the problem stream wait for the exchange of the last backup
static int join_comm(sdp_problem *p)
{
    if (p->comm_pending) {
        HIP_TRY(hipStreamWaitEvent(p->stream, p->ev_comm, 0));
        p->comm_pending = false;
    }
    return SDP_OK;
}

// Sparse peer exchange: before J leaves the device (or is read whole), every rank sends the rows
// it computed to every peer.  Collective, like the backups.
static int complete_J(sdp_problem *p)
{
    if (!p->comm || p->comm->nranks == 1 || !(p->peer_exchange || p->sendrecv) || !p->J_partial) return SDP_OK;
    int rc;
    if ((rc = join_comm(p))) return rc;
    if (p->sendrecv) {                                     // every rank's rows to every rank: the all-gather of each phase
        if (!p->ev_enter) HIP_TRY(hipEventCreateWithFlags(&p->ev_enter, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(p->ev_enter, p->stream));
        HIP_TRY(hipStreamWaitEvent(p->comm->stream, p->ev_enter, 0));
        for (int ph = 0; ph < p->n_phases; ++ph)
            if ((rc = gather_phase(p, ph))) return rc;
        HIP_TRY(hipEventRecord(p->ev_comm, p->comm->stream));
        p->comm_pending = true;
        if ((rc = join_comm(p))) return rc;
        p->J_partial = false;
        return SDP_OK;
    }
    p->peer_fence = true;                                  // nobody may still be reading its J
    if ((rc = open_pushes(p))) return rc;
    HIP_TRY(hipEventRecord(p->ev_enter, p->stream));
    for (int ph = 0; ph < p->n_phases; ++ph)
        if ((rc = push_phase(p, ph, p->ev_enter, true))) return rc;
    if ((rc = finish_pushes(p, p->ev_enter))) return rc;
    HIP_TRY(hipEventRecord(p->ev_comm, p->comm->stream));
    p->comm_pending = true;
    if ((rc = join_comm(p))) return rc;
    p->J_partial = false;
    return SDP_OK;
}

static int rel_shift(sdp_problem *p, int64_t ref_index, int slot)
{
    double *ref = (double *)p->refs.p + slot;
    unsigned blocks = (unsigned)((p->S + 255) / 256);
    if (blocks > (unsigned)p->cus * 16) blocks = p->cus * 16;
    if (p->dtype == SDP_F32) {
        hipLaunchKernelGGL(k_pick_ref<float>, dim3(1), dim3(64), 0, p->stream, (const float *)p->J.p, ref_index, ref);
        hipLaunchKernelGGL(k_shift<float>, dim3(blocks), dim3(256), 0, p->stream, (float *)p->J.p, p->S, ref);
    } else {
        hipLaunchKernelGGL(k_pick_ref<double>, dim3(1), dim3(64), 0, p->stream, (const double *)p->J.p, ref_index, ref);
        hipLaunchKernelGGL(k_shift<double>, dim3(blocks), dim3(256), 0, p->stream, (double *)p->J.p, p->S, ref);
    }
    HIP_TRY(hipGetLastError());
    return SDP_OK;
}

static int ensure_refs(sdp_problem *p, int n)
{
    if (n < 16) n = 16;
    if (p->refs_cap >= n) return SDP_OK;
    int rc = p->refs.alloc((size_t)n * 8);
    if (rc) return rc;
    p->refs_cap = n;
    return SDP_OK;
}

// ref_index arrives as a flat index in the reference's C order (like every
// host-side quantity of the API) and is turned into the handle's device order
static int check_ref(const sdp_problem *p, int rel_dp, int64_t &ref_index)
{
    if (!rel_dp) return SDP_OK;
    if (ref_index < 0 || ref_index >= p->S) return fail(SDP_EINVAL, "reference node %lld outside the grid", (long long)ref_index);
    if (p->layout == SDP_LAYOUT_COLUMNS) {
        const int64_t n0 = p->orders[0], P = p->S / n0;
        ref_index = (ref_index % P) * n0 + ref_index / P;
    }
    if (p->sparse && p->comm && p->comm->nranks > 1) {
        // sparse exchange: the shift reads J[ref] / V[ref] on every rank, so the node must be one this
        // rank computes or receives (the host puts the reference column into every need list)
        const int me = p->comm->rank;
        bool have = false;
        for (int ph = 0; ph < p->n_phases && !have; ++ph) {
            const int64_t *b = p->parts.data() + (size_t)ph * (p->comm->nranks + 1);
            have = ref_index >= b[me] && ref_index < b[me + 1];
        }
        for (size_t k = 0; k < p->need[(size_t)me].size() && !have; ++k)
            have = ref_index >= p->need[(size_t)me][k].first && ref_index < p->need[(size_t)me][k].second;
        if (!have)
            return fail(SDP_EINVAL, "sparse exchange: reference node %lld is neither computed nor received by rank %d "
                        "(it must be in every rank's need list)", (long long)ref_index, me);
    }
    return SDP_OK;
}

extern "C" int sdp_problem_vi_sweep(sdp_problem *p, double t_k, int rel_dp, int64_t ref_index,
                                    double *J_ref_out)
{
    if (!p) return fail(SDP_EINVAL, "NULL problem");
    p->peer_fence = true;                // first backup of a call (open_pushes)
    int rc;
    if ((rc = check_ref(p, rel_dp, ref_index))) return rc;
    if ((rc = ensure_refs(p, 1))) return rc;
    HIP_TRY(hipEventRecord(p->ev0, p->stream));
    if ((rc = run_backup(p, false, t_k))) return rc;
    HIP_TRY(hipEventRecord(p->ev1, p->stream));
    if ((rc = join_comm(p))) return rc;
    if (rel_dp && (rc = rel_shift(p, ref_index, 0))) return rc;
    HIP_TRY(hipStreamSynchronize(p->stream));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, p->ev0, p->ev1));
    p->last_kernel_ms = ms;
    if (rel_dp && J_ref_out) HIP_TRY(hipMemcpy(J_ref_out, p->refs.p, 8, hipMemcpyDeviceToHost));
    return SDP_OK;
}

// V <-> J ping-pong.  Every rank swaps in lockstep, so the mapped peer buffers swap too.
static void swap_buffers(sdp_problem *p)
{
    std::swap(p->V.p, p->J.p);
    std::swap(p->V.ever_exported, p->J.ever_exported);
    std::swap(p->V_partial, p->J_partial);
    ++p->V_gen;
    if (p->peer_exchange) p->peer_V.swap(p->peer_J);
}

extern "C" int sdp_problem_swap(sdp_problem *p)
{
    if (!p) return fail(SDP_EINVAL, "NULL problem");
    swap_buffers(p);
    return SDP_OK;
}

extern "C" int sdp_problem_eval_policy(sdp_problem *p, int32_t n_iter, int rel_dp,
                                       int64_t ref_index, double *J_ref_out)
{
    if (!p) return fail(SDP_EINVAL, "NULL problem");
    p->peer_fence = true;                // first backup of a call (open_pushes)
    if (n_iter < 0) return fail(SDP_EINVAL, "negative iteration count");
    if (!p->pol_in.p) return fail(SDP_EINVAL, "no policy set (sdp_problem_set_policy)");
    int rc;
    if ((rc = check_ref(p, rel_dp, ref_index))) return rc;
    if ((rc = ensure_refs(p, n_iter))) return rc;
    if (n_iter == 0) {                   // result = the starting value (stodynprog.py:714)
        HIP_TRY(hipMemcpyAsync(p->J.p, p->V.p, p->S * real_size(p->dtype), hipMemcpyDeviceToDevice, p->stream));
        HIP_TRY(hipStreamSynchronize(p->stream));
        return SDP_OK;
    }
    HIP_TRY(hipEventRecord(p->ev0, p->stream));
    // Relative DP (stodynprog.py:760-762) without writing the shifted array out
    // between steps: step k leaves the raw J_k in the J buffer; step k+1 reads
    // every vertex as V - V[ref] (same single rounding as the reference's
    // in-place `J_pol -= J_ref[k]`) and records J_ref[k] = V[ref]; only the last
    // step is followed by the explicit shift kernels.  One launch per step
    // instead of three.
    double *refs = (double *)p->refs.p;
    for (int k = 0; k < n_iter; ++k) {
        if (k > 0) swap_buffers(p);
        const bool fused = rel_dp && k > 0;
        if ((rc = run_backup(p, true, 0.0, fused ? ref_index : -1, fused ? refs + (k - 1) : nullptr))) return rc;
        if ((rc = join_comm(p))) return rc;
    }
    if (rel_dp && (rc = rel_shift(p, ref_index, n_iter - 1))) return rc;
    HIP_TRY(hipEventRecord(p->ev1, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, p->ev0, p->ev1));
    p->last_kernel_ms = ms;
    if (rel_dp && J_ref_out) HIP_TRY(hipMemcpy(J_ref_out, p->refs.p, (size_t)n_iter * 8, hipMemcpyDeviceToHost));
    return SDP_OK;
}

// dmin / dmax of J (the last backup) against V (the one before) over the nodes this rank computes -- the ranges of
// its parts, or [node_begin, node_end) -- with J / V shifted by their node ra / rb (device order, < 0: not shifted;
// k_diff_stats).  Several ranks: every rank's 3 key words are all-gathered and combined the same way on every rank,
// so all of them hold the same bits and take the same decision.  Reads back a few bytes: one synchronisation.
static int diff_stats(sdp_problem *p, int64_t ra, int64_t rb, double &dmin, double &dmax)
{
    const int n = p->comm ? p->comm->nranks : 1, me = p->comm ? p->comm->rank : 0;
    int rc;
    if (!p->stats.p && (rc = p->stats.alloc(3 * 8))) return rc;
    std::vector<std::pair<int64_t, int64_t>> ranges;
    if (!p->comm) {
        ranges.emplace_back(p->node_begin, p->node_end);
    } else {
        for (int ph = 0; ph < p->n_phases; ++ph) {
            const int64_t *b = p->parts.data() + (size_t)ph * (n + 1);
            if (b[me + 1] > b[me]) ranges.emplace_back(b[me], b[me + 1]);
        }
    }
    HIP_TRY(hipMemsetAsync(p->stats.p, 0, 3 * 8, p->stream));
    const int vec = p->dtype == SDP_F32 ? 4 : 2;
    for (size_t k0 = 0; k0 < ranges.size() || k0 == 0; k0 += SDP_STAT_RANGES) {
        SdpStatRanges r;
        r.n = 0;
        int64_t nodes = 0;
        for (size_t k = k0; k < ranges.size() && r.n < SDP_STAT_RANGES; ++k, ++r.n) {
            r.b[r.n] = ranges[k].first;
            r.e[r.n] = ranges[k].second;
            nodes += ranges[k].second - ranges[k].first;
        }
        // (four workgroups per CU: 64 us at 256^3 fp64 against 110 us with sixteen, which also meet 4 x as many atomics
        // on the three words)
        int64_t blocks = (nodes / vec + 255) / 256;
        if (blocks > (int64_t)p->cus * 4) blocks = (int64_t)p->cus * 4;
        if (blocks < 1) blocks = 1;
        unsigned long long *acc = (unsigned long long *)p->stats.p;
        if (p->dtype == SDP_F32)
            hipLaunchKernelGGL(k_diff_stats<float>, dim3((unsigned)blocks), dim3(256), 0, p->stream,
                               (const float *)p->J.p, (const float *)p->V.p, ra, rb, r, acc);
        else
            hipLaunchKernelGGL(k_diff_stats<double>, dim3((unsigned)blocks), dim3(256), 0, p->stream,
                               (const double *)p->J.p, (const double *)p->V.p, ra, rb, r, acc);
        HIP_TRY(hipGetLastError());
    }
    std::vector<unsigned long long> keys((size_t)n * 3, 0ull);
    if (n > 1) {
        if (!p->stats_all.p && (rc = p->stats_all.alloc((size_t)n * 3 * 8))) return rc;
        if (!p->ev_stats) HIP_TRY(hipEventCreateWithFlags(&p->ev_stats, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(p->ev_stats, p->stream));
        HIP_TRY(hipStreamWaitEvent(p->comm->stream, p->ev_stats, 0));
        NCCL_TRY(g_rccl.AllGather(p->stats.p, p->stats_all.p, 3, NCCL_FLOAT64, p->comm->comm, p->comm->stream));
        HIP_TRY(hipMemcpyAsync(keys.data(), p->stats_all.p, (size_t)n * 3 * 8, hipMemcpyDeviceToHost, p->comm->stream));
        HIP_TRY(hipStreamSynchronize(p->comm->stream));
    } else {
        HIP_TRY(hipMemcpyAsync(keys.data(), p->stats.p, 3 * 8, hipMemcpyDeviceToHost, p->stream));
        HIP_TRY(hipStreamSynchronize(p->stream));
    }
    unsigned long long kmin = 0, kmax = 0, knan = 0;
    for (int q = 0; q < n; ++q) {
        kmin = std::max(kmin, keys[(size_t)q * 3]);
        kmax = std::max(kmax, keys[(size_t)q * 3 + 1]);
        knan |= keys[(size_t)q * 3 + 2];
    }
    dmin = knan ? NAN : sdp_key_value(~kmin);
    dmax = knan ? NAN : sdp_key_value(kmax);
    return SDP_OK;
}

// The loops of sdp_problem_vi_sweep + sdp_problem_swap and of sdp_problem_eval_policy, queued back to back, with the
// convergence check after sweeps c, 2c, ... and after the last allowed one.
static int iterate_until(sdp_problem *p, bool evalpol, int32_t n_max, int rel_dp, int64_t ref_index,
                         int32_t check_every, double tol, int32_t *n_done, double *stats, double *J_ref_out)
{
    if (!p || !n_done || !stats) return fail(SDP_EINVAL, "NULL argument");
    if (n_max < 1) return fail(SDP_EINVAL, "n_max must be at least 1");
    if (check_every < 1) return fail(SDP_EINVAL, "check_every must be at least 1");
    if (!(tol >= 0)) return fail(SDP_EINVAL, "tol must be a number >= 0");
    if (evalpol && !p->pol_in.p) return fail(SDP_EINVAL, "no policy set (sdp_problem_set_policy)");
    int rc;
    if ((rc = check_ref(p, rel_dp, ref_index))) return rc;
    if ((rc = ensure_refs(p, n_max))) return rc;
    p->peer_fence = true;                // first backup of a call (open_pushes)
    double *refs = (double *)p->refs.p;
    int32_t done = 0, checks = 0;
    HIP_TRY(hipEventRecord(p->ev0, p->stream));
    for (int32_t k = 0; k < n_max; ++k) {
        if (k > 0) swap_buffers(p);
        if (evalpol) {
            // the fused relative shift of sdp_problem_eval_policy: step k > 0 reads V - V[ref], J holds raw values
            const bool fused = rel_dp && k > 0;
            if ((rc = run_backup(p, true, 0.0, fused ? ref_index : -1, fused ? refs + (k - 1) : nullptr))) return rc;
            if ((rc = join_comm(p))) return rc;
        } else {
            p->peer_fence = true;        // every sweep is one sdp_problem_vi_sweep call of the host loop
            if ((rc = run_backup(p, false, 0.0))) return rc;
            if ((rc = join_comm(p))) return rc;
            if (rel_dp && (rc = rel_shift(p, ref_index, k))) return rc;
        }
        done = k + 1;
        if (done % check_every == 0 || done == n_max) {
            // the statistics are those of the shifted sequence: the evaluation shifts both buffers here
            const int64_t ra = evalpol && rel_dp ? ref_index : -1, rb = evalpol && rel_dp && k > 0 ? ref_index : -1;
            double dmin, dmax;
            if ((rc = diff_stats(p, ra, rb, dmin, dmax))) return rc;
            stats[2 * checks] = dmin;
            stats[2 * checks + 1] = dmax;
            ++checks;
            if (dmax - dmin <= tol) break;                  // NaN never converges
        }
    }
    if (evalpol && rel_dp && (rc = rel_shift(p, ref_index, done - 1))) return rc;
    HIP_TRY(hipEventRecord(p->ev1, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, p->ev0, p->ev1));
    p->last_kernel_ms = ms;
    *n_done = done;
    if (rel_dp && J_ref_out) HIP_TRY(hipMemcpy(J_ref_out, p->refs.p, (size_t)done * 8, hipMemcpyDeviceToHost));
    return SDP_OK;
}

extern "C" int sdp_problem_vi_until(sdp_problem *p, int32_t n_max, int rel_dp, int64_t ref_index,
                                    int32_t check_every, double tol, int32_t *n_done, double *stats,
                                    double *J_ref_out)
{
    return iterate_until(p, false, n_max, rel_dp, ref_index, check_every, tol, n_done, stats, J_ref_out);
}

extern "C" int sdp_problem_eval_policy_until(sdp_problem *p, int32_t n_max, int rel_dp, int64_t ref_index,
                                             int32_t check_every, double tol, int32_t *n_done, double *stats,
                                             double *J_ref_out)
{
    return iterate_until(p, true, n_max, rel_dp, ref_index, check_every, tol, n_done, stats, J_ref_out);
}

// ---------------------------------------------------------------------------
// pinned host memory for the arrays that cross the API every call
// (DPSolver.value_iteration takes and returns numpy arrays, stodynprog.py:466,
// 494-498, 530-533): copies to and from page-locked memory run as one DMA at
// PCIe rate and asynchronously; pageable memory is staged by the runtime
// ---------------------------------------------------------------------------
extern "C" int sdp_host_alloc(size_t bytes, void **out)
{
    if (!out) return fail(SDP_EINVAL, "NULL argument");
    *out = nullptr;
    hipError_t e = hipHostMalloc(out, bytes ? bytes : 8, hipHostMallocDefault);
    if (e != hipSuccess) { *out = nullptr; return fail(SDP_ENOMEM, "hipHostMalloc(%zu bytes): %s", bytes, hipGetErrorString(e)); }
    return SDP_OK;
}

extern "C" int sdp_host_free(void *ptr)
{
    if (ptr) HIP_TRY(hipHostFree(ptr));
    return SDP_OK;
}

// device buffer in the handle's layout -> host (reference C order), enqueued on the
// problem stream WITHOUT a synchronisation; `slot` picks the conversion buffer
static int download_nodes_async(sdp_problem *p, void *host, const void *dev, size_t elem_bytes, int slot)
{
    const size_t bytes = (size_t)p->S * elem_bytes;
    if (p->layout != SDP_LAYOUT_COLUMNS) {
        HIP_TRY(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, p->stream));
        return SDP_OK;
    }
    if (p->stage_bytes[slot] < bytes) {
        int rc = p->stage[slot].alloc(bytes);
        if (rc) { p->stage_bytes[slot] = 0; return rc; }
        p->stage_bytes[slot] = bytes;
    }
    int rc = launch_transpose(dev, p->stage[slot].p, p->S / p->orders[0], p->orders[0],
                              (int)(elem_bytes / 4), p->stream);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(host, p->stage[slot].p, bytes, hipMemcpyDeviceToHost, p->stream));
    return SDP_OK;
}

static int gather_policy(sdp_problem *p);

// Rows [nb, ne) (device order) of a per-node array -> their place in the host array
// (reference C order), enqueued on `stream`.  Node layout: one contiguous copy.  Column
// layout: the rows are whole columns c0 .. c1-1, i.e. the host sub-block [:, c0:c1] of the
// [N0][P] array: transposed into the dense [N0][c1-c0] part of the conversion buffer, then
// one strided 2-D copy.
static int download_range_async(sdp_problem *p, void *host, const void *dev, size_t elem_bytes, int slot,
                                int64_t nb, int64_t ne, hipStream_t stream)
{
    if (ne <= nb) return SDP_OK;
    if (p->layout != SDP_LAYOUT_COLUMNS) {
        HIP_TRY(hipMemcpyAsync((char *)host + nb * elem_bytes, (const char *)dev + nb * elem_bytes,
                               (size_t)(ne - nb) * elem_bytes, hipMemcpyDeviceToHost, stream));
        return SDP_OK;
    }
    const size_t bytes = (size_t)p->S * elem_bytes;
    if (p->stage_bytes[slot] < bytes) {
        int rc = p->stage[slot].alloc(bytes);
        if (rc) { p->stage_bytes[slot] = 0; return rc; }
        p->stage_bytes[slot] = bytes;
    }
    const int64_t n0 = p->orders[0], P = p->S / n0, c0 = nb / n0, c1 = ne / n0;
    char *dense = (char *)p->stage[slot].p + (size_t)nb * elem_bytes;          // [N0][c1-c0]
    int rc = launch_transpose((const char *)dev + nb * elem_bytes, dense, c1 - c0, n0,
                              (int)(elem_bytes / 4), stream);
    if (rc) return rc;
    HIP_TRY(hipMemcpy2DAsync((char *)host + c0 * elem_bytes, (size_t)P * elem_bytes, dense,
                             (size_t)(c1 - c0) * elem_bytes, (size_t)(c1 - c0) * elem_bytes, (size_t)n0,
                             hipMemcpyDeviceToHost, stream));
    return SDP_OK;
}

// One value_iteration call with host arrays in and out (stodynprog.py:466-534):
// upload of J_next (skipped when host_V is NULL: the device keeps its value buffer),
// the backup, the relative-DP shift and the downloads of J_k and the policy values
// are queued back to back on the problem stream; ONE synchronisation at the end.
extern "C" int sdp_problem_backup_host(sdp_problem *p, const void *host_V, double t_k, int rel_dp,
                                       int64_t ref_index, void *host_J, void *host_pol,
                                       int32_t *host_idx, double *J_ref_out)
{
    if (!p || !host_J) return fail(SDP_EINVAL, "NULL argument");
    p->peer_fence = true;                // first backup of a call (open_pushes)
    int rc;
    if ((rc = check_ref(p, rel_dp, ref_index))) return rc;
    if ((rc = ensure_refs(p, 1))) return rc;
    const size_t rs = real_size(p->dtype);
    if (host_V) {
        const size_t bytes = (size_t)p->S * rs;
        ++p->V_gen;
        if (p->layout != SDP_LAYOUT_COLUMNS) {
            HIP_TRY(hipMemcpyAsync(p->V.p, host_V, bytes, hipMemcpyHostToDevice, p->stream));
        } else {
            if ((rc = ensure_scratch(p, bytes))) return rc;
            HIP_TRY(hipMemcpyAsync(p->scratch.p, host_V, bytes, hipMemcpyHostToDevice, p->stream));
            if ((rc = launch_transpose(p->scratch.p, p->V.p, p->orders[0], p->S / p->orders[0],
                                       (int)(rs / 4), p->stream))) return rc;
        }
    }
    // Large single-GPU problems: the backup runs in a few phases of the node range and the
    // finished rows of a phase go to the host (copy stream) UNDER the kernel of the next
    // phase, so only the last phase's download is exposed.  J waits for the relative-DP
    // shift when there is one; the policy never does.
    const int64_t unit = p->layout == SDP_LAYOUT_COLUMNS ? p->orders[0] : 1;
    const int64_t units = (p->node_end - p->node_begin) / unit;
    const int n_ph = 4;
    if (p->host_overlap && !p->comm && p->S * (int64_t)rs >= ((int64_t)8 << 20) && units >= 64 * n_ph &&
        p->node_begin == 0 && p->node_end == p->S) {
        if (!p->copy_stream) {
            HIP_TRY(hipStreamCreateWithFlags(&p->copy_stream, hipStreamNonBlocking));
            for (auto &e : p->ev_host) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&p->ev_copy, hipEventDisableTiming));
        }
        HIP_TRY(hipEventRecord(p->ev0, p->stream));
        for (int ph = 0; ph < n_ph; ++ph) {
            const int64_t nb = units * ph / n_ph * unit, ne = units * (ph + 1) / n_ph * unit;
            if ((rc = launch_sweep(p, t_k, nb, ne))) return rc;
            HIP_TRY(hipEventRecord(p->ev_host[ph], p->stream));
            HIP_TRY(hipStreamWaitEvent(p->copy_stream, p->ev_host[ph], 0));
            if (!rel_dp && (rc = download_range_async(p, host_J, p->J.p, rs, 0, nb, ne, p->copy_stream))) return rc;
            if (host_pol && (rc = download_range_async(p, host_pol, p->pol.p, (size_t)p->nu * rs, 1, nb, ne, p->copy_stream))) return rc;
            if (host_idx && (rc = download_range_async(p, host_idx, p->idx.p, 4, 2, nb, ne, p->copy_stream))) return rc;
        }
        HIP_TRY(hipEventRecord(p->ev1, p->stream));
        if (rel_dp) {
            if ((rc = rel_shift(p, ref_index, 0))) return rc;
            if ((rc = download_nodes_async(p, host_J, p->J.p, rs, 0))) return rc;    // (its own slot-0 buffer use:
        }                                                                             //  no phase copy of J is in flight)
        HIP_TRY(hipStreamSynchronize(p->copy_stream));
        HIP_TRY(hipStreamSynchronize(p->stream));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, p->ev0, p->ev1));
        p->last_kernel_ms = ms;
        if (rel_dp && J_ref_out) HIP_TRY(hipMemcpy(J_ref_out, p->refs.p, 8, hipMemcpyDeviceToHost));
        return SDP_OK;
    }
    HIP_TRY(hipEventRecord(p->ev0, p->stream));
    if ((rc = run_backup(p, false, t_k, -1, nullptr, true))) return rc;    // J goes to the host: all rows to all ranks
    HIP_TRY(hipEventRecord(p->ev1, p->stream));
    if ((rc = join_comm(p))) return rc;
    if (rel_dp && (rc = rel_shift(p, ref_index, 0))) return rc;
    if ((rc = download_nodes_async(p, host_J, p->J.p, rs, 0))) return rc;
    if (host_pol || host_idx) {
        if (p->comm && p->comm->nranks > 1 && (rc = gather_policy(p))) return rc;   // collective, synchronises
        if (host_pol && (rc = download_nodes_async(p, host_pol, p->pol.p, (size_t)p->nu * rs, 1))) return rc;
        if (host_idx && (rc = download_nodes_async(p, host_idx, p->idx.p, 4, 2))) return rc;
    }
    HIP_TRY(hipStreamSynchronize(p->stream));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, p->ev0, p->ev1));
    p->last_kernel_ms = ms;
    if (rel_dp && J_ref_out) HIP_TRY(hipMemcpy(J_ref_out, p->refs.p, 8, hipMemcpyDeviceToHost));
    return SDP_OK;
}

extern "C" int sdp_problem_set_host_overlap(sdp_problem *p, int on)
{
    if (!p) return fail(SDP_EINVAL, "NULL problem");
    p->host_overlap = on ? 1 : 0;
    return SDP_OK;
}

// Batched closed-loop simulation on the device (kernel sdp_simulate of the model's code
// object): see include/sdp_hip.h.
extern "C" int sdp_problem_simulate(sdp_problem *p, const void *host_pol, int64_t B, int64_t T,
                                    const void *host_x0, const void *host_w, double t0,
                                    void *host_x, void *host_u, void *host_g)
{
    if (!p || !host_pol || !host_x0 || !host_x || !host_u) return fail(SDP_EINVAL, "NULL argument");
    if (B < 0 || T < 0) return fail(SDP_EINVAL, "negative size");
    if (!p->f_simulate) return fail(SDP_EMODULE, "the model's code object has no sdp_simulate kernel");
    if (p->W > 0 && T > 0 && !host_w) return fail(SDP_EINVAL, "a stochastic system needs the perturbation sequences");
    if (B == 0) return SDP_OK;
    const size_t rs = real_size(p->dtype);
    DevBuf dpol, dx0, dw, dx, du, dg;
    int rc;
    if ((rc = upload(dpol, host_pol, (size_t)p->nu * p->S * rs))) return rc;
    if ((rc = upload(dx0, host_x0, (size_t)p->d * B * rs))) return rc;
    if (host_w && T > 0 && (rc = upload(dw, host_w, (size_t)T * (p->n_perturb > 1 ? p->n_perturb : 1) * B * rs))) return rc;     // [T][n_perturb][B]
    if ((rc = dx.alloc((size_t)(T + 1) * p->d * B * rs))) return rc;
    if ((rc = du.alloc((size_t)T * p->nu * B * rs))) return rc;
    if (host_g && (rc = dg.alloc((size_t)T * B * rs))) return rc;
    SdpSimArgs a;
    memset(&a, 0, sizeof(a));
    a.pol = dpol.p; a.axes = p->axes.p; a.x0 = dx0.p; a.w = (host_w && T > 0) ? dw.p : nullptr;
    a.x = dx.p; a.u = du.p; a.g = host_g ? dg.p : nullptr;
    a.B = B; a.T = T; a.S = p->S; a.t0 = t0;
    for (int k = 0; k < SDP_MAXD; ++k) { a.orders[k] = p->orders[k]; a.axis_off[k] = p->axis_off[k]; }
    size_t size = sizeof(a);
    void *extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a, HIP_LAUNCH_PARAM_BUFFER_SIZE, &size,
                     HIP_LAUNCH_PARAM_END};
    int64_t blocks = (B + 63) / 64;
    if (blocks > (int64_t)p->cus * 32) blocks = (int64_t)p->cus * 32;
    HIP_TRY(hipStreamSynchronize(p->stream));        // lifted constants set on the problem stream
    HIP_TRY(hipEventRecord(p->ev0, p->stream));
    HIP_TRY(hipModuleLaunchKernel(p->f_simulate, (unsigned)blocks, 1, 1, 64, 1, 1, 0, p->stream, nullptr, extra));
    HIP_TRY(hipEventRecord(p->ev1, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, p->ev0, p->ev1));
    p->last_kernel_ms = ms;
    HIP_TRY(hipMemcpy(host_x, dx.p, (size_t)(T + 1) * p->d * B * rs, hipMemcpyDeviceToHost));
    if (T > 0) HIP_TRY(hipMemcpy(host_u, du.p, (size_t)T * p->nu * B * rs, hipMemcpyDeviceToHost));
    if (host_g && T > 0) HIP_TRY(hipMemcpy(host_g, dg.p, (size_t)T * B * rs, hipMemcpyDeviceToHost));
    return SDP_OK;
}

// Monte Carlo policy evaluation on the device (kernel sdp_montecarlo of the model's code object):
// see include/sdp_hip.h.  The policy goes up once, the run is cut into launches of at most
// steps_per_launch steps with the state in device buffers between them, the reductions come back once.
extern "C" int sdp_problem_montecarlo(sdp_problem *p, const void *host_pol, int64_t B, int64_t T, int64_t n_burn,
                                      uint64_t seed, uint64_t traj_offset, const void *host_x0,
                                      const double *host_cum, int32_t n_law, const void *host_law_grid, double t0,
                                      int64_t steps_per_launch, void *host_cost_sum, int64_t *host_n_outside,
                                      void *host_x_final, uint64_t *host_occupancy)
{
    if (!p || !host_pol || !host_x0 || !host_cum || !host_law_grid || !host_cost_sum || !host_n_outside || !host_x_final)
        return fail(SDP_EINVAL, "NULL argument");
    if (B < 0 || T < 0) return fail(SDP_EINVAL, "negative size");
    if (n_burn < 0 || n_burn > T) return fail(SDP_EINVAL, "n_burn = %lld outside [0, %lld]", (long long)n_burn, (long long)T);
    if (steps_per_launch < 1) return fail(SDP_EINVAL, "steps_per_launch = %lld: at least 1", (long long)steps_per_launch);
    if (p->W <= 0) return fail(SDP_EINVAL, "a deterministic system has nothing to draw: use sdp_problem_simulate");
    if (n_law < 1 || n_law > 4096) return fail(SDP_EINVAL, "a law of %d points: 1 to 4096", (int)n_law);
    if (p->comm && p->comm->nranks > 1) return fail(SDP_EINVAL, "Monte Carlo evaluation runs on one GPU");
    if (!p->f_montecarlo) return fail(SDP_EMODULE, "the model's code object has no sdp_montecarlo kernel");
    if (B == 0) return SDP_OK;
    if (steps_per_launch > ((int64_t)1 << 30)) steps_per_launch = (int64_t)1 << 30;       // (the kernel counts a launch's steps in 32 bits)
    const size_t rs = real_size(p->dtype);
    const size_t nw = p->n_perturb > 1 ? (size_t)p->n_perturb : 1;
    // (the draw table in LDS: the cumulative sums, then the values of every variable)
    if ((size_t)(n_law - 1) * 8 + nw * n_law * rs > 65536)
        return fail(SDP_EINVAL, "a law of %d points of %d variables needs %zu bytes of LDS: at most 65536", (int)n_law, (int)nw, (size_t)(n_law - 1) * 8 + nw * n_law * rs);
    DevBuf dpol, dx, dacc, dout, dcum, dlaw, docc;
    int rc;
    if ((rc = upload(dpol, host_pol, (size_t)p->nu * p->S * rs))) return rc;
    if ((rc = upload(dx, host_x0, (size_t)p->d * B * rs))) return rc;
    if ((rc = upload(dcum, host_cum, (size_t)n_law * 8))) return rc;
    if ((rc = upload(dlaw, host_law_grid, (size_t)nw * n_law * rs))) return rc;      // [n_perturb][n_law]
    if ((rc = dacc.alloc((size_t)B * rs))) return rc;
    if ((rc = dout.alloc((size_t)B * 8))) return rc;
    HIP_TRY(hipMemsetAsync(dacc.p, 0, (size_t)B * rs, p->stream));
    HIP_TRY(hipMemsetAsync(dout.p, 0, (size_t)B * 8, p->stream));
    if (host_occupancy) {
        if ((rc = docc.alloc((size_t)p->S * 8))) return rc;
        HIP_TRY(hipMemsetAsync(docc.p, 0, (size_t)p->S * 8, p->stream));
    }
    SdpMcArgs a;
    memset(&a, 0, sizeof(a));
    a.pol = dpol.p; a.axes = p->axes.p; a.cum = (const double *)dcum.p; a.law_grid = dlaw.p;
    a.x = dx.p; a.acc = dacc.p; a.n_outside = (long long *)dout.p;
    a.occupancy = host_occupancy ? (unsigned long long *)docc.p : nullptr;
    a.B = B; a.S = p->S; a.seed = seed; a.traj_offset = traj_offset; a.n_burn = n_burn; a.t0 = t0; a.n_law = n_law;
    for (int k = 0; k < SDP_MAXD; ++k) { a.orders[k] = p->orders[k]; a.axis_off[k] = p->axis_off[k]; }
    size_t size = sizeof(a);
    void *extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a, HIP_LAUNCH_PARAM_BUFFER_SIZE, &size,
                     HIP_LAUNCH_PARAM_END};
    // one lane per trajectory; at most the workgroups of 256 that are resident at once (the kernel's registers and the
    // draw table decide how many a CU holds: 8 for the small models, 5 or 6 for the large ones), the rest in a
    // grid-stride loop
    const int threads = 256;
    const unsigned lds = (unsigned)((size_t)(n_law - 1) * 8 + nw * n_law * rs);      // cumulative table, then the values
    int per_cu = 0;
    if (hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, p->f_montecarlo, threads, lds) != hipSuccess) {
        (void)hipGetLastError();
        per_cu = 0;
    }
    if (per_cu < 1) per_cu = 1;
    if (per_cu > 8) per_cu = 8;
    int64_t blocks = (B + threads - 1) / threads;
    if (blocks > (int64_t)p->cus * per_cu) blocks = (int64_t)p->cus * per_cu;
    HIP_TRY(hipStreamSynchronize(p->stream));        // lifted constants set on the problem stream
    HIP_TRY(hipEventRecord(p->ev0, p->stream));
    for (int64_t k = 0; k < T; k += steps_per_launch) {
        a.step_begin = k;
        a.step_end = (T - k < steps_per_launch) ? T : k + steps_per_launch;
        HIP_TRY(hipModuleLaunchKernel(p->f_montecarlo, (unsigned)blocks, 1, 1, threads, 1, 1, lds, p->stream, nullptr, extra));
    }
    HIP_TRY(hipEventRecord(p->ev1, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, p->ev0, p->ev1));
    p->last_kernel_ms = ms;
    HIP_TRY(hipMemcpy(host_cost_sum, dacc.p, (size_t)B * rs, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(host_n_outside, dout.p, (size_t)B * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(host_x_final, dx.p, (size_t)p->d * B * rs, hipMemcpyDeviceToHost));
    if (host_occupancy) HIP_TRY(hipMemcpy(host_occupancy, docc.p, (size_t)p->S * 8, hipMemcpyDeviceToHost));
    return SDP_OK;
}

// ---- the same two loops under a time-indexed policy (kernels sdp_simulate_h / sdp_montecarlo_h of the model's code
// object, csrc/sdp_horizon_kernel.h): see include/sdp_hip.h.  The policy [n_pol_steps][nu][S] goes up a CHUNK of whole
// steps at a time (at most chunk_bytes; a step larger than that is a chunk of its own), every chunk is run before
// the next one is uploaded, and the state -- for Monte Carlo also the sums -- stays in device buffers in between.
static int horizon_checks(sdp_problem *p, const char *what, int64_t n_pol_steps, int64_t T, const void *host_prm,
                          int32_t n_params, int64_t chunk_bytes)
{
    if (n_pol_steps != T) return fail(SDP_EINVAL, "%s: %lld policy steps for %lld steps", what, (long long)n_pol_steps, (long long)T);
    if (chunk_bytes < 1) return fail(SDP_EINVAL, "%s: chunk_bytes = %lld: at least 1", what, (long long)chunk_bytes);
    if (n_params < 0 || (n_params > 0 && !host_prm)) return fail(SDP_EINVAL, "%s: bad parameter table", what);
    if ((size_t)n_params * real_size(p->dtype) != p->prm_bytes)
        return fail(SDP_EINVAL, "%s: the code object declares %zu parameter(s) per step, the table has %d", what,
                    p->prm_bytes / real_size(p->dtype), (int)n_params);
    return SDP_OK;
}

// steps of policy that one chunk holds
static int64_t horizon_chunk_steps(const sdp_problem *p, int64_t T, int64_t chunk_bytes)
{
    const size_t step_bytes = (size_t)p->nu * p->S * real_size(p->dtype);
    int64_t n = (int64_t)((size_t)chunk_bytes / step_bytes);
    if (n < 1) n = 1;
    if (n > T) n = T;
    return n;
}

extern "C" int sdp_problem_simulate_h(sdp_problem *p, int64_t n_pol_steps, const void *host_pol, const void *host_prm,
                                      int32_t n_params, int64_t chunk_bytes, int64_t B, int64_t T,
                                      const void *host_x0, const void *host_w, double t0,
                                      void *host_x, void *host_u, void *host_g)
{
    if (!p || !host_pol || !host_x0 || !host_x || !host_u) return fail(SDP_EINVAL, "NULL argument");
    if (B < 0 || T < 0) return fail(SDP_EINVAL, "negative size");
    int rc;
    if ((rc = horizon_checks(p, "sdp_problem_simulate_h", n_pol_steps, T, host_prm, n_params, chunk_bytes))) return rc;
    if (p->comm && p->comm->nranks > 1) return fail(SDP_EINVAL, "a time-indexed simulation runs on one GPU");
    if (!p->f_simulate_h) return fail(SDP_EMODULE, "the model's code object has no sdp_simulate_h kernel (built before the time-indexed loops)");
    if (p->W > 0 && T > 0 && !host_w) return fail(SDP_EINVAL, "a stochastic system needs the perturbation sequences");
    if (B == 0) return SDP_OK;
    const size_t rs = real_size(p->dtype);
    const size_t step_bytes = (size_t)p->nu * p->S * rs;
    const int64_t per_chunk = T > 0 ? horizon_chunk_steps(p, T, chunk_bytes) : 0;
    DevBuf dpol, dprm, dw, dx, du, dg;
    if (T > 0 && (rc = dpol.alloc((size_t)per_chunk * step_bytes))) return rc;
    if (n_params > 0 && T > 0 && (rc = upload(dprm, host_prm, (size_t)T * n_params * rs))) return rc;
    if (host_w && T > 0 && (rc = upload(dw, host_w, (size_t)T * (p->n_perturb > 1 ? p->n_perturb : 1) * B * rs))) return rc;     // [T][n_perturb][B]
    if ((rc = dx.alloc((size_t)(T + 1) * p->d * B * rs))) return rc;
    if ((rc = du.alloc((size_t)T * p->nu * B * rs))) return rc;
    if (host_g && (rc = dg.alloc((size_t)T * B * rs))) return rc;
    HIP_TRY(hipMemcpy(dx.p, host_x0, (size_t)p->d * B * rs, hipMemcpyHostToDevice));       // row 0 of x
    SdpSimHArgs a;
    memset(&a, 0, sizeof(a));
    a.pol = dpol.p; a.prm = (n_params > 0 && T > 0) ? dprm.p : nullptr; a.axes = p->axes.p;
    a.w = (host_w && T > 0) ? dw.p : nullptr;
    a.x = dx.p; a.u = du.p; a.g = host_g ? dg.p : nullptr;
    a.B = B; a.S = p->S; a.t0 = t0;
    for (int k = 0; k < SDP_MAXD; ++k) { a.orders[k] = p->orders[k]; a.axis_off[k] = p->axis_off[k]; }
    size_t size = sizeof(a);
    void *extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a, HIP_LAUNCH_PARAM_BUFFER_SIZE, &size,
                     HIP_LAUNCH_PARAM_END};
    int64_t blocks = (B + 63) / 64;
    if (blocks > (int64_t)p->cus * 32) blocks = (int64_t)p->cus * 32;
    HIP_TRY(hipStreamSynchronize(p->stream));
    double kernel_ms = 0;
    for (int64_t k = 0; k < T; k += per_chunk) {
        const int64_t n = (T - k < per_chunk) ? T - k : per_chunk;
        // (the kernel of the previous chunk has finished: the stream is synchronised at the end of every round)
        HIP_TRY(hipMemcpy(dpol.p, (const char *)host_pol + (size_t)k * step_bytes, (size_t)n * step_bytes, hipMemcpyHostToDevice));
        a.chunk_first = k; a.step_begin = k; a.step_end = k + n;
        HIP_TRY(hipEventRecord(p->ev0, p->stream));
        HIP_TRY(hipModuleLaunchKernel(p->f_simulate_h, (unsigned)blocks, 1, 1, 64, 1, 1, 0, p->stream, nullptr, extra));
        HIP_TRY(hipEventRecord(p->ev1, p->stream));
        HIP_TRY(hipStreamSynchronize(p->stream));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, p->ev0, p->ev1));
        kernel_ms += ms;
    }
    p->last_kernel_ms = kernel_ms;
    HIP_TRY(hipMemcpy(host_x, dx.p, (size_t)(T + 1) * p->d * B * rs, hipMemcpyDeviceToHost));
    if (T > 0) HIP_TRY(hipMemcpy(host_u, du.p, (size_t)T * p->nu * B * rs, hipMemcpyDeviceToHost));
    if (host_g && T > 0) HIP_TRY(hipMemcpy(host_g, dg.p, (size_t)T * B * rs, hipMemcpyDeviceToHost));
    return SDP_OK;
}

// ---------------------------------------------------------------------------
// One-step lookahead at arbitrary states (kernels sdp_lookahead / sdp_simulate_lookahead of a lookahead unit,
// csrc/sdp_lookahead_kernel.h): see include/sdp_hip.h.
// ---------------------------------------------------------------------------
static int lookahead_checks(sdp_problem *p, const char *what, bool device_box, const double *steps)
{
    if (p->comm && p->comm->nranks > 1) return fail(SDP_EINVAL, "%s runs on one GPU", what);
    if (p->layout != SDP_LAYOUT_NODES) return fail(SDP_EINVAL, "%s: a lookahead unit is in node order", what);
    if (!p->f_lookahead) return fail(SDP_EMODULE, "%s: the model's code object is not a lookahead unit (no sdp_lookahead kernel)", what);
    if (device_box) {
        if (!p->f_simulate_lookahead) return fail(SDP_EMODULE, "%s: the code object has no box function of its own (built without SDP_LOOKAHEAD_BOX)", what);
        if (!steps) return fail(SDP_EINVAL, "%s: a lattice made on the device needs the control step hints", what);
        for (int c = 0; c < p->nu; ++c)
            if (!(steps[c] == steps[c])) return fail(SDP_EINVAL, "%s: control step hint %d is NaN", what, c);
    }
    return SDP_OK;
}

extern "C" int sdp_problem_lookahead(sdp_problem *p, const void *host_V, int64_t B, const void *host_x,
                                     const void *host_lo, const void *host_hi, const int32_t *host_n,
                                     const double *steps, double t_k, void *host_J, void *host_u, int32_t *host_idx)
{
    if (!p || !host_V || !host_x || !host_J || !host_u || !host_idx) return fail(SDP_EINVAL, "NULL argument");
    if (B < 0) return fail(SDP_EINVAL, "negative size");
    if (host_n && (!host_lo || !host_hi)) return fail(SDP_EINVAL, "sdp_problem_lookahead: box arrays without their ends");
    int rc;
    if ((rc = lookahead_checks(p, "sdp_problem_lookahead", host_n == nullptr, steps))) return rc;
    if (B == 0) return SDP_OK;
    const size_t rs = real_size(p->dtype);
    DevBuf dV, dx, dlo, dhi, dn, dJ, du, didx;
    if ((rc = upload(dV, host_V, (size_t)p->S * rs))) return rc;
    if ((rc = upload(dx, host_x, (size_t)p->d * B * rs))) return rc;
    if (host_n) {
        if ((rc = upload(dlo, host_lo, (size_t)p->nu * B * rs))) return rc;
        if ((rc = upload(dhi, host_hi, (size_t)p->nu * B * rs))) return rc;
        if ((rc = upload(dn, host_n, (size_t)p->nu * B * sizeof(int32_t)))) return rc;
    }
    if ((rc = dJ.alloc((size_t)B * rs))) return rc;
    if ((rc = du.alloc((size_t)p->nu * B * rs))) return rc;
    if ((rc = didx.alloc((size_t)B * sizeof(int32_t)))) return rc;
    SdpLookArgs a;
    memset(&a, 0, sizeof(a));
    a.V = dV.p; a.axes = p->axes.p; a.wgrid = p->wgrid.p; a.proba = p->proba.p; a.x = dx.p;
    a.box_lo = host_n ? dlo.p : nullptr; a.box_hi = host_n ? dhi.p : nullptr; a.box_n = host_n ? (const int32_t *)dn.p : nullptr;
    a.J = dJ.p; a.idx = (int32_t *)didx.p; a.u = du.p;
    a.B = B; a.S = p->S; a.t_k = t_k; a.W = p->W;
    for (int c = 0; c < p->nu && steps; ++c) a.steps[c] = steps[c];
    for (int k = 0; k < SDP_MAXD; ++k) { a.orders[k] = p->orders[k]; a.axis_off[k] = p->axis_off[k]; }
    size_t size = sizeof(a);
    void *extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a, HIP_LAUNCH_PARAM_BUFFER_SIZE, &size,
                     HIP_LAUNCH_PARAM_END};
    const unsigned blocks = sweep_blocks(p, B);          // (a multiple of 8: the kernel walks the tiles XCD by XCD)
    HIP_TRY(hipStreamSynchronize(p->stream));            // lifted constants set on the problem stream
    HIP_TRY(hipEventRecord(p->ev0, p->stream));
    HIP_TRY(hipModuleLaunchKernel(p->f_lookahead, blocks, 1, 1, 256, 1, 1, 0, p->stream, nullptr, extra));
    HIP_TRY(hipEventRecord(p->ev1, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, p->ev0, p->ev1));
    p->last_kernel_ms = ms;
    HIP_TRY(hipMemcpy(host_J, dJ.p, (size_t)B * rs, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(host_u, du.p, (size_t)p->nu * B * rs, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(host_idx, didx.p, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost));
    return SDP_OK;
}

extern "C" int sdp_problem_simulate_lookahead(sdp_problem *p, int64_t n_V_steps, const void *host_V, int64_t chunk_bytes,
                                              int64_t B, int64_t T, const void *host_x0, const void *host_w,
                                              const double *steps, double t0,
                                              void *host_x, void *host_u, void *host_g, void *host_q)
{
    if (!p || !host_V || !host_x0 || !host_x || !host_u || !host_g || !host_q) return fail(SDP_EINVAL, "NULL argument");
    if (B < 0 || T < 0) return fail(SDP_EINVAL, "negative size");
    if (n_V_steps != 0 && n_V_steps != T)
        return fail(SDP_EINVAL, "sdp_problem_simulate_lookahead: %lld cost-to-go steps for %lld steps (0: one for every step)", (long long)n_V_steps, (long long)T);
    if (chunk_bytes < 1) return fail(SDP_EINVAL, "sdp_problem_simulate_lookahead: chunk_bytes = %lld: at least 1", (long long)chunk_bytes);
    int rc;
    if ((rc = lookahead_checks(p, "sdp_problem_simulate_lookahead", true, steps))) return rc;
    if (p->prm_bytes) return fail(SDP_EINVAL, "sdp_problem_simulate_lookahead: a unit with lifted constants takes the host path");
    if (p->W > 0 && T > 0 && !host_w) return fail(SDP_EINVAL, "a stochastic system needs the perturbation sequences");
    if (B == 0) return SDP_OK;
    const size_t rs = real_size(p->dtype);
    const size_t step_bytes = (size_t)p->S * rs;
    const bool timed = n_V_steps != 0;
    int64_t per_chunk = T;
    if (timed && T > 0) {
        per_chunk = (int64_t)((size_t)chunk_bytes / step_bytes);
        if (per_chunk < 1) per_chunk = 1;
        if (per_chunk > T) per_chunk = T;
    }
    DevBuf dV, dw, dx, du, dg, dq;
    if ((rc = dV.alloc((timed ? (size_t)per_chunk : 1) * step_bytes))) return rc;
    if (!timed) HIP_TRY(hipMemcpy(dV.p, host_V, step_bytes, hipMemcpyHostToDevice));
    if (host_w && T > 0 && (rc = upload(dw, host_w, (size_t)T * (p->n_perturb > 1 ? p->n_perturb : 1) * B * rs))) return rc;     // [T][n_perturb][B]
    if ((rc = dx.alloc((size_t)(T + 1) * p->d * B * rs))) return rc;
    if ((rc = du.alloc((size_t)T * p->nu * B * rs))) return rc;
    if ((rc = dg.alloc((size_t)T * B * rs))) return rc;
    if ((rc = dq.alloc((size_t)T * B * rs))) return rc;
    HIP_TRY(hipMemcpy(dx.p, host_x0, (size_t)p->d * B * rs, hipMemcpyHostToDevice));       // row 0 of x
    SdpLookSimArgs a;
    memset(&a, 0, sizeof(a));
    a.V = dV.p; a.axes = p->axes.p; a.wgrid = p->wgrid.p; a.proba = p->proba.p;
    a.w = (host_w && T > 0) ? dw.p : nullptr;
    a.x = dx.p; a.u = du.p; a.g = dg.p; a.q = dq.p;
    a.B = B; a.S = p->S; a.V_stride = timed ? p->S : 0; a.t0 = t0; a.W = p->W;
    for (int c = 0; c < p->nu; ++c) a.steps[c] = steps[c];
    for (int k = 0; k < SDP_MAXD; ++k) { a.orders[k] = p->orders[k]; a.axis_off[k] = p->axis_off[k]; }
    size_t size = sizeof(a);
    void *extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a, HIP_LAUNCH_PARAM_BUFFER_SIZE, &size,
                     HIP_LAUNCH_PARAM_END};
    const int64_t per_block = (int64_t)(64 / p->lanes) * 4;          // trajectories of a workgroup of 256
    int64_t blocks = (B + per_block - 1) / per_block;
    if (blocks > (int64_t)p->cus * 8) blocks = (int64_t)p->cus * 8;
    HIP_TRY(hipStreamSynchronize(p->stream));
    double kernel_ms = 0;
    for (int64_t k = 0; k < T; k += per_chunk) {
        const int64_t n = (T - k < per_chunk) ? T - k : per_chunk;
        // (the kernel of the previous chunk has finished: the stream is synchronised at the end of every round)
        if (timed) HIP_TRY(hipMemcpy(dV.p, (const char *)host_V + (size_t)k * step_bytes, (size_t)n * step_bytes, hipMemcpyHostToDevice));
        a.chunk_first = timed ? k : 0; a.step_begin = k; a.step_end = k + n;
        HIP_TRY(hipEventRecord(p->ev0, p->stream));
        HIP_TRY(hipModuleLaunchKernel(p->f_simulate_lookahead, (unsigned)blocks, 1, 1, 256, 1, 1, 0, p->stream, nullptr, extra));
        HIP_TRY(hipEventRecord(p->ev1, p->stream));
        HIP_TRY(hipStreamSynchronize(p->stream));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, p->ev0, p->ev1));
        kernel_ms += ms;
    }
    p->last_kernel_ms = kernel_ms;
    HIP_TRY(hipMemcpy(host_x, dx.p, (size_t)(T + 1) * p->d * B * rs, hipMemcpyDeviceToHost));
    if (T > 0) {
        HIP_TRY(hipMemcpy(host_u, du.p, (size_t)T * p->nu * B * rs, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(host_g, dg.p, (size_t)T * B * rs, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(host_q, dq.p, (size_t)T * B * rs, hipMemcpyDeviceToHost));
    }
    return SDP_OK;
}

// Monte Carlo evaluation under lookahead controls (kernel sdp_montecarlo_lookahead): the chunks of
// sdp_problem_simulate_lookahead, the launch cuts, draw table and reductions of sdp_problem_montecarlo_h.
extern "C" int sdp_problem_montecarlo_lookahead(sdp_problem *p, int64_t n_V_steps, const void *host_V, int64_t chunk_bytes,
                                                int64_t B, int64_t T, int64_t n_burn, uint64_t seed, uint64_t traj_offset,
                                                const void *host_x0, const double *host_cum, int32_t n_law,
                                                const void *host_law_grid, const double *steps, double t0,
                                                int64_t steps_per_launch, void *host_cost_sum, int64_t *host_n_outside,
                                                void *host_x_final, uint64_t *host_occupancy)
{
    if (!p || !host_V || !host_x0 || !host_cum || !host_law_grid || !host_cost_sum || !host_n_outside || !host_x_final)
        return fail(SDP_EINVAL, "NULL argument");
    if (B < 0 || T < 0) return fail(SDP_EINVAL, "negative size");
    if (n_V_steps != 0 && n_V_steps != T)
        return fail(SDP_EINVAL, "sdp_problem_montecarlo_lookahead: %lld cost-to-go steps for %lld steps (0: one for every step)", (long long)n_V_steps, (long long)T);
    if (chunk_bytes < 1) return fail(SDP_EINVAL, "sdp_problem_montecarlo_lookahead: chunk_bytes = %lld: at least 1", (long long)chunk_bytes);
    if (n_burn < 0 || n_burn > T) return fail(SDP_EINVAL, "n_burn = %lld outside [0, %lld]", (long long)n_burn, (long long)T);
    if (steps_per_launch < 1) return fail(SDP_EINVAL, "steps_per_launch = %lld: at least 1", (long long)steps_per_launch);
    if (p->W <= 0) return fail(SDP_EINVAL, "a deterministic system has nothing to draw: use sdp_problem_simulate_lookahead");
    if (n_law < 1 || n_law > 4096) return fail(SDP_EINVAL, "a law of %d points: 1 to 4096", (int)n_law);
    int rc;
    if ((rc = lookahead_checks(p, "sdp_problem_montecarlo_lookahead", true, steps))) return rc;
    if (p->prm_bytes) return fail(SDP_EINVAL, "sdp_problem_montecarlo_lookahead: a unit with lifted constants takes the host path");
    if (!p->f_montecarlo_lookahead) return fail(SDP_EMODULE, "the model's code object has no sdp_montecarlo_lookahead kernel (built before Monte Carlo under lookahead controls)");
    if (B == 0) return SDP_OK;
    if (steps_per_launch > ((int64_t)1 << 30)) steps_per_launch = (int64_t)1 << 30;       // (the kernel counts a launch's steps in 32 bits)
    const size_t rs = real_size(p->dtype);
    const size_t nw = p->n_perturb > 1 ? (size_t)p->n_perturb : 1;
    if ((size_t)(n_law - 1) * 8 + nw * n_law * rs > 65536)
        return fail(SDP_EINVAL, "a law of %d points of %d variables needs %zu bytes of LDS: at most 65536", (int)n_law, (int)nw, (size_t)(n_law - 1) * 8 + nw * n_law * rs);
    const size_t step_bytes = (size_t)p->S * rs;
    const bool timed = n_V_steps != 0;
    int64_t per_chunk = T;
    if (timed && T > 0) {
        per_chunk = (int64_t)((size_t)chunk_bytes / step_bytes);
        if (per_chunk < 1) per_chunk = 1;
        if (per_chunk > T) per_chunk = T;
    }
    DevBuf dV, dx, dacc, dout, dcum, dlaw, docc;
    if ((rc = dV.alloc((timed ? (size_t)per_chunk : 1) * step_bytes))) return rc;
    if (!timed) HIP_TRY(hipMemcpy(dV.p, host_V, step_bytes, hipMemcpyHostToDevice));
    if ((rc = upload(dx, host_x0, (size_t)p->d * B * rs))) return rc;
    if ((rc = upload(dcum, host_cum, (size_t)n_law * 8))) return rc;
    if ((rc = upload(dlaw, host_law_grid, (size_t)nw * n_law * rs))) return rc;      // [n_perturb][n_law]
    if ((rc = dacc.alloc((size_t)B * rs))) return rc;
    if ((rc = dout.alloc((size_t)B * 8))) return rc;
    HIP_TRY(hipMemsetAsync(dacc.p, 0, (size_t)B * rs, p->stream));
    HIP_TRY(hipMemsetAsync(dout.p, 0, (size_t)B * 8, p->stream));
    if (host_occupancy) {
        if ((rc = docc.alloc((size_t)p->S * 8))) return rc;
        HIP_TRY(hipMemsetAsync(docc.p, 0, (size_t)p->S * 8, p->stream));
    }
    SdpLookMcArgs a;
    memset(&a, 0, sizeof(a));
    a.V = dV.p; a.axes = p->axes.p; a.wgrid = p->wgrid.p; a.proba = p->proba.p;
    a.cum = (const double *)dcum.p; a.law_grid = dlaw.p;
    a.x = dx.p; a.acc = dacc.p; a.n_outside = (long long *)dout.p;
    a.occupancy = host_occupancy ? (unsigned long long *)docc.p : nullptr;
    a.B = B; a.S = p->S; a.V_stride = timed ? p->S : 0; a.seed = seed; a.traj_offset = traj_offset; a.n_burn = n_burn;
    a.t0 = t0; a.W = p->W; a.n_law = n_law;
    for (int c = 0; c < p->nu; ++c) a.steps[c] = steps[c];
    for (int k = 0; k < SDP_MAXD; ++k) { a.orders[k] = p->orders[k]; a.axis_off[k] = p->axis_off[k]; }
    size_t size = sizeof(a);
    void *extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a, HIP_LAUNCH_PARAM_BUFFER_SIZE, &size,
                     HIP_LAUNCH_PARAM_END};
    // (the launch shape of sdp_problem_simulate_lookahead; the draw table in dynamic LDS: cumulative sums, then the values)
    const unsigned lds = (unsigned)((size_t)(n_law - 1) * 8 + nw * n_law * rs);
    const int64_t per_block = (int64_t)(64 / p->lanes) * 4;          // trajectories of a workgroup of 256
    int64_t blocks = (B + per_block - 1) / per_block;
    if (blocks > (int64_t)p->cus * 8) blocks = (int64_t)p->cus * 8;
    HIP_TRY(hipStreamSynchronize(p->stream));
    double kernel_ms = 0;
    for (int64_t c = 0; c < T; c += per_chunk) {
        const int64_t c_end = (T - c < per_chunk) ? T : c + per_chunk;
        // (the kernels of the previous chunk have finished: the stream is synchronised at the end of every round)
        if (timed) HIP_TRY(hipMemcpy(dV.p, (const char *)host_V + (size_t)c * step_bytes, (size_t)(c_end - c) * step_bytes, hipMemcpyHostToDevice));
        a.chunk_first = timed ? c : 0;
        HIP_TRY(hipEventRecord(p->ev0, p->stream));
        for (int64_t k = c; k < c_end; k += steps_per_launch) {
            a.step_begin = k;
            a.step_end = (c_end - k < steps_per_launch) ? c_end : k + steps_per_launch;
            HIP_TRY(hipModuleLaunchKernel(p->f_montecarlo_lookahead, (unsigned)blocks, 1, 1, 256, 1, 1, lds, p->stream, nullptr, extra));
        }
        HIP_TRY(hipEventRecord(p->ev1, p->stream));
        HIP_TRY(hipStreamSynchronize(p->stream));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, p->ev0, p->ev1));
        kernel_ms += ms;
    }
    p->last_kernel_ms = kernel_ms;
    HIP_TRY(hipMemcpy(host_cost_sum, dacc.p, (size_t)B * rs, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(host_n_outside, dout.p, (size_t)B * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(host_x_final, dx.p, (size_t)p->d * B * rs, hipMemcpyDeviceToHost));
    if (host_occupancy) HIP_TRY(hipMemcpy(host_occupancy, docc.p, (size_t)p->S * 8, hipMemcpyDeviceToHost));
    return SDP_OK;
}

extern "C" int sdp_problem_montecarlo_h(sdp_problem *p, int64_t n_pol_steps, const void *host_pol, const void *host_prm,
                                        int32_t n_params, int64_t chunk_bytes, int64_t B, int64_t T, int64_t n_burn,
                                        uint64_t seed, uint64_t traj_offset, const void *host_x0,
                                        const double *host_cum, int32_t n_law, const void *host_law_grid, double t0,
                                        int64_t steps_per_launch, void *host_cost_sum, int64_t *host_n_outside,
                                        void *host_x_final, uint64_t *host_occupancy)
{
    if (!p || !host_pol || !host_x0 || !host_cum || !host_law_grid || !host_cost_sum || !host_n_outside || !host_x_final)
        return fail(SDP_EINVAL, "NULL argument");
    if (B < 0 || T < 0) return fail(SDP_EINVAL, "negative size");
    if (n_burn < 0 || n_burn > T) return fail(SDP_EINVAL, "n_burn = %lld outside [0, %lld]", (long long)n_burn, (long long)T);
    if (steps_per_launch < 1) return fail(SDP_EINVAL, "steps_per_launch = %lld: at least 1", (long long)steps_per_launch);
    if (p->W <= 0) return fail(SDP_EINVAL, "a deterministic system has nothing to draw: use sdp_problem_simulate_h");
    if (n_law < 1 || n_law > 4096) return fail(SDP_EINVAL, "a law of %d points: 1 to 4096", (int)n_law);
    if (p->comm && p->comm->nranks > 1) return fail(SDP_EINVAL, "Monte Carlo evaluation runs on one GPU");
    int rc;
    if ((rc = horizon_checks(p, "sdp_problem_montecarlo_h", n_pol_steps, T, host_prm, n_params, chunk_bytes))) return rc;
    if (!p->f_montecarlo_h) return fail(SDP_EMODULE, "the model's code object has no sdp_montecarlo_h kernel (built before the time-indexed loops)");
    if (B == 0) return SDP_OK;
    if (steps_per_launch > ((int64_t)1 << 30)) steps_per_launch = (int64_t)1 << 30;       // (the kernel counts a launch's steps in 32 bits)
    const size_t rs = real_size(p->dtype);
    const size_t nw = p->n_perturb > 1 ? (size_t)p->n_perturb : 1;
    if ((size_t)(n_law - 1) * 8 + nw * n_law * rs > 65536)
        return fail(SDP_EINVAL, "a law of %d points of %d variables needs %zu bytes of LDS: at most 65536", (int)n_law, (int)nw, (size_t)(n_law - 1) * 8 + nw * n_law * rs);
    const size_t step_bytes = (size_t)p->nu * p->S * rs;
    const int64_t per_chunk = T > 0 ? horizon_chunk_steps(p, T, chunk_bytes) : 0;
    DevBuf dpol, dprm, dx, dacc, dout, dcum, dlaw, docc;
    if (T > 0 && (rc = dpol.alloc((size_t)per_chunk * step_bytes))) return rc;
    if (n_params > 0 && T > 0 && (rc = upload(dprm, host_prm, (size_t)T * n_params * rs))) return rc;
    if ((rc = upload(dx, host_x0, (size_t)p->d * B * rs))) return rc;
    if ((rc = upload(dcum, host_cum, (size_t)n_law * 8))) return rc;
    if ((rc = upload(dlaw, host_law_grid, (size_t)nw * n_law * rs))) return rc;      // [n_perturb][n_law]
    if ((rc = dacc.alloc((size_t)B * rs))) return rc;
    if ((rc = dout.alloc((size_t)B * 8))) return rc;
    HIP_TRY(hipMemsetAsync(dacc.p, 0, (size_t)B * rs, p->stream));
    HIP_TRY(hipMemsetAsync(dout.p, 0, (size_t)B * 8, p->stream));
    if (host_occupancy) {
        if ((rc = docc.alloc((size_t)p->S * 8))) return rc;
        HIP_TRY(hipMemsetAsync(docc.p, 0, (size_t)p->S * 8, p->stream));
    }
    SdpMcHArgs a;
    memset(&a, 0, sizeof(a));
    a.pol = dpol.p; a.prm = (n_params > 0 && T > 0) ? dprm.p : nullptr; a.axes = p->axes.p;
    a.cum = (const double *)dcum.p; a.law_grid = dlaw.p;
    a.x = dx.p; a.acc = dacc.p; a.n_outside = (long long *)dout.p;
    a.occupancy = host_occupancy ? (unsigned long long *)docc.p : nullptr;
    a.B = B; a.S = p->S; a.seed = seed; a.traj_offset = traj_offset; a.n_burn = n_burn; a.t0 = t0; a.n_law = n_law;
    for (int k = 0; k < SDP_MAXD; ++k) { a.orders[k] = p->orders[k]; a.axis_off[k] = p->axis_off[k]; }
    size_t size = sizeof(a);
    void *extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a, HIP_LAUNCH_PARAM_BUFFER_SIZE, &size,
                     HIP_LAUNCH_PARAM_END};
    // (the launch shape of sdp_problem_montecarlo)
    const int threads = 256;
    const unsigned lds = (unsigned)((size_t)(n_law - 1) * 8 + nw * n_law * rs);      // cumulative table, then the values
    int per_cu = 0;
    if (hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, p->f_montecarlo_h, threads, lds) != hipSuccess) {
        (void)hipGetLastError();
        per_cu = 0;
    }
    if (per_cu < 1) per_cu = 1;
    if (per_cu > 8) per_cu = 8;
    int64_t blocks = (B + threads - 1) / threads;
    if (blocks > (int64_t)p->cus * per_cu) blocks = (int64_t)p->cus * per_cu;
    HIP_TRY(hipStreamSynchronize(p->stream));
    double kernel_ms = 0;
    for (int64_t c = 0; c < T; c += per_chunk) {
        const int64_t c_end = (T - c < per_chunk) ? T : c + per_chunk;
        HIP_TRY(hipMemcpy(dpol.p, (const char *)host_pol + (size_t)c * step_bytes, (size_t)(c_end - c) * step_bytes, hipMemcpyHostToDevice));
        a.chunk_first = c;
        HIP_TRY(hipEventRecord(p->ev0, p->stream));
        for (int64_t k = c; k < c_end; k += steps_per_launch) {
            a.step_begin = k;
            a.step_end = (c_end - k < steps_per_launch) ? c_end : k + steps_per_launch;
            HIP_TRY(hipModuleLaunchKernel(p->f_montecarlo_h, (unsigned)blocks, 1, 1, threads, 1, 1, lds, p->stream, nullptr, extra));
        }
        HIP_TRY(hipEventRecord(p->ev1, p->stream));
        HIP_TRY(hipStreamSynchronize(p->stream));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, p->ev0, p->ev1));
        kernel_ms += ms;
    }
    p->last_kernel_ms = kernel_ms;
    HIP_TRY(hipMemcpy(host_cost_sum, dacc.p, (size_t)B * rs, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(host_n_outside, dout.p, (size_t)B * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(host_x_final, dx.p, (size_t)p->d * B * rs, hipMemcpyDeviceToHost));
    if (host_occupancy) HIP_TRY(hipMemcpy(host_occupancy, docc.p, (size_t)p->S * 8, hipMemcpyDeviceToHost));
    return SDP_OK;
}

// ---------------------------------------------------------------------------
// Transition operator of a policy (stodynprog_amd/forward.py is the definition): the CSR of P^T on the device
// and the propagation of a state distribution, mu' = P^T mu.  See include/sdp_hip.h.
//   entries  : kernel sdp_transitions of the model's code object (csrc/sdp_trans_kernel.h), or the host's
//   CSR      : a STABLE sort of the entry positions by target (rocPRIM's radix sort, on the bits a node id has),
//              a gather of the values and of the sources, row pointers from a histogram and a scan
//   k_push   : one lane per short row; k_push_group: one WAVE per row of SDP_PUSH_LONG entries or more, its lanes forming
//              the products from coalesced loads and one chain adding them in entry order.  Either way the row's
//              adds happen in entry order (the library is compiled with -ffp-contract=off: one rounded multiply and
//              one rounded add per entry), so both give the bits of forward.py
// ---------------------------------------------------------------------------
struct sdp_transop {
    int dtype = SDP_F64;
    int64_t S = 0, nnz = 0;
    DevBuf indptr, indices, data, gbar, mu[2], stats;
    DevBuf long_rows;                      // ids of the rows of long_min entries or more (k_push_group), ascending:
    int64_t n_long = 0, n_wide = 0;        //   first the n_long - n_wide below SDP_PUSH_WIDE entries, then the n_wide others
    int32_t long_min = 0;                  // 0: every row takes the lane path
    std::vector<int64_t> h_indptr;         // host copy of the row pointers (the list is made from it)
    int cur = 0;                           // mu[cur] is the resident vector
    bool has_gbar = false, has_mu = false;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr, ev3 = nullptr;
    double last_kernel_ms = 0, entries_ms = 0, sort_ms = 0;
    int cus = 256;
    // the operators of a family (sdp_family_transop_create): P block-diagonal members of Sm rows each, S = P Sm.
    // flags[p] != 0: member p is still running and a push computes its rows (both push paths test it); running: the
    // list of those members on the device, for the reduction of a check; mstats: its three key words per listed member
    int P = 0;                             // 0: a solo operator, no flags
    int64_t Sm = 0;
    DevBuf flags, running, mstats;
    bool all_running = true;               // every flag is set
    ~sdp_transop()
    {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (ev2) (void)hipEventDestroy(ev2);
        if (ev3) (void)hipEventDestroy(ev3);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

__global__ void __launch_bounds__(256) k_iota(uint32_t *__restrict__ pos, int64_t n)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) pos[i] = (uint32_t)i;
}

// data[k] = val[pos[k]], indices[k] = the source of entry pos[k]: src[pos[k]], or pos[k] / per_node without a list
template <typename real>
__global__ void __launch_bounds__(256) k_trans_gather(const uint32_t *__restrict__ pos, const real *__restrict__ val,
                                                      const int32_t *__restrict__ src, uint32_t per_node,
                                                      real *__restrict__ data, int32_t *__restrict__ indices, int64_t n)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += stride) {
        const uint32_t e = pos[k];
        data[k] = val[e];
        indices[k] = src ? src[e] : (int32_t)(e / per_node);
    }
}

// counts[t + 1] += 1 per entry of target t (integer sums do not depend on the order); counts[0] stays 0
__global__ void __launch_bounds__(256) k_trans_count(const int32_t *__restrict__ tgt, int64_t n,
                                                     unsigned long long *__restrict__ counts)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += stride)
        atomicAdd(counts + 1 + tgt[k], 1ull);
}

// A row of this many entries or more is pushed by a whole wave (k_push_group), a shorter one by one lane (k_push).
// The lane path walks a row through a chain of dependent loads, one trip to memory per entry, and a grid of S lanes
// is under two waves per SIMD on the grids this library meets (measured on Searev's 115 351 rows: 2.3 us per trip,
// 72 trips on average); a wave costs one coalesced trip per 64 entries and then adds at register speed.  From 8
// entries on the trip saved outweighs the 56 idle lanes.
#define SDP_PUSH_LONG 8

// out[t] = sum over the row of data[k] * mu[indices[k]], k ascending: acc = 0; acc = acc + data[k] * mu[..]
// (row pointers and sources are trusted: the build made them from node ids, sdp_transop_from_coo checked its own).
// Rows of long_min entries or more are left to k_push_group (long_min = 0: none is).
// MEMBERS (the operators of a family, block-diagonal with Sm rows a member): the rows of a member whose flag is 0 are not
// computed and out[t] keeps what it holds.
template <typename real, bool MEMBERS>
__global__ void __launch_bounds__(256) k_push(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                              const real *__restrict__ data, const real *__restrict__ mu,
                                              real *__restrict__ out, int64_t S, int32_t long_min,
                                              const int32_t *__restrict__ flags, int32_t Sm)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < S; t += stride) {
        if (MEMBERS && !flags[(int32_t)t / Sm]) continue;
        const int64_t b = indptr[t], e = indptr[t + 1];
        if (long_min > 0 && e - b >= long_min) continue;
        real acc = real(0);
        for (int64_t k = b; k < e; ++k) acc = acc + data[k] * mu[indices[k]];
        out[t] = acc;
    }
}

// A listed row takes a GROUP of G lanes, 64 / G rows to a wave: G entries at a time, lane l of the group forms the
// product of entry off + l (coalesced loads of data and indices, a gather of mu), then ONE chain per group adds the
// products in entry order -- acc = acc + product of lane 0, 1, .. of the group, read through a cross-lane shuffle --
// so the sum has the roundings of the lane path; positions past the row's end add nothing.  One instruction of the
// chain serves the 64 / G rows of the wave.  acc is the same in every lane of a group; its lane 0 stores it.
// G = 16 for rows below SDP_PUSH_WIDE entries, G = 64 from there on (a trip to memory per 64 entries, not per 16).
#define SDP_PUSH_WIDE 256
// MEMBERS: as in k_push -- a listed row of a member whose flag is 0 is a dead group (no loads, no store).
template <typename real, int G, bool MEMBERS>
__global__ void __launch_bounds__(256) k_push_group(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                    const real *__restrict__ data, const real *__restrict__ mu,
                                                    real *__restrict__ out, const int32_t *__restrict__ rows, int64_t n_rows,
                                                    const int32_t *__restrict__ flags, int32_t Sm)
{
    constexpr int PER = 64 / G;                                // rows of a wave
    const int lane = threadIdx.x & 63, sub = lane & (G - 1), grp = lane / G;
    const int64_t wave = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int64_t waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t w = wave; w * PER < n_rows; w += waves) {     // the same trips in every lane of a wave
        const int64_t r = w * PER + grp;
        bool live = r < n_rows;
        const int32_t t = live ? rows[r] : 0;
        if (MEMBERS && live) live = flags[t / Sm] != 0;
        int64_t b = 0, e = 0;
        if (live) { b = indptr[t]; e = indptr[t + 1]; }
        long long longest = e - b;                             // of the wave's rows: every lane runs that many chunks
#pragma unroll
        for (int m = G; m < 64; m <<= 1) {
            const long long o = __shfl_xor(longest, m, 64);
            longest = o > longest ? o : longest;
        }
        real acc = real(0);
        for (int64_t off = 0; off < longest; off += G) {
            const int64_t k = b + off + sub;
            real p = real(0);
            if (k < e) p = data[k] * mu[indices[k]];
            const int64_t left = e - b - off;
            const int n = left < G ? (left > 0 ? (int)left : 0) : G;      // entries of this group's row in the chunk
#pragma unroll 16
            for (int i = 0; i < G; ++i) {
                const real q = __shfl(p, i, G);
                acc = i < n ? acc + q : acc;
            }
        }
        if (live && sub == 0) out[t] = acc;
    }
}

static unsigned stream_blocks(const sdp_transop *op, int64_t n)
{
    int64_t blocks = (n + 255) / 256;
    if (blocks > (int64_t)op->cus * 8) blocks = (int64_t)op->cus * 8;
    return (unsigned)(blocks < 1 ? 1 : blocks);
}

static int transop_new(int dtype, int64_t S, int64_t nnz, sdp_transop **out)
{
    sdp_transop *op = new sdp_transop();
    op->dtype = dtype; op->S = S; op->nnz = nnz; op->cus = device_cus();
    std::unique_ptr<sdp_transop> guard(op);
    HIP_TRY(hipStreamCreate(&op->stream));
    HIP_TRY(hipEventCreate(&op->ev0));
    HIP_TRY(hipEventCreate(&op->ev1));
    HIP_TRY(hipEventCreate(&op->ev2));
    HIP_TRY(hipEventCreate(&op->ev3));
    guard.release();
    *out = op;
    return SDP_OK;
}

// entries in emission order on the device (tgt, val; src or, without one, per_node entries per source) -> the CSR
// the list of rows of `min_len` entries or more, from the host copy of the row pointers (min_len <= 0: no list)
static int transop_list_long_rows(sdp_transop *op, int32_t min_len)
{
    std::vector<int32_t> rows, wide;
    if (min_len > 0)
        for (int64_t t = 0; t < op->S; ++t) {
            const int64_t len = op->h_indptr[(size_t)t + 1] - op->h_indptr[(size_t)t];
            if (len >= min_len) (len >= SDP_PUSH_WIDE ? wide : rows).push_back((int32_t)t);
        }
    op->n_wide = (int64_t)wide.size();
    rows.insert(rows.end(), wide.begin(), wide.end());
    HIP_TRY(hipStreamSynchronize(op->stream));             // (no push in flight reads the old list)
    int rc;
    if ((rc = upload(op->long_rows, rows.data(), rows.size() * 4))) return rc;
    op->n_long = (int64_t)rows.size();
    op->long_min = min_len > 0 ? min_len : 0;
    return SDP_OK;
}

// entries in emission order on the device (tgt, val; src or, without one, per_node entries per source) -> the CSR.
// Everything is allocated first; ev2 .. ev3 then bracket the device work alone (sort, gather, histogram, scan).
static int transop_build_csr(sdp_transop *op, const int32_t *tgt, const void *val, const int32_t *src, uint32_t per_node)
{
    const size_t rs = real_size(op->dtype);
    const int64_t n = op->nnz, S = op->S;
    int rc;
    DevBuf counts, keys_out, pos, pos_out, tmp_sort, tmp_scan;
    if ((rc = op->indptr.alloc((size_t)(S + 1) * 8))) return rc;
    if ((rc = op->indices.alloc((size_t)n * 4))) return rc;
    if ((rc = op->data.alloc((size_t)n * rs))) return rc;
    if ((rc = counts.alloc((size_t)(S + 1) * 8))) return rc;
    unsigned bits = 1;                                     // bits of the largest node id
    while (bits < 32 && ((int64_t)1 << bits) < S) ++bits;
    size_t sort_bytes = 0, scan_bytes = 0;
    if (n > 0) {
        if ((rc = keys_out.alloc((size_t)n * 4))) return rc;
        if ((rc = pos.alloc((size_t)n * 4))) return rc;
        if ((rc = pos_out.alloc((size_t)n * 4))) return rc;
        HIP_TRY(rocprim::radix_sort_pairs(nullptr, sort_bytes, (const uint32_t *)tgt, (uint32_t *)keys_out.p, (const uint32_t *)pos.p,
                                          (uint32_t *)pos_out.p, (size_t)n, 0u, bits, op->stream));
        if ((rc = tmp_sort.alloc(sort_bytes))) return rc;
    }
    HIP_TRY(rocprim::inclusive_scan(nullptr, scan_bytes, (const int64_t *)counts.p, (int64_t *)op->indptr.p, (size_t)(S + 1),
                                    rocprim::plus<int64_t>(), op->stream));
    if ((rc = tmp_scan.alloc(scan_bytes))) return rc;
    HIP_TRY(hipEventRecord(op->ev2, op->stream));
    HIP_TRY(hipMemsetAsync(counts.p, 0, (size_t)(S + 1) * 8, op->stream));
    if (n > 0) {
        hipLaunchKernelGGL(k_iota, dim3(stream_blocks(op, n)), dim3(256), 0, op->stream, (uint32_t *)pos.p, n);
        HIP_TRY(hipGetLastError());
        HIP_TRY(rocprim::radix_sort_pairs(tmp_sort.p, sort_bytes, (const uint32_t *)tgt, (uint32_t *)keys_out.p, (const uint32_t *)pos.p,
                                          (uint32_t *)pos_out.p, (size_t)n, 0u, bits, op->stream));
        if (op->dtype == SDP_F32)
            hipLaunchKernelGGL(k_trans_gather<float>, dim3(stream_blocks(op, n)), dim3(256), 0, op->stream, (const uint32_t *)pos_out.p,
                               (const float *)val, src, per_node, (float *)op->data.p, (int32_t *)op->indices.p, n);
        else
            hipLaunchKernelGGL(k_trans_gather<double>, dim3(stream_blocks(op, n)), dim3(256), 0, op->stream, (const uint32_t *)pos_out.p,
                               (const double *)val, src, per_node, (double *)op->data.p, (int32_t *)op->indices.p, n);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_trans_count, dim3(stream_blocks(op, n)), dim3(256), 0, op->stream, tgt, n, (unsigned long long *)counts.p);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(rocprim::inclusive_scan(tmp_scan.p, scan_bytes, (const int64_t *)counts.p, (int64_t *)op->indptr.p, (size_t)(S + 1),
                                    rocprim::plus<int64_t>(), op->stream));
    HIP_TRY(hipEventRecord(op->ev3, op->stream));
    op->h_indptr.resize((size_t)S + 1);
    HIP_TRY(hipMemcpyAsync(op->h_indptr.data(), op->indptr.p, (size_t)(S + 1) * 8, hipMemcpyDeviceToHost, op->stream));
    HIP_TRY(hipStreamSynchronize(op->stream));             // (the temporaries go out of scope)
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, op->ev2, op->ev3));
    op->sort_ms = ms;
    return transop_list_long_rows(op, SDP_PUSH_LONG);
}

extern "C" int sdp_transop_create(sdp_problem *p, const void *host_pol, double t_k, sdp_transop **out)
{
    if (!p || !host_pol || !out) return fail(SDP_EINVAL, "NULL argument");
    if (p->comm && p->comm->nranks > 1) return fail(SDP_EINVAL, "a transition operator is built on one GPU");
    if (!p->f_transitions) return fail(SDP_EMODULE, "the model's code object has no sdp_transitions kernel");
    const size_t rs = real_size(p->dtype);
    const int64_t W = p->W > 0 ? p->W : 1, V = (int64_t)1 << p->d;
    const int64_t nnz = p->S * W * V;
    if (nnz >= (int64_t)1 << 32)
        return fail(SDP_EINVAL, "an operator of %lld entries: entry positions are 32-bit words (at most 2^32 - 1 entries)", (long long)nnz);
    sdp_transop *op = nullptr;
    int rc;
    if ((rc = transop_new(p->dtype, p->S, nnz, &op))) return rc;
    std::unique_ptr<sdp_transop> guard(op);
    DevBuf dpol, done, tgt, val;
    if ((rc = upload(dpol, host_pol, (size_t)p->S * p->nu * rs))) return rc;
    if (p->W <= 0) {                                       // a deterministic system: the law of one point of weight 1
        const double one8 = 1.0;
        const float one4 = 1.0f;
        if ((rc = upload(done, p->dtype == SDP_F32 ? (const void *)&one4 : (const void *)&one8, rs))) return rc;
    }
    if ((rc = tgt.alloc((size_t)nnz * 4))) return rc;
    if ((rc = val.alloc((size_t)nnz * rs))) return rc;
    if ((rc = op->gbar.alloc((size_t)p->S * rs))) return rc;
    SdpTransArgs a;
    memset(&a, 0, sizeof(a));
    a.pol = dpol.p; a.axes = p->axes.p;
    a.wtab = p->W > 0 ? p->wgrid.p : nullptr;
    a.proba = p->W > 0 ? p->proba.p : done.p;
    a.tgt = (int32_t *)tgt.p; a.val = val.p; a.gbar = op->gbar.p;
    a.S = p->S; a.t_k = t_k; a.W = (int32_t)W;
    for (int k = 0; k < SDP_MAXD; ++k) { a.orders[k] = p->orders[k]; a.axis_off[k] = p->axis_off[k]; }
    size_t size = sizeof(a);
    void *extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a, HIP_LAUNCH_PARAM_BUFFER_SIZE, &size,
                     HIP_LAUNCH_PARAM_END};
    int64_t blocks = (p->S * V + 255) / 256;
    if (blocks > (int64_t)p->cus * 8) blocks = (int64_t)p->cus * 8;
    HIP_TRY(hipStreamSynchronize(p->stream));        // lifted constants set on the problem stream
    HIP_TRY(hipEventRecord(op->ev0, op->stream));
    HIP_TRY(hipModuleLaunchKernel(p->f_transitions, (unsigned)blocks, 1, 1, 256, 1, 1, 0, op->stream, nullptr, extra));
    HIP_TRY(hipEventRecord(op->ev1, op->stream));
    if ((rc = transop_build_csr(op, (const int32_t *)tgt.p, val.p, nullptr, (uint32_t)(W * V)))) return rc;
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, op->ev0, op->ev1));
    op->entries_ms = ms;
    op->last_kernel_ms = op->entries_ms + op->sort_ms;
    op->has_gbar = true;
    guard.release();
    *out = op;
    return SDP_OK;
}

extern "C" int sdp_transop_from_coo(int dtype, int64_t S, int64_t nnz, const int32_t *tgt, const int32_t *src,
                                    const void *val, sdp_transop **out)
{
    if (!out) return fail(SDP_EINVAL, "NULL argument");
    if (dtype != SDP_F64 && dtype != SDP_F32) return fail(SDP_EINVAL, "dtype must be SDP_F64 or SDP_F32");
    if (S < 1 || S >= (int64_t)1 << 31) return fail(SDP_EINVAL, "S = %lld: an operator has 1 to 2^31 - 1 nodes", (long long)S);
    if (nnz < 0 || nnz >= (int64_t)1 << 32) return fail(SDP_EINVAL, "nnz = %lld: 0 to 2^32 - 1 entries (32-bit entry positions)", (long long)nnz);
    if (nnz > 0 && (!tgt || !src || !val)) return fail(SDP_EINVAL, "NULL argument");
    for (int64_t k = 0; k < nnz; ++k) {                    // before anything is allocated or launched
        if (tgt[k] < 0 || tgt[k] >= S) return fail(SDP_EINVAL, "entry %lld: target %d outside [0, %lld)", (long long)k, (int)tgt[k], (long long)S);
        if (src[k] < 0 || src[k] >= S) return fail(SDP_EINVAL, "entry %lld: source %d outside [0, %lld)", (long long)k, (int)src[k], (long long)S);
    }
    const size_t rs = real_size(dtype);
    sdp_transop *op = nullptr;
    int rc;
    if ((rc = transop_new(dtype, S, nnz, &op))) return rc;
    std::unique_ptr<sdp_transop> guard(op);
    DevBuf dtgt, dsrc, dval;
    if ((rc = upload(dtgt, tgt, (size_t)nnz * 4))) return rc;
    if ((rc = upload(dsrc, src, (size_t)nnz * 4))) return rc;
    if ((rc = upload(dval, val, (size_t)nnz * rs))) return rc;
    if ((rc = transop_build_csr(op, (const int32_t *)dtgt.p, dval.p, (const int32_t *)dsrc.p, 1u))) return rc;
    op->last_kernel_ms = op->sort_ms;
    guard.release();
    *out = op;
    return SDP_OK;
}

extern "C" int sdp_transop_destroy(sdp_transop *op)
{
    if (op) { (void)hipStreamSynchronize(op->stream); delete op; }
    return SDP_OK;
}

template <typename real, bool MEMBERS>
static int transop_launch_push_as(sdp_transop *op)
{
    const int32_t *flags = MEMBERS ? (const int32_t *)op->flags.p : nullptr;
    const int32_t Sm = MEMBERS ? (int32_t)op->Sm : 1;
    const real *in = (const real *)op->mu[op->cur].p;
    real *outp = (real *)op->mu[1 - op->cur].p;
    const int64_t *indptr = (const int64_t *)op->indptr.p;
    const int32_t *indices = (const int32_t *)op->indices.p;
    const real *data = (const real *)op->data.p;
    // the short rows, one lane each: at most the workgroups that are resident, the rest in a grid-stride loop
    if (op->n_long < op->S) {
        int64_t blocks = (op->S + 255) / 256;
        if (blocks > (int64_t)op->cus * 8) blocks = (int64_t)op->cus * 8;
        hipLaunchKernelGGL((k_push<real, MEMBERS>), dim3((unsigned)blocks), dim3(256), 0, op->stream, indptr, indices, data, in, outp,
                           op->S, op->long_min, flags, Sm);
        HIP_TRY(hipGetLastError());
    }
    // the long rows: four to a wave (sixteen to a workgroup), the widest one to a wave
    const int32_t *rows = (const int32_t *)op->long_rows.p;
    const int64_t n_mid = op->n_long - op->n_wide;
    if (n_mid > 0) {
        int64_t blocks = (n_mid + 15) / 16;
        if (blocks > (int64_t)op->cus * 64) blocks = (int64_t)op->cus * 64;
        hipLaunchKernelGGL((k_push_group<real, 16, MEMBERS>), dim3((unsigned)blocks), dim3(256), 0, op->stream, indptr, indices, data,
                           in, outp, rows, n_mid, flags, Sm);
        HIP_TRY(hipGetLastError());
    }
    if (op->n_wide > 0) {
        int64_t blocks = (op->n_wide + 3) / 4;
        if (blocks > (int64_t)op->cus * 64) blocks = (int64_t)op->cus * 64;
        hipLaunchKernelGGL((k_push_group<real, 64, MEMBERS>), dim3((unsigned)blocks), dim3(256), 0, op->stream, indptr, indices, data,
                           in, outp, rows + n_mid, op->n_wide, flags, Sm);
        HIP_TRY(hipGetLastError());
    }
    op->cur = 1 - op->cur;
    return SDP_OK;
}

static int transop_launch_push(sdp_transop *op)
{
    // (the operators of a family test the members' flags only while some member has stopped)
    if (op->P > 0 && !op->all_running)
        return op->dtype == SDP_F32 ? transop_launch_push_as<float, true>(op) : transop_launch_push_as<double, true>(op);
    return op->dtype == SDP_F32 ? transop_launch_push_as<float, false>(op) : transop_launch_push_as<double, false>(op);
}

// every member of a family's operators runs again (a solo operator has no flags)
static int transop_all_running(sdp_transop *op)
{
    if (op->P < 1 || op->all_running) return SDP_OK;
    std::vector<int32_t> ones((size_t)op->P, 1);
    HIP_TRY(hipMemcpyAsync(op->flags.p, ones.data(), ones.size() * 4, hipMemcpyHostToDevice, op->stream));
    HIP_TRY(hipStreamSynchronize(op->stream));
    op->all_running = true;
    return SDP_OK;
}

static int transop_set(sdp_transop *op, const void *host_mu)
{
    const size_t bytes = (size_t)op->S * real_size(op->dtype);
    int rc;
    for (int k = 0; k < 2; ++k)
        if (!op->mu[k].p && (rc = op->mu[k].alloc(bytes))) return rc;
    if (host_mu) {
        HIP_TRY(hipMemcpyAsync(op->mu[op->cur].p, host_mu, bytes, hipMemcpyHostToDevice, op->stream));
        HIP_TRY(hipStreamSynchronize(op->stream));         // `host_mu` may be reused by the caller
        op->has_mu = true;
    }
    if (!op->has_mu) return fail(SDP_EINVAL, "no resident vector: the first push needs host_mu");
    return SDP_OK;
}

extern "C" int sdp_transop_push(sdp_transop *op, const void *host_mu, int32_t n_steps)
{
    if (!op) return fail(SDP_EINVAL, "NULL argument");
    if (n_steps < 0) return fail(SDP_EINVAL, "n_steps must not be negative");
    int rc;
    if ((rc = transop_set(op, host_mu))) return rc;
    if ((rc = transop_all_running(op))) return rc;
    HIP_TRY(hipEventRecord(op->ev0, op->stream));
    for (int32_t k = 0; k < n_steps; ++k)
        if ((rc = transop_launch_push(op))) return rc;
    HIP_TRY(hipEventRecord(op->ev1, op->stream));
    HIP_TRY(hipStreamSynchronize(op->stream));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, op->ev0, op->ev1));
    op->last_kernel_ms = ms;
    return SDP_OK;
}

// delta = max |new - old| over the nodes: max(dmax, -dmin) of k_diff_stats (NaN if any difference is); 24 bytes back
static int transop_delta(sdp_transop *op, double &delta)
{
    int rc;
    if (!op->stats.p && (rc = op->stats.alloc(3 * 8))) return rc;
    HIP_TRY(hipMemsetAsync(op->stats.p, 0, 3 * 8, op->stream));
    SdpStatRanges r;
    memset(&r, 0, sizeof(r));
    r.n = 1; r.b[0] = 0; r.e[0] = op->S;
    const int vec = op->dtype == SDP_F32 ? 4 : 2;
    int64_t blocks = (op->S / vec + 255) / 256;
    if (blocks > (int64_t)op->cus * 4) blocks = (int64_t)op->cus * 4;
    if (blocks < 1) blocks = 1;
    unsigned long long *acc = (unsigned long long *)op->stats.p;
    const void *cur = op->mu[op->cur].p, *old = op->mu[1 - op->cur].p;
    if (op->dtype == SDP_F32)
        hipLaunchKernelGGL(k_diff_stats<float>, dim3((unsigned)blocks), dim3(256), 0, op->stream,
                           (const float *)cur, (const float *)old, (int64_t)-1, (int64_t)-1, r, acc);
    else
        hipLaunchKernelGGL(k_diff_stats<double>, dim3((unsigned)blocks), dim3(256), 0, op->stream,
                           (const double *)cur, (const double *)old, (int64_t)-1, (int64_t)-1, r, acc);
    HIP_TRY(hipGetLastError());
    unsigned long long keys[3] = {0, 0, 0};
    HIP_TRY(hipMemcpyAsync(keys, op->stats.p, 3 * 8, hipMemcpyDeviceToHost, op->stream));
    HIP_TRY(hipStreamSynchronize(op->stream));
    if (keys[2]) { delta = NAN; return SDP_OK; }
    const double dmin = sdp_key_value(~keys[0]), dmax = sdp_key_value(keys[1]);
    delta = dmax > -dmin ? dmax : -dmin;
    return SDP_OK;
}

extern "C" int sdp_transop_push_until(sdp_transop *op, int32_t n_max, int32_t check_every, double tol,
                                      int32_t *n_done, double *delta)
{
    if (!op || !n_done || !delta) return fail(SDP_EINVAL, "NULL argument");
    if (n_max < 1) return fail(SDP_EINVAL, "n_max must be at least 1");
    if (check_every < 1) return fail(SDP_EINVAL, "check_every must be at least 1");
    if (!(tol >= 0)) return fail(SDP_EINVAL, "tol must be a number >= 0");
    int rc;
    if ((rc = transop_set(op, nullptr))) return rc;
    if ((rc = transop_all_running(op))) return rc;
    int32_t done = 0;
    double d = NAN;
    HIP_TRY(hipEventRecord(op->ev0, op->stream));
    for (int32_t k = 0; k < n_max; ++k) {
        if ((rc = transop_launch_push(op))) return rc;
        done = k + 1;
        if (done % check_every == 0 || done == n_max) {
            if ((rc = transop_delta(op, d))) return rc;
            if (d <= tol) break;                            // NaN never converges
        }
    }
    HIP_TRY(hipEventRecord(op->ev1, op->stream));
    HIP_TRY(hipStreamSynchronize(op->stream));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, op->ev0, op->ev1));
    op->last_kernel_ms = ms;
    *n_done = done;
    *delta = d;
    return SDP_OK;
}

extern "C" int sdp_transop_get(sdp_transop *op, void *host_mu)
{
    if (!op || !host_mu) return fail(SDP_EINVAL, "NULL argument");
    if (!op->has_mu) return fail(SDP_EINVAL, "no resident vector: nothing was pushed yet");
    HIP_TRY(hipMemcpyAsync(host_mu, op->mu[op->cur].p, (size_t)op->S * real_size(op->dtype), hipMemcpyDeviceToHost, op->stream));
    HIP_TRY(hipStreamSynchronize(op->stream));
    return SDP_OK;
}

extern "C" int sdp_transop_get_csr(sdp_transop *op, int64_t *indptr, int32_t *indices, void *data)
{
    if (!op) return fail(SDP_EINVAL, "NULL argument");
    if (indptr) HIP_TRY(hipMemcpyAsync(indptr, op->indptr.p, (size_t)(op->S + 1) * 8, hipMemcpyDeviceToHost, op->stream));
    if (indices && op->nnz) HIP_TRY(hipMemcpyAsync(indices, op->indices.p, (size_t)op->nnz * 4, hipMemcpyDeviceToHost, op->stream));
    if (data && op->nnz) HIP_TRY(hipMemcpyAsync(data, op->data.p, (size_t)op->nnz * real_size(op->dtype), hipMemcpyDeviceToHost, op->stream));
    HIP_TRY(hipStreamSynchronize(op->stream));
    return SDP_OK;
}

extern "C" int sdp_transop_get_mean_cost(sdp_transop *op, void *host_gbar)
{
    if (!op || !host_gbar) return fail(SDP_EINVAL, "NULL argument");
    if (!op->has_gbar) return fail(SDP_EINVAL, "an operator made of host entries has no mean cost");
    HIP_TRY(hipMemcpyAsync(host_gbar, op->gbar.p, (size_t)op->S * real_size(op->dtype), hipMemcpyDeviceToHost, op->stream));
    HIP_TRY(hipStreamSynchronize(op->stream));
    return SDP_OK;
}

extern "C" int sdp_transop_last_kernel_ms(sdp_transop *op, double *ms)
{
    if (!op || !ms) return fail(SDP_EINVAL, "NULL argument");
    *ms = op->last_kernel_ms;
    return SDP_OK;
}

extern "C" int sdp_transop_set_long_rows(sdp_transop *op, int32_t min_entries)
{
    if (!op) return fail(SDP_EINVAL, "NULL argument");
    if (min_entries < 0) return fail(SDP_EINVAL, "min_entries must not be negative");
    return transop_list_long_rows(op, min_entries);
}

extern "C" int sdp_transop_build_ms(sdp_transop *op, double *entries_ms, double *sort_ms)
{
    if (!op || !entries_ms || !sort_ms) return fail(SDP_EINVAL, "NULL argument");
    *entries_ms = op->entries_ms;
    *sort_ms = op->sort_ms;
    return SDP_OK;
}

// ---------------------------------------------------------------------------
// The transition operators of the steps of a horizon (csrc/sdp_trans_horizon_kernel.h): sdp_transop_create of every
// step in one launch and one sort, and a batch of distributions pushed through the chain mu_{k+1} = P_k^T mu_k on the
// device.  stodynprog_amd/forward.py (`chain_entries`, `propagate`) is the definition.  See include/sdp_hip.h.
// The steps' operators are ONE block-diagonal sdp_transop on n_steps S rows -- node s of step k is row k S + s -- so
// the CSR build of the solo operator serves it as it is (the family's operators with a step where they have a member);
// the stable sort and the steps' disjoint rows keep every step's rows in the solo entry order.  Sources are then made
// local to their step (k_chain_local_sources): block k maps the vectors of step k to those of step k + 1.
//   k_chain_push, k_chain_push_group : k_push and k_push_group on the rows of ONE block for B vectors, the batch on the
//              grid's second dimension; a row's adds happen in entry order, one rounded multiply and one rounded add
//              per entry.  The long-row rule (SDP_PUSH_LONG, SDP_PUSH_WIDE) holds per block.
// ---------------------------------------------------------------------------
struct sdp_chainop {
    sdp_transop *csr = nullptr;            // the block-diagonal operator: row pointers, LOCAL sources, values, gbar, the
                                           //   list of long rows (global row ids; per block first the mid rows, then the wide)
    int64_t S = 0, n_steps = 0;
    std::vector<int64_t> mid_at, n_mid, wide_at, n_wide;     // per block: where its rows start in csr->long_rows
    double push_ms = 0;
    ~sdp_chainop() { delete csr; }
};

__global__ void __launch_bounds__(256) k_chain_local_sources(int32_t *__restrict__ indices, int64_t n, int32_t S)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += stride) indices[k] = indices[k] % S;
}

// k_push on the S rows row0 .. row0 + S - 1 of the block-diagonal operator, for vector blockIdx.y of [B][S]
template <typename real>
__global__ void __launch_bounds__(256) k_chain_push(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                    const real *__restrict__ data, const real *__restrict__ mu,
                                                    real *__restrict__ out, int64_t row0, int64_t S, int32_t long_min)
{
    indptr += row0;
    mu += (int64_t)blockIdx.y * S;
    out += (int64_t)blockIdx.y * S;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < S; t += stride) {
        const int64_t b = indptr[t], e = indptr[t + 1];
        if (long_min > 0 && e - b >= long_min) continue;
        real acc = real(0);
        for (int64_t k = b; k < e; ++k) acc = acc + data[k] * mu[indices[k]];
        out[t] = acc;
    }
}

// k_push_group on the listed rows of one block (global row ids, each in [row0, row0 + S)), for vector blockIdx.y
template <typename real, int G>
__global__ void __launch_bounds__(256) k_chain_push_group(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                          const real *__restrict__ data, const real *__restrict__ mu,
                                                          real *__restrict__ out, const int32_t *__restrict__ rows,
                                                          int64_t n_rows, int64_t row0, int64_t S)
{
    constexpr int PER = 64 / G;                                // rows of a wave
    mu += (int64_t)blockIdx.y * S;
    out += (int64_t)blockIdx.y * S;
    const int lane = threadIdx.x & 63, sub = lane & (G - 1), grp = lane / G;
    const int64_t wave = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int64_t waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t w = wave; w * PER < n_rows; w += waves) {     // the same trips in every lane of a wave
        const int64_t r = w * PER + grp;
        const bool live = r < n_rows;
        const int64_t t = live ? rows[r] : row0;
        int64_t b = 0, e = 0;
        if (live) { b = indptr[t]; e = indptr[t + 1]; }
        long long longest = e - b;                             // of the wave's rows: every lane runs that many chunks
#pragma unroll
        for (int m = G; m < 64; m <<= 1) {
            const long long o = __shfl_xor(longest, m, 64);
            longest = o > longest ? o : longest;
        }
        real acc = real(0);
        for (int64_t off = 0; off < longest; off += G) {
            const int64_t k = b + off + sub;
            real p = real(0);
            if (k < e) p = data[k] * mu[indices[k]];
            const int64_t left = e - b - off;
            const int n = left < G ? (left > 0 ? (int)left : 0) : G;      // entries of this group's row in the chunk
#pragma unroll 16
            for (int i = 0; i < G; ++i) {
                const real q = __shfl(p, i, G);
                acc = i < n ? acc + q : acc;
            }
        }
        if (live && sub == 0) out[t - row0] = acc;
    }
}

// workgroups of one launch over `n` units of `per` each for B vectors: at most the `cap` that are resident, all vectors
// together, the rest in the kernel's stride loop
static unsigned chain_blocks(int64_t n, int64_t per, int64_t cap, int64_t B)
{
    int64_t blocks = (n + per - 1) / per;
    if (blocks > cap / B) blocks = cap / B;
    return (unsigned)(blocks < 1 ? 1 : blocks);
}

extern "C" int sdp_chainop_create(sdp_problem *p, int64_t n_steps, const void *host_pol, const void *host_prm,
                                  int32_t n_params, double t0, sdp_chainop **out)
{
    if (!p || !host_pol || !out) return fail(SDP_EINVAL, "NULL argument");
    if (n_steps < 1) return fail(SDP_EINVAL, "n_steps = %lld: a chain has at least one step", (long long)n_steps);
    if (p->comm && p->comm->nranks > 1) return fail(SDP_EINVAL, "a chain of transition operators is built on one GPU");
    if (!p->f_transitions_h) return fail(SDP_EMODULE, "the model's code object has no sdp_transitions_h kernel (built before the horizon operators)");
    if (n_params < 0 || (n_params > 0 && !host_prm)) return fail(SDP_EINVAL, "sdp_chainop_create: bad parameter table");
    const size_t rs = real_size(p->dtype);
    if ((size_t)n_params * rs != p->prm_bytes)
        return fail(SDP_EINVAL, "sdp_chainop_create: the code object declares %zu parameter(s) per step, the table has %d",
                    p->prm_bytes / rs, (int)n_params);
    const int64_t S = p->S, W = p->W > 0 ? p->W : 1, V = (int64_t)1 << p->d;
    if (n_steps >= ((int64_t)1 << 31) / S + 1 || n_steps * S >= (int64_t)1 << 31)
        return fail(SDP_EINVAL, "%lld steps of %lld nodes: the rows of their operators are 32-bit ids (at most 2^31 - 1 rows)", (long long)n_steps, (long long)S);
    const int64_t rows = n_steps * S;
    const int64_t nnz = rows * W * V;
    if (nnz >= (int64_t)1 << 32)
        return fail(SDP_EINVAL, "operators of %lld entries together: entry positions are 32-bit words (at most 2^32 - 1 entries)", (long long)nnz);
    std::unique_ptr<sdp_chainop> ch(new sdp_chainop());
    ch->S = S; ch->n_steps = n_steps;
    int rc;
    if ((rc = transop_new(p->dtype, rows, nnz, &ch->csr))) return rc;
    sdp_transop *op = ch->csr;
    DevBuf dpol, dprm, done, tgt, val;
    if ((rc = upload(dpol, host_pol, (size_t)rows * p->nu * rs))) return rc;              // [n_steps][nu][S]
    if (n_params > 0 && (rc = upload(dprm, host_prm, (size_t)n_steps * n_params * rs))) return rc;
    if (p->W <= 0) {                                       // a deterministic system: the law of one point of weight 1
        const double one8 = 1.0;
        const float one4 = 1.0f;
        if ((rc = upload(done, p->dtype == SDP_F32 ? (const void *)&one4 : (const void *)&one8, rs))) return rc;
    }
    if ((rc = tgt.alloc((size_t)nnz * 4))) return rc;
    if ((rc = val.alloc((size_t)nnz * rs))) return rc;
    if ((rc = op->gbar.alloc((size_t)rows * rs))) return rc;
    SdpTransHArgs a;
    memset(&a, 0, sizeof(a));
    a.pol = dpol.p; a.prm = n_params > 0 ? dprm.p : nullptr; a.axes = p->axes.p;
    a.wtab = p->W > 0 ? p->wgrid.p : nullptr;
    a.proba = p->W > 0 ? p->proba.p : done.p;
    a.tgt = (int32_t *)tgt.p; a.val = val.p; a.gbar = op->gbar.p;
    a.S = S; a.step_begin = 0; a.step_end = n_steps; a.chunk_first = 0; a.t0 = t0; a.W = (int32_t)W;
    for (int k = 0; k < SDP_MAXD; ++k) { a.orders[k] = p->orders[k]; a.axis_off[k] = p->axis_off[k]; }
    size_t size = sizeof(a);
    void *extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a, HIP_LAUNCH_PARAM_BUFFER_SIZE, &size,
                     HIP_LAUNCH_PARAM_END};
    // a tile of 256 >> d nodes of one step is a workgroup: at most the workgroups that are resident, the rest in the
    // kernel's stride loop
    const int64_t tile = 256 >> p->d;
    int64_t blocks = n_steps * ((S + tile - 1) / tile);
    if (blocks > (int64_t)p->cus * 8) blocks = (int64_t)p->cus * 8;
    HIP_TRY(hipStreamSynchronize(p->stream));        // lifted constants set on the problem stream
    HIP_TRY(hipEventRecord(op->ev0, op->stream));
    HIP_TRY(hipModuleLaunchKernel(p->f_transitions_h, (unsigned)blocks, 1, 1, 256, 1, 1, 0, op->stream, nullptr, extra));
    HIP_TRY(hipEventRecord(op->ev1, op->stream));
    if ((rc = transop_build_csr(op, (const int32_t *)tgt.p, val.p, nullptr, (uint32_t)(W * V)))) return rc;
    float ms = 0, ms_local = 0;
    HIP_TRY(hipEventElapsedTime(&ms, op->ev0, op->ev1));
    HIP_TRY(hipEventRecord(op->ev0, op->stream));
    hipLaunchKernelGGL(k_chain_local_sources, dim3(stream_blocks(op, nnz)), dim3(256), 0, op->stream, (int32_t *)op->indices.p, nnz, (int32_t)S);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(op->ev1, op->stream));
    HIP_TRY(hipStreamSynchronize(op->stream));
    HIP_TRY(hipEventElapsedTime(&ms_local, op->ev0, op->ev1));
    op->entries_ms = ms;
    op->sort_ms += ms_local;
    op->last_kernel_ms = op->entries_ms + op->sort_ms;
    op->has_gbar = true;
    // the list of long rows is ascending within its two halves (transop_list_long_rows), so a block's rows are one run of each
    ch->mid_at.assign((size_t)n_steps, 0); ch->n_mid.assign((size_t)n_steps, 0);
    ch->wide_at.assign((size_t)n_steps, 0); ch->n_wide.assign((size_t)n_steps, 0);
    for (int64_t k = 0; k < n_steps; ++k)
        for (int64_t t = k * S; t < (k + 1) * S; ++t) {
            const int64_t len = op->h_indptr[(size_t)t + 1] - op->h_indptr[(size_t)t];
            if (len >= SDP_PUSH_WIDE) ++ch->n_wide[(size_t)k];
            else if (len >= SDP_PUSH_LONG) ++ch->n_mid[(size_t)k];
        }
    int64_t at = 0;
    for (int64_t k = 0; k < n_steps; ++k) { ch->mid_at[(size_t)k] = at; at += ch->n_mid[(size_t)k]; }
    for (int64_t k = 0; k < n_steps; ++k) { ch->wide_at[(size_t)k] = at; at += ch->n_wide[(size_t)k]; }
    *out = ch.release();
    return SDP_OK;
}

template <typename real>
static int chainop_launch_steps(sdp_chainop *ch, int64_t B, real *mu)
{
    sdp_transop *op = ch->csr;
    const int64_t S = ch->S;
    const int64_t *indptr = (const int64_t *)op->indptr.p;
    const int32_t *indices = (const int32_t *)op->indices.p;
    const real *data = (const real *)op->data.p;
    const int32_t *rows = (const int32_t *)op->long_rows.p;
    for (int64_t k = 0; k < ch->n_steps; ++k) {
        const real *in = mu + k * B * S;
        real *outp = mu + (k + 1) * B * S;
        const int64_t n_mid = ch->n_mid[(size_t)k], n_wide = ch->n_wide[(size_t)k];
        // the short rows of block k, one lane each
        if (n_mid + n_wide < S) {
            hipLaunchKernelGGL((k_chain_push<real>), dim3(chain_blocks(S, 256, (int64_t)op->cus * 8, B), (unsigned)B), dim3(256), 0,
                               op->stream, indptr, indices, data, in, outp, k * S, S, (int32_t)SDP_PUSH_LONG);
            HIP_TRY(hipGetLastError());
        }
        // its long rows: four to a wave (sixteen to a workgroup), the widest one to a wave
        if (n_mid > 0) {
            hipLaunchKernelGGL((k_chain_push_group<real, 16>), dim3(chain_blocks(n_mid, 16, (int64_t)op->cus * 64, B), (unsigned)B), dim3(256), 0,
                               op->stream, indptr, indices, data, in, outp, rows + ch->mid_at[(size_t)k], n_mid, k * S, S);
            HIP_TRY(hipGetLastError());
        }
        if (n_wide > 0) {
            hipLaunchKernelGGL((k_chain_push_group<real, 64>), dim3(chain_blocks(n_wide, 4, (int64_t)op->cus * 64, B), (unsigned)B), dim3(256), 0,
                               op->stream, indptr, indices, data, in, outp, rows + ch->wide_at[(size_t)k], n_wide, k * S, S);
            HIP_TRY(hipGetLastError());
        }
    }
    return SDP_OK;
}

extern "C" int sdp_chainop_propagate(sdp_chainop *ch, int64_t B, const void *host_mu0, void *host_mu)
{
    if (!ch || !host_mu0 || !host_mu) return fail(SDP_EINVAL, "NULL argument");
    if (B < 1 || B > 65535) return fail(SDP_EINVAL, "B = %lld vectors: 1 to 65535 (the batch is the grid's second dimension)", (long long)B);
    sdp_transop *op = ch->csr;
    const size_t rs = real_size(op->dtype);
    const size_t vec = (size_t)B * ch->S * rs;
    DevBuf mu;
    int rc;
    if ((rc = mu.alloc((size_t)(ch->n_steps + 1) * vec))) return rc;
    HIP_TRY(hipMemcpyAsync(mu.p, host_mu0, vec, hipMemcpyHostToDevice, op->stream));
    HIP_TRY(hipEventRecord(op->ev0, op->stream));
    rc = op->dtype == SDP_F32 ? chainop_launch_steps<float>(ch, B, (float *)mu.p) : chainop_launch_steps<double>(ch, B, (double *)mu.p);
    if (rc) { (void)hipStreamSynchronize(op->stream); return rc; }
    HIP_TRY(hipEventRecord(op->ev1, op->stream));
    HIP_TRY(hipMemcpyAsync(host_mu, mu.p, (size_t)(ch->n_steps + 1) * vec, hipMemcpyDeviceToHost, op->stream));
    HIP_TRY(hipStreamSynchronize(op->stream));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, op->ev0, op->ev1));
    ch->push_ms = ms;
    return SDP_OK;
}

extern "C" int sdp_chainop_get_csr(sdp_chainop *ch, int64_t step, int64_t *indptr, int32_t *indices, void *data)
{
    if (!ch) return fail(SDP_EINVAL, "NULL argument");
    if (step < 0 || step >= ch->n_steps) return fail(SDP_EINVAL, "step %lld outside [0, %lld)", (long long)step, (long long)ch->n_steps);
    sdp_transop *op = ch->csr;
    const int64_t *row = op->h_indptr.data() + (size_t)(step * ch->S);
    const int64_t first = row[0], n = row[ch->S] - first;
    if (indptr)
        for (int64_t t = 0; t <= ch->S; ++t) indptr[t] = row[t] - first;
    if (indices && n) HIP_TRY(hipMemcpyAsync(indices, (const int32_t *)op->indices.p + first, (size_t)n * 4, hipMemcpyDeviceToHost, op->stream));
    if (data && n) HIP_TRY(hipMemcpyAsync(data, (const char *)op->data.p + (size_t)first * real_size(op->dtype), (size_t)n * real_size(op->dtype), hipMemcpyDeviceToHost, op->stream));
    HIP_TRY(hipStreamSynchronize(op->stream));
    return SDP_OK;
}

extern "C" int sdp_chainop_get_mean_cost(sdp_chainop *ch, void *host_gbar)
{
    if (!ch) return fail(SDP_EINVAL, "NULL argument");
    return sdp_transop_get_mean_cost(ch->csr, host_gbar);
}

extern "C" int sdp_chainop_times(sdp_chainop *ch, double *entries_ms, double *sort_ms, double *push_ms)
{
    if (!ch || !entries_ms || !sort_ms || !push_ms) return fail(SDP_EINVAL, "NULL argument");
    *entries_ms = ch->csr->entries_ms;
    *sort_ms = ch->csr->sort_ms;
    *push_ms = ch->push_ms;
    return SDP_OK;
}

extern "C" int sdp_chainop_destroy(sdp_chainop *ch)
{
    if (ch) { (void)hipStreamSynchronize(ch->csr->stream); delete ch; }
    return SDP_OK;
}

extern "C" int sdp_problem_get_value(sdp_problem *p, void *host_J)
{
    if (!p || !host_J) return fail(SDP_EINVAL, "NULL argument");
    int rc;
    if ((rc = complete_J(p))) return rc;                   // (sparse exchange: collective)
    return download_nodes(p, host_J, p->J.p, real_size(p->dtype));
}

// after a sharded sweep every rank holds the policy rows of its own parts only:
// collect the others (on request -- the sweep itself never pays for this)
static int gather_policy(sdp_problem *p)
{
    if (!p->comm || p->comm->nranks == 1) return SDP_OK;
    int rc;
    HIP_TRY(hipStreamSynchronize(p->stream));
    for (int ph = 0; ph < p->n_phases; ++ph) {
        if ((rc = gather_phase_of(p, ph, p->pol.p, (size_t)p->nu * real_size(p->dtype)))) return rc;
        if ((rc = gather_phase_of(p, ph, p->idx.p, 4))) return rc;
    }
    HIP_TRY(hipStreamSynchronize(p->comm->stream));
    return SDP_OK;
}

extern "C" int sdp_problem_get_policy(sdp_problem *p, void *host_pol, int32_t *host_idx)
{
    if (!p) return fail(SDP_EINVAL, "NULL problem");
    int rc;
    if ((rc = gather_policy(p))) return rc;
    if (host_pol && (rc = download_nodes(p, host_pol, p->pol.p, (size_t)p->nu * real_size(p->dtype)))) return rc;
    if (host_idx && (rc = download_nodes(p, host_idx, p->idx.p, 4))) return rc;
    return SDP_OK;
}

extern "C" int sdp_problem_last_kernel_ms(sdp_problem *p, double *ms)
{
    if (!p || !ms) return fail(SDP_EINVAL, "NULL argument");
    *ms = p->last_kernel_ms;
    return SDP_OK;
}

// diagnostic: clock stamps of SDP_STAMP code objects (see sdp_kernel_args.h)
extern "C" int sdp_problem_debug_stamps(sdp_problem *p, int enable, unsigned long long *host,
                                        int64_t n_words)
{
    if (!p) return fail(SDP_EINVAL, "NULL problem");
    if (enable && !p->stamps.p) {
        const int64_t words = (int64_t)65536 * 4;           // room for any grid the library launches
        int rc = p->stamps.alloc((size_t)words * 8);
        if (rc) return rc;
        HIP_TRY(hipMemset(p->stamps.p, 0, (size_t)words * 8));
        p->stamp_words = words;
    }
    if (host && n_words > 0) {
        if (!p->stamps.p) return fail(SDP_EINVAL, "stamps were never enabled");
        if (n_words > p->stamp_words) n_words = p->stamp_words;
        HIP_TRY(hipStreamSynchronize(p->stream));
        HIP_TRY(hipMemcpy(host, p->stamps.p, (size_t)n_words * 8, hipMemcpyDeviceToHost));
    }
    if (!enable && p->stamps.p) { (void)hipFree(p->stamps.p); p->stamps.p = nullptr; p->stamp_words = 0; }
    return SDP_OK;
}

#ifdef SDP_TEST_HOOKS
// TEST BUILD ONLY: fill the device arrays a backup writes (J, policy, index; the layout-conversion
// buffers when they exist) with recognisable bytes, so that a row that reaches the host WITHOUT having
// been written by the kernel / the conversion shows which buffer it came from (tools/host_phase_stress.py)
extern "C" int sdp_problem_debug_poison(sdp_problem *p)
{
    if (!p) return fail(SDP_EINVAL, "NULL problem");
    const size_t rs = real_size(p->dtype);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemset(p->J.p, 0xF1, (size_t)p->S * rs));
    HIP_TRY(hipMemset(p->pol.p, 0xF2, (size_t)p->S * rs * p->nu));
    HIP_TRY(hipMemset(p->idx.p, 0xF3, (size_t)p->S * 4));
    for (int k = 0; k < 3; ++k)
        if (p->stage[k].p) HIP_TRY(hipMemset(p->stage[k].p, 0xE0 + k, p->stage_bytes[k]));
    HIP_TRY(hipDeviceSynchronize());
    return SDP_OK;
}
// TEST BUILD ONLY: leave `bytes` of freed device memory filled with `byte` behind (what a later
// hipMalloc may hand out again)
extern "C" int sdp_debug_pollute(size_t bytes, int byte)
{
    void *q = nullptr;
    HIP_TRY(hipMalloc(&q, bytes));
    HIP_TRY(hipMemset(q, byte, bytes));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipFree(q));
    return SDP_OK;
}
#endif

extern "C" int sdp_problem_bench_sweeps(sdp_problem *p, int32_t reps, int rel_dp,
                                        int64_t ref_index, double *loop_ms, double *kernel_ms)
{
    if (!p || reps < 1) return fail(SDP_EINVAL, "bad arguments");
    p->peer_fence = true;                // first backup of a call (open_pushes)
    int rc;
    if ((rc = check_ref(p, rel_dp, ref_index))) return rc;
    if ((rc = ensure_refs(p, 1))) return rc;
    struct Events {                         // destroyed on every return path
        std::vector<hipEvent_t> v;
        ~Events() { for (auto e : v) if (e) (void)hipEventDestroy(e); }
    } events;
    events.v.assign(2 * (size_t)reps, nullptr);
    std::vector<hipEvent_t> &ev = events.v;
    for (auto &e : ev) HIP_TRY(hipEventCreate(&e));
    HIP_TRY(hipEventRecord(p->ev2, p->stream));
    for (int r = 0; r < reps; ++r) {
        if (r > 0) swap_buffers(p);
        HIP_TRY(hipEventRecord(ev[2 * r], p->stream));
        if ((rc = run_backup(p, false, 0.0))) return rc;
        HIP_TRY(hipEventRecord(ev[2 * r + 1], p->stream));
        if ((rc = join_comm(p))) return rc;
        if (rel_dp && (rc = rel_shift(p, ref_index, 0))) return rc;
    }
    HIP_TRY(hipEventRecord(p->ev3, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, p->ev2, p->ev3));
    if (loop_ms) *loop_ms = ms;
    double ksum = 0;
    for (int r = 0; r < reps; ++r) {
        HIP_TRY(hipEventElapsedTime(&ms, ev[2 * r], ev[2 * r + 1]));
        ksum += ms;
    }
    if (kernel_ms) *kernel_ms = ksum;
    p->last_kernel_ms = ksum / reps;
    return SDP_OK;
}

// Map every other rank's value / J buffer into this process (HIP IPC) and switch the exchange
// of the backups from RCCL all-gathers to peer writes (push_phase).  Collective: every rank of
// the communicator calls it, after sdp_problem_attach_comm.  The handles travel through the
// communicator itself (one all-gather of 2 x 64 bytes per rank).
extern "C" int sdp_problem_enable_peer_exchange(sdp_problem *p)
{
    if (!p || !p->comm) return fail(SDP_EINVAL, "no communicator attached");
    const int n = p->comm->nranks, me = p->comm->rank;
    if (n == 1) return SDP_OK;
    p->release_peers();
    static_assert(sizeof(hipIpcMemHandle_t) == 64, "HIP IPC handle size");
    std::vector<hipIpcMemHandle_t> all((size_t)2 * n);
    memset(all.data(), 0, all.size() * sizeof(hipIpcMemHandle_t));
    // From here to the agreement below every rank takes part in the same two collectives whatever
    // happens locally: a failure only raises `failed` (a rank that left early would leave the
    // others waiting in a collective).
    int failed = 0;
    char why[256] = "";
    {
        hipError_t e = hipIpcGetMemHandle(&all[2 * me], p->V.p);
        ipc_trace(e == hipSuccess ? "export V" : "export V FAILED", p->V.p, &all[2 * me], 0);
        if (e == hipSuccess) {
            p->V.ever_exported = true;
            e = hipIpcGetMemHandle(&all[2 * me + 1], p->J.p);
            ipc_trace(e == hipSuccess ? "export J" : "export J FAILED", p->J.p, &all[2 * me + 1], 0);
            if (e == hipSuccess) p->J.ever_exported = true;
        }
        if (e != hipSuccess) {
            failed = 1;
            snprintf(why, sizeof(why), "exporting this rank's buffers: %s", hipGetErrorString(e));
            (void)hipGetLastError();
        }
    }
    // Between the two agreements below nothing returns early: a local failure raises `failed`, and
    // a failure of the communicator's own calls (a broken communicator or device: the other ranks
    // would wait in a collective for ever) ends the process with a message.
#define COLLECTIVE_OR_DIE(expr)                                                                 \
    do {                                                                                        \
        const int r__ = (int)(expr);                                                            \
        if (r__ != 0) {                                                                         \
            fprintf(stderr, "sdp_problem_enable_peer_exchange: %s failed (%d) inside a collective "  \
                    "section; aborting this rank\n", #expr, r__);                               \
            abort();                                                                            \
        }                                                                                       \
    } while (0)
    hipStream_t cs = p->comm->stream;
    int *const d_agree = (int *)p->comm->d_scalar;          // 8 bytes owned by the communicator
    auto agree = [&](int mine) -> int {                     // max over the ranks of `mine`
        int any = 0;
        COLLECTIVE_OR_DIE(hipMemcpyAsync(d_agree, &mine, sizeof(int), hipMemcpyHostToDevice, cs));
        COLLECTIVE_OR_DIE(g_rccl.AllReduce(d_agree, d_agree, 1, NCCL_INT32, NCCL_MAX, p->comm->comm, cs));
        COLLECTIVE_OR_DIE(hipMemcpyAsync(&any, d_agree, sizeof(int), hipMemcpyDeviceToHost, cs));
        COLLECTIVE_OR_DIE(hipStreamSynchronize(cs));
        return any;
    };
    DevBuf stage;
    if (stage.alloc(sizeof(hipIpcMemHandle_t) * 2 * n) != SDP_OK && !failed) {
        failed = 1;
        snprintf(why, sizeof(why), "staging buffer for the handle exchange: out of device memory");
    }
    // first agreement: every rank can export its buffers and holds a staging buffer
    if (agree(failed)) {
        p->release_peers();
        return fail(SDP_ECOMM, "peer exchange not available (%s): the RCCL exchange stays in place",
                    failed ? why : "another rank could not export its buffers");
    }
    COLLECTIVE_OR_DIE(hipMemcpyAsync((char *)stage.p + (size_t)me * 128, &all[2 * me], 128, hipMemcpyHostToDevice, cs));
    COLLECTIVE_OR_DIE(g_rccl.AllGather((char *)stage.p + (size_t)me * 128, stage.p, 128, NCCL_INT8, p->comm->comm, cs));
    COLLECTIVE_OR_DIE(hipMemcpyAsync(all.data(), stage.p, (size_t)n * 128, hipMemcpyDeviceToHost, cs));
    COLLECTIVE_OR_DIE(hipStreamSynchronize(cs));
    p->peer_me = me;
    p->peer_V.assign(n, nullptr); p->peer_J.assign(n, nullptr);
    p->peer_stream.assign(n, nullptr); p->peer_done.assign(n, nullptr);
    p->peer_V[me] = p->V.p; p->peer_J[me] = p->J.p;
    for (int r = 0; r < n && !failed; ++r) {
        if (r == me) continue;
        hipError_t e = ipc_open(&p->peer_V[r], all[2 * r]);
        if (e != hipSuccess) p->peer_V[r] = nullptr;
        if (e == hipSuccess) {
            e = ipc_open(&p->peer_J[r], all[2 * r + 1]);
            if (e != hipSuccess) p->peer_J[r] = nullptr;
        }
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&p->peer_stream[r], hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&p->peer_done[r], hipEventDisableTiming);
        if (e != hipSuccess) {
            failed = 1;
            snprintf(why, sizeof(why), "mapping rank %d's buffers: %s", r, hipGetErrorString(e));
            (void)hipGetLastError();
        }
    }
    if (!failed && hipMalloc((void **)&p->d_flag, 8) != hipSuccess) { failed = 1; snprintf(why, sizeof(why), "hipMalloc"); }
    if (!failed && (hipEventCreateWithFlags(&p->ev_enter, hipEventDisableTiming) != hipSuccess ||
                    hipEventCreateWithFlags(&p->ev_fence, hipEventDisableTiming) != hipSuccess)) {
        failed = 1; snprintf(why, sizeof(why), "hipEventCreate");
    }
    if (!failed && hipMemset(p->d_flag, 0, 8) != hipSuccess) { failed = 1; snprintf(why, sizeof(why), "hipMemset"); }
    // second agreement, all ranks or none: the ranks agree on the outcome before anybody writes
    // into a peer (this also guarantees that every rank has mapped everything before the first write)
    if (agree(failed)) {
        p->release_peers();
        return fail(SDP_ECOMM, "peer exchange not available (%s): the RCCL exchange stays in place",
                    failed ? why : "another rank could not map its peers");
    }
#undef COLLECTIVE_OR_DIE
    p->peer_exchange = true;
    p->peer_fence = true;
    return SDP_OK;
}

extern "C" int sdp_problem_complete_value(sdp_problem *p)
{
    if (!p) return fail(SDP_EINVAL, "NULL problem");
    int rc;
    if ((rc = complete_J(p))) return rc;
    HIP_TRY(hipStreamSynchronize(p->stream));
    return SDP_OK;
}

extern "C" int sdp_problem_disable_peer_exchange(sdp_problem *p)
{
    if (!p) return fail(SDP_EINVAL, "NULL handle");
    HIP_TRY(hipDeviceSynchronize());                       // (nothing of this rank is still writing into a peer)
    // (a value array that the sparse exchange left incomplete stays marked so: this call is for tearing a problem
    // down, not for switching exchanges in the middle of a chain)
    p->release_peers();
    p->mask_valid = false;
    return SDP_OK;
}

extern "C" int sdp_problem_set_peer_needs(sdp_problem *p, const int64_t *need_off, const int64_t *ranges)
{
    if (!p) return fail(SDP_EINVAL, "NULL problem");
    if (!need_off || !ranges) { p->sparse = false; p->need.clear(); p->mask_valid = false; return SDP_OK; }
    if (!p->comm || !(p->peer_exchange || p->sendrecv)) return fail(SDP_EINVAL, "sparse exchange needs the peer exchange (sdp_problem_enable_peer_exchange) or the send / receive one (sdp_problem_set_sendrecv_exchange)");
    if (p->J_partial || p->V_partial) return fail(SDP_EINVAL, "the value arrays are incomplete: fetch or set them first");
    const int n = p->comm->nranks;
    const int64_t unit = p->layout == SDP_LAYOUT_COLUMNS ? p->orders[0] : 1;
    std::vector<std::vector<std::pair<int64_t, int64_t>>> need((size_t)n);
    for (int q = 0; q < n; ++q) {
        int64_t at = 0;
        for (int64_t k = need_off[q]; k < need_off[q + 1]; ++k) {
            const int64_t b = ranges[2 * k], e = ranges[2 * k + 1];
            if (b < at || e <= b || e > p->S || b % unit || e % unit)
                return fail(SDP_EINVAL, "peer needs: ranges must be sorted, disjoint, inside the grid%s",
                            unit > 1 ? " and made of whole columns" : "");
            need[(size_t)q].emplace_back(b, e);
            at = e;
        }
    }
    p->need.swap(need);
    p->sparse = true;
    p->mask_valid = false;
    return SDP_OK;
}

extern "C" int sdp_problem_set_sendrecv_exchange(sdp_problem *p, int on)
{
    if (!p) return fail(SDP_EINVAL, "NULL problem");
    if (!on) { p->sendrecv = false; return SDP_OK; }
    if (!p->comm) return fail(SDP_EINVAL, "no communicator attached");
    if (p->peer_exchange) return fail(SDP_EINVAL, "the send / receive exchange is an alternative to the peer exchange, not an addition");
    p->sendrecv = true;
    return SDP_OK;
}

extern "C" int sdp_problem_set_direct_exchange(sdp_problem *p, int on)
{
    if (!p) return fail(SDP_EINVAL, "NULL problem");
    if (!on) { p->direct = false; return SDP_OK; }
    if (!p->comm || !p->peer_exchange) return fail(SDP_EINVAL, "the direct exchange needs the peers' buffers mapped (sdp_problem_enable_peer_exchange)");
    if (p->comm->nranks > SDP_MAX_PEERS) return fail(SDP_EINVAL, "the direct exchange serves at most %d ranks (one node), the communicator has %d", SDP_MAX_PEERS, p->comm->nranks);
    if (!(p->meta[SDP_META_FLAGS] & SDP_META_F_PEER_STORES)) return fail(SDP_EMODULE, "the code object's kernels do not store through sdp_store_J");
    p->direct = true;
    p->peer_fence = true;
    return SDP_OK;
}

extern "C" int sdp_problem_set_lead_halo(sdp_problem *p, int64_t rows)
{
    if (!p) return fail(SDP_EINVAL, "NULL problem");
    p->lead_halo = rows;
    p->red_V = nullptr;
    return SDP_OK;
}

extern "C" int sdp_problem_attach_comm(sdp_problem *p, sdp_comm *c, int32_t n_phases,
                                       const int64_t *part_bounds)
{
    if (!p) return fail(SDP_EINVAL, "NULL problem");
    if (!c) { p->release_peers(); p->comm = nullptr; p->parts.clear(); p->n_phases = 0; return SDP_OK; }
    if (!part_bounds || n_phases < 1) return fail(SDP_EINVAL, "phase partition missing");
    if (p->n_perturb > 1 && c->nranks > 1) return fail(SDP_EINVAL, "several perturbation variables run on one GPU");
    const int n = c->nranks;
    std::vector<int64_t> parts(part_bounds, part_bounds + (size_t)n_phases * (n + 1));
    int64_t at = 0;
    const int64_t unit = p->layout == SDP_LAYOUT_COLUMNS ? p->orders[0] : 1;
    for (int ph = 0; ph < n_phases; ++ph) {
        const int64_t *b = parts.data() + (size_t)ph * (n + 1);
        if (b[0] != at) return fail(SDP_EINVAL, "phases must be contiguous and start at node 0");
        for (int r = 0; r < n; ++r) {
            if (b[r] > b[r + 1]) return fail(SDP_EINVAL, "phase partition must be non-decreasing");
            if (b[r] % unit) return fail(SDP_EINVAL, "column layout: parts must consist of whole columns");
        }
        at = b[n];
    }
    if (at != p->S) return fail(SDP_EINVAL, "phases must cover all %lld nodes", (long long)p->S);
    {
        // gather buffer for the J exchange of phases whose parts are uneven (gather_phase_of): sized now, so
        // that no backup ever allocates with collectives in flight
        size_t need = 0;
        for (int ph = 0; ph < n_phases; ++ph) {
            const int64_t *b = parts.data() + (size_t)ph * (n + 1);
            int64_t longest = 0;
            bool even = true;
            for (int r = 0; r < n; ++r) { longest = std::max(longest, b[r + 1] - b[r]); even = even && (b[r + 1] - b[r] == b[1] - b[0]); }
            if (!even) need = std::max(need, (size_t)longest * (size_t)n * real_size(p->dtype));
        }
        if (need > p->gstage_bytes) {
            int rc = p->gstage.alloc(need);
            if (rc) { p->gstage_bytes = 0; return rc; }
            p->gstage_bytes = need;
        }
    }
    for (auto &e : p->ev_phase) (void)hipEventDestroy(e);
    p->ev_phase.assign((size_t)n_phases, nullptr);
    for (auto &e : p->ev_phase) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    if (!p->ev_comm) HIP_TRY(hipEventCreateWithFlags(&p->ev_comm, hipEventDisableTiming));
    p->parts.swap(parts);
    p->n_phases = n_phases;
    p->comm = c;
    p->comm_pending = false;
    p->sparse = false;                     // (a new partition: the need lists no longer apply)
    p->need.clear();
    p->mask_valid = false;
    p->red_V = nullptr;
    return SDP_OK;
}

// ---------------------------------------------------------------------------
// a family of same-shaped problems (include/sdp_hip.h: sdp_family_*; kernel sdp_family_sweep of a family code
// object, csrc/sdp_family_kernel.h).  Every device array is member-major.  Two value buffers [P][S] are used in
// turn: sweep k reads one and writes the other, for the members still listed.  A member that has left the list
// (sdp_family_vi_until) is written by nobody, so its result stays in the buffer of its last sweep: `where` says
// which one.
// ---------------------------------------------------------------------------
template <typename real>
__global__ void k_family_pick_ref(const real *__restrict__ J, int64_t S, int64_t ref, const int32_t *__restrict__ members,
                                  int n_active, double *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_active) out[members[i]] = (double)J[(int64_t)members[i] * S + ref];
}

// k_shift per listed member: J[p][i] -= (real)ref[p]
template <typename real>
__global__ void __launch_bounds__(256) k_family_shift(real *__restrict__ J, int64_t S, const int32_t *__restrict__ members,
                                                      const double *__restrict__ ref)
{
    const int64_t p = members[blockIdx.y];
    const real r = (real)ref[p];
    real *__restrict__ Jp = J + p * S;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < S; i += stride)
        Jp[i] = Jp[i] - r;
}

// k_diff_stats per listed member: the three key words of member members[y] at acc[3 y ..].  ra / rb >= 0: J / V of
// every member is read shifted by its own node ra / rb, each rounded once (the policy evaluation's raw buffers)
template <typename real>
__global__ void __launch_bounds__(256) sdp_family_diff_stats(const real *__restrict__ J, const real *__restrict__ V, int64_t S,
                                                             const int32_t *__restrict__ members, int64_t ra, int64_t rb,
                                                             unsigned long long *__restrict__ acc)
{
    const int64_t p = members[blockIdx.y];
    const real *__restrict__ Jp = J + p * S, *__restrict__ Vp = V + p * S;
    const real ja = ra >= 0 ? Jp[ra] : real(0), vb = rb >= 0 ? Vp[rb] : real(0);
    real mn = real(INFINITY), mx = real(-INFINITY);
    int nan = 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < S; i += stride)
        stat_node(ra >= 0 ? Jp[i] - ja : Jp[i], rb >= 0 ? Vp[i] - vb : Vp[i], mn, mx, nan);
    for (int off = warpSize / 2; off > 0; off >>= 1) {
        const real omn = __shfl_xor(mn, off), omx = __shfl_xor(mx, off);
        mn = omn < mn ? omn : mn;
        mx = omx > mx ? omx : mx;
        nan |= __shfl_xor(nan, off);
    }
    __shared__ real s_mn[4], s_mx[4];
    __shared__ int s_nan[4];
    const int wave = threadIdx.x / warpSize;
    if (threadIdx.x % warpSize == 0) { s_mn[wave] = mn; s_mx[wave] = mx; s_nan[wave] = nan; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int waves = (blockDim.x + warpSize - 1) / warpSize;
        for (int w = 1; w < waves; ++w) {
            mn = s_mn[w] < mn ? s_mn[w] : mn;
            mx = s_mx[w] > mx ? s_mx[w] : mx;
            nan |= s_nan[w];
        }
        unsigned long long *a = acc + 3 * (size_t)blockIdx.y;
        atomicMax(a + 0, ~sdp_order_key((double)mn));
        atomicMax(a + 1, sdp_order_key((double)mx));
        if (nan) atomicMax(a + 2, 1ull);
    }
}

struct sdp_family {
    int dtype = SDP_F64, d = 0, nu = 0, W = 0, P = 0, n_params = 0, box_per_node = 0, lanes = 64;
    int64_t S = 0;
    int32_t orders[SDP_MAXD] = {0, 0, 0, 0};
    int32_t axis_off[SDP_MAXD] = {0, 0, 0, 0};
    int32_t n_axes = 0;
    DevBuf axes, wgrid, proba, prm, box_lo, box_hi, box_n, buf[2], pol, idx, members, refs, stats;
    // policy evaluation (sdp_family_load_policy_unit): the prescribed policy [P][S][nu] -- allocated at the first
    // sdp_family_set_policy / sdp_family_take_policy --, the members that leave the list at a check, the flags of
    // sdp_family_compare_policy, what the resident kernel reports
    DevBuf pol_in, leavers, flags, res_done, res_stats;
    bool has_policy = false;
    size_t res_stats_rows = 0;
    hipModule_t pmod = nullptr;
    hipFunction_t f_evalpol = nullptr, f_resident = nullptr;
    int res_threads = 0;
    int64_t res_nodes = 0;
    // Monte Carlo evaluation (sdp_family_load_mc_unit): the unit and its kernel; the arrays of a run live for the call
    hipModule_t mcmod = nullptr;
    hipFunction_t f_montecarlo = nullptr;
    // closed loops over a horizon (sdp_family_load_horizon_unit): the unit and its kernels (f_hz_montecarlo: a stochastic
    // family's only); the arrays of a run live for the call
    hipModule_t hzmod = nullptr;
    hipFunction_t f_hz_simulate = nullptr, f_hz_montecarlo = nullptr;
    // lookahead at arbitrary states (sdp_family_load_lookahead_unit): the unit, its two kernels, the lanes of a state and
    // the constants of its box function per member; the members' box constants and control steps (sdp_family_set_lookahead_box)
    hipModule_t lkmod = nullptr;
    hipFunction_t f_lookahead = nullptr, f_mc_lookahead = nullptr;
    int look_lanes = 0, n_box = 0;
    DevBuf bprm, look_steps;
    bool has_look_box = false;
    // closed loops under lookahead controls over a horizon (sdp_family_load_lookahead_horizon_unit): the unit and its
    // kernels (f_lh_montecarlo: a stochastic family's only).  look_lanes, n_box and the members' box rows are shared
    // with the lookahead unit: both are generated from the same lattice plan and the same box function
    hipModule_t lhmod = nullptr;
    hipFunction_t f_lh_simulate = nullptr, f_lh_montecarlo = nullptr;
    // transition operators (sdp_family_load_trans_unit): the unit, its kernel and the nodes of a workgroup's tile; an
    // operator owns its arrays (sdp_transop) and outlives the family
    hipModule_t trmod = nullptr;
    hipFunction_t f_transitions = nullptr;
    int trans_tile = 0;
    int cur = 0;                           // buf[cur] is read (V), buf[cur ^ 1] written (J)
    std::vector<int32_t> active;           // the members the next launch runs
    std::vector<int> where;                // [P] the buffer that holds the member's latest values
    bool list_changed = true;              // `active` differs from the device's copy
    int refs_rows = 0;
    hipModule_t mod = nullptr;
    hipFunction_t f_sweep = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    double last_kernel_ms = 0;
    int cus = 256;
    int32_t meta[SDP_META_WORDS] = {0};
    ~sdp_family()
    {
        if (mod) (void)hipModuleUnload(mod);
        if (pmod) (void)hipModuleUnload(pmod);
        if (mcmod) (void)hipModuleUnload(mcmod);
        if (hzmod) (void)hipModuleUnload(hzmod);
        if (lkmod) (void)hipModuleUnload(lkmod);
        if (lhmod) (void)hipModuleUnload(lhmod);
        if (trmod) (void)hipModuleUnload(trmod);
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

extern "C" int sdp_family_create(const sdp_family_desc *desc, sdp_family **out)
{
    if (!desc || !out) return fail(SDP_EINVAL, "NULL argument");
    if (desc->dtype != SDP_F64 && desc->dtype != SDP_F32) return fail(SDP_EINVAL, "dtype must be SDP_F64 or SDP_F32");
    if (desc->d < 1 || desc->d > SDP_MAXD)
        return fail(SDP_EDIM, "state dimension %d: multilinear interpolation supports 1..4", desc->d);
    if (desc->nu < 1 || desc->nu > SDP_MAXU) return fail(SDP_EINVAL, "number of controls %d outside 1..%d", desc->nu, SDP_MAXU);
    if (desc->W < 0) return fail(SDP_EINVAL, "negative perturbation count");
    if (desc->P < 1 || desc->P > 65535) return fail(SDP_EINVAL, "%d members: a family has 1..65535", (int)desc->P);
    if (desc->n_params < 0) return fail(SDP_EINVAL, "negative number of lifted constants");
    if (!desc->module_path) return fail(SDP_EMODULE, "no family code object given");
    if (!desc->axes) return fail(SDP_EINVAL, "state axes missing");
    if (!desc->box_lo || !desc->box_hi || !desc->box_n) return fail(SDP_EINVAL, "control box arrays missing");
    sdp_family *f = new sdp_family();
    std::unique_ptr<sdp_family> guard(f);
    f->dtype = desc->dtype; f->d = desc->d; f->nu = desc->nu; f->W = desc->W; f->P = desc->P;
    f->n_params = desc->n_params; f->box_per_node = desc->box_per_node ? 1 : 0; f->lanes = desc->lanes_per_node;
    if (f->lanes < 1 || f->lanes > 64 || (f->lanes & (f->lanes - 1))) return fail(SDP_EINVAL, "lanes_per_node must be a power of two in 1..64");
    const size_t rs = real_size(f->dtype);
    int64_t S = 1, total = 0;
    for (int k = 0; k < f->d; ++k) {
        if (desc->orders[k] < 2) return fail(SDP_EINVAL, "state axis %d has %lld points: at least 2 needed to interpolate", k, (long long)desc->orders[k]);
        f->orders[k] = (int32_t)desc->orders[k];
        f->axis_off[k] = (int32_t)total;
        total += desc->orders[k];
        S *= desc->orders[k];
        if (S >= (int64_t)1 << 31) return fail(SDP_EINVAL, "state grid too large: 32-bit vertex indices (pyx:164-165)");
    }
    f->S = S;
    f->n_axes = (int32_t)total;
    f->cus = device_cus();
    const size_t P = (size_t)f->P;
    int rc;
    if ((rc = upload(f->axes, desc->axes, P * (size_t)total * rs))) return rc;
    if (f->W > 0) {
        if (!desc->wgrid || !desc->proba) return fail(SDP_EINVAL, "perturbation grid/weights missing");
        if ((rc = upload(f->wgrid, desc->wgrid, P * f->W * rs))) return rc;
        if ((rc = upload(f->proba, desc->proba, P * f->W * rs))) return rc;
    }
    const size_t nbox = P * (size_t)f->nu * (f->box_per_node ? (size_t)S : 1);
    if ((rc = upload(f->box_lo, desc->box_lo, nbox * rs))) return rc;
    if ((rc = upload(f->box_hi, desc->box_hi, nbox * rs))) return rc;
    if ((rc = upload(f->box_n, desc->box_n, nbox * 4))) return rc;
    if ((rc = f->prm.alloc(P * (size_t)f->n_params * rs))) return rc;
    for (int b = 0; b < 2; ++b) {
        if ((rc = f->buf[b].alloc(P * S * rs))) return rc;
        HIP_TRY(hipMemset(f->buf[b].p, 0, P * S * rs));
    }
    if ((rc = f->pol.alloc(P * S * f->nu * rs))) return rc;
    if ((rc = f->idx.alloc(P * S * 4))) return rc;
    if ((rc = f->members.alloc(P * 4))) return rc;
    if ((rc = f->stats.alloc(P * 3 * 8))) return rc;
    HIP_TRY(hipMemset(f->pol.p, 0, P * S * f->nu * rs));
    HIP_TRY(hipMemset(f->idx.p, 0, P * S * 4));
    f->where.assign(P, 0);
    f->active.resize(P);
    for (size_t p = 0; p < P; ++p) f->active[p] = (int32_t)p;

    hipError_t e = hipModuleLoad(&f->mod, desc->module_path);
    if (e != hipSuccess) { f->mod = nullptr; return fail(SDP_EMODULE, "hipModuleLoad(%s): %s", desc->module_path, hipGetErrorString(e)); }
    {
        hipDeviceptr_t mptr = nullptr;
        size_t mbytes = 0;
        if (hipModuleGetGlobal(&mptr, &mbytes, f->mod, "sdp_meta") != hipSuccess || mbytes != sizeof(f->meta)) {
            (void)hipGetLastError();
            return fail(SDP_EMODULE, "code object %s does not declare `sdp_meta` (%d words, sdp_kernel_args.h): "
                        "cannot check that it was built for this family", desc->module_path, SDP_META_WORDS);
        }
        HIP_TRY(hipMemcpyDtoH(f->meta, mptr, sizeof(f->meta)));
        const int32_t *m = f->meta;
        const char *what = nullptr;
        char detail[160] = "";
#define META_CHECK(cond, ...) if (!what && !(cond)) { what = #cond; snprintf(detail, sizeof(detail), __VA_ARGS__); }
        META_CHECK(m[SDP_META_MAGIC_AT] == SDP_META_MAGIC, "bad magic 0x%x", (unsigned)m[SDP_META_MAGIC_AT]);
        META_CHECK((m[SDP_META_FLAGS] & SDP_META_F_FAMILY) != 0, "not a family unit (flags 0x%x)", (unsigned)m[SDP_META_FLAGS]);
        META_CHECK(m[SDP_META_REAL_BYTES] == (int)rs, "built for %d-byte reals, the family has %d-byte reals", m[SDP_META_REAL_BYTES], (int)rs);
        META_CHECK(m[SDP_META_D] == f->d, "built for %d state variables, the family has %d", m[SDP_META_D], f->d);
        META_CHECK(m[SDP_META_NU] == f->nu, "built for %d controls, the family has %d", m[SDP_META_NU], f->nu);
        META_CHECK((m[SDP_META_HAS_W] != 0) == (f->W > 0), "built %s a perturbation, the family has W = %d", m[SDP_META_HAS_W] ? "with" : "without", f->W);
        META_CHECK(m[SDP_META_NW] == 0, "built for %d perturbation variables, a family takes one", m[SDP_META_NW]);
#undef META_CHECK
        if (what)
            return fail(SDP_EMODULE, "code object %s was not built for this family: %s", desc->module_path, detail);
    }
    e = hipModuleGetFunction(&f->f_sweep, f->mod, "sdp_family_sweep");
    if (e != hipSuccess) return fail(SDP_EMODULE, "code object %s has no sdp_family_sweep kernel: %s", desc->module_path, hipGetErrorString(e));
    {
        // the table of constants is the caller's: the code object's own row only tells how many there are
        hipDeviceptr_t pptr = nullptr;
        size_t pbytes = 0;
        if (hipModuleGetGlobal(&pptr, &pbytes, f->mod, "sdp_model_prm") != hipSuccess) { (void)hipGetLastError(); pbytes = 0; }
        if (pbytes != (size_t)f->n_params * rs)
            return fail(SDP_EMODULE, "code object %s declares %zu lifted constant(s), the family has %d", desc->module_path, pbytes / rs, f->n_params);
    }
    HIP_TRY(hipStreamCreate(&f->stream));
    HIP_TRY(hipEventCreate(&f->ev0));
    HIP_TRY(hipEventCreate(&f->ev1));
    guard.release();
    *out = f;
    return SDP_OK;
}

extern "C" int sdp_family_destroy(sdp_family *f)
{
    if (f) { (void)hipDeviceSynchronize(); delete f; }
    return SDP_OK;
}

extern "C" int sdp_family_set_value(sdp_family *f, const void *host_V)
{
    if (!f || !host_V) return fail(SDP_EINVAL, "NULL argument");
    const size_t bytes = (size_t)f->P * f->S * real_size(f->dtype);
    HIP_TRY(hipMemcpyAsync(f->buf[f->cur].p, host_V, bytes, hipMemcpyHostToDevice, f->stream));
    HIP_TRY(hipStreamSynchronize(f->stream));
    f->active.resize((size_t)f->P);
    for (int p = 0; p < f->P; ++p) { f->active[(size_t)p] = p; f->where[(size_t)p] = f->cur; }
    f->list_changed = true;
    return SDP_OK;
}

extern "C" int sdp_family_set_params(sdp_family *f, const void *values, int32_t n)
{
    if (!f || n < 0 || (n > 0 && !values)) return fail(SDP_EINVAL, "sdp_family_set_params: bad arguments");
    if (n != f->n_params)
        return fail(SDP_EINVAL, "sdp_family_set_params: the family has %d lifted constant(s) per member, %d given", f->n_params, (int)n);
    const size_t bytes = (size_t)f->P * (size_t)n * real_size(f->dtype);
    if (!bytes) return SDP_OK;
    // on the family's stream: ordered after the launches that still read the old values
    HIP_TRY(hipMemcpyAsync(f->prm.p, values, bytes, hipMemcpyHostToDevice, f->stream));
    HIP_TRY(hipStreamSynchronize(f->stream));        // `values` may be reused by the caller
    return SDP_OK;
}

static int family_send_list(sdp_family *f)
{
    if (!f->list_changed) return SDP_OK;
    if (!f->active.empty()) {
        HIP_TRY(hipMemcpyAsync(f->members.p, f->active.data(), f->active.size() * 4, hipMemcpyHostToDevice, f->stream));
        HIP_TRY(hipStreamSynchronize(f->stream));    // (the list may change before the copy would have run)
    }
    f->list_changed = false;
    return SDP_OK;
}

static int family_ensure_refs(sdp_family *f, int rows)
{
    if (rows < 1) rows = 1;
    if (f->refs_rows < rows) {
        int rc = f->refs.alloc((size_t)rows * f->P * 8);
        if (rc) { f->refs_rows = 0; return rc; }
        f->refs_rows = rows;
    }
    HIP_TRY(hipMemsetAsync(f->refs.p, 0, (size_t)rows * f->P * 8, f->stream));
    return SDP_OK;
}

// one backup of the listed members, buf[cur] -> buf[cur ^ 1], and with rel_dp the shift of every one of them by its
// own J[ref] (k_pick_ref + k_shift of the single problem, per member), the subtracted values in row `slot` of refs
static int family_backup(sdp_family *f, double t_k, int rel_dp, int64_t ref_index, int slot)
{
    const int n = (int)f->active.size();
    if (n < 1) return SDP_OK;
    int rc;
    if ((rc = family_send_list(f))) return rc;
    SdpFamilyArgs a;
    memset(&a, 0, sizeof(a));
    a.V = f->buf[f->cur].p; a.J = f->buf[f->cur ^ 1].p; a.pol = f->pol.p; a.idx = (int32_t *)f->idx.p;
    a.axes = f->axes.p; a.wgrid = f->wgrid.p; a.proba = f->proba.p; a.prm = f->prm.p;
    a.box_lo = f->box_lo.p; a.box_hi = f->box_hi.p; a.box_n = (const int32_t *)f->box_n.p;
    a.members = (const int32_t *)f->members.p;
    a.S = f->S; a.t_k = t_k;
    for (int k = 0; k < SDP_MAXD; ++k) { a.orders[k] = f->orders[k]; a.axis_off[k] = f->axis_off[k]; }
    a.n_axes = f->n_axes; a.W = f->W; a.box_per_node = f->box_per_node; a.n_active = n;
    // a multiple of 8 workgroups (one share per XCD, sdp_family_kernel.h): per XCD as many as it has tiles to walk,
    // at most 8 per CU of the chip in all
    const int64_t tile = (64 / f->lanes) * 4;
    const int64_t tiles = (f->S + tile - 1) / tile;
    const int parts = n >= 8 ? 1 : 8 / n;
    int64_t per_xcd = n >= 8 ? (int64_t)((n + 7) / 8) * tiles : (tiles + parts - 1) / parts;
    if (per_xcd > f->cus) per_xcd = f->cus;
    if (per_xcd < 1) per_xcd = 1;
    size_t size = sizeof(a);
    void *extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a, HIP_LAUNCH_PARAM_BUFFER_SIZE, &size, HIP_LAUNCH_PARAM_END};
    HIP_TRY(hipModuleLaunchKernel(f->f_sweep, (unsigned)(per_xcd * 8), 1, 1, 256, 1, 1, 0, f->stream, nullptr, extra));
    if (rel_dp) {
        double *ref = (double *)f->refs.p + (size_t)slot * f->P;
        unsigned bx = (unsigned)((f->S + 255) / 256);
        if (bx > 64) bx = 64;
        const int32_t *members = (const int32_t *)f->members.p;
        if (f->dtype == SDP_F32) {
            hipLaunchKernelGGL(k_family_pick_ref<float>, dim3((n + 63) / 64), dim3(64), 0, f->stream, (const float *)a.J, f->S, ref_index, members, n, ref);
            hipLaunchKernelGGL(k_family_shift<float>, dim3(bx, n), dim3(256), 0, f->stream, (float *)a.J, f->S, members, ref);
        } else {
            hipLaunchKernelGGL(k_family_pick_ref<double>, dim3((n + 63) / 64), dim3(64), 0, f->stream, (const double *)a.J, f->S, ref_index, members, n, ref);
            hipLaunchKernelGGL(k_family_shift<double>, dim3(bx, n), dim3(256), 0, f->stream, (double *)a.J, f->S, members, ref);
        }
        HIP_TRY(hipGetLastError());
    }
    for (int32_t p : f->active) f->where[(size_t)p] = f->cur ^ 1;
    return SDP_OK;
}

static int family_check_ref(const sdp_family *f, int rel_dp, int64_t ref_index)
{
    if (rel_dp && (ref_index < 0 || ref_index >= f->S)) return fail(SDP_EINVAL, "reference node %lld outside the grid", (long long)ref_index);
    return SDP_OK;
}

static int family_finish(sdp_family *f, int rel_dp, int rows, double *J_ref_out)
{
    HIP_TRY(hipEventRecord(f->ev1, f->stream));
    HIP_TRY(hipStreamSynchronize(f->stream));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, f->ev0, f->ev1));
    f->last_kernel_ms = ms;
    if (rel_dp && J_ref_out && rows > 0) HIP_TRY(hipMemcpy(J_ref_out, f->refs.p, (size_t)rows * f->P * 8, hipMemcpyDeviceToHost));
    return SDP_OK;
}

extern "C" int sdp_family_vi_sweeps(sdp_family *f, int32_t n_iter, int rel_dp, int64_t ref_index, double *J_ref_out)
{
    if (!f) return fail(SDP_EINVAL, "NULL family");
    if (n_iter < 1) return fail(SDP_EINVAL, "n_iter must be at least 1");
    int rc;
    if ((rc = family_check_ref(f, rel_dp, ref_index))) return rc;
    if ((rc = family_ensure_refs(f, n_iter))) return rc;
    if ((rc = family_send_list(f))) return rc;
    HIP_TRY(hipEventRecord(f->ev0, f->stream));
    for (int32_t k = 0; k < n_iter; ++k) {
        if (k > 0) f->cur ^= 1;                      // J of the previous sweep becomes J_next
        if ((rc = family_backup(f, 0.0, rel_dp, ref_index, k))) return rc;
    }
    return family_finish(f, rel_dp, n_iter, J_ref_out);
}

extern "C" int sdp_family_vi_sweep(sdp_family *f, double t_k, int rel_dp, int64_t ref_index, double *J_ref_out)
{
    if (!f) return fail(SDP_EINVAL, "NULL family");
    int rc;
    if ((rc = family_check_ref(f, rel_dp, ref_index))) return rc;
    if ((rc = family_ensure_refs(f, 1))) return rc;
    if ((rc = family_send_list(f))) return rc;
    HIP_TRY(hipEventRecord(f->ev0, f->stream));
    if ((rc = family_backup(f, t_k, rel_dp, ref_index, 0))) return rc;
    return family_finish(f, rel_dp, 1, J_ref_out);
}

extern "C" int sdp_family_vi_until(sdp_family *f, int32_t n_max, int rel_dp, int64_t ref_index, int32_t check_every,
                                   double tol, int32_t *n_done, double *stats, double *J_ref_out)
{
    if (!f || !n_done || !stats) return fail(SDP_EINVAL, "NULL argument");
    if (n_max < 1) return fail(SDP_EINVAL, "n_max must be at least 1");
    if (check_every < 1) return fail(SDP_EINVAL, "check_every must be at least 1");
    if (!(tol >= 0)) return fail(SDP_EINVAL, "tol must be a number >= 0");
    int rc;
    if ((rc = family_check_ref(f, rel_dp, ref_index))) return rc;
    if ((rc = family_ensure_refs(f, n_max))) return rc;
    if ((rc = family_send_list(f))) return rc;
    for (int p = 0; p < f->P; ++p) n_done[p] = 0;
    std::vector<unsigned long long> keys((size_t)f->P * 3);
    int32_t checks = 0;
    HIP_TRY(hipEventRecord(f->ev0, f->stream));
    for (int32_t k = 0; k < n_max && !f->active.empty(); ++k) {
        if (k > 0) f->cur ^= 1;
        if ((rc = family_backup(f, 0.0, rel_dp, ref_index, k))) return rc;
        for (int32_t p : f->active) n_done[p] = k + 1;
        if ((k + 1) % check_every == 0 || k + 1 == n_max) {
            const int n = (int)f->active.size();
            HIP_TRY(hipMemsetAsync(f->stats.p, 0, (size_t)n * 3 * 8, f->stream));
            unsigned bx = (unsigned)((f->S + 255) / 256);
            if (bx > 64) bx = 64;
            unsigned long long *acc = (unsigned long long *)f->stats.p;
            const int32_t *members = (const int32_t *)f->members.p;
            if (f->dtype == SDP_F32)
                hipLaunchKernelGGL(sdp_family_diff_stats<float>, dim3(bx, n), dim3(256), 0, f->stream,
                                   (const float *)f->buf[f->cur ^ 1].p, (const float *)f->buf[f->cur].p, f->S, members, (int64_t)-1, (int64_t)-1, acc);
            else
                hipLaunchKernelGGL(sdp_family_diff_stats<double>, dim3(bx, n), dim3(256), 0, f->stream,
                                   (const double *)f->buf[f->cur ^ 1].p, (const double *)f->buf[f->cur].p, f->S, members, (int64_t)-1, (int64_t)-1, acc);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(keys.data(), f->stats.p, (size_t)n * 3 * 8, hipMemcpyDeviceToHost, f->stream));
            HIP_TRY(hipStreamSynchronize(f->stream));
            std::vector<int32_t> keep;
            for (int i = 0; i < n; ++i) {
                const int32_t p = f->active[(size_t)i];
                const bool nan = keys[(size_t)i * 3 + 2] != 0;
                const double dmin = nan ? NAN : sdp_key_value(~keys[(size_t)i * 3]);
                const double dmax = nan ? NAN : sdp_key_value(keys[(size_t)i * 3 + 1]);
                stats[((size_t)checks * f->P + p) * 2] = dmin;
                stats[((size_t)checks * f->P + p) * 2 + 1] = dmax;
                if (!(dmax - dmin <= tol)) keep.push_back(p);       // NaN never converges
            }
            ++checks;
            if (keep.size() != f->active.size()) { f->active.swap(keep); f->list_changed = true; }
        }
    }
    return family_finish(f, rel_dp, n_max, J_ref_out);
}

// ---------------------------------------------------------------------------
// policy evaluation of a family (kernels sdp_family_evalpol and sdp_family_evalpol_resident of an evaluation unit,
// csrc/sdp_family_policy_kernel.h).  The loops are those of sdp_problem_eval_policy and iterate_until(evalpol) per
// member: step k > 0 of the relative algorithm reads V - V[ref] and records J_ref[k - 1], only a member's last step
// is followed by the explicit shift, and the statistics are those of the shifted sequence.
// ---------------------------------------------------------------------------
// flags[p] = 1 where the policies a and b of member p differ in a value (`!(x == y)`: a NaN differs from everything)
template <typename real>
__global__ void __launch_bounds__(256) k_family_policy_differs(const real *__restrict__ a, const real *__restrict__ b, int64_t n,
                                                               int32_t *__restrict__ flags)
{
    const int64_t p = blockIdx.y;
    const real *__restrict__ ap = a + p * n, *__restrict__ bp = b + p * n;
    bool differs = false;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        differs |= !(ap[i] == bp[i]);
    if (differs) flags[p] = 1;             // (every lane that stores stores the same word)
}

extern "C" int sdp_family_load_policy_unit(sdp_family *f, const char *module_path)
{
    if (!f || !module_path) return fail(SDP_EINVAL, "NULL argument");
    if (f->pmod) { (void)hipModuleUnload(f->pmod); f->pmod = nullptr; f->f_evalpol = f->f_resident = nullptr; }
    const size_t rs = real_size(f->dtype);
    hipError_t e = hipModuleLoad(&f->pmod, module_path);
    if (e != hipSuccess) { f->pmod = nullptr; return fail(SDP_EMODULE, "hipModuleLoad(%s): %s", module_path, hipGetErrorString(e)); }
    int32_t m[SDP_META_WORDS] = {0};
    hipDeviceptr_t mptr = nullptr;
    size_t mbytes = 0;
    const char *why = nullptr;
    if (hipModuleGetGlobal(&mptr, &mbytes, f->pmod, "sdp_meta") != hipSuccess || mbytes != sizeof(m)) {
        (void)hipGetLastError();
        why = "it does not declare `sdp_meta`";
    } else {
        HIP_TRY(hipMemcpyDtoH(m, mptr, sizeof(m)));
        if (m[SDP_META_MAGIC_AT] != SDP_META_MAGIC) why = "bad magic";
        else if (!(m[SDP_META_FLAGS] & SDP_META_F_FAMILY_POLICY)) why = "not a family evaluation unit";
        else if (m[SDP_META_REAL_BYTES] != (int)rs) why = "built for other reals";
        else if (m[SDP_META_D] != f->d) why = "built for another number of state variables";
        else if (m[SDP_META_NU] != f->nu) why = "built for another number of controls";
        else if ((m[SDP_META_HAS_W] != 0) != (f->W > 0)) why = "built with / without a perturbation, unlike the family";
        else if (m[SDP_META_THREADS] < 64 || m[SDP_META_THREADS] > 1024 || m[SDP_META_COL_ROWS] < 1
                 || (size_t)m[SDP_META_COL_ROWS] * 2 * rs > (size_t)160 * 1024) why = "bad resident geometry";
    }
    hipDeviceptr_t pptr = nullptr;
    size_t pbytes = 0;
    if (!why) {
        if (hipModuleGetGlobal(&pptr, &pbytes, f->pmod, "sdp_model_prm") != hipSuccess) { (void)hipGetLastError(); pbytes = 0; }
        if (pbytes != (size_t)f->n_params * rs) why = "another number of lifted constants";
    }
    if (!why && hipModuleGetFunction(&f->f_evalpol, f->pmod, "sdp_family_evalpol") != hipSuccess) why = "no sdp_family_evalpol kernel";
    if (!why && hipModuleGetFunction(&f->f_resident, f->pmod, "sdp_family_evalpol_resident") != hipSuccess) why = "no sdp_family_evalpol_resident kernel";
    if (why) {
        (void)hipGetLastError();
        (void)hipModuleUnload(f->pmod);
        f->pmod = nullptr; f->f_evalpol = f->f_resident = nullptr;
        return fail(SDP_EMODULE, "code object %s was not built for this family's evaluation: %s", module_path, why);
    }
    f->res_threads = m[SDP_META_THREADS];
    f->res_nodes = m[SDP_META_COL_ROWS];
    return SDP_OK;
}

static int family_ensure_pol_in(sdp_family *f)
{
    if (f->pol_in.p) return SDP_OK;
    const size_t bytes = (size_t)f->P * f->S * f->nu * real_size(f->dtype);
    int rc;
    if ((rc = f->pol_in.alloc(bytes))) return rc;
    HIP_TRY(hipMemset(f->pol_in.p, 0, bytes));
    return SDP_OK;
}

extern "C" int sdp_family_set_policy(sdp_family *f, const void *host_pol)
{
    if (!f || !host_pol) return fail(SDP_EINVAL, "NULL argument");
    int rc;
    if ((rc = family_ensure_pol_in(f))) return rc;
    HIP_TRY(hipMemcpyAsync(f->pol_in.p, host_pol, (size_t)f->P * f->S * f->nu * real_size(f->dtype), hipMemcpyHostToDevice, f->stream));
    HIP_TRY(hipStreamSynchronize(f->stream));
    f->has_policy = true;
    return SDP_OK;
}

// the policy the last sweep wrote becomes the prescribed one, and the other buffer the next sweep's output: no copy
extern "C" int sdp_family_take_policy(sdp_family *f)
{
    if (!f) return fail(SDP_EINVAL, "NULL family");
    int rc;
    if ((rc = family_ensure_pol_in(f))) return rc;
    HIP_TRY(hipStreamSynchronize(f->stream));
    std::swap(f->pol.p, f->pol_in.p);
    f->has_policy = true;
    return SDP_OK;
}

extern "C" int sdp_family_set_members(sdp_family *f, const int32_t *members, int32_t n)
{
    if (!f || !members) return fail(SDP_EINVAL, "NULL argument");
    if (n < 1 || n > f->P) return fail(SDP_EINVAL, "%d members listed: a family of %d lists 1..%d", (int)n, f->P, f->P);
    std::vector<char> seen((size_t)f->P, 0);
    for (int32_t i = 0; i < n; ++i) {
        if (members[i] < 0 || members[i] >= f->P || seen[(size_t)members[i]])
            return fail(SDP_EINVAL, "listed member %d (position %d) is outside 0..%d or listed twice", (int)members[i], (int)i, f->P - 1);
        seen[(size_t)members[i]] = 1;
    }
    f->active.assign(members, members + n);
    f->list_changed = true;
    return SDP_OK;
}

// 1 where the policy of the last sweep equals the prescribed one, value by value
extern "C" int sdp_family_compare_policy(sdp_family *f, int32_t *same)
{
    if (!f || !same) return fail(SDP_EINVAL, "NULL argument");
    if (!f->has_policy || !f->pol_in.p) return fail(SDP_EINVAL, "no policy set (sdp_family_set_policy)");
    int rc;
    if (!f->flags.p && (rc = f->flags.alloc((size_t)f->P * 4))) return rc;
    HIP_TRY(hipMemsetAsync(f->flags.p, 0, (size_t)f->P * 4, f->stream));
    const int64_t n = f->S * f->nu;
    unsigned bx = (unsigned)((n + 255) / 256);
    if (bx > 64) bx = 64;
    if (f->dtype == SDP_F32)
        hipLaunchKernelGGL(k_family_policy_differs<float>, dim3(bx, (unsigned)f->P), dim3(256), 0, f->stream,
                           (const float *)f->pol.p, (const float *)f->pol_in.p, n, (int32_t *)f->flags.p);
    else
        hipLaunchKernelGGL(k_family_policy_differs<double>, dim3(bx, (unsigned)f->P), dim3(256), 0, f->stream,
                           (const double *)f->pol.p, (const double *)f->pol_in.p, n, (int32_t *)f->flags.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(same, f->flags.p, (size_t)f->P * 4, hipMemcpyDeviceToHost, f->stream));
    HIP_TRY(hipStreamSynchronize(f->stream));
    for (int p = 0; p < f->P; ++p) same[p] = !same[p];
    return SDP_OK;
}

static int family_eval_check(const sdp_family *f, int form)
{
    if (!f->f_evalpol || !f->f_resident) return fail(SDP_EINVAL, "no evaluation unit loaded (sdp_family_load_policy_unit)");
    if (!f->has_policy || !f->pol_in.p) return fail(SDP_EINVAL, "no policy set (sdp_family_set_policy)");
    if (form != SDP_FAMILY_EVAL_STEPS && form != SDP_FAMILY_EVAL_RESIDENT) return fail(SDP_EINVAL, "evaluation form %d: 0 (steps) or 1 (resident)", form);
    // the fit rule: two buffers of S reals beside what the reduction needs, in the LDS budget the kernel was built for
    if (form == SDP_FAMILY_EVAL_RESIDENT && f->S > f->res_nodes)
        return fail(SDP_EINVAL, "the resident form holds two buffers of at most %lld reals (%lld bytes): a member of %lld nodes needs %lld bytes",
                    (long long)f->res_nodes, (long long)(f->res_nodes * 2 * (int64_t)real_size(f->dtype)), (long long)f->S,
                    (long long)(f->S * 2 * (int64_t)real_size(f->dtype)));
    return SDP_OK;
}

static void family_eval_args(const sdp_family *f, SdpFamilyEvalArgs &e, int64_t ref_index)
{
    memset(&e, 0, sizeof(e));
    SdpFamilyArgs &a = e.f;
    a.V = f->buf[f->cur].p; a.J = f->buf[f->cur ^ 1].p; a.pol = f->pol_in.p;
    a.axes = f->axes.p; a.wgrid = f->wgrid.p; a.proba = f->proba.p; a.prm = f->prm.p;
    a.members = (const int32_t *)f->members.p;
    a.S = f->S; a.t_k = 0.0;                         // a time-dependent system is evaluated at time index 0
    for (int k = 0; k < SDP_MAXD; ++k) { a.orders[k] = f->orders[k]; a.axis_off[k] = f->axis_off[k]; }
    a.n_axes = f->n_axes; a.W = f->W; a.n_active = (int)f->active.size();
    e.ref_index = ref_index; e.refs = (double *)f->refs.p; e.P = f->P;
}

// one step of the listed members, buf[cur] -> buf[cur ^ 1] (raw values); fused: the relative shift of the step before
static int family_evalpol_step(sdp_family *f, bool fused, int64_t ref_index, int slot)
{
    const int n = (int)f->active.size();
    if (n < 1) return SDP_OK;
    int rc;
    if ((rc = family_send_list(f))) return rc;
    SdpFamilyEvalArgs e;
    family_eval_args(f, e, ref_index);
    e.shift = fused ? 1 : 0;
    e.slot = slot;
    // a multiple of 8 workgroups, as family_backup, with the evaluation's tile of 256 nodes (a workgroup)
    const int64_t tiles = (f->S + 255) / 256;
    const int parts = n >= 8 ? 1 : 8 / n;
    int64_t per_xcd = n >= 8 ? (int64_t)((n + 7) / 8) * tiles : (tiles + parts - 1) / parts;
    if (per_xcd > f->cus) per_xcd = f->cus;
    if (per_xcd < 1) per_xcd = 1;
    size_t size = sizeof(e);
    void *extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &e, HIP_LAUNCH_PARAM_BUFFER_SIZE, &size, HIP_LAUNCH_PARAM_END};
    HIP_TRY(hipModuleLaunchKernel(f->f_evalpol, (unsigned)(per_xcd * 8), 1, 1, 256, 1, 1, 0, f->stream, nullptr, extra));
    for (int32_t p : f->active) f->where[(size_t)p] = f->cur ^ 1;
    return SDP_OK;
}

// the explicit shift after a member's last step: `n` members listed in `list` (device), their raw values in `J`
static int family_last_shift(sdp_family *f, const int32_t *list, int n, void *J, int64_t ref_index, int slot)
{
    if (n < 1) return SDP_OK;
    double *ref = (double *)f->refs.p + (size_t)slot * f->P;
    unsigned bx = (unsigned)((f->S + 255) / 256);
    if (bx > 64) bx = 64;
    if (f->dtype == SDP_F32) {
        hipLaunchKernelGGL(k_family_pick_ref<float>, dim3((n + 63) / 64), dim3(64), 0, f->stream, (const float *)J, f->S, ref_index, list, n, ref);
        hipLaunchKernelGGL(k_family_shift<float>, dim3(bx, n), dim3(256), 0, f->stream, (float *)J, f->S, list, ref);
    } else {
        hipLaunchKernelGGL(k_family_pick_ref<double>, dim3((n + 63) / 64), dim3(64), 0, f->stream, (const double *)J, f->S, ref_index, list, n, ref);
        hipLaunchKernelGGL(k_family_shift<double>, dim3(bx, n), dim3(256), 0, f->stream, (double *)J, f->S, list, ref);
    }
    HIP_TRY(hipGetLastError());
    return SDP_OK;
}

// all steps of the listed members in one launch, buf[cur] -> buf[cur ^ 1] (final values); check_every 0: no check
static int family_resident(sdp_family *f, int32_t n_iter, int rel_dp, int64_t ref_index, int32_t check_every, double tol,
                           size_t n_checks)
{
    const int n = (int)f->active.size();
    if (n < 1) return SDP_OK;
    int rc;
    if ((rc = family_send_list(f))) return rc;
    if (f->S > f->res_nodes) return fail(SDP_EINVAL, "a member of %lld nodes is not resident (%lld at most)", (long long)f->S, (long long)f->res_nodes);
    if (!f->res_done.p && (rc = f->res_done.alloc((size_t)f->P * 4))) return rc;
    HIP_TRY(hipMemsetAsync(f->res_done.p, 0, (size_t)f->P * 4, f->stream));
    if (n_checks > 0) {
        if (f->res_stats_rows < n_checks) {
            if ((rc = f->res_stats.alloc(n_checks * f->P * 16))) { f->res_stats_rows = 0; return rc; }
            f->res_stats_rows = n_checks;
        }
        HIP_TRY(hipMemsetAsync(f->res_stats.p, 0xff, n_checks * f->P * 16, f->stream));      // (NaN: a check that did not run)
    }
    SdpFamilyEvalArgs e;
    family_eval_args(f, e, ref_index);
    e.rel_dp = rel_dp ? 1 : 0; e.n_iter = n_iter; e.check_every = check_every; e.tol = tol;
    e.n_done = (int32_t *)f->res_done.p;
    e.stats = n_checks > 0 ? (double *)f->res_stats.p : nullptr;
    // one workgroup a member and, with the whole LDS of a CU each, one workgroup a CU: the grid strides over the list
    int blocks = n;
    if (blocks > f->cus) blocks = f->cus;
    size_t size = sizeof(e);
    void *extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &e, HIP_LAUNCH_PARAM_BUFFER_SIZE, &size, HIP_LAUNCH_PARAM_END};
    HIP_TRY(hipModuleLaunchKernel(f->f_resident, (unsigned)blocks, 1, 1, (unsigned)f->res_threads, 1, 1, 0, f->stream, nullptr, extra));
    for (int32_t p : f->active) f->where[(size_t)p] = f->cur ^ 1;
    return SDP_OK;
}

extern "C" int sdp_family_eval_policy(sdp_family *f, int32_t n_iter, int rel_dp, int64_t ref_index, int32_t form, double *J_ref_out)
{
    if (!f) return fail(SDP_EINVAL, "NULL family");
    if (n_iter < 0) return fail(SDP_EINVAL, "negative iteration count");
    int rc;
    if ((rc = family_eval_check(f, form))) return rc;
    if ((rc = family_check_ref(f, rel_dp, ref_index))) return rc;
    f->last_kernel_ms = 0;
    if (n_iter == 0) return SDP_OK;                  // the result is the starting value
    if ((rc = family_ensure_refs(f, n_iter))) return rc;
    if ((rc = family_send_list(f))) return rc;
    HIP_TRY(hipEventRecord(f->ev0, f->stream));
    if (form == SDP_FAMILY_EVAL_RESIDENT) {
        if ((rc = family_resident(f, n_iter, rel_dp, ref_index, 0, 0.0, 0))) return rc;
    } else {
        for (int32_t k = 0; k < n_iter; ++k) {
            if (k > 0) f->cur ^= 1;
            if ((rc = family_evalpol_step(f, rel_dp && k > 0, ref_index, k - 1))) return rc;
        }
        if (rel_dp && (rc = family_last_shift(f, (const int32_t *)f->members.p, (int)f->active.size(), f->buf[f->cur ^ 1].p, ref_index, n_iter - 1))) return rc;
    }
    return family_finish(f, rel_dp, n_iter, J_ref_out);
}

extern "C" int sdp_family_eval_policy_until(sdp_family *f, int32_t n_max, int rel_dp, int64_t ref_index, int32_t check_every,
                                            double tol, int32_t form, int32_t *n_done, double *stats, double *J_ref_out)
{
    if (!f || !n_done || !stats) return fail(SDP_EINVAL, "NULL argument");
    if (n_max < 1) return fail(SDP_EINVAL, "n_max must be at least 1");
    if (check_every < 1) return fail(SDP_EINVAL, "check_every must be at least 1");
    if (!(tol >= 0)) return fail(SDP_EINVAL, "tol must be a number >= 0");
    int rc;
    if ((rc = family_eval_check(f, form))) return rc;
    if ((rc = family_check_ref(f, rel_dp, ref_index))) return rc;
    if ((rc = family_ensure_refs(f, n_max))) return rc;
    if ((rc = family_send_list(f))) return rc;
    for (int p = 0; p < f->P; ++p) n_done[p] = 0;
    const size_t P = (size_t)f->P;
    if (form == SDP_FAMILY_EVAL_RESIDENT) {
        const size_t n_checks = (size_t)(n_max / check_every + (n_max % check_every ? 1 : 0));
        const std::vector<int32_t> listed = f->active;
        HIP_TRY(hipEventRecord(f->ev0, f->stream));
        if ((rc = family_resident(f, n_max, rel_dp, ref_index, check_every, tol, n_checks))) return rc;
        if ((rc = family_finish(f, rel_dp, n_max, J_ref_out))) return rc;
        // everything is read back once, at the end
        std::vector<int32_t> done(P);
        std::vector<double> st(n_checks * P * 2);
        HIP_TRY(hipMemcpy(done.data(), f->res_done.p, P * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(st.data(), f->res_stats.p, st.size() * 8, hipMemcpyDeviceToHost));
        for (int32_t p : listed) {
            n_done[p] = done[(size_t)p];
            for (size_t c = 0; c < n_checks; ++c) {
                stats[(c * P + p) * 2] = st[(c * P + p) * 2];
                stats[(c * P + p) * 2 + 1] = st[(c * P + p) * 2 + 1];
            }
        }
        return SDP_OK;
    }
    std::vector<unsigned long long> keys(P * 3);
    if (!f->leavers.p && (rc = f->leavers.alloc(P * 4))) return rc;
    int32_t checks = 0;
    HIP_TRY(hipEventRecord(f->ev0, f->stream));
    for (int32_t k = 0; k < n_max && !f->active.empty(); ++k) {
        if (k > 0) f->cur ^= 1;
        if ((rc = family_evalpol_step(f, rel_dp && k > 0, ref_index, k - 1))) return rc;
        for (int32_t p : f->active) n_done[p] = k + 1;
        if ((k + 1) % check_every == 0 || k + 1 == n_max) {
            // one reduction launch over the listed members and 24 bytes a member back: the statistics of the shifted
            // sequence, from the raw buffers
            const int n = (int)f->active.size();
            HIP_TRY(hipMemsetAsync(f->stats.p, 0, (size_t)n * 3 * 8, f->stream));
            unsigned bx = (unsigned)((f->S + 255) / 256);
            if (bx > 64) bx = 64;
            unsigned long long *acc = (unsigned long long *)f->stats.p;
            const int32_t *members = (const int32_t *)f->members.p;
            const int64_t ra = rel_dp ? ref_index : -1, rb = rel_dp && k > 0 ? ref_index : -1;
            if (f->dtype == SDP_F32)
                hipLaunchKernelGGL(sdp_family_diff_stats<float>, dim3(bx, n), dim3(256), 0, f->stream,
                                   (const float *)f->buf[f->cur ^ 1].p, (const float *)f->buf[f->cur].p, f->S, members, ra, rb, acc);
            else
                hipLaunchKernelGGL(sdp_family_diff_stats<double>, dim3(bx, n), dim3(256), 0, f->stream,
                                   (const double *)f->buf[f->cur ^ 1].p, (const double *)f->buf[f->cur].p, f->S, members, ra, rb, acc);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(keys.data(), f->stats.p, (size_t)n * 3 * 8, hipMemcpyDeviceToHost, f->stream));
            HIP_TRY(hipStreamSynchronize(f->stream));
            std::vector<int32_t> keep, leave;
            for (int i = 0; i < n; ++i) {
                const int32_t p = f->active[(size_t)i];
                const bool nan = keys[(size_t)i * 3 + 2] != 0;
                const double dmin = nan ? NAN : sdp_key_value(~keys[(size_t)i * 3]);
                const double dmax = nan ? NAN : sdp_key_value(keys[(size_t)i * 3 + 1]);
                stats[((size_t)checks * P + p) * 2] = dmin;
                stats[((size_t)checks * P + p) * 2 + 1] = dmax;
                if (!(dmax - dmin <= tol) && k + 1 < n_max) keep.push_back(p);       // NaN never converges
                else leave.push_back(p);
            }
            ++checks;
            if (!leave.empty()) {
                // a member that stops here takes its explicit shift now: its raw values stay in the buffer of this step
                if (rel_dp) {
                    HIP_TRY(hipMemcpyAsync(f->leavers.p, leave.data(), leave.size() * 4, hipMemcpyHostToDevice, f->stream));
                    HIP_TRY(hipStreamSynchronize(f->stream));
                    if ((rc = family_last_shift(f, (const int32_t *)f->leavers.p, (int)leave.size(), f->buf[f->cur ^ 1].p, ref_index, k))) return rc;
                }
                f->active.swap(keep);
                f->list_changed = true;
            }
        }
    }
    return family_finish(f, rel_dp, n_max, J_ref_out);
}

// ---------------------------------------------------------------------------
// Monte Carlo policy evaluation of a family (csrc/sdp_family_mc_kernel.h): sdp_problem_montecarlo of every member in
// one launch per cut of the steps.  The unit is loaded beside the sweep unit; the arrays of a run live for the call.
// ---------------------------------------------------------------------------
extern "C" int sdp_family_load_mc_unit(sdp_family *f, const char *module_path)
{
    if (!f || !module_path) return fail(SDP_EINVAL, "NULL argument");
    if (f->mcmod) { (void)hipModuleUnload(f->mcmod); f->mcmod = nullptr; f->f_montecarlo = nullptr; }
    const size_t rs = real_size(f->dtype);
    hipError_t e = hipModuleLoad(&f->mcmod, module_path);
    if (e != hipSuccess) { f->mcmod = nullptr; return fail(SDP_EMODULE, "hipModuleLoad(%s): %s", module_path, hipGetErrorString(e)); }
    int32_t m[SDP_META_WORDS] = {0};
    hipDeviceptr_t mptr = nullptr;
    size_t mbytes = 0;
    const char *why = nullptr;
    if (hipModuleGetGlobal(&mptr, &mbytes, f->mcmod, "sdp_meta") != hipSuccess || mbytes != sizeof(m)) {
        (void)hipGetLastError();
        why = "it does not declare `sdp_meta`";
    } else {
        HIP_TRY(hipMemcpyDtoH(m, mptr, sizeof(m)));
        if (m[SDP_META_MAGIC_AT] != SDP_META_MAGIC) why = "bad magic";
        else if (!(m[SDP_META_FLAGS] & SDP_META_F_FAMILY_MC)) why = "not a family Monte Carlo unit";
        else if (m[SDP_META_THREADS] != 256) why = "built for another workgroup size";
        else if (m[SDP_META_REAL_BYTES] != (int)rs) why = "built for other reals";
        else if (m[SDP_META_D] != f->d) why = "built for another number of state variables";
        else if (m[SDP_META_NU] != f->nu) why = "built for another number of controls";
        else if (!m[SDP_META_HAS_W] || f->W <= 0) why = "a deterministic system has nothing to draw";
    }
    hipDeviceptr_t pptr = nullptr;
    size_t pbytes = 0;
    if (!why) {
        if (hipModuleGetGlobal(&pptr, &pbytes, f->mcmod, "sdp_model_prm") != hipSuccess) { (void)hipGetLastError(); pbytes = 0; }
        if (pbytes != (size_t)f->n_params * rs) why = "another number of lifted constants";
    }
    if (!why && hipModuleGetFunction(&f->f_montecarlo, f->mcmod, "sdp_family_montecarlo") != hipSuccess) why = "no sdp_family_montecarlo kernel";
    if (why) {
        (void)hipGetLastError();
        (void)hipModuleUnload(f->mcmod);
        f->mcmod = nullptr; f->f_montecarlo = nullptr;
        return fail(SDP_EMODULE, "code object %s was not built for this family's Monte Carlo evaluation: %s", module_path, why);
    }
    return SDP_OK;
}

extern "C" int sdp_family_montecarlo(sdp_family *f, const void *host_pol, int64_t B, int64_t T, int64_t n_burn,
                                     const uint64_t *host_seeds, uint64_t traj_offset, const void *host_x0,
                                     const double *host_cum, int32_t n_law, const void *host_law_grid, double t0,
                                     int64_t steps_per_launch, void *host_cost_sum, int64_t *host_n_outside,
                                     void *host_x_final, uint64_t *host_occupancy)
{
    if (!f || !host_pol || !host_seeds || !host_x0 || !host_cum || !host_law_grid || !host_cost_sum || !host_n_outside || !host_x_final)
        return fail(SDP_EINVAL, "NULL argument");
    if (B < 0 || T < 0) return fail(SDP_EINVAL, "negative size");
    if (n_burn < 0 || n_burn > T) return fail(SDP_EINVAL, "n_burn = %lld outside [0, %lld]", (long long)n_burn, (long long)T);
    if (steps_per_launch < 1) return fail(SDP_EINVAL, "steps_per_launch = %lld: at least 1", (long long)steps_per_launch);
    if (f->W <= 0) return fail(SDP_EINVAL, "a deterministic system has nothing to draw");
    if (n_law < 1 || n_law > 4096) return fail(SDP_EINVAL, "a law of %d points: 1 to 4096", (int)n_law);
    if (!f->f_montecarlo) return fail(SDP_EINVAL, "no Monte Carlo unit loaded (sdp_family_load_mc_unit)");
    if (B == 0) return SDP_OK;
    if (steps_per_launch > ((int64_t)1 << 30)) steps_per_launch = (int64_t)1 << 30;       // (the kernel counts a launch's steps in 32 bits)
    const size_t rs = real_size(f->dtype);
    const size_t P = (size_t)f->P;
    // (the draw table of one member in LDS: the cumulative sums, then the values)
    const size_t lds_bytes = (size_t)(n_law - 1) * 8 + (size_t)n_law * rs;
    if (lds_bytes > 65536)
        return fail(SDP_EINVAL, "a law of %d points needs %zu bytes of LDS: at most 65536", (int)n_law, lds_bytes);
    DevBuf dpol, dx, dacc, dout, dcum, dlaw, dseed, docc;
    int rc;
    if ((rc = upload(dpol, host_pol, P * (size_t)f->nu * f->S * rs))) return rc;          // [P][nu][S]
    if ((rc = upload(dx, host_x0, P * (size_t)f->d * B * rs))) return rc;                 // [P][d][B]
    if ((rc = upload(dcum, host_cum, P * (size_t)n_law * 8))) return rc;
    if ((rc = upload(dlaw, host_law_grid, P * (size_t)n_law * rs))) return rc;
    if ((rc = upload(dseed, host_seeds, P * 8))) return rc;
    if ((rc = dacc.alloc(P * (size_t)B * rs))) return rc;
    if ((rc = dout.alloc(P * (size_t)B * 8))) return rc;
    HIP_TRY(hipMemsetAsync(dacc.p, 0, P * (size_t)B * rs, f->stream));
    HIP_TRY(hipMemsetAsync(dout.p, 0, P * (size_t)B * 8, f->stream));
    if (host_occupancy) {
        if ((rc = docc.alloc(P * (size_t)f->S * 8))) return rc;
        HIP_TRY(hipMemsetAsync(docc.p, 0, P * (size_t)f->S * 8, f->stream));
    }
    SdpFamilyMcArgs a;
    memset(&a, 0, sizeof(a));
    a.pol = dpol.p; a.axes = f->axes.p; a.prm = f->prm.p; a.cum = (const double *)dcum.p; a.law_grid = dlaw.p;
    a.seed = (const uint64_t *)dseed.p; a.x = dx.p; a.acc = dacc.p; a.n_outside = (long long *)dout.p;
    a.occupancy = host_occupancy ? (unsigned long long *)docc.p : nullptr;
    a.B = B; a.S = f->S; a.traj_offset = traj_offset; a.n_burn = n_burn; a.t0 = t0;
    a.n_law = n_law; a.n_axes = f->n_axes; a.P = f->P;
    for (int k = 0; k < SDP_MAXD; ++k) { a.orders[k] = f->orders[k]; a.axis_off[k] = f->axis_off[k]; }
    size_t size = sizeof(a);
    void *extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a, HIP_LAUNCH_PARAM_BUFFER_SIZE, &size, HIP_LAUNCH_PARAM_END};
    // a tile of 256 trajectories of one member is a workgroup.  A multiple of 8 workgroups (one share per XCD,
    // sdp_family_mc_kernel.h): per XCD as many as it has tiles to walk, in all at most the workgroups that are resident
    // at once (the kernel's registers and the draw table decide how many a CU holds, 8 at most), the rest in the stride loop
    const int threads = 256;
    const unsigned lds = (unsigned)lds_bytes;
    int per_cu = 0;
    if (hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, f->f_montecarlo, threads, lds) != hipSuccess) {
        (void)hipGetLastError();
        per_cu = 0;
    }
    if (per_cu < 1) per_cu = 1;
    if (per_cu > 8) per_cu = 8;
    const int64_t tiles = (B + threads - 1) / threads;
    const int parts = f->P >= 8 ? 1 : 8 / f->P;
    int64_t per_xcd = f->P >= 8 ? (int64_t)((f->P + 7) / 8) * tiles : (tiles + parts - 1) / parts;
    const int64_t cap = (int64_t)f->cus * per_cu / 8;
    if (per_xcd > cap) per_xcd = cap;
    if (per_xcd < 1) per_xcd = 1;
    HIP_TRY(hipStreamSynchronize(f->stream));        // lifted constants set on the family's stream
    HIP_TRY(hipEventRecord(f->ev0, f->stream));
    for (int64_t k = 0; k < T; k += steps_per_launch) {
        a.step_begin = k;
        a.step_end = (T - k < steps_per_launch) ? T : k + steps_per_launch;
        HIP_TRY(hipModuleLaunchKernel(f->f_montecarlo, (unsigned)(per_xcd * 8), 1, 1, threads, 1, 1, lds, f->stream, nullptr, extra));
    }
    HIP_TRY(hipEventRecord(f->ev1, f->stream));
    HIP_TRY(hipStreamSynchronize(f->stream));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, f->ev0, f->ev1));
    f->last_kernel_ms = ms;
    HIP_TRY(hipMemcpy(host_cost_sum, dacc.p, P * (size_t)B * rs, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(host_n_outside, dout.p, P * (size_t)B * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(host_x_final, dx.p, P * (size_t)f->d * B * rs, hipMemcpyDeviceToHost));
    if (host_occupancy) HIP_TRY(hipMemcpy(host_occupancy, docc.p, P * (size_t)f->S * 8, hipMemcpyDeviceToHost));
    return SDP_OK;
}

// ---------------------------------------------------------------------------
// Transition operators of a family's policies (csrc/sdp_family_trans_kernel.h): sdp_transop_create of every member in
// one launch and one sort.  The members' operators are ONE block-diagonal sdp_transop on P S rows -- member p's node s
// is row p S + s -- so the CSR build, both push paths and every accessor of the solo operator serve it as they are; the
// stable sort and the members' disjoint rows keep every member's rows in the solo entry order.  The operator owns its
// arrays and outlives the family.  sdp_transop_push_until_members is the power iteration with a stop per member.
// ---------------------------------------------------------------------------
extern "C" int sdp_family_load_trans_unit(sdp_family *f, const char *module_path)
{
    if (!f || !module_path) return fail(SDP_EINVAL, "NULL argument");
    if (f->trmod) { (void)hipModuleUnload(f->trmod); f->trmod = nullptr; f->f_transitions = nullptr; }
    const size_t rs = real_size(f->dtype);
    hipError_t e = hipModuleLoad(&f->trmod, module_path);
    if (e != hipSuccess) { f->trmod = nullptr; return fail(SDP_EMODULE, "hipModuleLoad(%s): %s", module_path, hipGetErrorString(e)); }
    int32_t m[SDP_META_WORDS] = {0};
    hipDeviceptr_t mptr = nullptr;
    size_t mbytes = 0;
    const char *why = nullptr;
    if (hipModuleGetGlobal(&mptr, &mbytes, f->trmod, "sdp_meta") != hipSuccess || mbytes != sizeof(m)) {
        (void)hipGetLastError();
        why = "it does not declare `sdp_meta`";
    } else {
        HIP_TRY(hipMemcpyDtoH(m, mptr, sizeof(m)));
        if (m[SDP_META_MAGIC_AT] != SDP_META_MAGIC) why = "bad magic";
        else if (!(m[SDP_META_FLAGS] & SDP_META_F_FAMILY_TRANS)) why = "not a family transition unit";
        else if (m[SDP_META_THREADS] != 256) why = "built for another workgroup size";
        else if (m[SDP_META_COL_ROWS] != (256 >> f->d)) why = "built for another tile";
        else if (m[SDP_META_REAL_BYTES] != (int)rs) why = "built for other reals";
        else if (m[SDP_META_D] != f->d) why = "built for another number of state variables";
        else if (m[SDP_META_NU] != f->nu) why = "built for another number of controls";
        else if ((m[SDP_META_HAS_W] != 0) != (f->W > 0)) why = "built for a model with / without a perturbation";
    }
    hipDeviceptr_t pptr = nullptr;
    size_t pbytes = 0;
    if (!why) {
        if (hipModuleGetGlobal(&pptr, &pbytes, f->trmod, "sdp_model_prm") != hipSuccess) { (void)hipGetLastError(); pbytes = 0; }
        if (pbytes != (size_t)f->n_params * rs) why = "another number of lifted constants";
    }
    if (!why && hipModuleGetFunction(&f->f_transitions, f->trmod, "sdp_family_transitions") != hipSuccess) why = "no sdp_family_transitions kernel";
    if (why) {
        (void)hipGetLastError();
        (void)hipModuleUnload(f->trmod);
        f->trmod = nullptr; f->f_transitions = nullptr;
        return fail(SDP_EMODULE, "code object %s was not built for this family's transition operators: %s", module_path, why);
    }
    f->trans_tile = m[SDP_META_COL_ROWS];
    return SDP_OK;
}

extern "C" int sdp_family_transop_create(sdp_family *f, const void *host_pol, double t_k, sdp_transop **out)
{
    if (!f || !host_pol || !out) return fail(SDP_EINVAL, "NULL argument");
    if (!f->f_transitions) return fail(SDP_EINVAL, "no transition unit loaded (sdp_family_load_trans_unit)");
    const size_t rs = real_size(f->dtype);
    const int64_t P = f->P, S = f->S, W = f->W > 0 ? f->W : 1, V = (int64_t)1 << f->d;
    const int64_t rows = P * S;
    if (rows >= (int64_t)1 << 31)
        return fail(SDP_EINVAL, "%lld members of %lld nodes: the rows of their operators are 32-bit ids (at most 2^31 - 1 rows)", (long long)P, (long long)S);
    const int64_t nnz = rows * W * V;
    if (nnz >= (int64_t)1 << 32)
        return fail(SDP_EINVAL, "operators of %lld entries together: entry positions are 32-bit words (at most 2^32 - 1 entries)", (long long)nnz);
    sdp_transop *op = nullptr;
    int rc;
    if ((rc = transop_new(f->dtype, rows, nnz, &op))) return rc;
    std::unique_ptr<sdp_transop> guard(op);
    op->P = (int)P; op->Sm = S;
    DevBuf dpol, done, tgt, val;
    if ((rc = upload(dpol, host_pol, (size_t)rows * f->nu * rs))) return rc;          // [P][S][nu]
    if (f->W <= 0) {                                       // deterministic members: the law of one point of weight 1
        const double one8 = 1.0;
        const float one4 = 1.0f;
        if ((rc = upload(done, f->dtype == SDP_F32 ? (const void *)&one4 : (const void *)&one8, rs))) return rc;
    }
    if ((rc = tgt.alloc((size_t)nnz * 4))) return rc;
    if ((rc = val.alloc((size_t)nnz * rs))) return rc;
    if ((rc = op->gbar.alloc((size_t)rows * rs))) return rc;
    {
        const std::vector<int32_t> ones((size_t)P, 1);
        if ((rc = upload(op->flags, ones.data(), (size_t)P * 4))) return rc;
    }
    if ((rc = op->running.alloc((size_t)P * 4))) return rc;
    if ((rc = op->mstats.alloc((size_t)P * 3 * 8))) return rc;
    SdpFamilyTransArgs a;
    memset(&a, 0, sizeof(a));
    a.f.pol = dpol.p; a.f.axes = f->axes.p; a.f.prm = f->prm.p;
    a.f.wgrid = f->W > 0 ? f->wgrid.p : nullptr;
    a.f.proba = f->W > 0 ? f->proba.p : done.p;
    a.f.S = S; a.f.t_k = t_k;
    for (int k = 0; k < SDP_MAXD; ++k) { a.f.orders[k] = f->orders[k]; a.f.axis_off[k] = f->axis_off[k]; }
    a.f.n_axes = f->n_axes; a.f.W = f->W; a.f.n_active = (int32_t)P;
    a.tgt = (int32_t *)tgt.p; a.val = val.p; a.gbar = op->gbar.p; a.W = (int32_t)W;
    size_t size = sizeof(a);
    void *extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a, HIP_LAUNCH_PARAM_BUFFER_SIZE, &size, HIP_LAUNCH_PARAM_END};
    // a tile of 256 >> d nodes of one member is a workgroup: at most the workgroups that are resident, the rest in the
    // kernel's stride loop
    const int64_t tiles = (S + f->trans_tile - 1) / f->trans_tile;
    int64_t blocks = P * tiles;
    if (blocks > (int64_t)f->cus * 8) blocks = (int64_t)f->cus * 8;
    HIP_TRY(hipStreamSynchronize(f->stream));        // lifted constants set on the family's stream
    HIP_TRY(hipEventRecord(op->ev0, op->stream));
    HIP_TRY(hipModuleLaunchKernel(f->f_transitions, (unsigned)blocks, 1, 1, 256, 1, 1, 0, op->stream, nullptr, extra));
    HIP_TRY(hipEventRecord(op->ev1, op->stream));
    if ((rc = transop_build_csr(op, (const int32_t *)tgt.p, val.p, nullptr, (uint32_t)(W * V)))) return rc;
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, op->ev0, op->ev1));
    op->entries_ms = ms;
    op->last_kernel_ms = op->entries_ms + op->sort_ms;
    op->has_gbar = true;
    guard.release();
    *out = op;
    return SDP_OK;
}

extern "C" int sdp_transop_push_until_members(sdp_transop *op, int32_t n_max, int32_t check_every, double tol,
                                              int32_t *n_done, double *delta)
{
    if (!op || !n_done || !delta) return fail(SDP_EINVAL, "NULL argument");
    if (op->P < 1) return fail(SDP_EINVAL, "not the operators of a family (sdp_family_transop_create)");
    if (n_max < 1) return fail(SDP_EINVAL, "n_max must be at least 1");
    if (check_every < 1) return fail(SDP_EINVAL, "check_every must be at least 1");
    if (!(tol >= 0)) return fail(SDP_EINVAL, "tol must be a number >= 0");
    int rc;
    if ((rc = transop_set(op, nullptr))) return rc;
    if ((rc = transop_all_running(op))) return rc;
    const size_t P = (size_t)op->P;
    const size_t slice = (size_t)op->Sm * real_size(op->dtype);
    std::vector<int32_t> running(P), flags(P, 1), keep, leave;
    for (size_t p = 0; p < P; ++p) { running[p] = (int32_t)p; n_done[p] = 0; delta[p] = NAN; }
    HIP_TRY(hipMemcpyAsync(op->running.p, running.data(), P * 4, hipMemcpyHostToDevice, op->stream));
    HIP_TRY(hipStreamSynchronize(op->stream));
    std::vector<unsigned long long> keys(P * 3);
    HIP_TRY(hipEventRecord(op->ev0, op->stream));
    for (int32_t k = 0; k < n_max && !running.empty(); ++k) {
        if ((rc = transop_launch_push(op))) return rc;     // the rows of the members still running
        for (int32_t p : running) n_done[p] = k + 1;
        if ((k + 1) % check_every != 0 && k + 1 != n_max) continue;
        // one reduction launch over the members still running and 24 bytes a member back
        const int n = (int)running.size();
        HIP_TRY(hipMemsetAsync(op->mstats.p, 0, (size_t)n * 3 * 8, op->stream));
        unsigned bx = (unsigned)((op->Sm + 255) / 256);
        if (bx > 64) bx = 64;
        unsigned long long *acc = (unsigned long long *)op->mstats.p;
        const int32_t *members = (const int32_t *)op->running.p;
        const void *cur = op->mu[op->cur].p, *old = op->mu[1 - op->cur].p;
        if (op->dtype == SDP_F32)
            hipLaunchKernelGGL(sdp_family_diff_stats<float>, dim3(bx, n), dim3(256), 0, op->stream,
                               (const float *)cur, (const float *)old, op->Sm, members, (int64_t)-1, (int64_t)-1, acc);
        else
            hipLaunchKernelGGL(sdp_family_diff_stats<double>, dim3(bx, n), dim3(256), 0, op->stream,
                               (const double *)cur, (const double *)old, op->Sm, members, (int64_t)-1, (int64_t)-1, acc);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(keys.data(), op->mstats.p, (size_t)n * 3 * 8, hipMemcpyDeviceToHost, op->stream));
        HIP_TRY(hipStreamSynchronize(op->stream));
        keep.clear(); leave.clear();
        for (int i = 0; i < n; ++i) {
            const int32_t p = running[(size_t)i];
            double d = NAN;
            if (!keys[(size_t)i * 3 + 2]) {
                const double dmin = sdp_key_value(~keys[(size_t)i * 3]), dmax = sdp_key_value(keys[(size_t)i * 3 + 1]);
                d = dmax > -dmin ? dmax : -dmin;
            }
            delta[p] = d;
            if (d <= tol || k + 1 == n_max) leave.push_back(p);          // NaN never converges
            else keep.push_back(p);
        }
        if (leave.empty()) continue;
        if (!keep.empty()) {
            // a member that stops here is computed no more: its iterate goes into the other buffer as well, so it is
            // in the buffer sdp_transop_get reads however many pushes the others still run
            for (int32_t p : leave) {
                flags[(size_t)p] = 0;
                HIP_TRY(hipMemcpyAsync((char *)op->mu[1 - op->cur].p + (size_t)p * slice, (const char *)op->mu[op->cur].p + (size_t)p * slice,
                                       slice, hipMemcpyDeviceToDevice, op->stream));
            }
            HIP_TRY(hipMemcpyAsync(op->flags.p, flags.data(), P * 4, hipMemcpyHostToDevice, op->stream));
            HIP_TRY(hipMemcpyAsync(op->running.p, keep.data(), keep.size() * 4, hipMemcpyHostToDevice, op->stream));
            HIP_TRY(hipStreamSynchronize(op->stream));     // (the lists change before the copies would have run)
            op->all_running = false;
        }
        running.swap(keep);
    }
    HIP_TRY(hipEventRecord(op->ev1, op->stream));
    HIP_TRY(hipStreamSynchronize(op->stream));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, op->ev0, op->ev1));
    op->last_kernel_ms = ms;
    return SDP_OK;
}

// ---------------------------------------------------------------------------
// Closed loops of a family over a horizon (csrc/sdp_family_horizon_kernel.h): sdp_problem_simulate_h and
// sdp_problem_montecarlo_h of every member in one launch per cut of the steps.  The unit is loaded beside the sweep
// unit; the arrays of a run live for the call.  The policy [P][pol_steps][nu][S] is time-indexed (pol_steps == T: it
// goes up a chunk of whole steps of all members at a time, at most chunk_bytes) or stationary (pol_steps == 1: one
// slice per member, uploaded once and read with a step stride of 0); the table of constants [P][rows][n_prm] has
// rows == T or, for a model that is symbolic in time, rows == 1 and a step stride of 0.
// ---------------------------------------------------------------------------
extern "C" int sdp_family_load_horizon_unit(sdp_family *f, const char *module_path)
{
    if (!f || !module_path) return fail(SDP_EINVAL, "NULL argument");
    if (f->hzmod) { (void)hipModuleUnload(f->hzmod); f->hzmod = nullptr; f->f_hz_simulate = nullptr; f->f_hz_montecarlo = nullptr; }
    const size_t rs = real_size(f->dtype);
    hipError_t e = hipModuleLoad(&f->hzmod, module_path);
    if (e != hipSuccess) { f->hzmod = nullptr; return fail(SDP_EMODULE, "hipModuleLoad(%s): %s", module_path, hipGetErrorString(e)); }
    int32_t m[SDP_META_WORDS] = {0};
    hipDeviceptr_t mptr = nullptr;
    size_t mbytes = 0;
    const char *why = nullptr;
    if (hipModuleGetGlobal(&mptr, &mbytes, f->hzmod, "sdp_meta") != hipSuccess || mbytes != sizeof(m)) {
        (void)hipGetLastError();
        why = "it does not declare `sdp_meta`";
    } else {
        HIP_TRY(hipMemcpyDtoH(m, mptr, sizeof(m)));
        if (m[SDP_META_MAGIC_AT] != SDP_META_MAGIC) why = "bad magic";
        else if (!(m[SDP_META_FLAGS] & SDP_META_F_FAMILY_HORIZON)) why = "not a family horizon unit";
        else if (m[SDP_META_COL_ROWS] != 64) why = "its closed loop is built for another workgroup size";
        else if (m[SDP_META_REAL_BYTES] != (int)rs) why = "built for other reals";
        else if (m[SDP_META_D] != f->d) why = "built for another number of state variables";
        else if (m[SDP_META_NU] != f->nu) why = "built for another number of controls";
        else if ((m[SDP_META_HAS_W] != 0) != (f->W > 0)) why = "built for another kind of perturbation";
        else if (f->W > 0 && m[SDP_META_THREADS] != 256) why = "its Monte Carlo loop is built for another workgroup size";
    }
    hipDeviceptr_t pptr = nullptr;
    size_t pbytes = 0;
    if (!why) {
        if (hipModuleGetGlobal(&pptr, &pbytes, f->hzmod, "sdp_model_prm") != hipSuccess) { (void)hipGetLastError(); pbytes = 0; }
        if (pbytes != (size_t)f->n_params * rs) why = "another number of lifted constants";
    }
    if (!why && hipModuleGetFunction(&f->f_hz_simulate, f->hzmod, "sdp_family_simulate") != hipSuccess) why = "no sdp_family_simulate kernel";
    if (!why && f->W > 0 && hipModuleGetFunction(&f->f_hz_montecarlo, f->hzmod, "sdp_family_montecarlo_h") != hipSuccess)
        why = "no sdp_family_montecarlo_h kernel";
    if (why) {
        (void)hipGetLastError();
        (void)hipModuleUnload(f->hzmod);
        f->hzmod = nullptr; f->f_hz_simulate = nullptr; f->f_hz_montecarlo = nullptr;
        return fail(SDP_EMODULE, "code object %s was not built for this family's closed loops over a horizon: %s", module_path, why);
    }
    return SDP_OK;
}

// what both calls check of the policy and the table, and the steps of policy one upload holds (of all members)
static int family_horizon_checks(sdp_family *f, const char *what, int64_t pol_steps, int32_t pol_timed, const void *host_prm,
                                 int32_t n_prm, int64_t chunk_bytes, int64_t T, int64_t *per_chunk)
{
    if (T < 1) return fail(SDP_EINVAL, "%s: %lld steps: at least 1", what, (long long)T);
    if (pol_steps != (pol_timed ? T : 1))
        return fail(SDP_EINVAL, "%s: %lld policy steps for %lld steps (%s)", what, (long long)pol_steps, (long long)T,
                    pol_timed ? "a time-indexed policy has one per step" : "a stationary policy has one");
    if (chunk_bytes < 1) return fail(SDP_EINVAL, "%s: chunk_bytes = %lld: at least 1", what, (long long)chunk_bytes);
    if (n_prm != f->n_params || (n_prm > 0 && !host_prm))
        return fail(SDP_EINVAL, "%s: the family has %d lifted constant(s) per member and step, the table has %d", what,
                    (int)f->n_params, (int)n_prm);
    const size_t step_bytes = (size_t)f->P * f->nu * f->S * real_size(f->dtype);
    int64_t n = pol_timed ? (int64_t)((size_t)chunk_bytes / step_bytes) : T;
    if (n < 1) n = 1;
    if (n > T) n = T;
    *per_chunk = n;
    return SDP_OK;
}

// the slices [first, first + n) of every member's time-indexed array (`slice` bytes a step) into the device's [P][per_chunk][slice]
static int family_horizon_upload_slices(sdp_family *f, DevBuf &dev, const void *host, size_t slice, int64_t steps,
                                        int64_t per_chunk, int64_t first, int64_t n)
{
    for (size_t p = 0; p < (size_t)f->P; ++p)
        HIP_TRY(hipMemcpy((char *)dev.p + p * (size_t)per_chunk * slice,
                          (const char *)host + (p * (size_t)steps + (size_t)first) * slice, (size_t)n * slice,
                          hipMemcpyHostToDevice));
    return SDP_OK;
}

// the slices [first, first + n) of every member's policy into the device's [P][per_chunk][nu][S]
static int family_horizon_upload_policy(sdp_family *f, DevBuf &dpol, const void *host_pol, int64_t pol_steps,
                                        int64_t per_chunk, int64_t first, int64_t n)
{
    return family_horizon_upload_slices(f, dpol, host_pol, (size_t)f->nu * f->S * real_size(f->dtype), pol_steps, per_chunk, first, n);
}

// workgroups per XCD of a launch whose members have `tiles` tiles each (sdp_family_horizon_kernel.h), at most `cap`
static int64_t family_horizon_per_xcd(const sdp_family *f, int64_t tiles, int64_t cap)
{
    const int parts = f->P >= 8 ? 1 : 8 / f->P;
    int64_t per_xcd = f->P >= 8 ? (int64_t)((f->P + 7) / 8) * tiles : (tiles + parts - 1) / parts;
    if (per_xcd > cap) per_xcd = cap;
    if (per_xcd < 1) per_xcd = 1;
    return per_xcd;
}

extern "C" int sdp_family_simulate(sdp_family *f, const void *host_pol, int64_t pol_steps, int32_t pol_timed,
                                   const void *host_prm, int32_t n_prm, int32_t prm_timed, int64_t chunk_bytes,
                                   int64_t B, int64_t T, const void *host_x0, const void *host_w, double t0,
                                   void *host_x, void *host_u, void *host_g)
{
    if (!f || !host_pol || !host_x0 || !host_x || !host_u || !host_g) return fail(SDP_EINVAL, "NULL argument");
    if (B < 0) return fail(SDP_EINVAL, "negative size");
    if (!f->f_hz_simulate) return fail(SDP_EINVAL, "no horizon unit loaded (sdp_family_load_horizon_unit)");
    int rc;
    int64_t per_chunk = 0;
    if ((rc = family_horizon_checks(f, "sdp_family_simulate", pol_steps, pol_timed, host_prm, n_prm, chunk_bytes, T, &per_chunk))) return rc;
    if (f->W > 0 && !host_w) return fail(SDP_EINVAL, "a stochastic family needs the perturbation sequences");
    if (B == 0) return SDP_OK;
    const size_t rs = real_size(f->dtype);
    const size_t P = (size_t)f->P;
    const size_t slice = (size_t)f->nu * f->S * rs;
    const int64_t prm_rows = prm_timed ? T : 1;
    DevBuf dpol, dprm, dw, dx, du, dg;
    if ((rc = dpol.alloc(P * (size_t)(pol_timed ? per_chunk : 1) * slice))) return rc;
    if (n_prm > 0 && (rc = upload(dprm, host_prm, P * (size_t)prm_rows * n_prm * rs))) return rc;
    if (f->W > 0 && (rc = upload(dw, host_w, P * (size_t)T * B * rs))) return rc;                // [P][T][B]
    if ((rc = dx.alloc(P * (size_t)(T + 1) * f->d * B * rs))) return rc;
    if ((rc = du.alloc(P * (size_t)T * f->nu * B * rs))) return rc;
    if ((rc = dg.alloc(P * (size_t)T * B * rs))) return rc;
    // row 0 of every member's x
    for (size_t p = 0; p < P; ++p)
        HIP_TRY(hipMemcpy((char *)dx.p + p * (size_t)(T + 1) * f->d * B * rs, (const char *)host_x0 + p * (size_t)f->d * B * rs,
                          (size_t)f->d * B * rs, hipMemcpyHostToDevice));
    SdpFamilySimHArgs a;
    memset(&a, 0, sizeof(a));
    a.pol = dpol.p; a.prm = n_prm > 0 ? dprm.p : nullptr; a.axes = f->axes.p; a.w = f->W > 0 ? dw.p : nullptr;
    a.x = dx.p; a.u = du.p; a.g = dg.p;
    a.B = B; a.S = f->S; a.T = T; a.t0 = t0; a.n_axes = f->n_axes; a.P = f->P;
    a.pol_step_stride = pol_timed ? (int64_t)f->nu * f->S : 0;
    a.pol_member_stride = (int64_t)(pol_timed ? per_chunk : 1) * f->nu * f->S;
    a.prm_step_stride = prm_timed ? (int64_t)n_prm : 0;
    a.prm_member_stride = prm_rows * (int64_t)n_prm;
    for (int k = 0; k < SDP_MAXD; ++k) { a.orders[k] = f->orders[k]; a.axis_off[k] = f->axis_off[k]; }
    size_t size = sizeof(a);
    void *extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a, HIP_LAUNCH_PARAM_BUFFER_SIZE, &size, HIP_LAUNCH_PARAM_END};
    // a tile of 64 trajectories of one member is a workgroup.  A multiple of 8 workgroups (one share per XCD): per XCD as
    // many as it has tiles to walk, at most the solo call's cus * 32 split over the 8 XCDs, the rest in the stride loop
    const int64_t per_xcd = family_horizon_per_xcd(f, (B + 63) / 64, (int64_t)f->cus * 32 / 8);
    HIP_TRY(hipStreamSynchronize(f->stream));
    double kernel_ms = 0;
    if (!pol_timed && (rc = family_horizon_upload_policy(f, dpol, host_pol, 1, 1, 0, 1))) return rc;
    for (int64_t k = 0; k < T; k += per_chunk) {
        const int64_t n = (T - k < per_chunk) ? T - k : per_chunk;
        // (the kernel of the previous chunk has finished: the stream is synchronised at the end of every round)
        if (pol_timed && (rc = family_horizon_upload_policy(f, dpol, host_pol, pol_steps, per_chunk, k, n))) return rc;
        a.chunk_first = k; a.step_begin = k; a.step_end = k + n;
        HIP_TRY(hipEventRecord(f->ev0, f->stream));
        HIP_TRY(hipModuleLaunchKernel(f->f_hz_simulate, (unsigned)(per_xcd * 8), 1, 1, 64, 1, 1, 0, f->stream, nullptr, extra));
        HIP_TRY(hipEventRecord(f->ev1, f->stream));
        HIP_TRY(hipStreamSynchronize(f->stream));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, f->ev0, f->ev1));
        kernel_ms += ms;
    }
    f->last_kernel_ms = kernel_ms;
    HIP_TRY(hipMemcpy(host_x, dx.p, P * (size_t)(T + 1) * f->d * B * rs, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(host_u, du.p, P * (size_t)T * f->nu * B * rs, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(host_g, dg.p, P * (size_t)T * B * rs, hipMemcpyDeviceToHost));
    return SDP_OK;
}

extern "C" int sdp_family_montecarlo_h(sdp_family *f, const void *host_pol, int64_t pol_steps, int32_t pol_timed,
                                       const void *host_prm, int32_t n_prm, int32_t prm_timed, int64_t chunk_bytes,
                                       int64_t B, int64_t T, int64_t n_burn, const uint64_t *host_seeds,
                                       uint64_t traj_offset, const void *host_x0, const double *host_cum, int32_t n_law,
                                       const void *host_law_grid, double t0, int64_t steps_per_launch,
                                       void *host_cost_sum, int64_t *host_n_outside, void *host_x_final,
                                       uint64_t *host_occupancy)
{
    if (!f || !host_pol || !host_seeds || !host_x0 || !host_cum || !host_law_grid || !host_cost_sum || !host_n_outside || !host_x_final)
        return fail(SDP_EINVAL, "NULL argument");
    if (B < 0) return fail(SDP_EINVAL, "negative size");
    if (n_burn < 0 || n_burn > T) return fail(SDP_EINVAL, "n_burn = %lld outside [0, %lld]", (long long)n_burn, (long long)T);
    if (steps_per_launch < 1) return fail(SDP_EINVAL, "steps_per_launch = %lld: at least 1", (long long)steps_per_launch);
    if (f->W <= 0) return fail(SDP_EINVAL, "a deterministic system has nothing to draw: use sdp_family_simulate");
    if (n_law < 1 || n_law > 4096) return fail(SDP_EINVAL, "a law of %d points: 1 to 4096", (int)n_law);
    if (!f->f_hz_montecarlo) return fail(SDP_EINVAL, "no horizon unit loaded (sdp_family_load_horizon_unit)");
    int rc;
    int64_t per_chunk = 0;
    if ((rc = family_horizon_checks(f, "sdp_family_montecarlo_h", pol_steps, pol_timed, host_prm, n_prm, chunk_bytes, T, &per_chunk))) return rc;
    if (B == 0) return SDP_OK;
    if (steps_per_launch > ((int64_t)1 << 30)) steps_per_launch = (int64_t)1 << 30;       // (the kernel counts a launch's steps in 32 bits)
    const size_t rs = real_size(f->dtype);
    const size_t P = (size_t)f->P;
    const size_t slice = (size_t)f->nu * f->S * rs;
    const int64_t prm_rows = prm_timed ? T : 1;
    // (the draw table of one member in LDS: the cumulative sums, then the values)
    const size_t lds_bytes = (size_t)(n_law - 1) * 8 + (size_t)n_law * rs;
    if (lds_bytes > 65536)
        return fail(SDP_EINVAL, "a law of %d points needs %zu bytes of LDS: at most 65536", (int)n_law, lds_bytes);
    DevBuf dpol, dprm, dx, dacc, dout, dcum, dlaw, dseed, docc;
    if ((rc = dpol.alloc(P * (size_t)(pol_timed ? per_chunk : 1) * slice))) return rc;
    if (n_prm > 0 && (rc = upload(dprm, host_prm, P * (size_t)prm_rows * n_prm * rs))) return rc;
    if ((rc = upload(dx, host_x0, P * (size_t)f->d * B * rs))) return rc;                 // [P][d][B]
    if ((rc = upload(dcum, host_cum, P * (size_t)n_law * 8))) return rc;
    if ((rc = upload(dlaw, host_law_grid, P * (size_t)n_law * rs))) return rc;
    if ((rc = upload(dseed, host_seeds, P * 8))) return rc;
    if ((rc = dacc.alloc(P * (size_t)B * rs))) return rc;
    if ((rc = dout.alloc(P * (size_t)B * 8))) return rc;
    HIP_TRY(hipMemsetAsync(dacc.p, 0, P * (size_t)B * rs, f->stream));
    HIP_TRY(hipMemsetAsync(dout.p, 0, P * (size_t)B * 8, f->stream));
    if (host_occupancy) {
        if ((rc = docc.alloc(P * (size_t)f->S * 8))) return rc;
        HIP_TRY(hipMemsetAsync(docc.p, 0, P * (size_t)f->S * 8, f->stream));
    }
    SdpFamilyMcHArgs a;
    memset(&a, 0, sizeof(a));
    a.pol = dpol.p; a.prm = n_prm > 0 ? dprm.p : nullptr; a.axes = f->axes.p; a.cum = (const double *)dcum.p; a.law_grid = dlaw.p;
    a.seed = (const uint64_t *)dseed.p; a.x = dx.p; a.acc = dacc.p; a.n_outside = (long long *)dout.p;
    a.occupancy = host_occupancy ? (unsigned long long *)docc.p : nullptr;
    a.B = B; a.S = f->S; a.traj_offset = traj_offset; a.n_burn = n_burn; a.t0 = t0;
    a.n_law = n_law; a.n_axes = f->n_axes; a.P = f->P;
    a.pol_step_stride = pol_timed ? (int64_t)f->nu * f->S : 0;
    a.pol_member_stride = (int64_t)(pol_timed ? per_chunk : 1) * f->nu * f->S;
    a.prm_step_stride = prm_timed ? (int64_t)n_prm : 0;
    a.prm_member_stride = prm_rows * (int64_t)n_prm;
    for (int k = 0; k < SDP_MAXD; ++k) { a.orders[k] = f->orders[k]; a.axis_off[k] = f->axis_off[k]; }
    size_t size = sizeof(a);
    void *extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a, HIP_LAUNCH_PARAM_BUFFER_SIZE, &size, HIP_LAUNCH_PARAM_END};
    // (the launch shape of sdp_family_montecarlo)
    const int threads = 256;
    const unsigned lds = (unsigned)lds_bytes;
    int per_cu = 0;
    if (hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, f->f_hz_montecarlo, threads, lds) != hipSuccess) {
        (void)hipGetLastError();
        per_cu = 0;
    }
    if (per_cu < 1) per_cu = 1;
    if (per_cu > 8) per_cu = 8;
    const int64_t per_xcd = family_horizon_per_xcd(f, (B + threads - 1) / threads, (int64_t)f->cus * per_cu / 8);
    HIP_TRY(hipStreamSynchronize(f->stream));
    double kernel_ms = 0;
    if (!pol_timed && (rc = family_horizon_upload_policy(f, dpol, host_pol, 1, 1, 0, 1))) return rc;
    for (int64_t c = 0; c < T; c += per_chunk) {
        const int64_t c_end = (T - c < per_chunk) ? T : c + per_chunk;
        if (pol_timed && (rc = family_horizon_upload_policy(f, dpol, host_pol, pol_steps, per_chunk, c, c_end - c))) return rc;
        a.chunk_first = c;
        HIP_TRY(hipEventRecord(f->ev0, f->stream));
        for (int64_t k = c; k < c_end; k += steps_per_launch) {
            a.step_begin = k;
            a.step_end = (c_end - k < steps_per_launch) ? c_end : k + steps_per_launch;
            HIP_TRY(hipModuleLaunchKernel(f->f_hz_montecarlo, (unsigned)(per_xcd * 8), 1, 1, threads, 1, 1, lds, f->stream, nullptr, extra));
        }
        HIP_TRY(hipEventRecord(f->ev1, f->stream));
        HIP_TRY(hipStreamSynchronize(f->stream));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, f->ev0, f->ev1));
        kernel_ms += ms;
    }
    f->last_kernel_ms = kernel_ms;
    HIP_TRY(hipMemcpy(host_cost_sum, dacc.p, P * (size_t)B * rs, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(host_n_outside, dout.p, P * (size_t)B * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(host_x_final, dx.p, P * (size_t)f->d * B * rs, hipMemcpyDeviceToHost));
    if (host_occupancy) HIP_TRY(hipMemcpy(host_occupancy, docc.p, P * (size_t)f->S * 8, hipMemcpyDeviceToHost));
    return SDP_OK;
}

// ---------------------------------------------------------------------------
// One-step lookahead at arbitrary states, and its Monte Carlo score, for a family (csrc/sdp_family_lookahead_kernel.h):
// sdp_problem_lookahead and sdp_problem_montecarlo_lookahead of every member in one launch (per cut of the steps).  The
// unit is loaded beside the sweep unit; J_next is the handle's value array (sdp_family_set_value).
// ---------------------------------------------------------------------------
extern "C" int sdp_family_load_lookahead_unit(sdp_family *f, const char *module_path)
{
    if (!f || !module_path) return fail(SDP_EINVAL, "NULL argument");
    if (f->lkmod) { (void)hipModuleUnload(f->lkmod); f->lkmod = nullptr; f->f_lookahead = nullptr; f->f_mc_lookahead = nullptr; }
    f->has_look_box = false;
    const size_t rs = real_size(f->dtype);
    hipError_t e = hipModuleLoad(&f->lkmod, module_path);
    if (e != hipSuccess) { f->lkmod = nullptr; return fail(SDP_EMODULE, "hipModuleLoad(%s): %s", module_path, hipGetErrorString(e)); }
    int32_t m[SDP_META_WORDS] = {0};
    hipDeviceptr_t mptr = nullptr;
    size_t mbytes = 0;
    const char *why = nullptr;
    if (hipModuleGetGlobal(&mptr, &mbytes, f->lkmod, "sdp_meta") != hipSuccess || mbytes != sizeof(m)) {
        (void)hipGetLastError();
        why = "it does not declare `sdp_meta`";
    } else {
        HIP_TRY(hipMemcpyDtoH(m, mptr, sizeof(m)));
        if (m[SDP_META_MAGIC_AT] != SDP_META_MAGIC) why = "bad magic";
        else if (!(m[SDP_META_FLAGS] & SDP_META_F_FAMILY_LOOKAHEAD)) why = "not a family lookahead unit";
        else if (m[SDP_META_THREADS] != 256) why = "built for another workgroup size";
        else if (m[SDP_META_REAL_BYTES] != (int)rs) why = "built for other reals";
        else if (m[SDP_META_D] != f->d) why = "built for another number of state variables";
        else if (m[SDP_META_NU] != f->nu) why = "built for another number of controls";
        else if ((m[SDP_META_HAS_W] != 0) != (f->W > 0)) why = "built for another kind of perturbation";
        else if (m[SDP_META_COL_ROWS] < 1 || m[SDP_META_COL_ROWS] > 64 || (m[SDP_META_COL_ROWS] & (m[SDP_META_COL_ROWS] - 1))) why = "its lanes per state are no power of two in 1..64";
        else if (m[SDP_META_UTAB] < 0) why = "a negative number of box constants";
    }
    hipDeviceptr_t pptr = nullptr;
    size_t pbytes = 0;
    if (!why) {
        if (hipModuleGetGlobal(&pptr, &pbytes, f->lkmod, "sdp_model_prm") != hipSuccess) { (void)hipGetLastError(); pbytes = 0; }
        if (pbytes != (size_t)f->n_params * rs) why = "another number of lifted constants";
    }
    if (!why && hipModuleGetFunction(&f->f_lookahead, f->lkmod, "sdp_family_lookahead") != hipSuccess) why = "no sdp_family_lookahead kernel";
    if (!why && f->W > 0 && hipModuleGetFunction(&f->f_mc_lookahead, f->lkmod, "sdp_family_montecarlo_lookahead") != hipSuccess)
        why = "no sdp_family_montecarlo_lookahead kernel";
    if (why) {
        (void)hipGetLastError();
        (void)hipModuleUnload(f->lkmod);
        f->lkmod = nullptr; f->f_lookahead = nullptr; f->f_mc_lookahead = nullptr;
        return fail(SDP_EMODULE, "code object %s was not built for this family's lookahead: %s", module_path, why);
    }
    // (a unit over a horizon that was built for other lanes or another box function is of an earlier plan: it goes)
    if (f->lhmod && (f->look_lanes != m[SDP_META_COL_ROWS] || f->n_box != m[SDP_META_UTAB])) {
        (void)hipModuleUnload(f->lhmod);
        f->lhmod = nullptr; f->f_lh_simulate = nullptr; f->f_lh_montecarlo = nullptr;
    }
    f->look_lanes = m[SDP_META_COL_ROWS];
    f->n_box = m[SDP_META_UTAB];
    return SDP_OK;
}

extern "C" int sdp_family_set_lookahead_box(sdp_family *f, const double *box_params, int32_t n_box, const double *steps)
{
    if (!f || !steps || n_box < 0 || (n_box > 0 && !box_params)) return fail(SDP_EINVAL, "sdp_family_set_lookahead_box: bad arguments");
    if (!f->f_lookahead && !f->f_lh_simulate)
        return fail(SDP_EINVAL, "no lookahead unit loaded (sdp_family_load_lookahead_unit, sdp_family_load_lookahead_horizon_unit)");
    if (n_box != f->n_box)
        return fail(SDP_EINVAL, "sdp_family_set_lookahead_box: the unit's box function has %d constant(s) per member, %d given", f->n_box, (int)n_box);
    const size_t P = (size_t)f->P;
    for (size_t i = 0; i < P * (size_t)f->nu; ++i)
        if (!(steps[i] == steps[i])) return fail(SDP_EINVAL, "sdp_family_set_lookahead_box: control step hint %zu of member %zu is NaN", i % f->nu, i / f->nu);
    f->has_look_box = false;
    int rc;
    HIP_TRY(hipStreamSynchronize(f->stream));        // (launches that still read the old rows)
    // (a row of at least one double, so that a box without constants still has a table to point to)
    if ((rc = f->bprm.alloc(P * (size_t)(n_box > 0 ? n_box : 1) * 8))) return rc;
    if (n_box > 0) HIP_TRY(hipMemcpy(f->bprm.p, box_params, P * (size_t)n_box * 8, hipMemcpyHostToDevice));
    if ((rc = upload(f->look_steps, steps, P * (size_t)f->nu * 8))) return rc;
    f->has_look_box = true;
    return SDP_OK;
}

// what both lookahead launches start from: the unit, the members' box rows, J_next of every member in buf[cur]
static int family_lookahead_checks(const sdp_family *f, const char *what)
{
    if (!f->f_lookahead) return fail(SDP_EINVAL, "%s: no lookahead unit loaded (sdp_family_load_lookahead_unit)", what);
    if (!f->has_look_box) return fail(SDP_EINVAL, "%s: the members' box constants and control steps are not set (sdp_family_set_lookahead_box)", what);
    for (int p = 0; p < f->P; ++p)
        if (f->where[(size_t)p] != f->cur)
            return fail(SDP_EINVAL, "%s: the cost-to-go is the value array of sdp_family_set_value: set it before the call", what);
    return SDP_OK;
}

static void family_lookahead_block(const sdp_family *f, SdpFamilyArgs &a, double t_k)
{
    memset(&a, 0, sizeof(a));
    a.V = f->buf[f->cur].p;
    a.axes = f->axes.p; a.wgrid = f->wgrid.p; a.proba = f->proba.p; a.prm = f->prm.p;
    a.S = f->S; a.t_k = t_k;
    for (int k = 0; k < SDP_MAXD; ++k) { a.orders[k] = f->orders[k]; a.axis_off[k] = f->axis_off[k]; }
    a.n_axes = f->n_axes; a.W = f->W; a.box_per_node = 0; a.n_active = f->P;
}

// a tile of (64 / lanes) * 4 states of one member is a workgroup of 256.  A multiple of 8 workgroups (one share per XCD,
// sdp_family_lookahead_kernel.h): per XCD as many as it has tiles to walk, in all at most the workgroups that are resident
// at once (8 per CU at most), the rest in the stride loop
static unsigned family_lookahead_grid(const sdp_family *f, hipFunction_t fn, int64_t B, unsigned lds)
{
    int per_cu = 0;
    if (hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 256, lds) != hipSuccess) {
        (void)hipGetLastError();
        per_cu = 0;
    }
    if (per_cu < 1) per_cu = 1;
    if (per_cu > 8) per_cu = 8;
    const int64_t tile = (int64_t)(64 / f->look_lanes) * 4;
    const int64_t tiles = (B + tile - 1) / tile;
    const int parts = f->P >= 8 ? 1 : 8 / f->P;
    int64_t per_xcd = f->P >= 8 ? (int64_t)((f->P + 7) / 8) * tiles : (tiles + parts - 1) / parts;
    const int64_t cap = (int64_t)f->cus * per_cu / 8;
    if (per_xcd > cap) per_xcd = cap;
    if (per_xcd < 1) per_xcd = 1;
    return (unsigned)(per_xcd * 8);
}

extern "C" int sdp_family_lookahead(sdp_family *f, int64_t B, const void *host_x, double t_k, void *host_J, void *host_u,
                                    int32_t *host_idx)
{
    if (!f || !host_x || !host_J || !host_u || !host_idx) return fail(SDP_EINVAL, "NULL argument");
    if (B < 0) return fail(SDP_EINVAL, "negative size");
    int rc;
    if ((rc = family_lookahead_checks(f, "sdp_family_lookahead"))) return rc;
    if (B == 0) return SDP_OK;
    const size_t rs = real_size(f->dtype);
    const size_t P = (size_t)f->P;
    DevBuf dx, dJ, du, didx;
    if ((rc = upload(dx, host_x, P * (size_t)f->d * B * rs))) return rc;                  // [P][d][B]
    if ((rc = dJ.alloc(P * (size_t)B * rs))) return rc;
    if ((rc = du.alloc(P * (size_t)f->nu * B * rs))) return rc;
    if ((rc = didx.alloc(P * (size_t)B * 4))) return rc;
    SdpFamilyLookArgs a;
    memset(&a, 0, sizeof(a));
    family_lookahead_block(f, a.f, t_k);
    a.bprm = (const double *)f->bprm.p; a.steps = (const double *)f->look_steps.p;
    a.x = dx.p; a.J = dJ.p; a.idx = (int32_t *)didx.p; a.u = du.p; a.B = B;
    size_t size = sizeof(a);
    void *extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a, HIP_LAUNCH_PARAM_BUFFER_SIZE, &size, HIP_LAUNCH_PARAM_END};
    const unsigned blocks = family_lookahead_grid(f, f->f_lookahead, B, 0);
    HIP_TRY(hipStreamSynchronize(f->stream));        // lifted constants and values set on the family's stream
    HIP_TRY(hipEventRecord(f->ev0, f->stream));
    HIP_TRY(hipModuleLaunchKernel(f->f_lookahead, blocks, 1, 1, 256, 1, 1, 0, f->stream, nullptr, extra));
    HIP_TRY(hipEventRecord(f->ev1, f->stream));
    HIP_TRY(hipStreamSynchronize(f->stream));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, f->ev0, f->ev1));
    f->last_kernel_ms = ms;
    HIP_TRY(hipMemcpy(host_J, dJ.p, P * (size_t)B * rs, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(host_u, du.p, P * (size_t)f->nu * B * rs, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(host_idx, didx.p, P * (size_t)B * 4, hipMemcpyDeviceToHost));
    return SDP_OK;
}

extern "C" int sdp_family_montecarlo_lookahead(sdp_family *f, int64_t B, int64_t T, int64_t n_burn, const uint64_t *host_seeds,
                                               uint64_t traj_offset, const void *host_x0, const double *host_cum, int32_t n_law,
                                               const void *host_law_grid, double t0, int64_t steps_per_launch,
                                               void *host_cost_sum, int64_t *host_n_outside, void *host_x_final,
                                               uint64_t *host_occupancy)
{
    if (!f || !host_seeds || !host_x0 || !host_cum || !host_law_grid || !host_cost_sum || !host_n_outside || !host_x_final)
        return fail(SDP_EINVAL, "NULL argument");
    if (B < 0 || T < 0) return fail(SDP_EINVAL, "negative size");
    if (n_burn < 0 || n_burn > T) return fail(SDP_EINVAL, "n_burn = %lld outside [0, %lld]", (long long)n_burn, (long long)T);
    if (steps_per_launch < 1) return fail(SDP_EINVAL, "steps_per_launch = %lld: at least 1", (long long)steps_per_launch);
    if (f->W <= 0) return fail(SDP_EINVAL, "a deterministic system has nothing to draw");
    if (n_law < 1 || n_law > 4096) return fail(SDP_EINVAL, "a law of %d points: 1 to 4096", (int)n_law);
    int rc;
    if ((rc = family_lookahead_checks(f, "sdp_family_montecarlo_lookahead"))) return rc;
    if (!f->f_mc_lookahead) return fail(SDP_EINVAL, "the lookahead unit has no sdp_family_montecarlo_lookahead kernel");
    if (B == 0) return SDP_OK;
    if (steps_per_launch > ((int64_t)1 << 30)) steps_per_launch = (int64_t)1 << 30;       // (the kernel counts a launch's steps in 32 bits)
    const size_t rs = real_size(f->dtype);
    const size_t P = (size_t)f->P;
    // (the draw table of one member in LDS: the cumulative sums, then the values)
    const size_t lds_bytes = (size_t)(n_law - 1) * 8 + (size_t)n_law * rs;
    if (lds_bytes > 65536)
        return fail(SDP_EINVAL, "a law of %d points needs %zu bytes of LDS: at most 65536", (int)n_law, lds_bytes);
    DevBuf dx, dacc, dout, dcum, dlaw, dseed, docc;
    if ((rc = upload(dx, host_x0, P * (size_t)f->d * B * rs))) return rc;                 // [P][d][B]
    if ((rc = upload(dcum, host_cum, P * (size_t)n_law * 8))) return rc;
    if ((rc = upload(dlaw, host_law_grid, P * (size_t)n_law * rs))) return rc;
    if ((rc = upload(dseed, host_seeds, P * 8))) return rc;
    if ((rc = dacc.alloc(P * (size_t)B * rs))) return rc;
    if ((rc = dout.alloc(P * (size_t)B * 8))) return rc;
    HIP_TRY(hipMemsetAsync(dacc.p, 0, P * (size_t)B * rs, f->stream));
    HIP_TRY(hipMemsetAsync(dout.p, 0, P * (size_t)B * 8, f->stream));
    if (host_occupancy) {
        if ((rc = docc.alloc(P * (size_t)f->S * 8))) return rc;
        HIP_TRY(hipMemsetAsync(docc.p, 0, P * (size_t)f->S * 8, f->stream));
    }
    SdpFamilyLookMcArgs a;
    memset(&a, 0, sizeof(a));
    family_lookahead_block(f, a.f, t0);
    a.bprm = (const double *)f->bprm.p; a.steps = (const double *)f->look_steps.p;
    a.cum = (const double *)dcum.p; a.law_grid = dlaw.p; a.seed = (const uint64_t *)dseed.p;
    a.x = dx.p; a.acc = dacc.p; a.n_outside = (long long *)dout.p;
    a.occupancy = host_occupancy ? (unsigned long long *)docc.p : nullptr;
    a.B = B; a.traj_offset = traj_offset; a.n_burn = n_burn; a.t0 = t0; a.n_law = n_law;
    size_t size = sizeof(a);
    void *extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a, HIP_LAUNCH_PARAM_BUFFER_SIZE, &size, HIP_LAUNCH_PARAM_END};
    const unsigned lds = (unsigned)lds_bytes;
    const unsigned blocks = family_lookahead_grid(f, f->f_mc_lookahead, B, lds);
    HIP_TRY(hipStreamSynchronize(f->stream));        // lifted constants and values set on the family's stream
    HIP_TRY(hipEventRecord(f->ev0, f->stream));
    for (int64_t k = 0; k < T; k += steps_per_launch) {
        a.step_begin = k;
        a.step_end = (T - k < steps_per_launch) ? T : k + steps_per_launch;
        HIP_TRY(hipModuleLaunchKernel(f->f_mc_lookahead, blocks, 1, 1, 256, 1, 1, lds, f->stream, nullptr, extra));
    }
    HIP_TRY(hipEventRecord(f->ev1, f->stream));
    HIP_TRY(hipStreamSynchronize(f->stream));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, f->ev0, f->ev1));
    f->last_kernel_ms = ms;
    HIP_TRY(hipMemcpy(host_cost_sum, dacc.p, P * (size_t)B * rs, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(host_n_outside, dout.p, P * (size_t)B * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(host_x_final, dx.p, P * (size_t)f->d * B * rs, hipMemcpyDeviceToHost));
    if (host_occupancy) HIP_TRY(hipMemcpy(host_occupancy, docc.p, P * (size_t)f->S * 8, hipMemcpyDeviceToHost));
    return SDP_OK;
}

// ---------------------------------------------------------------------------
// Closed loops of a family under lookahead controls over a horizon (csrc/sdp_family_lookahead_horizon_kernel.h):
// sdp_problem_simulate_lookahead and sdp_problem_montecarlo_lookahead of every member in one launch per cut of the
// steps.  The unit is loaded beside the sweep unit; the arrays of a run live for the call (the handle's value arrays and
// its rows of constants are not read).  The cost-to-go [P][V_steps][S] is time-indexed (V_steps == T: it goes up a chunk
// of whole steps of all members at a time, at most chunk_bytes, by the rule of sdp_family_simulate for its policy) or one
// per member (V_steps == 1: uploaded once and read with a step stride of 0); the table of constants [P][rows][n_prm] has
// rows == T or, for a model that is symbolic in time, rows == 1 and a step stride of 0.  The members' box constants and
// control steps are those of sdp_family_set_lookahead_box.
// ---------------------------------------------------------------------------
extern "C" int sdp_family_load_lookahead_horizon_unit(sdp_family *f, const char *module_path)
{
    if (!f || !module_path) return fail(SDP_EINVAL, "NULL argument");
    if (f->lhmod) { (void)hipModuleUnload(f->lhmod); f->lhmod = nullptr; f->f_lh_simulate = nullptr; f->f_lh_montecarlo = nullptr; }
    f->has_look_box = false;
    const size_t rs = real_size(f->dtype);
    hipError_t e = hipModuleLoad(&f->lhmod, module_path);
    if (e != hipSuccess) { f->lhmod = nullptr; return fail(SDP_EMODULE, "hipModuleLoad(%s): %s", module_path, hipGetErrorString(e)); }
    int32_t m[SDP_META_WORDS] = {0};
    hipDeviceptr_t mptr = nullptr;
    size_t mbytes = 0;
    const char *why = nullptr;
    if (hipModuleGetGlobal(&mptr, &mbytes, f->lhmod, "sdp_meta") != hipSuccess || mbytes != sizeof(m)) {
        (void)hipGetLastError();
        why = "it does not declare `sdp_meta`";
    } else {
        HIP_TRY(hipMemcpyDtoH(m, mptr, sizeof(m)));
        if (m[SDP_META_MAGIC_AT] != SDP_META_MAGIC) why = "bad magic";
        else if (!(m[SDP_META_FLAGS] & SDP_META_F_FAMILY_LOOKAHEAD_HORIZON)) why = "not a family lookahead unit over a horizon";
        else if (m[SDP_META_THREADS] != 256) why = "built for another workgroup size";
        else if (m[SDP_META_REAL_BYTES] != (int)rs) why = "built for other reals";
        else if (m[SDP_META_D] != f->d) why = "built for another number of state variables";
        else if (m[SDP_META_NU] != f->nu) why = "built for another number of controls";
        else if ((m[SDP_META_HAS_W] != 0) != (f->W > 0)) why = "built for another kind of perturbation";
        else if (m[SDP_META_COL_ROWS] < 1 || m[SDP_META_COL_ROWS] > 64 || (m[SDP_META_COL_ROWS] & (m[SDP_META_COL_ROWS] - 1))) why = "its lanes per state are no power of two in 1..64";
        else if (m[SDP_META_UTAB] < 0) why = "a negative number of box constants";
    }
    hipDeviceptr_t pptr = nullptr;
    size_t pbytes = 0;
    if (!why) {
        if (hipModuleGetGlobal(&pptr, &pbytes, f->lhmod, "sdp_model_prm") != hipSuccess) { (void)hipGetLastError(); pbytes = 0; }
        if (pbytes != (size_t)f->n_params * rs) why = "another number of lifted constants";
    }
    if (!why && hipModuleGetFunction(&f->f_lh_simulate, f->lhmod, "sdp_family_simulate_lookahead") != hipSuccess) why = "no sdp_family_simulate_lookahead kernel";
    if (!why && f->W > 0 && hipModuleGetFunction(&f->f_lh_montecarlo, f->lhmod, "sdp_family_montecarlo_lookahead_h") != hipSuccess)
        why = "no sdp_family_montecarlo_lookahead_h kernel";
    if (why) {
        (void)hipGetLastError();
        (void)hipModuleUnload(f->lhmod);
        f->lhmod = nullptr; f->f_lh_simulate = nullptr; f->f_lh_montecarlo = nullptr;
        return fail(SDP_EMODULE, "code object %s was not built for this family's lookahead over a horizon: %s", module_path, why);
    }
    // (a lookahead unit that was built for other lanes or another box function is of an earlier plan: it goes)
    if (f->lkmod && (f->look_lanes != m[SDP_META_COL_ROWS] || f->n_box != m[SDP_META_UTAB])) {
        (void)hipModuleUnload(f->lkmod);
        f->lkmod = nullptr; f->f_lookahead = nullptr; f->f_mc_lookahead = nullptr;
    }
    f->look_lanes = m[SDP_META_COL_ROWS];
    f->n_box = m[SDP_META_UTAB];
    return SDP_OK;
}

// what both calls check of the cost-to-go and the table, and the steps of cost-to-go one upload holds (of all members)
static int family_lookahead_horizon_checks(sdp_family *f, const char *what, const void *host_V, int64_t V_steps, int32_t V_timed,
                                           const void *host_prm, int32_t n_prm, int64_t chunk_bytes, int64_t B, int64_t T,
                                           int64_t *per_chunk)
{
    if (!host_V) return fail(SDP_EINVAL, "NULL argument");
    if (B < 0) return fail(SDP_EINVAL, "negative size");
    if (T < 1) return fail(SDP_EINVAL, "%s: %lld steps: at least 1", what, (long long)T);
    if (!f->f_lh_simulate) return fail(SDP_EINVAL, "%s: no lookahead unit over a horizon loaded (sdp_family_load_lookahead_horizon_unit)", what);
    if (!f->has_look_box) return fail(SDP_EINVAL, "%s: the members' box constants and control steps are not set (sdp_family_set_lookahead_box)", what);
    if (V_steps != (V_timed ? T : 1))
        return fail(SDP_EINVAL, "%s: %lld cost-to-go steps for %lld steps (%s)", what, (long long)V_steps, (long long)T,
                    V_timed ? "a time-indexed cost-to-go has one per step" : "otherwise there is one");
    if (chunk_bytes < 1) return fail(SDP_EINVAL, "%s: chunk_bytes = %lld: at least 1", what, (long long)chunk_bytes);
    if (n_prm != f->n_params || (n_prm > 0 && !host_prm))
        return fail(SDP_EINVAL, "%s: the family has %d lifted constant(s) per member and step, the table has %d", what,
                    (int)f->n_params, (int)n_prm);
    const size_t step_bytes = (size_t)f->P * f->S * real_size(f->dtype);
    int64_t n = V_timed ? (int64_t)((size_t)chunk_bytes / step_bytes) : T;
    if (n < 1) n = 1;
    if (n > T) n = T;
    *per_chunk = n;
    return SDP_OK;
}

// the block of the sweep for a launch over a horizon: the cost-to-go and the table of constants are the call's own
static void family_lookahead_horizon_block(const sdp_family *f, SdpFamilyArgs &a, const void *dV, const void *dprm, double t0)
{
    family_lookahead_block(f, a, t0);
    a.V = dV;
    a.prm = dprm;
}

extern "C" int sdp_family_simulate_lookahead(sdp_family *f, const void *host_V, int64_t V_steps, int32_t V_timed,
                                             const void *host_prm, int32_t n_prm, int32_t prm_timed, int64_t chunk_bytes,
                                             int64_t B, int64_t T, const void *host_x0, const void *host_w, double t0,
                                             void *host_x, void *host_u, void *host_g, void *host_q)
{
    if (!f || !host_x0 || !host_x || !host_u || !host_g || !host_q) return fail(SDP_EINVAL, "NULL argument");
    int rc;
    int64_t per_chunk = 0;
    if ((rc = family_lookahead_horizon_checks(f, "sdp_family_simulate_lookahead", host_V, V_steps, V_timed, host_prm, n_prm,
                                              chunk_bytes, B, T, &per_chunk))) return rc;
    if (f->W > 0 && !host_w) return fail(SDP_EINVAL, "a stochastic family needs the perturbation sequences");
    if (B == 0) return SDP_OK;
    const size_t rs = real_size(f->dtype);
    const size_t P = (size_t)f->P;
    const size_t slice = (size_t)f->S * rs;
    const int64_t prm_rows = prm_timed ? T : 1;
    DevBuf dV, dprm, dw, dx, du, dg, dq;
    if ((rc = dV.alloc(P * (size_t)(V_timed ? per_chunk : 1) * slice))) return rc;
    if (n_prm > 0 && (rc = upload(dprm, host_prm, P * (size_t)prm_rows * n_prm * rs))) return rc;
    if (f->W > 0 && (rc = upload(dw, host_w, P * (size_t)T * B * rs))) return rc;                // [P][T][B]
    if ((rc = dx.alloc(P * (size_t)(T + 1) * f->d * B * rs))) return rc;
    if ((rc = du.alloc(P * (size_t)T * f->nu * B * rs))) return rc;
    if ((rc = dg.alloc(P * (size_t)T * B * rs))) return rc;
    if ((rc = dq.alloc(P * (size_t)T * B * rs))) return rc;
    // row 0 of every member's x
    for (size_t p = 0; p < P; ++p)
        HIP_TRY(hipMemcpy((char *)dx.p + p * (size_t)(T + 1) * f->d * B * rs, (const char *)host_x0 + p * (size_t)f->d * B * rs,
                          (size_t)f->d * B * rs, hipMemcpyHostToDevice));
    SdpFamilyLookSimArgs a;
    memset(&a, 0, sizeof(a));
    family_lookahead_horizon_block(f, a.f, dV.p, n_prm > 0 ? dprm.p : nullptr, t0);
    a.bprm = (const double *)f->bprm.p; a.steps = (const double *)f->look_steps.p;
    a.w = f->W > 0 ? dw.p : nullptr; a.x = dx.p; a.u = du.p; a.g = dg.p; a.q = dq.p;
    a.B = B; a.T = T; a.t0 = t0;
    a.V_step_stride = V_timed ? f->S : 0;
    a.V_member_stride = (int64_t)(V_timed ? per_chunk : 1) * f->S;
    a.prm_step_stride = prm_timed ? (int64_t)n_prm : 0;
    a.prm_member_stride = prm_rows * (int64_t)n_prm;
    size_t size = sizeof(a);
    void *extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a, HIP_LAUNCH_PARAM_BUFFER_SIZE, &size, HIP_LAUNCH_PARAM_END};
    const unsigned blocks = family_lookahead_grid(f, f->f_lh_simulate, B, 0);
    HIP_TRY(hipStreamSynchronize(f->stream));
    double kernel_ms = 0;
    if (!V_timed && (rc = family_horizon_upload_slices(f, dV, host_V, slice, 1, 1, 0, 1))) return rc;
    for (int64_t k = 0; k < T; k += per_chunk) {
        const int64_t n = (T - k < per_chunk) ? T - k : per_chunk;
        // (the kernel of the previous chunk has finished: the stream is synchronised at the end of every round)
        if (V_timed && (rc = family_horizon_upload_slices(f, dV, host_V, slice, V_steps, per_chunk, k, n))) return rc;
        a.chunk_first = V_timed ? k : 0; a.step_begin = k; a.step_end = k + n;
        HIP_TRY(hipEventRecord(f->ev0, f->stream));
        HIP_TRY(hipModuleLaunchKernel(f->f_lh_simulate, blocks, 1, 1, 256, 1, 1, 0, f->stream, nullptr, extra));
        HIP_TRY(hipEventRecord(f->ev1, f->stream));
        HIP_TRY(hipStreamSynchronize(f->stream));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, f->ev0, f->ev1));
        kernel_ms += ms;
    }
    f->last_kernel_ms = kernel_ms;
    HIP_TRY(hipMemcpy(host_x, dx.p, P * (size_t)(T + 1) * f->d * B * rs, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(host_u, du.p, P * (size_t)T * f->nu * B * rs, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(host_g, dg.p, P * (size_t)T * B * rs, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(host_q, dq.p, P * (size_t)T * B * rs, hipMemcpyDeviceToHost));
    return SDP_OK;
}

extern "C" int sdp_family_montecarlo_lookahead_h(sdp_family *f, const void *host_V, int64_t V_steps, int32_t V_timed,
                                                 const void *host_prm, int32_t n_prm, int32_t prm_timed, int64_t chunk_bytes,
                                                 int64_t B, int64_t T, int64_t n_burn, const uint64_t *host_seeds,
                                                 uint64_t traj_offset, const void *host_x0, const double *host_cum,
                                                 int32_t n_law, const void *host_law_grid, double t0, int64_t steps_per_launch,
                                                 void *host_cost_sum, int64_t *host_n_outside, void *host_x_final,
                                                 uint64_t *host_occupancy)
{
    if (!f || !host_seeds || !host_x0 || !host_cum || !host_law_grid || !host_cost_sum || !host_n_outside || !host_x_final)
        return fail(SDP_EINVAL, "NULL argument");
    if (n_burn < 0 || n_burn > T) return fail(SDP_EINVAL, "n_burn = %lld outside [0, %lld]", (long long)n_burn, (long long)T);
    if (steps_per_launch < 1) return fail(SDP_EINVAL, "steps_per_launch = %lld: at least 1", (long long)steps_per_launch);
    if (f->W <= 0) return fail(SDP_EINVAL, "a deterministic system has nothing to draw: use sdp_family_simulate_lookahead");
    if (n_law < 1 || n_law > 4096) return fail(SDP_EINVAL, "a law of %d points: 1 to 4096", (int)n_law);
    int rc;
    int64_t per_chunk = 0;
    if ((rc = family_lookahead_horizon_checks(f, "sdp_family_montecarlo_lookahead_h", host_V, V_steps, V_timed, host_prm, n_prm,
                                              chunk_bytes, B, T, &per_chunk))) return rc;
    if (!f->f_lh_montecarlo) return fail(SDP_EINVAL, "the unit has no sdp_family_montecarlo_lookahead_h kernel");
    if (B == 0) return SDP_OK;
    if (steps_per_launch > ((int64_t)1 << 30)) steps_per_launch = (int64_t)1 << 30;       // (the kernel counts a launch's steps in 32 bits)
    const size_t rs = real_size(f->dtype);
    const size_t P = (size_t)f->P;
    const size_t slice = (size_t)f->S * rs;
    const int64_t prm_rows = prm_timed ? T : 1;
    // (the draw table of one member in LDS: the cumulative sums, then the values)
    const size_t lds_bytes = (size_t)(n_law - 1) * 8 + (size_t)n_law * rs;
    if (lds_bytes > 65536)
        return fail(SDP_EINVAL, "a law of %d points needs %zu bytes of LDS: at most 65536", (int)n_law, lds_bytes);
    DevBuf dV, dprm, dx, dacc, dout, dcum, dlaw, dseed, docc;
    if ((rc = dV.alloc(P * (size_t)(V_timed ? per_chunk : 1) * slice))) return rc;
    if (n_prm > 0 && (rc = upload(dprm, host_prm, P * (size_t)prm_rows * n_prm * rs))) return rc;
    if ((rc = upload(dx, host_x0, P * (size_t)f->d * B * rs))) return rc;                 // [P][d][B]
    if ((rc = upload(dcum, host_cum, P * (size_t)n_law * 8))) return rc;
    if ((rc = upload(dlaw, host_law_grid, P * (size_t)n_law * rs))) return rc;
    if ((rc = upload(dseed, host_seeds, P * 8))) return rc;
    if ((rc = dacc.alloc(P * (size_t)B * rs))) return rc;
    if ((rc = dout.alloc(P * (size_t)B * 8))) return rc;
    HIP_TRY(hipMemsetAsync(dacc.p, 0, P * (size_t)B * rs, f->stream));
    HIP_TRY(hipMemsetAsync(dout.p, 0, P * (size_t)B * 8, f->stream));
    if (host_occupancy) {
        if ((rc = docc.alloc(P * (size_t)f->S * 8))) return rc;
        HIP_TRY(hipMemsetAsync(docc.p, 0, P * (size_t)f->S * 8, f->stream));
    }
    SdpFamilyLookMcHArgs a;
    memset(&a, 0, sizeof(a));
    family_lookahead_horizon_block(f, a.f, dV.p, n_prm > 0 ? dprm.p : nullptr, t0);
    a.bprm = (const double *)f->bprm.p; a.steps = (const double *)f->look_steps.p;
    a.cum = (const double *)dcum.p; a.law_grid = dlaw.p; a.seed = (const uint64_t *)dseed.p;
    a.x = dx.p; a.acc = dacc.p; a.n_outside = (long long *)dout.p;
    a.occupancy = host_occupancy ? (unsigned long long *)docc.p : nullptr;
    a.B = B; a.traj_offset = traj_offset; a.n_burn = n_burn; a.t0 = t0; a.n_law = n_law;
    a.V_step_stride = V_timed ? f->S : 0;
    a.V_member_stride = (int64_t)(V_timed ? per_chunk : 1) * f->S;
    a.prm_step_stride = prm_timed ? (int64_t)n_prm : 0;
    a.prm_member_stride = prm_rows * (int64_t)n_prm;
    size_t size = sizeof(a);
    void *extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a, HIP_LAUNCH_PARAM_BUFFER_SIZE, &size, HIP_LAUNCH_PARAM_END};
    const unsigned lds = (unsigned)lds_bytes;
    const unsigned blocks = family_lookahead_grid(f, f->f_lh_montecarlo, B, lds);
    HIP_TRY(hipStreamSynchronize(f->stream));
    double kernel_ms = 0;
    if (!V_timed && (rc = family_horizon_upload_slices(f, dV, host_V, slice, 1, 1, 0, 1))) return rc;
    for (int64_t c = 0; c < T; c += per_chunk) {
        const int64_t c_end = (T - c < per_chunk) ? T : c + per_chunk;
        if (V_timed && (rc = family_horizon_upload_slices(f, dV, host_V, slice, V_steps, per_chunk, c, c_end - c))) return rc;
        a.chunk_first = V_timed ? c : 0;
        HIP_TRY(hipEventRecord(f->ev0, f->stream));
        for (int64_t k = c; k < c_end; k += steps_per_launch) {
            a.step_begin = k;
            a.step_end = (c_end - k < steps_per_launch) ? c_end : k + steps_per_launch;
            HIP_TRY(hipModuleLaunchKernel(f->f_lh_montecarlo, blocks, 1, 1, 256, 1, 1, lds, f->stream, nullptr, extra));
        }
        HIP_TRY(hipEventRecord(f->ev1, f->stream));
        HIP_TRY(hipStreamSynchronize(f->stream));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, f->ev0, f->ev1));
        kernel_ms += ms;
    }
    f->last_kernel_ms = kernel_ms;
    HIP_TRY(hipMemcpy(host_cost_sum, dacc.p, P * (size_t)B * rs, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(host_n_outside, dout.p, P * (size_t)B * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(host_x_final, dx.p, P * (size_t)f->d * B * rs, hipMemcpyDeviceToHost));
    if (host_occupancy) HIP_TRY(hipMemcpy(host_occupancy, docc.p, P * (size_t)f->S * 8, hipMemcpyDeviceToHost));
    return SDP_OK;
}

// [P][S] elements of `elem_bytes` from the two buffers, every member from the one its last sweep wrote
static int family_download(sdp_family *f, void *host, size_t elem_bytes)
{
    const size_t row = (size_t)f->S * elem_bytes;
    for (int p = 0; p < f->P;) {
        int q = p + 1;
        while (q < f->P && f->where[(size_t)q] == f->where[(size_t)p]) ++q;      // (a run of members in one buffer: one copy)
        HIP_TRY(hipMemcpyAsync((char *)host + (size_t)p * row, (const char *)f->buf[f->where[(size_t)p]].p + (size_t)p * row,
                               (size_t)(q - p) * row, hipMemcpyDeviceToHost, f->stream));
        p = q;
    }
    HIP_TRY(hipStreamSynchronize(f->stream));
    return SDP_OK;
}

extern "C" int sdp_family_get_value(sdp_family *f, void *host_J)
{
    if (!f || !host_J) return fail(SDP_EINVAL, "NULL argument");
    return family_download(f, host_J, real_size(f->dtype));
}

extern "C" int sdp_family_get_policy(sdp_family *f, void *host_pol, int32_t *host_idx)
{
    if (!f) return fail(SDP_EINVAL, "NULL family");
    const size_t n = (size_t)f->P * f->S;
    if (host_pol) HIP_TRY(hipMemcpyAsync(host_pol, f->pol.p, n * f->nu * real_size(f->dtype), hipMemcpyDeviceToHost, f->stream));
    if (host_idx) HIP_TRY(hipMemcpyAsync(host_idx, f->idx.p, n * 4, hipMemcpyDeviceToHost, f->stream));
    HIP_TRY(hipStreamSynchronize(f->stream));
    return SDP_OK;
}

extern "C" int sdp_family_last_kernel_ms(sdp_family *f, double *ms)
{
    if (!f || !ms) return fail(SDP_EINVAL, "NULL argument");
    *ms = f->last_kernel_ms;
    return SDP_OK;
}
