// mp_host.h — what the host sources of the C ABI share (mp_capi.cpp, mp_summaries.cpp, mp_sampler.cpp, mp_monitor.cpp, mp_optimizer.cpp,
// mp_nested.cpp, mp_simplex.cpp, mp_smc.cpp).
//
// Internal: not installed, never seen by a kernel source.  Error reporting, owners of device memory, pinned memory and events,
// the two types behind the ABI's handle -- Evaluator, everything that lives on ONE device, and mp_handle, the dealer that owns
// one evaluator per device and the lock -- the helpers of mp_capi.cpp that the summaries and the resident drivers call, and the
// skeleton that the optimizer, the nested sampler, the simplex search and the SMC sampler stand on (Resident and what follows it).
// Each driver's own struct stays in its source file; the sampler's four chain monitors are a unit of their own (mp_monitor.h),
// which the probe libraries of their kernels link as well.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <numeric>
#include <vector>

#include "mp_device.h"

// Nothing declared here is part of the ABI: hidden, so that the library exports the mp_* functions of include/magprop_amd.h only.
#pragma GCC visibility push(hidden)

// records the message behind mp_last_error() for the calling thread and returns code (defined in mp_capi.cpp)
int fail(int code, const char *fmt, ...);

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return fail(MP_EHIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// what a launcher returned (a hipError_t as int), as the entry point's return code
inline int launched(int e) {
    return e ? fail(MP_EHIP, "kernel launch failed: %s", hipGetErrorString((hipError_t)e)) : MP_OK;
}

struct DeviceScope {  // make an evaluator's device current for the duration of a call
    int prev = -1;
    bool ok = true;
    explicit DeviceScope(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceScope() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

struct HostDataset {
    bool set = false;
    std::vector<int32_t> g, tile_ptr;
    std::vector<double> dx, idt, y, yerr;
};

// Device memory owned by its holder: freed on destruction (on the device current then: the destroy functions delete their object
// inside a DeviceScope of its device), never copied.
template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    int ensure(size_t n) {
        if (n <= cap) return MP_OK;
        release();
        size_t want = std::max<size_t>(n, 16);
        HIP_TRY(hipMalloc((void **)&p, want * sizeof(T)));
        cap = want;
        return MP_OK;
    }
};

// Allocates a driver's buffers (ensure) and points the fields of its launch arguments at them: bind(buffer, size, field).  The
// first failure sticks in rc, and the allocations behind it are skipped.
struct Binder {
    int rc = MP_OK;
    template <typename T, typename P>
    void operator()(DevBuf<T> &b, size_t n, P *&field) {
        if (!rc && !(rc = b.ensure(n))) field = b.p;
    }
};

// Page-locked host staging area of the host-buffer entry points: copies to and from it are true asynchronous DMA
// (pageable user buffers would be staged by the runtime copy by copy).
struct PinnedBuf {
    unsigned char *p = nullptr;
    unsigned char *dev = nullptr;   // the same memory as the device sees it (mapped, coherent): kernels may read and write it in place
    size_t cap = 0;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf &) = delete;
    PinnedBuf &operator=(const PinnedBuf &) = delete;
    ~PinnedBuf() { if (p) (void)hipHostFree(p); }
    int ensure(size_t n) {
        if (n <= cap) return MP_OK;
        if (p) (void)hipHostFree(p);
        p = dev = nullptr;
        cap = 0;
        const size_t want = std::max<size_t>(n, 4096);
        HIP_TRY(hipHostMalloc((void **)&p, want, hipHostMallocMapped | hipHostMallocCoherent));
        HIP_TRY(hipHostGetDevicePointer((void **)&dev, p, 0));
        cap = want;
        return MP_OK;
    }
};

// An event owned by its holder (created by it when first needed, destroyed with it)
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(const Event &) = delete;
    Event &operator=(const Event &) = delete;
    ~Event() { if (e) (void)hipEventDestroy(e); }
};

// Device-to-host copies of the state of a driver: read_back(dst, src, n, dst2, src2, n2, ...) copies n elements of src to dst
// for every triple whose dst is not NULL.
inline int read_back() { return MP_OK; }
template <typename T, typename... Rest>
int read_back(T *dst, const T *src, size_t n, Rest... rest) {
    if (dst) HIP_TRY(hipMemcpy(dst, src, n * sizeof(T), hipMemcpyDeviceToHost));
    return read_back(rest...);
}

// The resets of a driver's set function, enqueued on st: zero_async(st, p, n, p2, n2, ...) clears n elements of p for every pair.
inline int zero_async(hipStream_t) { return MP_OK; }
template <typename T, typename... Rest>
int zero_async(hipStream_t st, T *p, size_t n, Rest... rest) {
    HIP_TRY(hipMemsetAsync(p, 0, n * sizeof(T), st));
    return zero_async(st, rest...);
}

// Everything of a handle that lives on one device: stream, constants and tables, the dataset arena, the workspaces of the
// host-buffer entry points.  Made by evaluator_create and freed by evaluator_destroy (mp_capi.cpp), which deletes it inside a
// DeviceScope of its device -- not by a destructor body, which would end before the members' destructors free their memory.
// It has no lock of its own: its handle's lock covers it.
struct Evaluator {
    int device = 0;
    hipStream_t stream = nullptr;
    std::vector<double> tgrid;
    int n_tiles = 0;
    HostDataset ds[MP_MAX_DATASETS];
    mp::DevShared sh{};
    // device copies of the shared data
    DevBuf<double> d_wtab;
    DevBuf<double> d_tgrid, d_obs_dx, d_obs_idt, d_obs_y, d_obs_yerr;
    DevBuf<int32_t> d_obs_g, d_tile_ptr;
    DevBuf<mp::DsDesc> d_ds;
    // The packed observation arrays are an append-only arena: a new light curve goes behind the last one (obs_used /
    // tp_used entries are live or stale), a replaced one leaves its old entries behind as garbage until the next rebuild.
    size_t obs_used = 0, tp_used = 0;
    std::vector<mp::DsDesc> desc;   // host mirror of d_ds
    // Workspaces of the host-buffer entry points.  Every user runs under the handle's lock and synchronises the stream before it
    // returns, so no two calls have a workspace in use at once and the entry points may share them.
    DevBuf<double> w_pars, w_lnprob;
    // w_curves: the curve rows of whichever call runs.  The curve pass of mp_model_lc, mp_model_band, mp_model_derived,
    // mp_model_pointwise, mp_model_flows and mp_model_flow_band (mp_summaries.cpp): [wanted curves][chunk][n_grid]; mp_lnprob_batch with ltot_out: [n][n_grid]; mp_rhs_batch:
    // [pars | t | y] in and [dydt | lam] out.
    DevBuf<double> w_curves;
    DevBuf<double> w_band, w_band_out;   // mp_model_band: [n_grid][n] one component's curves transposed; [components][nq][n_grid]
    DevBuf<uint32_t> w_band_units;       // mp_model_band_weighted: [n] the rows' weights in integer units
    DevBuf<double> w_derive_out;         // mp_model_derived: [chunk][MP_DERIVED_N]
    DevBuf<double> w_flow_cells, w_flow_out;      // mp_model_flows: [MP_FLOW_NCURVES][chunk][n_grid] cell curves; [chunk][MP_FLOW_N]
    DevBuf<double> w_flow_band;                   // mp_model_flow_band: [selected curves][n][n_grid]; kept between calls for one curve only
    DevBuf<double> w_pw_z, w_pw_obs, w_pw_tail;   // mp_model_pointwise: [n_obs][n] cells; [n_obs][MP_POINTWISE_N]; [n_obs][T(n)]
    DevBuf<double> w_rw_lw, w_rw_out, w_rw_tail;  // mp_model_reweight: [n_alt][n] log weights; [n_alt][MP_REWEIGHT_N]; [n_alt][T(n)]
    DevBuf<double> w_rw_alt;                      // mp_model_reweight: [n_alt][3] the alternatives, then [n_alt][n_obs] the observation weights
    DevBuf<int32_t> w_rw_kind;                    // mp_model_reweight: [n_alt]
    DevBuf<double> w_sim;                         // mp_simulate: [dx | idt | yerr][table rows][n_obs], then [y | yerr | model | z][chunk][n_obs]
    DevBuf<int32_t> w_sim_g;                      // mp_simulate: [table rows][n_obs] the brackets' g, then [n] the rows' zero-error marks
    DevBuf<int32_t> w_dsid, w_status, w_sweeps;
    DevBuf<int32_t> w_tile_log;
    std::vector<int32_t> last_tile_log;   // tile words of the rows of its block of the most recent host-buffer batch
    PinnedBuf h_io;               // mp_lnprob_batch: [pars | ds_id] in, [lnprob | status | sweeps | tiles] out, read and written in place by the kernel
    // Launch order of mixed-length batches (mp_kernels.hip order_kernel): a ring of index buffers, one per launch in flight.
    // A slot is written by the launch that takes it and read by that launch's workgroups as they start; the launch that
    // takes it kOrderRing launches later waits (stream-level, on the event recorded behind the earlier launch) for that
    // launch to have finished -- launches fewer than kOrderRing apart share nothing.
    static constexpr int kOrderRing = 8;
    DevBuf<int32_t> order[kOrderRing];
    Event order_done[kOrderRing];
    unsigned order_next = 0;
    int pend_n = 0;               // rows of its block of the host-buffer batch between batch_begin and batch_end
    size_t pend_in_bytes = 0;
    double last_tot_sweeps = 0.0, last_tot_tiles = 0.0;   // over the walkers of its last block that finished (status ok) ...
    int last_cnt_ok = 0;                                  // ... and how many those were
};

// The handle of the ABI: a dealer over one evaluator per device (mp_create: one; mp_create_multi: one per listed device) and
// no device state of its own.  Datasets and the prior go to every evaluator, a host-buffer batch is dealt out in contiguous
// blocks, whatever serves one walker or one device runs on the first.
struct mp_handle {
    std::vector<Evaluator *> ev;  // owned: freed by mp_destroy
    bool multi = false;           // made by mp_create_multi: the entries that belong to ONE device refuse it, even over one device
    // Threading / stream contract (include/magprop_amd.h): every entry point that takes a handle or a sampler holds
    // `mu` for its duration.  Launches share nothing writable but their own outputs (round 4: no per-walker scratch rows),
    // so launches of one handle on different streams may overlap freely.
    std::recursive_mutex mu;
    bool tile_log_on = false;
    // the most recent host-buffer batch, all blocks (diagnostic): per walker, and the means over the walkers that finished
    std::vector<int32_t> last_sweeps, last_tiles;
    double last_mean_sweeps = 0.0, last_mean_tiles = 0.0;
    Evaluator *first() const { return ev[0]; }   // the scalar settings are the same on every evaluator
};

using Lock = std::lock_guard<std::recursive_mutex>;

// What an entry point holds for its duration: the handle's lock, then the evaluator's device made current.
struct Held {
    Lock lock;
    DeviceScope scope;
    Held(mp_handle *h, const Evaluator *e) : lock(h->mu), scope(e->device) {}
};

// ---------------------------------------------------------------- defined in mp_capi.cpp, used by the summaries and the drivers
int launch_lnprob_ordered(Evaluator *h, const mp::LaunchArgs &a_in, hipStream_t st);
int check_box(const char *fn, int ndim, const double *lower, const double *upper);
int check_inside(const char *what, const double *rows, size_t n, int ndim, const double *lower, const double *upper);
int upload_ds_rows(int32_t *dst, const int32_t *ds_id, int n_groups, int rows);
int groups_running(Evaluator *h, const int32_t *d_flags, int n, int *running);

// The checks of the drivers' create functions (fn), in the order they fail: a multi-device handle (`multi`: what the message says about
// it), ndim (the posterior, target 0, needs 6 or more), the driver's own arguments (args(): MP_OK or the code of a failure), the
// alternative dipole torque, and the dataset of every one of n_groups groups (`group` g: ds_id[g], dataset 0 without ds_id).
// The caller holds the handle's lock.
template <class Args>
int check_create(mp_handle *h, const char *fn, const char *multi, int ndim, int target, const char *group, int n_groups,
                 const int32_t *ds_id, Args &&args) {
    if (h->multi) return fail(MP_ESTATE, "%s: %s", fn, multi);
    if (ndim < 1 || ndim > MP_MAX_NDIM || (target == 0 && ndim < 6)) return fail(MP_EINVAL, "%s: bad ndim %d", fn, ndim);
    const int rc = args();
    if (rc) return rc;
    if (target != 0) return MP_OK;
    if (h->first()->sh.cfg.dipole_torque != 0)
        return fail(MP_ESTATE, "%s: the alternative dipole torque (cfg.dipole_torque = 1) is served by the curve kernels only", fn);
    for (int g = 0; g < n_groups; ++g) {
        const int d = ds_id ? ds_id[g] : 0;
        if (d < 0 || d >= MP_MAX_DATASETS || !h->first()->ds[d].set) return fail(MP_ESTATE, "%s: %s %d refers to unset dataset %d", fn, group, g, d);
    }
    return MP_OK;
}

// ---------------------------------------------------------------- the skeleton of the resident drivers besides the ensemble sampler
// (the optimizer, the nested sampler, the simplex search and the SMC sampler; mp_nested_run keeps a loop of its own, run_chunked's
// with the dead rows read back around every chunk)
// What each of the four structs (mp_optimizer, mp_nested, mp_simplex, mp_smc) derives from.  Each adds its launch arguments `a`
// (with the box a.lower / a.upper) and its buffers, d_dsid among them.
struct Resident {
    mp_handle *h = nullptr;         // the lock
    Evaluator *ev = nullptr;        // the device state: the handle's one evaluator
    bool have_state = false;        // the driver's set function has run
};

template <class D>
int resident_destroy(D *d) {
    if (!d) return MP_OK;
    Held held(d->h, d->ev);
    (void)hipStreamSynchronize(d->ev->stream);
    delete d;
    return MP_OK;
}

// A create function `fn` from end to end: the NULL check, the handle's lock, check_create (multi, group and args() as there), the
// new driver with the box copied in, then fill(d, bind) -- the driver's own arguments and its bind(...) list -- inside a
// DeviceScope, and the datasets of the groups' rows (ds_rows rows each) uploaded to d_dsid.  NULL and the message on any failure.
template <class D, class Args, class Fill>
D *resident_create(mp_handle *h, const char *fn, const char *multi, int ndim, int target, const char *group, int n_groups,
                   const int32_t *ds_id, int ds_rows, const double *lower, const double *upper, Args &&args, Fill &&fill) {
    if (!h || !lower || !upper) { fail(MP_EINVAL, "%s: NULL argument", fn); return nullptr; }
    Lock lock(h->mu);
    if (check_create(h, fn, multi, ndim, target, group, n_groups, ds_id, args)) return nullptr;
    D *d = new D();
    d->h = h;
    d->ev = h->first();
    for (int k = 0; k < ndim; ++k) { d->a.lower[k] = lower[k]; d->a.upper[k] = upper[k]; }
    DeviceScope scope(d->ev->device);
    Binder bind;
    fill(d, bind);
    if (bind.rc || upload_ds_rows(d->d_dsid.p, ds_id, n_groups, ds_rows)) {
        fail(MP_EHIP, "%s: device allocation failed", fn);
        resident_destroy(d);
        return nullptr;
    }
    return d;
}

// The entry of a run function `fn` of driver d: the arguments (`ok`; `bad` says what is wrong with them or with a NULL d), the
// state that the function `set` makes, then the handle's lock and the evaluator's device for the rest of the body (`held`).
#define RESIDENT_ENTER(d, ok, fn, bad, set)                                              \
    if (!(d) || !(ok)) return fail(MP_EINVAL, fn ": " bad);                              \
    if (!(d)->have_state) return fail(MP_ESTATE, fn ": call " set " first");             \
    Held held((d)->h, (d)->ev)
// The entry of a getter: the same, and the work on the evaluator's stream has finished.
#define RESIDENT_READ(d, ok, fn, bad, set) \
    RESIDENT_ENTER(d, ok, fn, bad, set);   \
    HIP_TRY(hipStreamSynchronize((d)->ev->stream))

// The run loop: up to `limit` units in chunks of at most chunk_max, enqueue() once per unit with no wait inside a chunk.  The
// groups' flags are read back once before the first chunk and once behind every chunk, and the loop ends early once no group is
// running; *n_running (unless NULL) is the last count.
template <class Enqueue>
int run_chunked(Evaluator *ev, const int32_t *d_flags, int n_groups, int chunk_max, int limit, int *n_running, Enqueue &&enqueue) {
    int running, rc;
    if ((rc = groups_running(ev, d_flags, n_groups, &running))) return rc;
    for (int done = 0; done < limit && running > 0;) {
        const int chunk = std::min(chunk_max, limit - done);
        for (int c = 0; c < chunk; ++c)
            if ((rc = enqueue())) return rc;
        if ((rc = groups_running(ev, d_flags, n_groups, &running))) return rc;
        done += chunk;
    }
    if (n_running) *n_running = running;
    return MP_OK;
}

#pragma GCC visibility pop
