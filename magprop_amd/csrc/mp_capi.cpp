// mp_capi.cpp — host side of the C ABI declared in include/magprop_amd.h.
//
// Plain HIP runtime only (no torch, no hipBLAS): device buffers, one stream per handle, the
// host-side digestion of observed light curves into the tile-bucketed layout the kernel reads,
// and thin launch wrappers.  There is NO CPU fallback: without a HIP device mp_create() fails.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <numeric>
#include <string>
#include <thread>
#include <vector>

#include "mp_band.h"
#include "mp_device.h"

namespace {

thread_local std::string g_err;

int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return fail(MP_EHIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

struct DeviceScope {  // make the handle's device current for the duration of a call
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
    int ensure(size_t n) {
        if (n <= cap) return MP_OK;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
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
int read_back() { return MP_OK; }
template <typename T, typename... Rest>
int read_back(T *dst, const T *src, size_t n, Rest... rest) {
    if (dst) HIP_TRY(hipMemcpy(dst, src, n * sizeof(T), hipMemcpyDeviceToHost));
    return read_back(rest...);
}

}  // namespace

struct mp_handle {
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
    // workspace of the host-buffer entry points
    DevBuf<double> w_pars, w_lnprob, w_curves;
    DevBuf<double> w_band, w_band_out;   // mp_model_band: [components][n][n_grid] curves | [n_grid][n] transposed; [components][nq][n_grid]
    DevBuf<int32_t> w_dsid, w_status, w_sweeps;
    double last_mean_tiles = 0.0;
    bool tile_log_on = false;
    DevBuf<int32_t> w_tile_log;
    std::vector<int32_t> last_tile_log;
    PinnedBuf h_io;               // mp_lnprob_batch: [pars | ds_id] in, [lnprob | status | sweeps | tiles] out, read and written in place by the kernel
    double last_mean_sweeps = 0.0;
    std::vector<int32_t> last_sweeps, last_tiles;   // per walker, most recent host-buffer batch (diagnostic)
    // Launch order of mixed-length batches (mp_kernels.hip order_kernel): a ring of index buffers, one per launch in flight.
    // A slot is written by the launch that takes it and read by that launch's workgroups as they start; the launch that
    // takes it kOrderRing launches later waits (stream-level, on the event recorded behind the earlier launch) for that
    // launch to have finished -- launches fewer than kOrderRing apart share nothing.
    static constexpr int kOrderRing = 8;
    DevBuf<int32_t> order[kOrderRing];
    Event order_done[kOrderRing];
    unsigned order_next = 0;
    // Threading / stream contract (include/magprop_amd.h): every entry point that takes a handle or a sampler holds
    // `mu` for its duration.  Launches share nothing writable but their own outputs (round 4: no per-walker scratch rows),
    // so launches of one handle on different streams may overlap freely.
    std::recursive_mutex mu;
    // Multi-device handle (mp_create_multi): one evaluator per listed device; this object then holds no device state of
    // its own -- datasets and prior are forwarded to every evaluator, a host-buffer batch is dealt out in contiguous blocks.
    std::vector<mp_handle *> sub;
    int pend_n = 0;               // rows of the host-buffer batch between batch_begin and batch_end
    size_t pend_in_bytes = 0;
    double last_tot_sweeps = 0.0, last_tot_tiles = 0.0;   // over the walkers of the last batch that finished (status ok) ...
    int last_cnt_ok = 0;                                  // ... and how many those were
};

namespace {
using Lock = std::lock_guard<std::recursive_mutex>;

// Launch the log-posterior kernel over a batch.  A batch that refers to light curves of more than 64 points next to short
// ones and needs more than one round of the device's wave slots (two per SIMD) is evaluated longest light curves first.
int launch_lnprob_ordered(mp_handle *h, const mp::LaunchArgs &a_in, hipStream_t st) {
    mp::LaunchArgs a = a_in;
    int slot = -1;
    const bool curves = a.ltot || a.lprop || a.ldip || a.mdisc || a.omega;
    if (h->sh.has_long && h->sh.n_ds > 1 && a.ds_id && a.want_chi2 && !curves && a.n > 2 * h->sh.n_simd) {
        slot = (int)(h->order_next++ % mp_handle::kOrderRing);
        if (h->order[slot].cap < (size_t)a.n) {
            // (growing frees the old buffer, which waits for the device: nothing in flight reads it any more)
            const int rc = h->order[slot].ensure((size_t)a.n);
            if (rc) return rc;
        }
        if (!h->order_done[slot].e) HIP_TRY(hipEventCreateWithFlags(&h->order_done[slot].e, hipEventDisableTiming));
        else HIP_TRY(hipStreamWaitEvent(st, h->order_done[slot].e, 0));
        const int eo = mp::launch_order(h->sh, a.ds_id, a.n, h->order[slot].p, (void *)st);
        if (eo) return fail(MP_EHIP, "kernel launch failed: %s", hipGetErrorString((hipError_t)eo));
        a.order = h->order[slot].p;
    }
    const int e = mp::launch_lnprob(h->sh, a, (void *)st);
    if (e) return fail(MP_EHIP, "kernel launch failed: %s", hipGetErrorString((hipError_t)e));
    if (slot >= 0) HIP_TRY(hipEventRecord(h->order_done[slot].e, st));
    return MP_OK;
}
}  // namespace

static void publish_datasets(mp_handle *h) {
    int n_ds = 0, extra = 0;
    for (int d = 0; d < MP_MAX_DATASETS; ++d)
        if (h->ds[d].set) { n_ds = d + 1; extra = std::max(extra, (int)h->ds[d].g.size() - 64); }
    h->sh.ds = h->d_ds.p;
    h->sh.n_ds = n_ds;
    h->sh.tile_ptr = h->d_tile_ptr.p;
    h->sh.obs_g = h->d_obs_g.p;
    h->sh.obs_dx = h->d_obs_dx.p;
    h->sh.obs_idt = h->d_obs_idt.p;
    h->sh.obs_y = h->d_obs_y.p;
    h->sh.obs_yerr = h->d_obs_yerr.p;
    h->sh.has_long = extra > 0 ? 1 : 0;
}

// Copy light curve d behind the arena's last entry and publish its descriptor (slots never set keep n_obs = 0, which
// the kernels answer with MP_STATUS_BADDATASET).  Nothing in flight reads the target regions: no synchronisation.
static int append_dataset(mp_handle *h, int d) {
    const HostDataset &s = h->ds[d];
    const size_t n = s.g.size(), o = h->obs_used, t = h->tp_used;
    HIP_TRY(hipMemcpy(h->d_obs_g.p + o, s.g.data(), n * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->d_obs_dx.p + o, s.dx.data(), n * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->d_obs_idt.p + o, s.idt.data(), n * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->d_obs_y.p + o, s.y.data(), n * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->d_obs_yerr.p + o, s.yerr.data(), n * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->d_tile_ptr.p + t, s.tile_ptr.data(), s.tile_ptr.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    int32_t flags = mp::kDsOnKnots;
    for (size_t j = 0; j < n; ++j) if (s.dx[j] != 0.0) { flags = 0; break; }
    h->desc[d] = mp::DsDesc{(int32_t)n, (int32_t)o, (int32_t)t, flags};
    HIP_TRY(hipMemcpy(h->d_ds.p + d, &h->desc[d], sizeof(mp::DsDesc), hipMemcpyHostToDevice));
    h->obs_used = o + n;
    h->tp_used = t + s.tile_ptr.size();
    return MP_OK;
}

// Rebuild the arena from the host copies (first use, growth, or a replaced slot): waits for the device, because
// kernels in flight may still read the old buffers, and leaves room for the sets to come.
static int rebuild_datasets(mp_handle *h) {
    size_t n_obs = 0, n_tp = 0;
    for (int d = 0; d < MP_MAX_DATASETS; ++d)
        if (h->ds[d].set) { n_obs += h->ds[d].g.size(); n_tp += h->ds[d].tile_ptr.size(); }
    HIP_TRY(hipDeviceSynchronize());
    const size_t cap_obs = std::max<size_t>(2 * n_obs, 4096), cap_tp = std::max<size_t>(2 * n_tp, 8 * ((size_t)h->n_tiles + 1));
    int rc;
    if ((rc = h->d_obs_g.ensure(cap_obs)) || (rc = h->d_obs_dx.ensure(cap_obs)) || (rc = h->d_obs_idt.ensure(cap_obs)) ||
        (rc = h->d_obs_y.ensure(cap_obs)) || (rc = h->d_obs_yerr.ensure(cap_obs)) || (rc = h->d_tile_ptr.ensure(cap_tp)) ||
        (rc = h->d_ds.ensure(MP_MAX_DATASETS)))
        return rc;
    h->desc.assign(MP_MAX_DATASETS, mp::DsDesc{0, 0, 0, 0});
    HIP_TRY(hipMemset(h->d_ds.p, 0, MP_MAX_DATASETS * sizeof(mp::DsDesc)));
    h->obs_used = h->tp_used = 0;
    for (int d = 0; d < MP_MAX_DATASETS; ++d)
        if (h->ds[d].set && (rc = append_dataset(h, d))) return rc;
    publish_datasets(h);
    return MP_OK;
}

// After h->ds[d] has been (re)set on the host.
static int upload_dataset(mp_handle *h, int d, bool replaced) {
    const HostDataset &s = h->ds[d];
    const bool fits = h->d_ds.p && h->obs_used + s.g.size() <= h->d_obs_g.cap && h->tp_used + s.tile_ptr.size() <= h->d_tile_ptr.cap;
    if (replaced || !fits) return rebuild_datasets(h);
    const int rc = append_dataset(h, d);
    if (rc) return rc;
    publish_datasets(h);
    return MP_OK;
}

// ---------------------------------------------------------------- what the resident drivers share
// (the ensemble sampler, the differential-evolution optimizer and the nested sampler: mp_sampler_*, mp_optimizer_*, mp_nested_*)

// The checks of their create functions (fn), in the order they fail: a multi-device handle (`multi`: what the message says about
// it), ndim (the posterior, target 0, needs 6 or more), the driver's own arguments (args(): MP_OK or the code of a failure), the
// alternative dipole torque, and the dataset of every one of n_groups groups (`group` g: ds_id[g], dataset 0 without ds_id).
// The caller holds the handle's lock.
template <class Args>
static int check_create(mp_handle *h, const char *fn, const char *multi, int ndim, int target, const char *group, int n_groups,
                        const int32_t *ds_id, Args &&args) {
    if (!h->sub.empty()) return fail(MP_ESTATE, "%s: %s", fn, multi);
    if (ndim < 1 || ndim > MP_MAX_NDIM || (target == 0 && ndim < 6)) return fail(MP_EINVAL, "%s: bad ndim %d", fn, ndim);
    const int rc = args();
    if (rc) return rc;
    if (target != 0) return MP_OK;
    if (h->sh.cfg.dipole_torque != 0)
        return fail(MP_ESTATE, "%s: the alternative dipole torque (cfg.dipole_torque = 1) is served by the curve kernels only", fn);
    for (int g = 0; g < n_groups; ++g) {
        const int d = ds_id ? ds_id[g] : 0;
        if (d < 0 || d >= MP_MAX_DATASETS || !h->ds[d].set) return fail(MP_ESTATE, "%s: %s %d refers to unset dataset %d", fn, group, g, d);
    }
    return MP_OK;
}

// the bounds box of the optimizer and the nested sampler: finite, lower < upper in every coordinate
static int check_box(const char *fn, int ndim, const double *lower, const double *upper) {
    for (int d = 0; d < ndim; ++d)
        if (!(std::isfinite(lower[d]) && std::isfinite(upper[d]) && lower[d] < upper[d]))
            return fail(MP_EINVAL, "%s: bounds of coordinate %d are empty or not finite", fn, d);
    return MP_OK;
}

// the dataset of every row, ds_id[g] (dataset 0 without ds_id) for the `rows` consecutive rows of group g, uploaded to dst
static int upload_ds_rows(int32_t *dst, const int32_t *ds_id, int n_groups, int rows) {
    std::vector<int32_t> ds((size_t)n_groups * rows);
    for (int g = 0; g < n_groups; ++g) std::fill_n(ds.begin() + (size_t)g * rows, rows, ds_id ? ds_id[g] : 0);
    HIP_TRY(hipMemcpy(dst, ds.data(), ds.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    return MP_OK;
}

// *running = the groups whose flag (d_flags[n], read back behind the work on the handle's stream) is not 1 (converged, stopped)
static int groups_running(mp_handle *h, const int32_t *d_flags, int n, int *running) {
    std::vector<int32_t> f((size_t)n);
    HIP_TRY(hipMemcpyAsync(f.data(), d_flags, f.size() * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    *running = n - (int)std::count(f.begin(), f.end(), 1);
    return MP_OK;
}

extern "C" {

int mp_abi_version(void) { return MP_ABI_VERSION; }

const char *mp_last_error(void) { return g_err.c_str(); }

void mp_cfg_synth(mp_model_cfg *c) {
    if (!c) return;
    *c = mp_model_cfg{0.35, 3.0, 10.0, 10.0, 0.1, 1.0, 0.9, 1.0, 1.0, 1.0, 0.27, 1, 0, 0.0, 0.0, 0, 0};
}

void mp_cfg_lib(mp_model_cfg *c) {
    if (!c) return;
    *c = mp_model_cfg{0.8, 1.0, 1.0, 1.0, 0.1, 1.0, 0.9, 0.05, 0.4, 1.0, 0.0, 0, 0, 0.0, 0.0, 0, 0};
}

mp_handle *mp_create(const mp_model_cfg *cfg, const double *tgrid, int n_grid, int device) {
    if (!cfg || !tgrid || n_grid < 2) {
        fail(MP_EINVAL, "mp_create: cfg/tgrid NULL or n_grid < 2");
        return nullptr;
    }
    for (int i = 1; i < n_grid; ++i)
        if (!(tgrid[i] > tgrid[i - 1]) || !std::isfinite(tgrid[i])) {
            fail(MP_EINVAL, "mp_create: tgrid must be finite and strictly increasing (index %d)", i);
            return nullptr;
        }
    // The integrator is built on a geometric grid (np.logspace), the only kind the reference uses
    // (magnetar/funcs.py:132-137, code/synthetic_datasets/funcs.py:19).
    if (!(tgrid[0] > 0.0)) {
        fail(MP_EINVAL, "mp_create: tgrid must be positive");
        return nullptr;
    }
    // the kernels generate the step end times themselves, t_i = t_0 q^i: the grid has to be geometric to rounding
    const double lnq_check = std::log(tgrid[n_grid - 1] / tgrid[0]) / (double)(n_grid - 1);
    for (int i = 1; i < n_grid; ++i)
        if (std::fabs(tgrid[i] / (tgrid[0] * std::exp((double)i * lnq_check)) - 1.0) > 1.0e-12) {
            fail(MP_EINVAL, "mp_create: tgrid must be log-spaced (np.logspace); it leaves t0*q^i at index %d", i);
            return nullptr;
        }
    if (!(cfg->inertia_factor > 0) || !(cfg->alpha > 0) || !(cfg->cs7 > 0) || !(cfg->k > 0) ||
        !(cfg->rm_massflow_factor > 0)) {
        fail(MP_EINVAL, "mp_create: non-positive model constant in cfg");
        return nullptr;
    }
    if (!(cfg->sweep_tol >= 0.0) || cfg->sweep_tol > 1.0e-3) {
        fail(MP_EINVAL, "mp_create: cfg.sweep_tol must be 0 (library default) or in (0, 1e-3]");
        return nullptr;
    }
    if (!(cfg->stride_tol >= 0.0) || cfg->stride_tol > 1.0e-3 ||
        !(cfg->max_stride == 0 || cfg->max_stride == 1 || cfg->max_stride == 2 || cfg->max_stride == 4 ||
          cfg->max_stride == 8)) {
        fail(MP_EINVAL, "mp_create: cfg.max_stride must be 0, 1, 2, 4 or 8 and cfg.stride_tol 0 or in (0, 1e-3]");
        return nullptr;
    }
    if (cfg->dipole_torque != 0 && cfg->dipole_torque != 1) {
        fail(MP_EINVAL, "mp_create: cfg.dipole_torque must be 0 (the packages' dipole torque) or 1 (code/figure_3.py's Bucciantini law)");
        return nullptr;
    }
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
        fail(MP_ENODEV, "mp_create: no HIP device visible (this library has no CPU fallback)");
        return nullptr;
    }
    if (device < 0 && hipGetDevice(&device) != hipSuccess) device = 0;
    if (device >= count) {
        fail(MP_ENODEV, "mp_create: device %d out of range (%d visible)", device, count);
        return nullptr;
    }
    mp_handle *h = new mp_handle();
    h->device = device;
    DeviceScope scope(device);
    hipDeviceProp_t prop;
    if (!scope.ok || hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess ||
        hipGetDeviceProperties(&prop, device) != hipSuccess) {
        fail(MP_EHIP, "mp_create: cannot select device %d / create stream", device);
        mp_destroy(h);
        return nullptr;
    }
    h->tgrid.assign(tgrid, tgrid + n_grid);
    h->n_tiles = (n_grid - 1 + mp::kTile - 1) / mp::kTile;
    if (h->d_tgrid.ensure((size_t)n_grid) != MP_OK ||
        hipMemcpy(h->d_tgrid.p, tgrid, sizeof(double) * (size_t)n_grid, hipMemcpyHostToDevice) != hipSuccess) {
        fail(MP_EHIP, "mp_create: cannot upload the time grid");
        mp_destroy(h);
        return nullptr;
    }
    mp::DevShared &s = h->sh;
    s.tgrid = h->d_tgrid.p;
    s.n_grid = n_grid;
    s.n_tiles = h->n_tiles;
    s.cfg = *cfg;
    s.n_prior = 0;
    s.log_mask = 0;
    // star constants, magnetar/funcs.py:7-13,75-76
    const double M = 1.4 * mp::kMsol;
    s.GM = mp::kG * M;
    s.inertia = cfg->inertia_factor * M * mp::kR * mp::kR;
    s.inv_inertia = 1.0 / s.inertia;
    const double beta = s.GM / (mp::kR * mp::kC * mp::kC);
    const double modW = 0.6 * M * mp::kC * mp::kC * (beta / (1.0 - 0.5 * beta));
    s.crot = 0.5 * s.inertia / modW;
    s.sqrtGM = std::sqrt(s.GM);
    s.inv_sqrtGM = 1.0 / s.sqrtGM;
    s.sqrtR = std::sqrt(mp::kR);
    s.crm_unit = std::pow(1.0e15 * mp::kR * mp::kR * mp::kR, 4.0 / 7.0) * std::pow(s.GM, -1.0 / 7.0) *
                 std::pow(cfg->rm_massflow_factor, -2.0 / 7.0);
    s.t0 = tgrid[0];
    const double lnq = std::log(tgrid[n_grid - 1] / tgrid[0]) / (double)(n_grid - 1);
    s.lnq8 = lnq / 8.0;
    s.pre_fine = std::min(32, n_grid - 1);                         // oracle/mp_oracle.c MPO_PRE_FINE
    s.sweep_tol = cfg->sweep_tol > 0.0 ? cfg->sweep_tol : MP_SWEEP_TOL_DEFAULT;
    s.stride_tol = cfg->stride_tol > 0.0 ? cfg->stride_tol : MP_STRIDE_TOL_DEFAULT;
    {
        const int ms = cfg->max_stride > 0 ? cfg->max_stride : MP_MAX_STRIDE_DEFAULT;
        s.max_kind = ms == 1 ? 1 : (ms == 2 ? 2 : (ms == 4 ? 3 : 4));
    }
    s.n_simd = std::max(1, prop.multiProcessorCount) * 4;         // 4 SIMDs per CU (1 024 on MI355X)
    s.force_spl = 0;
    s.force_waves = 0;
    // The constants of the stride policy (oracle/mp_oracle.c carries the same ones).  They are not
    // settings: the shipped library takes them from here only, mp_get_policy() reports them.
    s.coarse_max_sweeps = 5;
    s.fine_max_sweeps = 12;                                        // (round 3: 8.  A tile over single intervals that is cut after 8 sweeps
                                                                   // restarts with a fresh extrapolation inside the slow zone -- where the
                                                                   // Jacobian changes from step to step and the converged region grows by
                                                                   // about one lane per sweep -- and the restart can be far worse than going
                                                                   // on: 1 walker in 1 000 prior-wide ones then needed 120 - 160 sweeps in one
                                                                   // tile.  12: worst walker 83 sweeps, means unchanged; profiles/r04_tail.log)
    s.trouble_limit = 2;
    s.early_hold_t = MP_EARLY_HOLD_SECONDS;                       // oracle/mp_oracle.c MPO_EARLY_HOLD_SECONDS
    s.coarse_tol_factor = 0.1;
    s.k4_tol_factor = 0.1;
    s.stop_factor = MP_STOP_FACTOR;                               // (mp_eval.hpp: the end of a tile's sweeps)
#ifdef MP_EXPERIMENTS
    // Developer build only (`make -C magprop_amd/csrc experiments` -> libmagprop_amd_exp.so, selected with MAGPROP_AMD_LIB):
    // environment overrides of the policy constants for A/B runs (tools/).  The shipped library does not read the
    // environment, so no benchmark or soak artefact can be produced with loosened settings and leave no trace
    // (mp_get_policy()[MP_POLICY_EXPERIMENTS] tells the two builds apart; bench.py prints it).
    {
        auto env_i = [](const char *name, int lo, int hi, int32_t &dst) { if (const char *e = std::getenv(name)) { const int v = std::atoi(e); if (v >= lo && v <= hi) dst = v; } };
        auto env_d = [](const char *name, double lo, double hi, double &dst) { if (const char *e = std::getenv(name)) { const double v = std::atof(e); if (v >= lo && v <= hi) dst = v; } };
        if (const char *e = std::getenv("MAGPROP_AMD_MAX_STRIDE")) {
            const int v = std::atoi(e);
            if (v == 1 || v == 2 || v == 4 || v == 8) s.max_kind = v == 1 ? 1 : (v == 2 ? 2 : (v == 4 ? 3 : 4));
        }
        if (const char *e = std::getenv("MAGPROP_AMD_SPL")) { const int v = std::atoi(e); if (v == 2 || v == 4) s.force_spl = v; }
        if (const char *e = std::getenv("MAGPROP_AMD_WAVES")) { const int v = std::atoi(e); if (v == 1 || v == 2 || v == 4) s.force_waves = v; }
        env_d("MAGPROP_AMD_SWEEP_TOL", 1.0e-14, 1.0e-3, s.sweep_tol);       // (the cfg validation range)
        env_d("MAGPROP_AMD_STRIDE_TOL", 1.0e-14, 1.0e-3, s.stride_tol);
        env_d("MAGPROP_AMD_EARLY_HOLD_SECONDS", 0.0, 1.0e6, s.early_hold_t);
        env_i("MAGPROP_AMD_TROUBLE_LIMIT", 0, 1000, s.trouble_limit);
        env_i("MAGPROP_AMD_COARSE_MAX_SWEEPS", 2, 64, s.coarse_max_sweeps);
        env_i("MAGPROP_AMD_FINE_MAX_SWEEPS", 2, 272, s.fine_max_sweeps);
        env_d("MAGPROP_AMD_COARSE_TOL_FACTOR", 1.0e-3, 1.0, s.coarse_tol_factor);
        env_d("MAGPROP_AMD_K4_TOL_FACTOR", 1.0e-3, 1.0, s.k4_tol_factor);
        env_d("MAGPROP_AMD_STOP_FACTOR", 0.0, 1.0, s.stop_factor);        // (0: every tile runs its verification sweep)
    }
#endif
    // Constants of the tile kinds: steps over 1/8, 1, 2, 4, 8 grid intervals (mp_device.h StrideK).
    // Quadrature matrices of the exponential Adams-Moulton formulas on nodes t_{j+1}, t_j, t_{j-1}, ... of a geometric
    // grid of ratio Q (in units of the step, origin t_j: 1, 0, -1/Q, -(1/Q + 1/Q^2), ...):
    // W[k][m] = m! * [theta^m] l_k(theta), l_k the Lagrange basis on the nodes.
    auto quad_weights = [](double Q, int K, double *W) {
        double x[8];
        x[0] = 1.0; x[1] = 0.0;
        { double acc = 0.0, f = 1.0; for (int k = 2; k < K; ++k) { f /= Q; acc -= f; x[k] = acc; } }
        for (int k = 0; k < K; ++k) {
            double co[8] = {1.0, 0, 0, 0, 0, 0, 0, 0};
            int deg = 0;
            double denom = 1.0;
            for (int j = 0; j < K; ++j) {
                if (j == k) continue;
                for (int m = deg + 1; m >= 1; --m) co[m] = co[m - 1] - x[j] * co[m];
                co[0] = -x[j] * co[0];
                ++deg;
                denom *= x[k] - x[j];
            }
            double fact = 1.0;
            for (int m = 0; m < K; ++m) { if (m > 1) fact *= (double)m; W[k * K + m] = fact * co[m] / denom; }
        }
    };
    std::vector<double> wtab((size_t)mp::kWtabSize, 0.0);
    for (int kind = 0; kind < mp::kKinds; ++kind) {
        mp::StrideK &K = s.sk[kind];
        const double lnQ = kind == 0 ? lnq / 8.0 : lnq * (double)(1 << (kind - 1));
        K.lnQ = lnQ;
        K.inv_Q = std::exp(-lnQ);
        K.one_m_invQ = -std::expm1(-lnQ);
        const int ns = kind == 0 ? 1 : (1 << (kind - 1));
        double *T = wtab.data() + (size_t)kind * mp::kWtabStride;
        for (int i = 0; i < 8; ++i)
            T[mp::kWtabTheta + i] = (i < ns && ns > 1) ? std::expm1(lnq * (double)i) / std::expm1(lnQ) : 0.0;
        double W5[25];
        quad_weights(std::exp(lnQ), 5, W5);
        for (int k = 0; k < 5; ++k)
            for (int m = 0; m < 5; ++m) T[6 * k + m] = W5[k * 5 + m];
        // dense output of Mdisc where the step is longer than tvisc (mp_device.h kWtabDense): cubic Lagrange weights at the
        // skipped grid points, the step being the first / middle / last interval of its four nodes (times in units of the
        // step, origin at its start; consecutive steps grow by Q)
        if (kind >= 2) {
            const double Q = std::exp(lnQ);
            const double nodes[3][4] = {{0.0, 1.0, 1.0 + Q, 1.0 + Q + Q * Q},
                                        {-1.0 / Q, 0.0, 1.0, 1.0 + Q},
                                        {-1.0 / Q - 1.0 / (Q * Q), -1.0 / Q, 0.0, 1.0}};
            for (int i = 1; i < ns; ++i) {
                const double th = T[mp::kWtabTheta + i];
                double *D = wtab.data() + mp::kWtabDense + ((kind - 2) * 7 + (i - 1)) * 12;
                for (int v = 0; v < 3; ++v)
                    for (int k = 0; k < 4; ++k) {
                        double l = 1.0;
                        for (int m = 0; m < 4; ++m)
                            if (m != k) l *= (th - nodes[v][m]) / (nodes[v][k] - nodes[v][m]);
                        D[v * 4 + k] = l;
                    }
            }
        }
    }
    // behind it: Q^k of the kinds 1 .. 4 (mp_device.h DevShared::ttab)
    const size_t ttab_off = wtab.size();
    wtab.resize(ttab_off + (size_t)(mp::kKinds - 1) * mp::kTtabN);
    for (int kind = 1; kind < mp::kKinds; ++kind)
        for (int k = 0; k < mp::kTtabN; ++k) wtab[ttab_off + (size_t)(kind - 1) * mp::kTtabN + k] = std::exp((double)k * s.sk[kind].lnQ);
    if (h->d_wtab.ensure(wtab.size()) != MP_OK ||
        hipMemcpy(h->d_wtab.p, wtab.data(), wtab.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
        fail(MP_EHIP, "mp_create: cannot upload the quadrature tables");
        mp_destroy(h);
        return nullptr;
    }
    s.wtab = h->d_wtab.p;
    s.ttab = h->d_wtab.p + ttab_off;
    if (rebuild_datasets(h) != MP_OK) {
        mp_destroy(h);
        return nullptr;
    }
    return h;
}

mp_handle *mp_create_multi(const mp_model_cfg *cfg, const double *tgrid, int n_grid, const int *devices, int n_devices) {
    if (!devices || n_devices < 1 || n_devices > 64) {
        fail(MP_EINVAL, "mp_create_multi: devices NULL or n_devices outside 1..64");
        return nullptr;
    }
    mp_handle *h = new mp_handle();
    for (int g = 0; g < n_devices; ++g) {
        mp_handle *s = mp_create(cfg, tgrid, n_grid, devices[g]);     // (validates cfg / tgrid; its message stays in mp_last_error)
        if (!s) {
            mp_destroy(h);
            return nullptr;
        }
        h->sub.push_back(s);
    }
    h->device = h->sub[0]->device;
    h->tgrid = h->sub[0]->tgrid;
    h->n_tiles = h->sub[0]->n_tiles;
    h->sh = h->sub[0]->sh;          // the scalar settings (policy, tolerances, n_simd of the first device); no device pointer of it is used
    return h;
}

int mp_n_devices(const mp_handle *h) { return h ? (h->sub.empty() ? 1 : (int)h->sub.size()) : 0; }

int mp_destroy(mp_handle *h) {
    if (!h) return MP_OK;
    if (!h->sub.empty()) {
        for (mp_handle *s : h->sub) (void)mp_destroy(s);
        delete h;
        return MP_OK;
    }
    DeviceScope scope(h->device);
    (void)hipDeviceSynchronize();
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;   // (frees the buffers and events, on the handle's device)
    return MP_OK;
}

int mp_set_dataset(mp_handle *h, int ds_id, const double *x, const double *y, const double *yerr, int n_obs) {
    if (!h || !x || !y || !yerr) return fail(MP_EINVAL, "mp_set_dataset: NULL argument");
    if (ds_id < 0 || ds_id >= MP_MAX_DATASETS) return fail(MP_EINVAL, "mp_set_dataset: ds_id %d out of range", ds_id);
    if (n_obs <= 0) return fail(MP_EINVAL, "mp_set_dataset: n_obs must be positive");
    Lock lock(h->mu);
    if (!h->sub.empty()) {
        for (mp_handle *s : h->sub) { const int rc = mp_set_dataset(s, ds_id, x, y, yerr, n_obs); if (rc) return rc; }
        h->sh.n_ds = h->sub[0]->sh.n_ds;
        return MP_OK;
    }
    const std::vector<double> &t = h->tgrid;
    const int n = (int)t.size();
    for (int j = 0; j < n_obs; ++j) {
        if (!(x[j] >= t.front()) || !(x[j] <= t.back()))  // interp1d(bounds_error=True), magnetar/funcs.py:214-215
            return fail(MP_ERANGE, "A value in x_new is %s the interpolation range.",
                        (x[j] < t.front()) ? "below" : "above");
    }
    std::vector<int> order(n_obs);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return x[a] < x[b]; });
    HostDataset d;
    d.set = true;
    d.tile_ptr.assign((size_t)h->n_tiles + 1, 0);
    for (int k = 0; k < n_obs; ++k) {
        const int j = order[k];
        int g = (int)(std::upper_bound(t.begin(), t.end(), x[j]) - t.begin()) - 1;  // t[g] <= x < t[g+1]
        g = std::min(std::max(g, 0), n - 2);
        d.g.push_back(g);
        d.dx.push_back(x[j] - t[g]);
        d.idt.push_back(1.0 / (t[g + 1] - t[g]));
        d.y.push_back(y[j]);
        d.yerr.push_back(yerr[j]);
        d.tile_ptr[(size_t)(g / mp::kTile) + 1] += 1;
    }
    for (size_t k = 1; k < d.tile_ptr.size(); ++k) d.tile_ptr[k] += d.tile_ptr[k - 1];
    const bool replaced = h->ds[ds_id].set;
    h->ds[ds_id] = std::move(d);
    DeviceScope scope(h->device);
    return upload_dataset(h, ds_id, replaced);
}

int mp_set_prior(mp_handle *h, const double *lower, const double *upper, int ndim, uint32_t log_mask) {
    if (!h) return fail(MP_EINVAL, "mp_set_prior: NULL handle");
    if (ndim < 0 || ndim > MP_MAX_NDIM) return fail(MP_EINVAL, "mp_set_prior: ndim %d out of range", ndim);
    if (ndim > 0 && (!lower || !upper)) return fail(MP_EINVAL, "mp_set_prior: NULL bounds");
    Lock lock(h->mu);
    for (mp_handle *s : h->sub) { const int rc = mp_set_prior(s, lower, upper, ndim, log_mask); if (rc) return rc; }
    for (int i = 0; i < MP_MAX_NDIM; ++i) {
        h->sh.lower[i] = i < ndim ? lower[i] : -INFINITY;
        h->sh.upper[i] = i < ndim ? upper[i] : INFINITY;
    }
    h->sh.n_prior = ndim;
    h->sh.log_mask = log_mask;
    return MP_OK;
}

static int check_batch_args(const mp_handle *h, const void *pars, int n, int ndim, const void *lnprob) {
    if (!h || !pars || !lnprob) return fail(MP_EINVAL, "lnprob batch: NULL argument");
    if (n < 0) return fail(MP_EINVAL, "lnprob batch: negative n");
    if (ndim < 6 || ndim > MP_MAX_NDIM) return fail(MP_EINVAL, "lnprob batch: ndim must be 6..9, got %d", ndim);
    if (h->sh.n_ds <= 0) return fail(MP_ESTATE, "lnprob batch: no dataset registered (mp_set_dataset)");
    return MP_OK;
}

int mp_lnprob_batch_dev(mp_handle *h, const double *d_pars, const int32_t *d_ds_id, int n, int ndim,
                        double *d_lnprob, int32_t *d_status, double *d_ltot, void *stream) {
    int rc = check_batch_args(h, d_pars, n, ndim, d_lnprob);
    if (rc) return rc;
    if (!h->sub.empty()) return fail(MP_ESTATE, "mp_lnprob_batch_dev: device pointers belong to ONE device; a multi-device handle serves the host-buffer entries");
    Lock lock(h->mu);
    if (!d_ds_id && !h->ds[0].set) return fail(MP_ESTATE, "lnprob batch: ds_id is NULL but dataset 0 is not set");
    DeviceScope scope(h->device);
    mp::LaunchArgs a{};
    a.pars = d_pars;
    a.ds_id = d_ds_id;
    a.n = n;
    a.ndim = ndim;
    a.physical = 0;
    a.want_chi2 = 1;
    a.lnprob = d_lnprob;
    a.status = d_status;
    a.ltot = d_ltot;
    return launch_lnprob_ordered(h, a, (hipStream_t)stream);
}

// The host-buffer batch in two halves, so that a multi-device handle can have every device's launch in flight before it
// waits for the first: batch_begin stages the rows and enqueues the kernel on the handle's stream, batch_end waits and
// hands the results over.  (Caller holds h->mu and has validated the arguments.)
static int batch_begin(mp_handle *h, const double *pars, const int32_t *ds_id, int n, int ndim, double *ltot_out) {
    int rc;
    DeviceScope scope(h->device);
    const size_t ng = h->tgrid.size();
    // One page-locked staging block owned by the handle, mapped into the device's address space: [pars n*ndim f64 | ds_id n i32]
    // in, [lnprob n f64 | status n i32 | sweeps n i32 | tiles n i32] out.  The kernel reads a walker's 48 - 72 bytes and writes
    // its 20 bytes IN PLACE over PCIe (round 5): no copy command either way -- one launch and one wait per call where the
    // two asynchronous copies around the kernel cost as much as the kernel itself.
    const size_t in_pars = sizeof(double) * (size_t)n * ndim, in_ids = ds_id ? sizeof(int32_t) * (size_t)n : 0;
    const size_t in_bytes = (in_pars + in_ids + 7) & ~(size_t)7;
    const size_t out_bytes = (sizeof(double) + 4 * sizeof(int32_t)) * (size_t)n;   // lnprob | status | sweeps | tiles (+ pad)
    if ((rc = h->h_io.ensure(in_bytes + out_bytes)) || (ltot_out && (rc = h->w_curves.ensure((size_t)n * ng))))
        return rc;
    hipStream_t st = h->stream;
    std::memcpy(h->h_io.p, pars, in_pars);
    if (ds_id) std::memcpy(h->h_io.p + in_pars, ds_id, in_ids);
    unsigned char *d_out = h->h_io.dev + in_bytes;
    mp::LaunchArgs a{};
    a.pars = (const double *)h->h_io.dev;
    a.ds_id = ds_id ? (const int32_t *)(h->h_io.dev + in_pars) : nullptr;
    a.n = n;
    a.ndim = ndim;
    a.physical = 0;
    a.want_chi2 = 1;
    a.lnprob = (double *)d_out;
    a.status = (int32_t *)(d_out + sizeof(double) * (size_t)n);
    a.sweeps = a.status + n;
    a.tiles = a.sweeps + n;
    a.ltot = ltot_out ? h->w_curves.p : nullptr;   // rows of walkers that fail are NaN-filled by the kernel
    if (h->tile_log_on) {
        if ((rc = h->w_tile_log.ensure((size_t)n * MP_TILE_LOG))) return rc;
        HIP_TRY(hipMemsetAsync(h->w_tile_log.p, 0xFF, (size_t)n * MP_TILE_LOG * sizeof(int32_t), st));
        a.tile_log = h->w_tile_log.p;
    }
    if ((rc = launch_lnprob_ordered(h, a, st))) return rc;
    if (h->tile_log_on) {
        h->last_tile_log.resize((size_t)n * MP_TILE_LOG);
        HIP_TRY(hipMemcpyAsync(h->last_tile_log.data(), h->w_tile_log.p, (size_t)n * MP_TILE_LOG * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    } else h->last_tile_log.clear();
    if (ltot_out)
        HIP_TRY(hipMemcpyAsync(ltot_out, h->w_curves.p, sizeof(double) * (size_t)n * ng, hipMemcpyDeviceToHost, st));
    h->pend_n = n;
    h->pend_in_bytes = in_bytes;
    return MP_OK;
}

static int batch_end(mp_handle *h, double *lnprob_out, int32_t *status_out) {
    DeviceScope scope(h->device);
    const int n = h->pend_n;
    HIP_TRY(hipStreamSynchronize(h->stream));
    const unsigned char *h_out = h->h_io.p + h->pend_in_bytes;
    std::memcpy(lnprob_out, h_out, sizeof(double) * (size_t)n);
    const int32_t *status = (const int32_t *)(h_out + sizeof(double) * (size_t)n), *sweeps = status + n, *tiles = sweeps + n;
    if (status_out) std::memcpy(status_out, status, sizeof(int32_t) * (size_t)n);
    double tot = 0.0, tot_tiles = 0.0;
    int cnt = 0;
    h->last_sweeps.assign(sweeps, sweeps + n);
    h->last_tiles.assign(tiles, tiles + n);
    for (int i = 0; i < n; ++i)
        if (status[i] == MP_STATUS_OK) { tot += sweeps[i]; tot_tiles += tiles[i]; ++cnt; }
    h->last_tot_sweeps = tot; h->last_tot_tiles = tot_tiles; h->last_cnt_ok = cnt;
    h->last_mean_sweeps = tot_tiles > 0.0 ? tot / tot_tiles : 0.0;
    h->last_mean_tiles = cnt ? tot_tiles / (double)cnt : 0.0;
    return MP_OK;
}

int mp_lnprob_batch(mp_handle *h, const double *pars, const int32_t *ds_id, int n, int ndim, double *lnprob_out,
                    int32_t *status_out, double *ltot_out) {
    int rc = check_batch_args(h, pars, n, ndim, lnprob_out);
    if (rc) return rc;
    if (n == 0) return MP_OK;
    Lock lock(h->mu);
    const mp_handle *hd = h->sub.empty() ? h : h->sub[0];     // (the datasets of a multi-device handle live in its evaluators)
    if (ds_id) {
        for (int i = 0; i < n; ++i)
            if (ds_id[i] < 0 || ds_id[i] >= MP_MAX_DATASETS || !hd->ds[ds_id[i]].set)
                return fail(MP_EINVAL, "lnprob batch: walker %d refers to unset dataset %d", i, ds_id[i]);
    } else if (!hd->ds[0].set) {
        return fail(MP_ESTATE, "lnprob batch: ds_id is NULL but dataset 0 is not set");
    }
    if (h->sub.empty()) {
        if ((rc = batch_begin(h, pars, ds_id, n, ndim, ltot_out))) return rc;
        return batch_end(h, lnprob_out, status_out);
    }
    // Multi-device: contiguous blocks of ceil(n / G) rows (SURVEY.md 8(e)'s partitioning), every device's kernel enqueued before
    // the first is waited for; one host thread drives them all (a launch returns in microseconds, the kernels run side by side).
    const int G = (int)h->sub.size(), per = (n + G - 1) / G;
    const size_t ng = h->tgrid.size();
    int used = 0;
    for (int g = 0; g < G; ++g) {
        const int lo = std::min(g * per, n), cnt = std::min(lo + per, n) - lo;
        if (cnt <= 0) break;
        mp_handle *s = h->sub[(size_t)g];
        Lock sl(s->mu);
        if ((rc = batch_begin(s, pars + (size_t)lo * ndim, ds_id ? ds_id + lo : nullptr, cnt, ndim, ltot_out ? ltot_out + (size_t)lo * ng : nullptr))) {
            for (int k = 0; k < used; ++k) (void)hipStreamSynchronize(h->sub[(size_t)k]->stream);   // nothing may still write the caller's buffers
            return rc;
        }
        ++used;
    }
    int first_rc = MP_OK;
    h->last_sweeps.clear();
    h->last_tiles.clear();
    double tot = 0.0, tot_tiles = 0.0;
    int cnt_ok = 0;
    for (int g = 0; g < used; ++g) {
        mp_handle *s = h->sub[(size_t)g];
        const int lo = g * per;
        Lock sl(s->mu);
        rc = batch_end(s, lnprob_out + lo, status_out ? status_out + lo : nullptr);
        if (rc && !first_rc) first_rc = rc;
        h->last_sweeps.insert(h->last_sweeps.end(), s->last_sweeps.begin(), s->last_sweeps.end());
        h->last_tiles.insert(h->last_tiles.end(), s->last_tiles.begin(), s->last_tiles.end());
        tot += s->last_tot_sweeps; tot_tiles += s->last_tot_tiles; cnt_ok += s->last_cnt_ok;
    }
    if (first_rc) return first_rc;
    h->last_mean_sweeps = tot_tiles > 0.0 ? tot / tot_tiles : 0.0;
    h->last_mean_tiles = cnt_ok ? tot_tiles / (double)cnt_ok : 0.0;
    return MP_OK;
}

int mp_model_lc(mp_handle *h, const double *pars, int ndim, double *out, double *traj, int32_t *status) {
    if (!h || !pars || !out) return fail(MP_EINVAL, "mp_model_lc: NULL argument");
    if (ndim < 6 || ndim > MP_MAX_NDIM) return fail(MP_EINVAL, "mp_model_lc: ndim must be 6..9, got %d", ndim);
    if (!h->sub.empty()) return mp_model_lc(h->sub[0], pars, ndim, out, traj, status);   // one walker: the first device
    Lock lock(h->mu);
    DeviceScope scope(h->device);
    const size_t ng = h->tgrid.size();
    int rc;
    if ((rc = h->w_pars.ensure(MP_MAX_NDIM)) || (rc = h->w_lnprob.ensure(1)) || (rc = h->w_status.ensure(1)) ||
        (rc = h->w_curves.ensure(5 * ng)))
        return rc;
    hipStream_t st = h->stream;
    HIP_TRY(hipMemcpyAsync(h->w_pars.p, pars, sizeof(double) * (size_t)ndim, hipMemcpyHostToDevice, st));
    mp::LaunchArgs a{};
    a.pars = h->w_pars.p;
    a.n = 1;
    a.ndim = ndim;
    a.physical = 1;
    a.want_chi2 = 0;
    a.lnprob = h->w_lnprob.p;
    a.status = h->w_status.p;
    a.ltot = h->w_curves.p;
    a.lprop = h->w_curves.p + ng;
    a.ldip = h->w_curves.p + 2 * ng;
    a.mdisc = h->w_curves.p + 3 * ng;
    a.omega = h->w_curves.p + 4 * ng;
    if ((rc = launch_lnprob_ordered(h, a, st))) return rc;
    int32_t stt = 0;
    std::memcpy(out, h->tgrid.data(), sizeof(double) * ng);
    HIP_TRY(hipMemcpyAsync(out + ng, h->w_curves.p, sizeof(double) * 3 * ng, hipMemcpyDeviceToHost, st));
    if (traj) HIP_TRY(hipMemcpyAsync(traj, h->w_curves.p + 3 * ng, sizeof(double) * 2 * ng, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&stt, h->w_status.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (status) *status = stt;
    return MP_OK;
}

int mp_model_band(mp_handle *h, const double *pars, int n, int ndim, int physical, const double *q, int nq, uint32_t components,
                  double *band_out, int32_t *status_out, int32_t *n_used) {
    if (!h || !pars || !q || !band_out) return fail(MP_EINVAL, "mp_model_band: NULL argument");
    if (n < 1 || n > MP_BAND_MAX_SAMPLES) return fail(MP_EINVAL, "mp_model_band: n must be 1..%d (MP_BAND_MAX_SAMPLES), got %d", MP_BAND_MAX_SAMPLES, n);
    if (ndim < 6 || ndim > MP_MAX_NDIM) return fail(MP_EINVAL, "mp_model_band: ndim must be 6..9, got %d", ndim);
    if (nq < 1 || nq > MP_BAND_MAX_Q) return fail(MP_EINVAL, "mp_model_band: nq must be 1..%d (MP_BAND_MAX_Q), got %d", MP_BAND_MAX_Q, nq);
    for (int j = 0; j < nq; ++j)
        if (!(q[j] >= 0.0 && q[j] <= 1.0)) return fail(MP_EINVAL, "mp_model_band: q[%d] = %g is not in [0, 1]", j, q[j]);
    const uint32_t all = MP_BAND_LTOT | MP_BAND_LPROP | MP_BAND_LDIP;
    if (components == 0 || (components & ~all)) return fail(MP_EINVAL, "mp_model_band: components 0x%x is not a non-empty mask of MP_BAND_*", components);
    if (!h->sub.empty()) return mp_model_band(h->sub[0], pars, n, ndim, physical, q, nq, components, band_out, status_out, n_used);
    Lock lock(h->mu);
    DeviceScope scope(h->device);
    const size_t ng = h->tgrid.size(), rows = (size_t)n * ng;
    const int ncomp = __builtin_popcount(components);
    int rc;
    if ((rc = h->w_pars.ensure((size_t)n * ndim)) || (rc = h->w_lnprob.ensure((size_t)n)) || (rc = h->w_status.ensure((size_t)n)) ||
        (rc = h->w_band.ensure(rows * (size_t)(ncomp + 1))) || (rc = h->w_band_out.ensure((size_t)ncomp * nq * ng)))
        return rc;
    hipStream_t st = h->stream;
    HIP_TRY(hipMemcpyAsync(h->w_pars.p, pars, sizeof(double) * (size_t)n * ndim, hipMemcpyHostToDevice, st));
    mp::LaunchArgs a{};
    a.pars = h->w_pars.p;
    a.n = n;
    a.ndim = ndim;
    a.physical = physical ? 1 : 0;
    a.want_chi2 = 0;                          // curves only: no dataset needed
    a.lnprob = h->w_lnprob.p;
    a.status = h->w_status.p;
    double *curve[3] = {nullptr, nullptr, nullptr};
    for (int c = 0, k = 0; c < 3; ++c)
        if (components & (1u << c)) curve[c] = h->w_band.p + (size_t)k++ * rows;
    a.ltot = curve[0];                        // rows of walkers that did not finish are NaN-filled by the kernel
    a.lprop = curve[1];
    a.ldip = curve[2];
    if ((rc = launch_lnprob_ordered(h, a, st))) return rc;
    mp::BandQ bq{};
    for (int j = 0; j < nq; ++j) bq.q[j] = q[j];
    bq.nq = nq;
    double *cols = h->w_band.p + (size_t)ncomp * rows;
    for (int c = 0, k = 0; c < 3; ++c) {
        if (!curve[c]) continue;
        int e = mp::launch_band_transpose(curve[c], cols, n, (int)ng, (void *)st);
        if (!e) e = mp::launch_band_select(cols, n, (int)ng, bq, h->w_band_out.p + (size_t)k * nq * ng, (void *)st);
        if (e) return fail(MP_EHIP, "band kernel launch failed: %s", hipGetErrorString((hipError_t)e));
        ++k;
    }
    std::vector<int32_t> stt((size_t)n);
    HIP_TRY(hipMemcpyAsync(band_out, h->w_band_out.p, sizeof(double) * (size_t)ncomp * nq * ng, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(stt.data(), h->w_status.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (status_out) std::memcpy(status_out, stt.data(), sizeof(int32_t) * (size_t)n);
    if (n_used) *n_used = (int32_t)std::count(stt.begin(), stt.end(), (int32_t)MP_STATUS_OK);
    return MP_OK;
}

int mp_rhs_batch(mp_handle *h, const double *pars, int ndim, const double *t, const double *y, int n, double *dydt,
                 double *lam) {
    if (!h || !pars || !t || !y || !dydt) return fail(MP_EINVAL, "mp_rhs_batch: NULL argument");
    if (ndim < 6 || ndim > MP_MAX_NDIM) return fail(MP_EINVAL, "mp_rhs_batch: ndim must be 6..9, got %d", ndim);
    if (n < 0) return fail(MP_EINVAL, "mp_rhs_batch: negative n");
    if (n == 0) return MP_OK;
    if (!h->sub.empty()) return mp_rhs_batch(h->sub[0], pars, ndim, t, y, n, dydt, lam);
    Lock lock(h->mu);
    DeviceScope scope(h->device);
    // one device block: [pars n*ndim | t n | y 2n] in, [dydt 2n | lam n] out
    const size_t n_in = (size_t)n * (ndim + 3), n_out = (size_t)n * 3;
    int rc;
    if ((rc = h->w_curves.ensure(n_in + n_out))) return rc;
    double *d = h->w_curves.p;
    hipStream_t st = h->stream;
    HIP_TRY(hipMemcpyAsync(d, pars, sizeof(double) * (size_t)n * ndim, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d + (size_t)n * ndim, t, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d + (size_t)n * (ndim + 1), y, sizeof(double) * 2 * (size_t)n, hipMemcpyHostToDevice, st));
    mp::RhsArgs r{};
    r.pars = d;
    r.t = d + (size_t)n * ndim;
    r.y = d + (size_t)n * (ndim + 1);
    r.dydt = d + n_in;
    r.lam = d + n_in + 2 * (size_t)n;
    r.n = n;
    r.ndim = ndim;
    const int e = mp::launch_rhs(h->sh, r, st);
    if (e) return fail(MP_EHIP, "kernel launch failed: %s", hipGetErrorString((hipError_t)e));
    HIP_TRY(hipMemcpyAsync(dydt, r.dydt, sizeof(double) * 2 * (size_t)n, hipMemcpyDeviceToHost, st));
    if (lam) HIP_TRY(hipMemcpyAsync(lam, r.lam, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return MP_OK;
}

int mp_synchronize(mp_handle *h) {
    if (!h) return fail(MP_EINVAL, "mp_synchronize: NULL handle");
    Lock lock(h->mu);
    if (!h->sub.empty()) {
        for (mp_handle *s : h->sub) { const int rc = mp_synchronize(s); if (rc) return rc; }
        return MP_OK;
    }
    DeviceScope scope(h->device);
    HIP_TRY(hipStreamSynchronize(h->stream));
    return MP_OK;
}

// ---------------------------------------------------------------- ensemble sampler (stretch move)
struct mp_sampler {
    mp_handle *h = nullptr;
    int n_walkers = 0, n_ensembles = 0, n_total = 0, ndim = 0, target = 0;
    uint64_t seed = 0;
    double a = 2.0;
    uint64_t steps_done = 0;
    bool have_state = false;
    DevBuf<double> d_pos, d_lnprob, d_chain, d_chain_lnp, d_bad, d_spec;
    std::vector<int32_t> ens_ds;   // dataset of every ensemble
    int whole_step = 1;   // mp_sampler_run: one launch per step where the ensemble is small enough (mp_sampler_set_whole_step)
    DevBuf<int64_t> d_acc;
    DevBuf<int32_t> d_perm, d_dsid, d_status;
    DevBuf<uint32_t> d_bad_count;
    PinnedBuf h_perm;   // page-locked staging of the random splits: their upload overlaps the running half-steps
    // walker-sharded driving (mp_sampler_halfstep_shard / _apply): splits of kWin steps at a time, double-buffered
    static constexpr int kWin = 32;
    DevBuf<int32_t> d_win[2];
    PinnedBuf h_win[2];
    Event win_copied[2];
    int64_t win_id[2] = {-1, -1};
    bool ext_stream_work = false;   // half-steps were enqueued on a caller's stream since the last device-wide wait
    // failed proposals (the reference's fbad file): the device window d_bad is drained into this log
    std::vector<double> bad_log;    // [rows][ndim]
    int64_t n_bad = 0;              // exact count since creation (rows beyond the window between two drains are counted, not kept)
    // parallel tempering (mp_sampler_set_temperatures): ensemble e runs at beta[e % n_temps]; 0 = untempered
    int n_temps = 0;
    DevBuf<double> d_beta;          // [n_ensembles]
    DevBuf<int64_t> d_swaps;        // [n_ensembles / n_temps][n_temps - 1] accepted swaps
    // proposal moves (mp_sampler_set_moves); empty: the stretch move with scale a
    struct Move {
        int32_t kind;
        double p0, p1;              // stretch: a; DE: g0 (resolved), s = sigma sqrt(3); snooker: gamma_s; KDE: f (resolved)
    };
    std::vector<Move> moves;
    std::vector<double> move_cum;   // cumulative weights, summed in order
};

// Move the device window of failed proposals into the host log and reset it.  The caller has made sure that no kernel
// of this sampler is in flight.
static int drain_bad(mp_sampler *s) {
    uint32_t cnt = 0;
    HIP_TRY(hipMemcpy(&cnt, s->d_bad_count.p, sizeof cnt, hipMemcpyDeviceToHost));
    if (cnt == 0) return MP_OK;
    const size_t cap = s->d_bad.cap / (size_t)s->ndim, rows = std::min<size_t>(cnt, cap);
    const size_t old = s->bad_log.size();
    s->bad_log.resize(old + rows * (size_t)s->ndim);
    HIP_TRY(hipMemcpy(s->bad_log.data() + old, s->d_bad.p, rows * s->ndim * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemset(s->d_bad_count.p, 0, sizeof(uint32_t)));
    s->n_bad += (int64_t)cnt;
    return MP_OK;
}

// random split of every ensemble for step `step` (emcee's randomize_split): Fisher-Yates, counter (step, ensemble, i, 'split')
static void draw_split(const mp_sampler *s, uint64_t step64, int32_t *perm) {
    const uint32_t step = (uint32_t)step64;
    for (int e = 0; e < s->n_ensembles; ++e) {
        int32_t *p = perm + (size_t)e * s->n_walkers;
        std::iota(p, p + s->n_walkers, 0);
        for (int i = s->n_walkers - 1; i > 0; --i) {
            uint32_t r[4];
            mp::philox4x32_10((uint32_t)s->seed, (uint32_t)(s->seed >> 32), step, (uint32_t)e, (uint32_t)i, 0x5117u, r);
            const uint64_t r64 = ((uint64_t)r[0] << 32) | r[1];
            std::swap(p[i], p[(size_t)(r64 % (uint64_t)(i + 1))]);
        }
    }
}

// splits of `count` consecutive steps into perm[count][n_total]; the steps are independent (counter-based generator), so
// large ensembles are drawn by a few host threads (8 192 walkers: 0.4 ms per step on one core, more than a half-step of a
// walker-sharded ensemble takes on the GPU)
static void draw_splits(const mp_sampler *s, uint64_t step0, int count, int32_t *perm) {
    const size_t nt = (size_t)s->n_total;
    const int n_thr = (int)std::min<size_t>({(size_t)count, (size_t)4, (nt * (size_t)count) / 8192});
    auto work = [&](int first, int stride) {
        for (int i = first; i < count; i += stride) draw_split(s, step0 + (uint64_t)i, perm + (size_t)i * nt);
    };
    if (n_thr <= 1) { work(0, 1); return; }
    std::vector<std::thread> pool;
    for (int k = 1; k < n_thr; ++k) pool.emplace_back(work, k, n_thr);
    work(0, n_thr);
    for (auto &th : pool) th.join();
}

// the move of step `step` (an index into s->moves): r = Philox(seed; step, 3, 0, 0x30FE), the first m with u01(r0, r1) C_last < C_m
static int draw_move(const mp_sampler *s, uint64_t step64) {
    const int n = (int)s->moves.size();
    if (n <= 1) return 0;
    uint32_t r[4];
    mp::philox4x32_10((uint32_t)s->seed, (uint32_t)(s->seed >> 32), (uint32_t)step64, 3u, 0u, 0x30FEu, r);
    const double x = mp::u01(r[0], r[1]) * s->move_cum[(size_t)n - 1];
    for (int m = 0; m < n - 1; ++m)
        if (x < s->move_cum[(size_t)m]) return m;
    return n - 1;
}

static mp::StretchArgs stretch_args(const mp_sampler *s, const int32_t *d_perm, uint64_t step, int half) {
    mp::StretchArgs g{};
    g.pos = s->d_pos.p; g.lnprob = s->d_lnprob.p; g.n_accepted = s->d_acc.p;
    g.perm = d_perm;
    g.ds_id = s->d_dsid.p;
    g.n_walkers = s->n_walkers; g.n_half = s->n_walkers / 2; g.n_ensembles = s->n_ensembles;
    g.n_total = s->n_total; g.ndim = s->ndim; g.half = half; g.target = s->target;
    g.step = (uint32_t)step; g.seed = s->seed; g.a = s->a;
    g.bad_log = s->d_bad.p; g.bad_count = s->d_bad_count.p; g.bad_cap = (uint32_t)(s->d_bad.cap / (size_t)std::max(s->ndim, 1));
    g.beta = s->n_temps ? s->d_beta.p : nullptr;
    // Ensembles on light curves of different lengths (BASELINE config 5: 50 / 410 / 8 / 1 944 points): the half-step launch
    // starts the ensemble with the longest light curve first, so that its waves do not begin last and finish alone.  The order
    // is a function of the datasets only, so every rank of a walker-sharded run derives the same one.
    if (s->target == 0 && s->n_ensembles > 1 && s->n_ensembles <= 16) {
        int idx[16];
        std::iota(idx, idx + s->n_ensembles, 0);
        std::stable_sort(idx, idx + s->n_ensembles, [&](int x, int y) {
            return s->h->ds[s->ens_ds[(size_t)x]].g.size() > s->h->ds[s->ens_ds[(size_t)y]].g.size();
        });
        bool identity = true;
        for (int e = 0; e < s->n_ensembles; ++e) identity = identity && idx[e] == e;
        if (!identity)
            for (int e = 0; e < s->n_ensembles; ++e) g.ens_order |= (uint64_t)idx[e] << (4 * e);
    }
    return g;
}

mp_sampler *mp_sampler_create(mp_handle *h, int n_walkers, int n_ensembles, int ndim, const int32_t *ens_ds_id,
                              uint64_t seed, double a, int target) {
    if (!h) { fail(MP_EINVAL, "mp_sampler_create: NULL handle"); return nullptr; }
    Lock lock(h->mu);
    const int rc = check_create(h, "mp_sampler_create", "the device-resident sampler lives on ONE device (walker sharding across devices: magprop_amd/distributed.py)",
                                ndim, target, "ensemble", n_ensembles, ens_ds_id, [&] {
        if (n_walkers < 2 || (n_walkers & 1)) return fail(MP_EINVAL, "mp_sampler_create: n_walkers must be even and >= 2");
        if (n_ensembles < 1) return fail(MP_EINVAL, "mp_sampler_create: bad n_ensembles");
        if (!(a > 1.0)) return fail(MP_EINVAL, "mp_sampler_create: stretch scale a must exceed 1");
        return MP_OK;
    });
    if (rc) return nullptr;
    mp_sampler *s = new mp_sampler();
    s->h = h; s->n_walkers = n_walkers; s->n_ensembles = n_ensembles; s->n_total = n_walkers * n_ensembles;
    s->ndim = ndim; s->target = target; s->seed = seed; s->a = a;
    DeviceScope scope(h->device);
    const size_t nt = (size_t)s->n_total;
    for (int e = 0; e < n_ensembles; ++e) s->ens_ds.push_back(ens_ds_id ? ens_ds_id[e] : 0);
    constexpr size_t kBadRows = MP_BAD_WINDOW;   // device window of failed proposals between two drains (drain_bad)
    if (s->d_pos.ensure(nt * ndim) || s->d_lnprob.ensure(nt) || s->d_acc.ensure(nt) || s->d_dsid.ensure(nt) ||
        s->d_status.ensure(nt) || s->d_bad.ensure(kBadRows * ndim) || s->d_bad_count.ensure(1) ||
        upload_ds_rows(s->d_dsid.p, ens_ds_id, n_ensembles, n_walkers) ||
        hipMemset(s->d_acc.p, 0, nt * sizeof(int64_t)) != hipSuccess ||
        hipMemset(s->d_bad_count.p, 0, sizeof(uint32_t)) != hipSuccess ||
        hipEventCreateWithFlags(&s->win_copied[0].e, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&s->win_copied[1].e, hipEventDisableTiming) != hipSuccess) {
        fail(MP_EHIP, "mp_sampler_create: device allocation failed");
        mp_sampler_destroy(s);
        return nullptr;
    }
    return s;
}

int mp_sampler_destroy(mp_sampler *s) {
    if (!s) return MP_OK;
    Lock lock(s->h->mu);
    DeviceScope scope(s->h->device);
    (void)hipDeviceSynchronize();
    delete s;
    return MP_OK;
}

int mp_sampler_set_temperatures(mp_sampler *s, int n_temps, const double *betas) {
    if (!s || !betas) return fail(MP_EINVAL, "mp_sampler_set_temperatures: NULL argument");
    Lock lock(s->h->mu);
    if (s->have_state) return fail(MP_ESTATE, "mp_sampler_set_temperatures: call it before the first mp_sampler_set_positions");
    if (n_temps < 2) return fail(MP_EINVAL, "mp_sampler_set_temperatures: a ladder needs at least 2 temperatures, got %d", n_temps);
    if (s->n_ensembles % n_temps) return fail(MP_EINVAL, "mp_sampler_set_temperatures: %d ensembles are not groups of %d temperatures", s->n_ensembles, n_temps);
    if (betas[0] != 1.0) return fail(MP_EINVAL, "mp_sampler_set_temperatures: betas[0] must be 1, got %g", betas[0]);
    for (int t = 1; t < n_temps; ++t)
        // (beta = 0 is refused: failed models have lnprob = -inf, and 0 x -inf is NaN)
        if (!std::isfinite(betas[t]) || !(betas[t] > 0.0) || !(betas[t] < betas[t - 1]))
            return fail(MP_EINVAL, "mp_sampler_set_temperatures: betas must be finite, > 0 and strictly decreasing (betas[%d] = %g)", t, betas[t]);
    for (int e = 0; e < s->n_ensembles; ++e)
        if (s->ens_ds[(size_t)e] != s->ens_ds[(size_t)(e - e % n_temps)])
            return fail(MP_EINVAL, "mp_sampler_set_temperatures: ensembles %d and %d of one group have different datasets", e - e % n_temps, e);
    DeviceScope scope(s->h->device);
    std::vector<double> b((size_t)s->n_ensembles);
    for (int e = 0; e < s->n_ensembles; ++e) b[(size_t)e] = betas[e % n_temps];
    const size_t n_pairs = (size_t)(s->n_ensembles / n_temps) * (size_t)(n_temps - 1);
    int rc;
    if ((rc = s->d_beta.ensure(b.size())) || (rc = s->d_swaps.ensure(n_pairs))) return rc;
    HIP_TRY(hipMemcpy(s->d_beta.p, b.data(), b.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(s->d_swaps.p, 0, n_pairs * sizeof(int64_t)));
    s->n_temps = n_temps;
    return MP_OK;
}

int mp_sampler_set_moves(mp_sampler *s, int n_moves, const int32_t *kinds, const double *weights, const double *params) {
    if (!s) return fail(MP_EINVAL, "mp_sampler_set_moves: NULL sampler");
    if (n_moves < 0 || n_moves > MP_MAX_MOVES) return fail(MP_EINVAL, "mp_sampler_set_moves: n_moves must be in [0, %d], got %d", MP_MAX_MOVES, n_moves);
    if (n_moves > 0 && (!kinds || !weights || !params)) return fail(MP_EINVAL, "mp_sampler_set_moves: NULL argument");
    const int n_half = s->n_walkers / 2;
    std::vector<mp_sampler::Move> mv;
    std::vector<double> cum;
    double c = 0.0;
    for (int m = 0; m < n_moves; ++m) {
        const double w = weights[m], p0 = params[2 * m], p1 = params[2 * m + 1];
        if (!std::isfinite(w) || !(w > 0.0)) return fail(MP_EINVAL, "mp_sampler_set_moves: weight %d must be finite and > 0, got %g", m, w);
        mp_sampler::Move x{kinds[m], 0.0, 0.0};
        switch (kinds[m]) {
        case MP_MOVE_STRETCH:
            if (!std::isfinite(p0) || !(p0 > 1.0)) return fail(MP_EINVAL, "mp_sampler_set_moves: stretch scale a must be finite and > 1, got %g", p0);
            x.p0 = p0;
            break;
        case MP_MOVE_DE:
            if (!std::isfinite(p0) || p0 < 0.0) return fail(MP_EINVAL, "mp_sampler_set_moves: DE g0 must be finite and >= 0 (0: 2.38/sqrt(2 ndim)), got %g", p0);
            if (!(p1 >= 0.0) || !(p1 * std::sqrt(3.0) < 1.0)) return fail(MP_EINVAL, "mp_sampler_set_moves: DE sigma must be in [0, 1/sqrt(3)), got %g", p1);
            if (n_half < 2) return fail(MP_EINVAL, "mp_sampler_set_moves: the DE move needs n_walkers >= 4 (two partners in the other half)");
            x.p0 = p0 > 0.0 ? p0 : 2.38 / std::sqrt(2.0 * s->ndim);
            x.p1 = p1 * std::sqrt(3.0);
            break;
        case MP_MOVE_SNOOKER:
            if (!std::isfinite(p0) || !(p0 > 0.0)) return fail(MP_EINVAL, "mp_sampler_set_moves: snooker gamma_s must be finite and > 0, got %g", p0);
            if (n_half < 3) return fail(MP_EINVAL, "mp_sampler_set_moves: the snooker move needs n_walkers >= 6 (three partners in the other half)");
            x.p0 = p0;
            break;
        case MP_MOVE_KDE: {
            const int n_comp = s->n_walkers - n_half, d = s->ndim;
            if (!(p0 == 0.0 || p0 == -1.0 || (std::isfinite(p0) && p0 > 0.0)))
                return fail(MP_EINVAL, "mp_sampler_set_moves: KDE bandwidth must be 0 (Scott), -1 (Silverman) or a finite factor > 0, got %g", p0);
            if (p1 != 0.0) return fail(MP_EINVAL, "mp_sampler_set_moves: KDE params[1] must be 0, got %g", p1);
            if (n_comp < d + 1)
                return fail(MP_EINVAL, "mp_sampler_set_moves: the KDE move needs n_walkers - n_walkers / 2 >= ndim + 1 (a full-rank covariance of the other half), got %d", n_comp);
            // scipy.stats.gaussian_kde's scotts_factor / silverman_factor with neff = n_comp
            x.p0 = p0 > 0.0 ? p0 : std::pow(p0 == 0.0 ? (double)n_comp : n_comp * (d + 2.0) / 4.0, -1.0 / (d + 4));
            break;
        }
        default:
            return fail(MP_EINVAL, "mp_sampler_set_moves: unknown move kind %d", (int)kinds[m]);
        }
        mv.push_back(x);
        c += w;
        cum.push_back(c);
    }
    Lock lock(s->h->mu);
    s->moves = std::move(mv);
    s->move_cum = std::move(cum);
    return MP_OK;
}

int mp_sampler_get_swaps(mp_sampler *s, int64_t *n_swaps_accepted) {
    if (!s || !n_swaps_accepted) return fail(MP_EINVAL, "mp_sampler_get_swaps: NULL argument");
    Lock lock(s->h->mu);
    if (!s->n_temps) return fail(MP_ESTATE, "mp_sampler_get_swaps: the sampler is not tempered (mp_sampler_set_temperatures)");
    DeviceScope scope(s->h->device);
    HIP_TRY(hipDeviceSynchronize());
    const size_t n_pairs = (size_t)(s->n_ensembles / s->n_temps) * (size_t)(s->n_temps - 1);
    HIP_TRY(hipMemcpy(n_swaps_accepted, s->d_swaps.p, n_pairs * sizeof(int64_t), hipMemcpyDeviceToHost));
    return MP_OK;
}

int mp_sampler_set_positions(mp_sampler *s, const double *pos) {
    if (!s || !pos) return fail(MP_EINVAL, "mp_sampler_set_positions: NULL argument");
    mp_handle *h = s->h;
    Lock lock(h->mu);
    DeviceScope scope(h->device);
    const size_t nt = (size_t)s->n_total;
    for (size_t i = 0; i < nt * s->ndim; ++i)
        if (!std::isfinite(pos[i])) return fail(MP_EINVAL, "mp_sampler_set_positions: non-finite coordinate");
    HIP_TRY(hipDeviceSynchronize());   // the sharded entry points may have work in flight on a caller's stream
    s->ext_stream_work = false;
    HIP_TRY(hipMemcpyAsync(s->d_pos.p, pos, nt * s->ndim * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (s->target == 1) {
        std::vector<double> lp(nt, 0.0);
        for (size_t k = 0; k < nt; ++k)
            for (int i = 0; i < s->ndim; ++i) lp[k] -= 0.5 * pos[k * s->ndim + i] * pos[k * s->ndim + i];
        HIP_TRY(hipMemcpyAsync(s->d_lnprob.p, lp.data(), nt * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
    } else {
        mp::LaunchArgs a{};
        a.pars = s->d_pos.p; a.ds_id = s->d_dsid.p; a.n = s->n_total; a.ndim = s->ndim; a.want_chi2 = 1;
        a.lnprob = s->d_lnprob.p; a.status = s->d_status.p;
        const int rc = launch_lnprob_ordered(h, a, h->stream);
        if (rc) return rc;
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    s->have_state = true;
    return MP_OK;
}

// Enqueue step steps_done + row of mp_sampler_run on the handle's stream: split d_perm, chain row `row` of the device slab when
// chain is set, move mv (nullptr: the stretch move of mp_sampler_create).  A whole step per launch (stretch_step_kernel and the
// commit kernel) where `whole` and the move is the stretch move, else two half-step launches; then the swap sweep when tempered.
static int enqueue_step(mp_sampler *s, const int32_t *d_perm, int row, const mp_sampler::Move *mv, bool chain, bool whole) {
    mp_handle *h = s->h;
    mp::StretchArgs g = stretch_args(s, d_perm, s->steps_done + (uint64_t)row, 0);
    g.chain = chain ? s->d_chain.p : nullptr;
    g.chain_lnp = chain ? s->d_chain_lnp.p : nullptr;
    g.chain_row = row;
    if (mv) {
        g.move = mv->kind;
        if (mv->kind == MP_MOVE_STRETCH) g.a = mv->p0;
        else if (mv->kind == MP_MOVE_DE) { g.de_g0 = mv->p0; g.de_s = mv->p1; }
        else if (mv->kind == MP_MOVE_SNOOKER) g.gamma_s = mv->p0;
        else g.kde_f = mv->p0;
    }
    int e;
    if (whole && g.move == MP_MOVE_STRETCH) {
        g.spec = s->d_spec.p;
        e = mp::launch_stretch_step(h->sh, g, 3 * g.n_half * g.n_ensembles, h->stream);
        if (!e) e = mp::launch_stretch_step_commit(g, h->stream);
    } else {
        e = mp::launch_stretch(h->sh, g, g.n_half * g.n_ensembles, h->stream);
        g.half = 1;
        if (!e) e = mp::launch_stretch(h->sh, g, g.n_half * g.n_ensembles, h->stream);
    }
    if (!e && s->n_temps) e = mp::launch_stretch_swap(g, s->n_temps, s->d_swaps.p, h->stream);
    if (e) return fail(MP_EHIP, "kernel launch failed: %s", hipGetErrorString((hipError_t)e));
    return MP_OK;
}

int mp_sampler_run(mp_sampler *s, int n_steps, double *chain, double *chain_lnprob) {
    if (!s || n_steps < 0) return fail(MP_EINVAL, "mp_sampler_run: bad argument");
    if (!s->have_state) return fail(MP_ESTATE, "mp_sampler_run: call mp_sampler_set_positions first");
    if ((chain == nullptr) != (chain_lnprob == nullptr)) return fail(MP_EINVAL, "mp_sampler_run: chain and chain_lnprob go together");
    mp_handle *h = s->h;
    Lock lock(h->mu);
    DeviceScope scope(h->device);
    const size_t nt = (size_t)s->n_total, row = nt * s->ndim;
    // chunks of steps so that the device-resident chain slab stays below ~256 MB, the splits below ~64 MB, and the
    // window of failed proposals (drained after every chunk) overflows only if more than 1 in 32 proposals fails
    const size_t perm_cap = std::max<size_t>(1, std::min<size_t>((size_t)16 << 20, (size_t)32 * MP_BAD_WINDOW) / nt);
    const int chunk_max = (int)std::min<size_t>(
        (size_t)std::max(n_steps, 1),
        chain ? std::max<size_t>(1, std::min<size_t>(perm_cap, (256u << 20) / (row * sizeof(double)))) : perm_cap);
    constexpr int kSub = 8;   // steps per batch of splits: the host draws the next batch while the GPU runs this one
    int rc;
    // A whole step per launch (mp_kernels.hip stretch_step_kernel: 3 n/2 evaluations, a third of them speculative) while
    // that beats two half-step launches (mp_device.h stretch_whole_step_fits); larger ensembles fill the device with one half-step
    // at a time.
    const int n_slots = (s->n_walkers / 2) * s->n_ensembles;
    const bool whole = s->whole_step && mp::stretch_whole_step_fits(h->sh, 3 * (long long)n_slots);
    if (whole && (rc = s->d_spec.ensure((size_t)3 * n_slots * (size_t)(s->ndim + mp::kSpecExtra)))) return rc;
    if (s->ext_stream_work) {   // sharded half-steps on a caller's stream may still be updating the state
        HIP_TRY(hipDeviceSynchronize());
        s->ext_stream_work = false;
    }
    for (int done = 0; done < n_steps;) {
        const int chunk = std::min(chunk_max, n_steps - done);
        if ((rc = s->h_perm.ensure((size_t)chunk * nt * sizeof(int32_t))) || (rc = s->d_perm.ensure((size_t)chunk * nt))) return rc;
        int32_t *perm = (int32_t *)s->h_perm.p;
        if (chain) {
            if ((rc = s->d_chain.ensure((size_t)chunk * row)) || (rc = s->d_chain_lnp.ensure((size_t)chunk * nt))) return rc;
        }
        for (int sub = 0; sub < chunk; sub += kSub) {
            const int sub_end = std::min(chunk, sub + kSub);
            draw_splits(s, s->steps_done + (uint64_t)sub, sub_end - sub, perm + (size_t)sub * nt);
            int step_move[kSub];   // with a move table: the move of every step of the batch, drawn next to its splits
            for (int st = sub; st < sub_end; ++st) step_move[st - sub] = draw_move(s, s->steps_done + (uint64_t)st);
            HIP_TRY(hipMemcpyAsync(s->d_perm.p + (size_t)sub * nt, perm + (size_t)sub * nt,
                                   (size_t)(sub_end - sub) * nt * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
            for (int st = sub; st < sub_end; ++st) {
                const mp_sampler::Move *mv = s->moves.empty() ? nullptr : &s->moves[(size_t)step_move[st - sub]];
                if ((rc = enqueue_step(s, s->d_perm.p + (size_t)st * nt, st, mv, chain != nullptr, whole))) return rc;
            }
        }
        if (chain) {
            HIP_TRY(hipMemcpyAsync(chain + (size_t)done * row, s->d_chain.p, (size_t)chunk * row * sizeof(double), hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(hipMemcpyAsync(chain_lnprob + (size_t)done * nt, s->d_chain_lnp.p, (size_t)chunk * nt * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        }
        HIP_TRY(hipStreamSynchronize(h->stream));
        if ((rc = drain_bad(s))) return rc;
        s->steps_done += (uint64_t)chunk;
        done += chunk;
    }
    return MP_OK;
}

int mp_sampler_set_whole_step(mp_sampler *s, int enable) {
    if (!s) return fail(MP_EINVAL, "mp_sampler_set_whole_step: NULL sampler");
    Lock lock(s->h->mu);
    s->whole_step = enable != 0;
    return MP_OK;
}

// ---- walker-sharded driving: the caller (one process per GPU) runs, per half-step,
//        mp_sampler_halfstep_shard(its block of slots) -> all-gather of the outcome rows -> mp_sampler_halfstep_apply.
// Device pointer of the split of the current step; uploads the next window of kWin splits when the step enters it.
static int current_split(mp_sampler *s, hipStream_t st, const int32_t **d_perm) {
    const size_t nt = (size_t)s->n_total;
    const int64_t win = (int64_t)(s->steps_done / mp_sampler::kWin);
    const int b = (int)(win & 1);
    if (s->win_id[b] != win) {
        int rc;
        const size_t bytes = (size_t)mp_sampler::kWin * nt * sizeof(int32_t);
        if ((rc = s->h_win[b].ensure(bytes)) || (rc = s->d_win[b].ensure((size_t)mp_sampler::kWin * nt))) return rc;
        if (s->win_id[b] >= 0) HIP_TRY(hipEventSynchronize(s->win_copied[b].e));   // staged two windows ago: long done
        int32_t *perm = (int32_t *)s->h_win[b].p;
        draw_splits(s, (uint64_t)win * mp_sampler::kWin, mp_sampler::kWin, perm);
        // stream order puts the copy behind every kernel that still reads this buffer's previous contents
        HIP_TRY(hipMemcpyAsync(s->d_win[b].p, perm, bytes, hipMemcpyHostToDevice, st));
        HIP_TRY(hipEventRecord(s->win_copied[b].e, st));
        s->win_id[b] = win;
    }
    *d_perm = s->d_win[b].p + (size_t)(s->steps_done % mp_sampler::kWin) * nt;
    return MP_OK;
}

int mp_sampler_row_doubles(const mp_sampler *s) { return s ? s->ndim + 3 : 0; }
int mp_sampler_n_slots(const mp_sampler *s) { return s ? (s->n_walkers / 2) * s->n_ensembles : 0; }

// The prologue of the four sharded entry points (fn: the entry point, which every message starts with): a sampler without state,
// a tempered one and one with a move table are refused (those run through mp_sampler_run only); otherwise the handle's lock and
// device are held for the call, d_perm is the split of the current step and the sampler notes work on a caller's stream.
struct ShardCall {
    Lock lock;
    DeviceScope scope;
    const int32_t *d_perm = nullptr;
    int rc = MP_OK;
    ShardCall(mp_sampler *s, const char *fn, void *stream) : lock(s->h->mu), scope(s->h->device) {
        if (!s->have_state) rc = fail(MP_ESTATE, "%s: call mp_sampler_set_positions first", fn);
        else if (s->n_temps) rc = fail(MP_ESTATE, "%s: a tempered sampler runs on one device only (mp_sampler_run)", fn);
        else if (!s->moves.empty())
            rc = fail(MP_ESTATE, "%s: a sampler with a move table (mp_sampler_set_moves) runs on one device only (mp_sampler_run)", fn);
        else if (!(rc = current_split(s, (hipStream_t)stream, &d_perm))) s->ext_stream_work = true;
    }
};

int mp_sampler_halfstep_shard(mp_sampler *s, int half, int slot_lo, int slot_hi, double *d_rows, void *stream) {
    if (!s || (half != 0 && half != 1)) return fail(MP_EINVAL, "mp_sampler_halfstep_shard: bad argument");
    ShardCall c(s, "mp_sampler_halfstep_shard", stream);
    if (c.rc) return c.rc;
    const int n_slots = (s->n_walkers / 2) * s->n_ensembles;
    if (slot_lo < 0 || slot_hi > n_slots || slot_lo > slot_hi) return fail(MP_EINVAL, "mp_sampler_halfstep_shard: slots [%d, %d) outside [0, %d)", slot_lo, slot_hi, n_slots);
    if (slot_hi > slot_lo && !d_rows) return fail(MP_EINVAL, "mp_sampler_halfstep_shard: NULL row buffer");
    if (slot_hi == slot_lo) return MP_OK;
    mp::StretchArgs g = stretch_args(s, c.d_perm, s->steps_done, half);
    g.upd = d_rows;
    g.slot_lo = slot_lo;
    const int e = mp::launch_stretch(s->h->sh, g, slot_hi - slot_lo, stream);
    if (e) return fail(MP_EHIP, "kernel launch failed: %s", hipGetErrorString((hipError_t)e));
    return MP_OK;
}

int mp_sampler_halfstep_apply(mp_sampler *s, int half, const double *d_rows, double *d_chain_row, double *d_chain_lnp_row,
                              void *stream) {
    if (!s || !d_rows || (half != 0 && half != 1)) return fail(MP_EINVAL, "mp_sampler_halfstep_apply: bad argument");
    if ((d_chain_row == nullptr) != (d_chain_lnp_row == nullptr)) return fail(MP_EINVAL, "mp_sampler_halfstep_apply: chain row and lnprob row go together");
    ShardCall c(s, "mp_sampler_halfstep_apply", stream);
    if (c.rc) return c.rc;
    mp::StretchArgs g = stretch_args(s, c.d_perm, s->steps_done, half);
    g.upd = const_cast<double *>(d_rows);
    g.chain = d_chain_row;
    g.chain_lnp = d_chain_lnp_row;
    g.chain_row = 0;
    const int e = mp::launch_stretch_apply(g, stream);
    if (e) return fail(MP_EHIP, "kernel launch failed: %s", hipGetErrorString((hipError_t)e));
    if (half == 1) s->steps_done += 1;
    return MP_OK;
}

// ---- the same for a whole step per launch (mp_kernels.hip stretch_step_kernel): the caller runs, per STEP,
//        mp_sampler_step_shard(its share of the 3 * n_slots blocks) -> ONE all-gather of the rows -> mp_sampler_step_apply.
int mp_sampler_step_blocks(const mp_sampler *s) { return s ? 3 * (s->n_walkers / 2) * s->n_ensembles : 0; }
int mp_sampler_step_row_doubles(const mp_sampler *s) { return s ? s->ndim + mp::kSpecExtra : 0; }

int mp_sampler_step_shard(mp_sampler *s, int block_lo, int block_hi, double *d_rows, void *stream) {
    if (!s) return fail(MP_EINVAL, "mp_sampler_step_shard: NULL sampler");
    ShardCall c(s, "mp_sampler_step_shard", stream);
    if (c.rc) return c.rc;
    const int n_blocks = 3 * (s->n_walkers / 2) * s->n_ensembles;
    if (block_lo < 0 || block_hi > n_blocks || block_lo > block_hi) return fail(MP_EINVAL, "mp_sampler_step_shard: blocks [%d, %d) outside [0, %d)", block_lo, block_hi, n_blocks);
    if (block_hi > block_lo && !d_rows) return fail(MP_EINVAL, "mp_sampler_step_shard: NULL row buffer");
    if (block_hi == block_lo) return MP_OK;
    mp::StretchArgs g = stretch_args(s, c.d_perm, s->steps_done, 0);
    g.spec = d_rows;
    g.slot_lo = block_lo;
    const int e = mp::launch_stretch_step(s->h->sh, g, block_hi - block_lo, stream);
    if (e) return fail(MP_EHIP, "kernel launch failed: %s", hipGetErrorString((hipError_t)e));
    return MP_OK;
}

int mp_sampler_step_apply(mp_sampler *s, const double *d_rows, double *d_chain_row, double *d_chain_lnp_row, void *stream) {
    if (!s || !d_rows) return fail(MP_EINVAL, "mp_sampler_step_apply: bad argument");
    if ((d_chain_row == nullptr) != (d_chain_lnp_row == nullptr)) return fail(MP_EINVAL, "mp_sampler_step_apply: chain row and lnprob row go together");
    ShardCall c(s, "mp_sampler_step_apply", stream);
    if (c.rc) return c.rc;
    mp::StretchArgs g = stretch_args(s, c.d_perm, s->steps_done, 0);
    g.spec = const_cast<double *>(d_rows);
    g.chain = d_chain_row;
    g.chain_lnp = d_chain_lnp_row;
    g.chain_row = 0;
    const int e = mp::launch_stretch_step_commit(g, stream);
    if (e) return fail(MP_EHIP, "kernel launch failed: %s", hipGetErrorString((hipError_t)e));
    s->steps_done += 1;
    return MP_OK;
}

int mp_sampler_state_ptrs(mp_sampler *s, double **d_pos, double **d_lnprob) {
    if (!s) return fail(MP_EINVAL, "mp_sampler_state_ptrs: NULL sampler");
    if (d_pos) *d_pos = s->d_pos.p;
    if (d_lnprob) *d_lnprob = s->d_lnprob.p;
    return MP_OK;
}

int mp_sampler_get_bad(mp_sampler *s, int64_t first_row, double *pars, int max_rows, int64_t *n_bad, int64_t *n_logged) {
    if (!s || max_rows < 0 || first_row < 0 || (max_rows > 0 && !pars)) return fail(MP_EINVAL, "mp_sampler_get_bad: bad argument");
    mp_handle *h = s->h;
    Lock lock(h->mu);
    DeviceScope scope(h->device);
    HIP_TRY(hipDeviceSynchronize());
    const int rc = drain_bad(s);
    if (rc) return rc;
    const int64_t logged = (int64_t)(s->bad_log.size() / (size_t)s->ndim);
    if (n_bad) *n_bad = s->n_bad;
    if (n_logged) *n_logged = logged;
    const int64_t rows = std::max<int64_t>(0, std::min<int64_t>(logged - first_row, (int64_t)max_rows));
    if (rows) std::memcpy(pars, s->bad_log.data() + (size_t)first_row * s->ndim, (size_t)rows * s->ndim * sizeof(double));
    return (int)rows;
}

int mp_sampler_get_state(mp_sampler *s, double *pos, double *lnprob, int64_t *n_accepted, int64_t *steps_done) {
    if (!s) return fail(MP_EINVAL, "mp_sampler_get_state: NULL sampler");
    mp_handle *h = s->h;
    Lock lock(h->mu);
    DeviceScope scope(h->device);
    const size_t nt = (size_t)s->n_total;
    HIP_TRY(hipDeviceSynchronize());
    const int rc = read_back(pos, s->d_pos.p, nt * s->ndim, lnprob, s->d_lnprob.p, nt, n_accepted, s->d_acc.p, nt);
    if (rc) return rc;
    if (steps_done) *steps_done = (int64_t)s->steps_done;
    return MP_OK;
}

// ---------------------------------------------------------------- differential-evolution optimizer (mp_opt.hip)
struct mp_optimizer {
    mp_handle *h = nullptr;
    mp::OptArgs a{};                // pointers: cur / next as of the next launch
    int n_total = 0;
    uint32_t gen = 0;               // generations launched so far (0: only the initial evaluation)
    bool have_state = false;
    DevBuf<double> d_pop[2], d_lnp[2];
    DevBuf<int32_t> d_st[2], d_dsid, d_best, d_conv, d_nit;
    DevBuf<int64_t> d_nfev;
};

static void opt_swap(mp_optimizer *o) {
    std::swap(o->a.pop_cur, o->a.pop_next);
    std::swap(o->a.lnp_cur, o->a.lnp_next);
    std::swap(o->a.st_cur, o->a.st_next);
}

// one generation (trial = 1) or the initial evaluation (trial = 0) on the handle's stream, then the buffers change roles
static int opt_enqueue(mp_optimizer *o, int trial) {
    o->a.trial = trial;
    o->a.gen = o->gen;
    int e = mp::launch_opt_trial(o->h->sh, o->a, o->h->stream);
    if (!e) e = mp::launch_opt_reduce(o->a, o->h->stream);
    if (e) return fail(MP_EHIP, "kernel launch failed: %s", hipGetErrorString((hipError_t)e));
    opt_swap(o);
    return MP_OK;
}

mp_optimizer *mp_optimizer_create(mp_handle *h, int popsize, int n_pops, int ndim, const int32_t *pop_ds_id, uint64_t seed,
                                  int strategy, double f_lo, double f_hi, double cr, double tol, double atol,
                                  const double *lower, const double *upper, int target) {
    if (!h || !lower || !upper) { fail(MP_EINVAL, "mp_optimizer_create: NULL argument"); return nullptr; }
    Lock lock(h->mu);
    const int rc = check_create(h, "mp_optimizer_create", "the optimizer lives on ONE device (a multi-device handle serves host-buffer batches only)",
                                ndim, target, "population", n_pops, pop_ds_id, [&] {
        if (popsize < 5 || popsize > 1024) return fail(MP_EINVAL, "mp_optimizer_create: popsize must be 5 .. 1024, got %d", popsize);
        if (n_pops < 1 || n_pops > MP_MAX_DATASETS) return fail(MP_EINVAL, "mp_optimizer_create: n_pops must be 1 .. %d", MP_MAX_DATASETS);
        if (target != 0 && target != 1) return fail(MP_EINVAL, "mp_optimizer_create: target must be 0 (posterior) or 1 (unit Gaussian)");
        if (strategy != MP_DE_BEST1BIN && strategy != MP_DE_RAND1BIN) return fail(MP_EINVAL, "mp_optimizer_create: unknown strategy %d", strategy);
        if (!(f_lo >= 0.0 && f_lo <= f_hi && f_hi < 2.0)) return fail(MP_EINVAL, "mp_optimizer_create: need 0 <= f_lo <= f_hi < 2");
        if (!(cr >= 0.0 && cr <= 1.0)) return fail(MP_EINVAL, "mp_optimizer_create: cr must lie in [0, 1]");
        if (!(std::isfinite(tol) && tol >= 0.0 && std::isfinite(atol) && atol >= 0.0)) return fail(MP_EINVAL, "mp_optimizer_create: tol and atol must be finite and >= 0");
        return check_box("mp_optimizer_create", ndim, lower, upper);
    });
    if (rc) return nullptr;
    mp_optimizer *o = new mp_optimizer();
    o->h = h;
    o->n_total = popsize * n_pops;
    mp::OptArgs &a = o->a;
    a.popsize = popsize; a.n_pops = n_pops; a.ndim = ndim; a.strategy = strategy; a.target = target; a.seed = seed;
    a.f_lo = f_lo; a.f_hi = f_hi; a.cr = cr; a.tol = tol; a.atol = atol;
    for (int d = 0; d < ndim; ++d) { a.lower[d] = lower[d]; a.upper[d] = upper[d]; }
    DeviceScope scope(h->device);
    const size_t nt = (size_t)o->n_total;
    Binder bind;
    bind(o->d_pop[0], nt * ndim, a.pop_cur); bind(o->d_pop[1], nt * ndim, a.pop_next);
    bind(o->d_lnp[0], nt, a.lnp_cur); bind(o->d_lnp[1], nt, a.lnp_next);
    bind(o->d_st[0], nt, a.st_cur); bind(o->d_st[1], nt, a.st_next);
    bind(o->d_dsid, nt, a.ds_id);
    bind(o->d_best, n_pops, a.best); bind(o->d_conv, n_pops, a.converged); bind(o->d_nit, n_pops, a.nit); bind(o->d_nfev, n_pops, a.nfev);
    if (bind.rc || upload_ds_rows(o->d_dsid.p, pop_ds_id, n_pops, popsize)) {
        fail(MP_EHIP, "mp_optimizer_create: device allocation failed");
        mp_optimizer_destroy(o);
        return nullptr;
    }
    return o;
}

int mp_optimizer_destroy(mp_optimizer *o) {
    if (!o) return MP_OK;
    Lock lock(o->h->mu);
    DeviceScope scope(o->h->device);
    (void)hipStreamSynchronize(o->h->stream);
    delete o;
    return MP_OK;
}

int mp_optimizer_set_population(mp_optimizer *o, const double *pop) {
    if (!o || !pop) return fail(MP_EINVAL, "mp_optimizer_set_population: NULL argument");
    mp_handle *h = o->h;
    const size_t nt = (size_t)o->n_total, n_pops = (size_t)o->a.n_pops;
    for (size_t i = 0; i < nt * o->a.ndim; ++i)
        if (!std::isfinite(pop[i])) return fail(MP_EINVAL, "mp_optimizer_set_population: non-finite coordinate");
    Lock lock(h->mu);
    DeviceScope scope(h->device);
    HIP_TRY(hipMemcpyAsync(o->a.pop_cur, pop, nt * o->a.ndim * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemsetAsync(o->a.converged, 0, n_pops * sizeof(int32_t), h->stream));
    HIP_TRY(hipMemsetAsync(o->a.nit, 0, n_pops * sizeof(int32_t), h->stream));
    HIP_TRY(hipMemsetAsync(o->a.nfev, 0, n_pops * sizeof(int64_t), h->stream));
    o->gen = 0;
    int rc = opt_enqueue(o, 0);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    o->have_state = true;
    return MP_OK;
}

int mp_optimizer_run(mp_optimizer *o, int max_generations, int *n_running) {
    if (!o || max_generations < 0) return fail(MP_EINVAL, "mp_optimizer_run: bad argument");
    if (!o->have_state) return fail(MP_ESTATE, "mp_optimizer_run: call mp_optimizer_set_population first");
    mp_handle *h = o->h;
    Lock lock(h->mu);
    DeviceScope scope(h->device);
    // Chunks of generations enqueued back to back (no allocation, no wait inside a chunk); the flags are read back behind each
    // chunk, and the run ends early once every population has converged.  A frozen population costs an empty workgroup per
    // member and launch.
    constexpr int kChunk = 16;
    int running, rc;
    if ((rc = groups_running(h, o->a.converged, o->a.n_pops, &running))) return rc;
    for (int done = 0; done < max_generations && running > 0;) {
        const int chunk = std::min(kChunk, max_generations - done);
        for (int g = 0; g < chunk; ++g) {
            ++o->gen;
            if ((rc = opt_enqueue(o, 1))) return rc;
        }
        if ((rc = groups_running(h, o->a.converged, o->a.n_pops, &running))) return rc;
        done += chunk;
    }
    if (n_running) *n_running = running;
    return MP_OK;
}

int mp_optimizer_get_state(mp_optimizer *o, double *pop, double *lnprob, int32_t *status, int32_t *best, int32_t *nit,
                           int32_t *converged, int64_t *nfev) {
    if (!o) return fail(MP_EINVAL, "mp_optimizer_get_state: NULL optimizer");
    if (!o->have_state) return fail(MP_ESTATE, "mp_optimizer_get_state: call mp_optimizer_set_population first");
    mp_handle *h = o->h;
    Lock lock(h->mu);
    DeviceScope scope(h->device);
    const size_t nt = (size_t)o->n_total, np = (size_t)o->a.n_pops;
    HIP_TRY(hipStreamSynchronize(h->stream));
    const mp::OptArgs &a = o->a;
    return read_back(pop, a.pop_cur, nt * a.ndim, lnprob, a.lnp_cur, nt, status, a.st_cur, nt,
                     best, a.best, np, nit, a.nit, np, converged, a.converged, np, nfev, a.nfev, np);
}

// ---------------------------------------------------------------- nested sampler (mp_nest.hip)
struct mp_nested {
    mp_handle *h = nullptr;
    mp::NestArgs a{};
    int n_total = 0;                // n_runs * nlive
    int chunk = 0;                  // iterations per chunk (slots of the dead buffers)
    uint32_t iter = 0;              // iterations launched since mp_nested_set_live
    bool have_state = false;
    DevBuf<double> d_live, d_lnl, d_lstar, d_dpars, d_dlnl, d_lnx, d_lnz;
    DevBuf<int32_t> d_st, d_acc, d_dsid, d_dslot, d_surv, d_dn, d_stop, d_nit;
    DevBuf<int64_t> d_ncall, d_nacc, d_nzero, d_nexp, d_ncon, d_nfail;
    mp::NestSlice sl{};             // slice mode (sl.slices > 0) from the next iteration on
    std::vector<std::vector<double>> dead_pars, dead_lnl;   // per run, in order
    std::vector<std::vector<int32_t>> dead_n;
};

mp_nested *mp_nested_create(mp_handle *h, int nlive, int nbatch, int n_runs, int ndim, const int32_t *run_ds_id, uint64_t seed,
                            int walks, double g0, double sigma, double dlogz, const double *lower, const double *upper, int target) {
    if (!h || !lower || !upper) { fail(MP_EINVAL, "mp_nested_create: NULL argument"); return nullptr; }
    Lock lock(h->mu);
    const int rc = check_create(h, "mp_nested_create", "the nested sampler lives on ONE device (a multi-device handle serves host-buffer batches only)",
                                ndim, target, "run", n_runs, run_ds_id, [&] {
        if (nlive < MP_NEST_MIN_LIVE || nlive > MP_NEST_MAX_LIVE) return fail(MP_EINVAL, "mp_nested_create: nlive must be %d .. %d, got %d", MP_NEST_MIN_LIVE, MP_NEST_MAX_LIVE, nlive);
        if (nbatch < 1 || nbatch > nlive / 2) return fail(MP_EINVAL, "mp_nested_create: nbatch must be 1 .. nlive / 2, got %d", nbatch);
        if (n_runs < 1 || n_runs > MP_MAX_DATASETS) return fail(MP_EINVAL, "mp_nested_create: n_runs must be 1 .. %d", MP_MAX_DATASETS);
        if (target != 0 && target != 1) return fail(MP_EINVAL, "mp_nested_create: target must be 0 (posterior) or 1 (unit Gaussian)");
        if (walks < 1 || walks > MP_NEST_MAX_WALKS) return fail(MP_EINVAL, "mp_nested_create: walks must be 1 .. %d", MP_NEST_MAX_WALKS);
        if (!std::isfinite(g0)) return fail(MP_EINVAL, "mp_nested_create: g0 must be finite (<= 0: the default)");
        if (!(sigma >= 0.0 && sigma < 1.0 / std::sqrt(3.0))) return fail(MP_EINVAL, "mp_nested_create: sigma must lie in [0, 1/sqrt(3))");
        if (!(std::isfinite(dlogz) && dlogz > 0.0)) return fail(MP_EINVAL, "mp_nested_create: dlogz must be finite and > 0");
        return check_box("mp_nested_create", ndim, lower, upper);
    });
    if (rc) return nullptr;
    mp_nested *ns = new mp_nested();
    ns->h = h;
    ns->n_total = nlive * n_runs;
    // dead buffers of about 16 MB at most, up to 32 iterations per chunk
    const size_t row = (size_t)n_runs * nbatch * (ndim + 2) * sizeof(double);
    ns->chunk = (int)std::max<size_t>(1, std::min<size_t>(32, (16u << 20) / row));
    mp::NestArgs &a = ns->a;
    a.nlive = nlive; a.nbatch = nbatch; a.n_runs = n_runs; a.ndim = ndim; a.walks = walks; a.target = target; a.seed = seed;
    a.g0 = g0 > 0.0 ? g0 : 2.38 / std::sqrt(2.0 * ndim);
    a.sig3 = sigma * std::sqrt(3.0);
    a.dlogz = dlogz;
    for (int d = 0; d < ndim; ++d) { a.lower[d] = lower[d]; a.upper[d] = upper[d]; }
    ns->dead_pars.resize(n_runs); ns->dead_lnl.resize(n_runs); ns->dead_n.resize(n_runs);
    DeviceScope scope(h->device);
    const size_t nt = (size_t)ns->n_total, nr = (size_t)n_runs, nk = nr * nbatch, nc = (size_t)ns->chunk * nk;
    Binder bind;
    bind(ns->d_live, nt * ndim, a.live); bind(ns->d_lnl, nt, a.lnl); bind(ns->d_st, nt, a.st); bind(ns->d_acc, nt, a.acc);
    bind(ns->d_dsid, nr, a.ds_id); bind(ns->d_dslot, nk, a.dead_slot); bind(ns->d_surv, nr * (nlive - nbatch), a.surv);
    bind(ns->d_lstar, nr, a.lstar); bind(ns->d_dpars, nc * ndim, a.dead_pars); bind(ns->d_dlnl, nc, a.dead_lnl); bind(ns->d_dn, nc, a.dead_n);
    bind(ns->d_lnx, nr, a.lnx); bind(ns->d_lnz, nr, a.lnz); bind(ns->d_stop, nr, a.stopped); bind(ns->d_nit, nr, a.nit);
    bind(ns->d_ncall, nr, a.ncall); bind(ns->d_nacc, nr, a.nacc); bind(ns->d_nzero, nr, a.nzero);
    bind(ns->d_nexp, nr, ns->sl.nexpand); bind(ns->d_ncon, nr, ns->sl.ncontract); bind(ns->d_nfail, nr, ns->sl.nfail);
    if (bind.rc || upload_ds_rows(ns->d_dsid.p, run_ds_id, n_runs, 1)) {
        fail(MP_EHIP, "mp_nested_create: device allocation failed");
        mp_nested_destroy(ns);
        return nullptr;
    }
    return ns;
}

int mp_nested_destroy(mp_nested *ns) {
    if (!ns) return MP_OK;
    Lock lock(ns->h->mu);
    DeviceScope scope(ns->h->device);
    (void)hipStreamSynchronize(ns->h->stream);
    delete ns;
    return MP_OK;
}

int mp_nested_set_live(mp_nested *ns, const double *live) {
    if (!ns || !live) return fail(MP_EINVAL, "mp_nested_set_live: NULL argument");
    mp_handle *h = ns->h;
    mp::NestArgs &a = ns->a;
    const size_t nt = (size_t)ns->n_total, nr = (size_t)a.n_runs;
    for (size_t i = 0; i < nt; ++i)
        for (int d = 0; d < a.ndim; ++d) {
            const double v = live[i * a.ndim + d];
            if (!(v >= a.lower[d] && v <= a.upper[d])) return fail(MP_EINVAL, "mp_nested_set_live: live point %zu lies outside the box", i);
        }
    Lock lock(h->mu);
    DeviceScope scope(h->device);
    const std::vector<double> zero(nr, 0.0), ninf(nr, -INFINITY);
    HIP_TRY(hipMemcpyAsync(a.live, live, nt * a.ndim * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(a.lnx, zero.data(), nr * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(a.lnz, ninf.data(), nr * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemsetAsync(a.stopped, 0, nr * sizeof(int32_t), h->stream));
    HIP_TRY(hipMemsetAsync(a.nit, 0, nr * sizeof(int32_t), h->stream));
    HIP_TRY(hipMemsetAsync(a.ncall, 0, nr * sizeof(int64_t), h->stream));
    HIP_TRY(hipMemsetAsync(a.nacc, 0, nr * sizeof(int64_t), h->stream));
    HIP_TRY(hipMemsetAsync(a.nzero, 0, nr * sizeof(int64_t), h->stream));
    HIP_TRY(hipMemsetAsync(ns->sl.nexpand, 0, nr * sizeof(int64_t), h->stream));
    HIP_TRY(hipMemsetAsync(ns->sl.ncontract, 0, nr * sizeof(int64_t), h->stream));
    HIP_TRY(hipMemsetAsync(ns->sl.nfail, 0, nr * sizeof(int64_t), h->stream));
    a.mode = 1;
    a.iter = 0;
    const int e = mp::launch_nest_walk(h->sh, a, h->stream);
    if (e) return fail(MP_EHIP, "kernel launch failed: %s", hipGetErrorString((hipError_t)e));
    HIP_TRY(hipStreamSynchronize(h->stream));
    ns->iter = 0;
    for (size_t r = 0; r < nr; ++r) { ns->dead_pars[r].clear(); ns->dead_lnl[r].clear(); ns->dead_n[r].clear(); }
    ns->have_state = true;
    return MP_OK;
}

int mp_nested_run(mp_nested *ns, int max_iterations, int *n_running) {
    if (!ns || max_iterations < 0) return fail(MP_EINVAL, "mp_nested_run: bad argument");
    if (!ns->have_state) return fail(MP_ESTATE, "mp_nested_run: call mp_nested_set_live first");
    mp_handle *h = ns->h;
    mp::NestArgs &a = ns->a;
    Lock lock(h->mu);
    DeviceScope scope(h->device);
    // Chunks of iterations enqueued back to back (select, walk, select, walk, ...; no wait inside a chunk), then a stop check on
    // the live set as it stands and one read-back of the counters and the dead rows; the run ends early once every run stopped.
    const int nr = a.n_runs, K = a.nbatch, nd = a.ndim;
    const size_t per = (size_t)nr * K;
    std::vector<int32_t> nit0((size_t)nr), nit1((size_t)nr);
    std::vector<double> hp, hl;
    std::vector<int32_t> hn;
    int running, rc;
    if ((rc = groups_running(h, a.stopped, nr, &running))) return rc;
    for (int done = 0; done < max_iterations && running > 0;) {
        const int chunk = std::min(ns->chunk, max_iterations - done);
        HIP_TRY(hipMemcpyAsync(nit0.data(), a.nit, nr * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        for (int c = 0; c < chunk; ++c) {
            a.slot = c;
            a.iter = ns->iter++;
            a.mode = 0;
            int e = mp::launch_nest_select(a, h->stream);
            if (!e) e = ns->sl.slices ? mp::launch_nest_slice(h->sh, a, ns->sl, h->stream) : mp::launch_nest_walk(h->sh, a, h->stream);
            if (e) return fail(MP_EHIP, "kernel launch failed: %s", hipGetErrorString((hipError_t)e));
        }
        a.mode = 1;
        int e = mp::launch_nest_select(a, h->stream);
        if (e) return fail(MP_EHIP, "kernel launch failed: %s", hipGetErrorString((hipError_t)e));
        hp.resize((size_t)chunk * per * nd);
        hl.resize((size_t)chunk * per);
        hn.resize((size_t)chunk * per);
        HIP_TRY(hipMemcpyAsync(hp.data(), a.dead_pars, hp.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipMemcpyAsync(hl.data(), a.dead_lnl, hl.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipMemcpyAsync(hn.data(), a.dead_n, hn.size() * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipMemcpyAsync(nit1.data(), a.nit, nr * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        if ((rc = groups_running(h, a.stopped, nr, &running))) return rc;   // (behind the copies above: they have landed)
        // run r ran the first nit1 - nit0 iterations of the chunk (a stopped run stays stopped)
        for (int r = 0; r < nr; ++r)
            for (int c = 0; c < nit1[r] - nit0[r]; ++c) {
                const size_t o = ((size_t)c * nr + r) * K;
                ns->dead_pars[r].insert(ns->dead_pars[r].end(), hp.begin() + o * nd, hp.begin() + (o + K) * nd);
                ns->dead_lnl[r].insert(ns->dead_lnl[r].end(), hl.begin() + o, hl.begin() + o + K);
                ns->dead_n[r].insert(ns->dead_n[r].end(), hn.begin() + o, hn.begin() + o + K);
            }
        done += chunk;
    }
    if (n_running) *n_running = running;
    return MP_OK;
}

int mp_nested_get_dead(mp_nested *ns, int run, int64_t max_rows, double *pars, double *lnl, int32_t *n_live, int64_t *n_rows) {
    if (!ns || run < 0 || run >= ns->a.n_runs || max_rows < 0) return fail(MP_EINVAL, "mp_nested_get_dead: bad argument");
    if (!ns->have_state) return fail(MP_ESTATE, "mp_nested_get_dead: call mp_nested_set_live first");
    Lock lock(ns->h->mu);
    const int64_t have = (int64_t)ns->dead_lnl[run].size(), n = std::min(have, max_rows);
    if (pars) std::copy(ns->dead_pars[run].begin(), ns->dead_pars[run].begin() + n * ns->a.ndim, pars);
    if (lnl) std::copy(ns->dead_lnl[run].begin(), ns->dead_lnl[run].begin() + n, lnl);
    if (n_live) std::copy(ns->dead_n[run].begin(), ns->dead_n[run].begin() + n, n_live);
    if (n_rows) *n_rows = have;
    return MP_OK;
}

int mp_nested_get_state(mp_nested *ns, double *live, double *lnl, int32_t *status, int32_t *acc, int32_t *nit, int32_t *stopped,
                        double *lnx, double *lnz, int64_t *ncall, int64_t *nacc, int64_t *nzero) {
    if (!ns) return fail(MP_EINVAL, "mp_nested_get_state: NULL sampler");
    if (!ns->have_state) return fail(MP_ESTATE, "mp_nested_get_state: call mp_nested_set_live first");
    mp_handle *h = ns->h;
    const mp::NestArgs &a = ns->a;
    Lock lock(h->mu);
    DeviceScope scope(h->device);
    const size_t nt = (size_t)ns->n_total, nr = (size_t)a.n_runs;
    HIP_TRY(hipStreamSynchronize(h->stream));
    return read_back(live, a.live, nt * a.ndim, lnl, a.lnl, nt, status, a.st, nt, acc, a.acc, nt, nit, a.nit, nr,
                     stopped, a.stopped, nr, lnx, a.lnx, nr, lnz, a.lnz, nr, ncall, a.ncall, nr, nacc, a.nacc, nr, nzero, a.nzero, nr);
}

int mp_nested_set_slice(mp_nested *ns, int slices, double mu, int max_steps_out, int max_shrink) {
    if (!ns) return fail(MP_EINVAL, "mp_nested_set_slice: NULL sampler");
    if (slices < 0 || slices > MP_NEST_MAX_SLICES) return fail(MP_EINVAL, "mp_nested_set_slice: slices must be 0 .. %d, got %d", MP_NEST_MAX_SLICES, slices);
    if (!(std::isfinite(mu) && mu > 0.0)) return fail(MP_EINVAL, "mp_nested_set_slice: mu must be finite and > 0");
    if (max_steps_out < 1 || max_steps_out > MP_NEST_MAX_STEPS_OUT)
        return fail(MP_EINVAL, "mp_nested_set_slice: max_steps_out must be 1 .. %d, got %d", MP_NEST_MAX_STEPS_OUT, max_steps_out);
    if (max_shrink < 1 || max_shrink > MP_NEST_MAX_SHRINK)
        return fail(MP_EINVAL, "mp_nested_set_slice: max_shrink must be 1 .. %d, got %d", MP_NEST_MAX_SHRINK, max_shrink);
    Lock lock(ns->h->mu);   // (read by the next mp_nested_run)
    ns->sl.slices = slices;
    ns->sl.mu = mu;
    ns->sl.max_steps_out = max_steps_out;
    ns->sl.max_shrink = max_shrink;
    return MP_OK;
}

int mp_nested_get_slice_stats(mp_nested *ns, int64_t *nexpand, int64_t *ncontract, int64_t *nfail) {
    if (!ns) return fail(MP_EINVAL, "mp_nested_get_slice_stats: NULL sampler");
    if (!ns->have_state) return fail(MP_ESTATE, "mp_nested_get_slice_stats: call mp_nested_set_live first");
    mp_handle *h = ns->h;
    Lock lock(h->mu);
    DeviceScope scope(h->device);
    const size_t nr = (size_t)ns->a.n_runs;
    HIP_TRY(hipStreamSynchronize(h->stream));
    return read_back(nexpand, ns->sl.nexpand, nr, ncontract, ns->sl.ncontract, nr, nfail, ns->sl.nfail, nr);
}

int mp_device(const mp_handle *h) { return h ? h->device : -1; }
void *mp_stream(const mp_handle *h) { return h ? (void *)h->stream : nullptr; }   // (a multi-device handle has none: NULL)
int mp_n_grid(const mp_handle *h) { return h ? (int)h->tgrid.size() : 0; }
double mp_last_mean_sweeps(const mp_handle *h) { return h ? h->last_mean_sweeps : 0.0; }
double mp_last_mean_tiles(const mp_handle *h) { return h ? h->last_mean_tiles : 0.0; }
int mp_last_sweeps(const mp_handle *h, int32_t *out, int n) {
    if (!h || !out || n < 0) return fail(MP_EINVAL, "mp_last_sweeps: bad argument");
    const int m = std::min<int>(n, (int)h->last_sweeps.size());
    std::copy(h->last_sweeps.begin(), h->last_sweeps.begin() + m, out);
    return m;
}
int mp_tile_log(mp_handle *h, int enable) {
    if (!h) return fail(MP_EINVAL, "mp_tile_log: NULL handle");
    Lock lock(h->mu);
    for (mp_handle *s : h->sub) (void)mp_tile_log(s, enable);
    h->tile_log_on = enable != 0;
    return MP_OK;
}
int mp_last_tile_log(const mp_handle *h, int walker, int32_t *out, int n) {
    if (!h || !out || n < 0 || walker < 0) return fail(MP_EINVAL, "mp_last_tile_log: bad argument");
    if (!h->sub.empty()) {   // the walker's block and its row inside it (contiguous blocks of ceil(n / G) rows)
        const int G = (int)h->sub.size(), total = (int)h->last_tiles.size(), per = (total + G - 1) / std::max(G, 1);
        if (per <= 0 || walker >= total) return 0;
        return mp_last_tile_log(h->sub[(size_t)(walker / per)], walker % per, out, n);
    }
    const size_t off = (size_t)walker * MP_TILE_LOG;
    if (off + MP_TILE_LOG > h->last_tile_log.size()) return 0;
    int m = 0;
    while (m < n && m < MP_TILE_LOG && h->last_tile_log[off + m] != -1) { out[m] = h->last_tile_log[off + m]; ++m; }
    return m;
}
int mp_last_tiles(const mp_handle *h, int32_t *out, int n) {
    if (!h || !out || n < 0) return fail(MP_EINVAL, "mp_last_tiles: bad argument");
    const int m = std::min<int>(n, (int)h->last_tiles.size());
    std::copy(h->last_tiles.begin(), h->last_tiles.begin() + m, out);
    return m;
}
double mp_sweep_tol(const mp_handle *h) { return h ? h->sh.sweep_tol : 0.0; }
int mp_get_policy(const mp_handle *h, double *out, int n) {
    if (!h || !out || n < 0) return fail(MP_EINVAL, "mp_get_policy: bad argument");
    const mp::DevShared &s = h->sh;
    double v[MP_POLICY_COUNT];
    v[MP_POLICY_MAX_STRIDE] = (double)(s.max_kind <= 1 ? 1 : (1 << (s.max_kind - 1)));
    v[MP_POLICY_STRIDE_TOL] = s.stride_tol;
    v[MP_POLICY_SWEEP_TOL] = s.sweep_tol;
    v[MP_POLICY_EARLY_HOLD_SECONDS] = s.early_hold_t;
    v[MP_POLICY_K4_TOL_FACTOR] = s.k4_tol_factor;
    v[MP_POLICY_COARSE_TOL_FACTOR] = s.coarse_tol_factor;
    v[MP_POLICY_COARSE_MAX_SWEEPS] = (double)s.coarse_max_sweeps;
    v[MP_POLICY_FINE_MAX_SWEEPS] = (double)s.fine_max_sweeps;
    v[MP_POLICY_TROUBLE_LIMIT] = (double)s.trouble_limit;
    v[MP_POLICY_STOP_FACTOR] = s.stop_factor;
    v[MP_POLICY_FORCED_STEPS_PER_LANE] = (double)s.force_spl;
#ifdef MP_EXPERIMENTS
    v[MP_POLICY_EXPERIMENTS] = 1.0;
#else
    v[MP_POLICY_EXPERIMENTS] = (MP_POLICY_MACROS_MODIFIED) ? 1.0 : 0.0;   // a -D build of the policy macros is an experiments build too
#endif
    v[MP_POLICY_LIGHT_TOL] = MP_LIGHT_TOL;
    v[MP_POLICY_CUT_BY_RATIO] = (double)MP_CUT_BY_RATIO;
    v[MP_POLICY_ABORT_SKIP_RATIO] = MP_ABORT_SKIP_RATIO;
    v[MP_POLICY_LOGPRED_MIN_KIND] = (double)MP_LOGPRED_MIN_KIND;
    v[MP_POLICY_PRE_EARLY_END_FACTOR] = MP_PRE_EARLY_END_FACTOR;
    const int m = std::min(n, (int)MP_POLICY_COUNT);
    std::copy(v, v + m, out);
    return m;
}
int mp_n_simd(const mp_handle *h) { return h ? h->sh.n_simd : 0; }

}  // extern "C"
