// mp_capi.cpp — host side of the C ABI declared in include/magprop_amd.h: the handle and its evaluators.
//
// Plain HIP runtime only (no torch, no hipBLAS).  First the per-device evaluator (mp_host.h Evaluator): device buffers,
// one stream, the dataset arena, thin launch wrappers, its constants and tables, evaluator_create / evaluator_destroy, and
// the helpers that the resident drivers share (the drivers themselves: mp_sampler.cpp, mp_optimizer.cpp, mp_nested.cpp,
// mp_simplex.cpp, mp_smc.cpp; the summaries of model curves: mp_summaries.cpp).  Then the mp_* entry points on the handle, a
// dealer over one evaluator per device -- datasets and prior, the batch entries, mp_rhs_batch and the introspection getters:
// each has ONE code path, which loops over the evaluators, deals a batch out among them, or runs on the first; mp_create's
// handle is the case of one evaluator.  The host-side digestion of observed light curves into the tile-bucketed layout the kernel reads happens
// once per mp_set_dataset.  There is NO CPU fallback: without a HIP device mp_create() fails.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "mp_host.h"
#include "mp_simulate.h"

static thread_local std::string g_err;

int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

// Launch the log-posterior kernel over a batch.  A batch that refers to light curves of more than 64 points next to short
// ones and needs more than one round of the device's wave slots (two per SIMD) is evaluated longest light curves first.
int launch_lnprob_ordered(Evaluator *ev, const mp::LaunchArgs &a_in, hipStream_t st) {
    mp::LaunchArgs a = a_in;
    int slot = -1;
    const bool curves = a.ltot || a.lprop || a.ldip || a.mdisc || a.omega;
    if (ev->sh.has_long && ev->sh.n_ds > 1 && a.ds_id && a.want_chi2 && !curves && a.n > 2 * ev->sh.n_simd) {
        slot = (int)(ev->order_next++ % Evaluator::kOrderRing);
        if (ev->order[slot].cap < (size_t)a.n) {
            // (growing frees the old buffer, which waits for the device: nothing in flight reads it any more)
            const int rc = ev->order[slot].ensure((size_t)a.n);
            if (rc) return rc;
        }
        if (!ev->order_done[slot].e) HIP_TRY(hipEventCreateWithFlags(&ev->order_done[slot].e, hipEventDisableTiming));
        else HIP_TRY(hipStreamWaitEvent(st, ev->order_done[slot].e, 0));
        const int eo = mp::launch_order(ev->sh, a.ds_id, a.n, ev->order[slot].p, (void *)st);
        if (eo) return launched(eo);
        a.order = ev->order[slot].p;
    }
    const int e = mp::launch_lnprob(ev->sh, a, (void *)st);
    if (e) return launched(e);
    if (slot >= 0) HIP_TRY(hipEventRecord(ev->order_done[slot].e, st));
    return MP_OK;
}

static void publish_datasets(Evaluator *ev) {
    int n_ds = 0, extra = 0;
    for (int d = 0; d < MP_MAX_DATASETS; ++d)
        if (ev->ds[d].set) { n_ds = d + 1; extra = std::max(extra, (int)ev->ds[d].g.size() - 64); }
    ev->sh.ds = ev->d_ds.p;
    ev->sh.n_ds = n_ds;
    ev->sh.tile_ptr = ev->d_tile_ptr.p;
    ev->sh.obs_g = ev->d_obs_g.p;
    ev->sh.obs_dx = ev->d_obs_dx.p;
    ev->sh.obs_idt = ev->d_obs_idt.p;
    ev->sh.obs_y = ev->d_obs_y.p;
    ev->sh.obs_yerr = ev->d_obs_yerr.p;
    ev->sh.has_long = extra > 0 ? 1 : 0;
}

// Copy light curve d behind the arena's last entry and publish its descriptor (slots never set keep n_obs = 0, which
// the kernels answer with MP_STATUS_BADDATASET).  Nothing in flight reads the target regions: no synchronisation.
static int append_dataset(Evaluator *ev, int d) {
    const HostDataset &s = ev->ds[d];
    const size_t n = s.g.size(), o = ev->obs_used, t = ev->tp_used;
    HIP_TRY(hipMemcpy(ev->d_obs_g.p + o, s.g.data(), n * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(ev->d_obs_dx.p + o, s.dx.data(), n * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(ev->d_obs_idt.p + o, s.idt.data(), n * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(ev->d_obs_y.p + o, s.y.data(), n * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(ev->d_obs_yerr.p + o, s.yerr.data(), n * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(ev->d_tile_ptr.p + t, s.tile_ptr.data(), s.tile_ptr.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    int32_t flags = mp::kDsOnKnots;
    for (size_t j = 0; j < n; ++j) if (s.dx[j] != 0.0) { flags = 0; break; }
    ev->desc[d] = mp::DsDesc{(int32_t)n, (int32_t)o, (int32_t)t, flags};
    HIP_TRY(hipMemcpy(ev->d_ds.p + d, &ev->desc[d], sizeof(mp::DsDesc), hipMemcpyHostToDevice));
    ev->obs_used = o + n;
    ev->tp_used = t + s.tile_ptr.size();
    return MP_OK;
}

// Rebuild the arena from the host copies (first use, growth, or a replaced slot): waits for the device, because
// kernels in flight may still read the old buffers, and leaves room for the sets to come.
static int rebuild_datasets(Evaluator *ev) {
    size_t n_obs = 0, n_tp = 0;
    for (int d = 0; d < MP_MAX_DATASETS; ++d)
        if (ev->ds[d].set) { n_obs += ev->ds[d].g.size(); n_tp += ev->ds[d].tile_ptr.size(); }
    HIP_TRY(hipDeviceSynchronize());
    const size_t cap_obs = std::max<size_t>(2 * n_obs, 4096), cap_tp = std::max<size_t>(2 * n_tp, 8 * ((size_t)ev->n_tiles + 1));
    int rc;
    if ((rc = ev->d_obs_g.ensure(cap_obs)) || (rc = ev->d_obs_dx.ensure(cap_obs)) || (rc = ev->d_obs_idt.ensure(cap_obs)) ||
        (rc = ev->d_obs_y.ensure(cap_obs)) || (rc = ev->d_obs_yerr.ensure(cap_obs)) || (rc = ev->d_tile_ptr.ensure(cap_tp)) ||
        (rc = ev->d_ds.ensure(MP_MAX_DATASETS)))
        return rc;
    ev->desc.assign(MP_MAX_DATASETS, mp::DsDesc{0, 0, 0, 0});
    HIP_TRY(hipMemset(ev->d_ds.p, 0, MP_MAX_DATASETS * sizeof(mp::DsDesc)));
    ev->obs_used = ev->tp_used = 0;
    for (int d = 0; d < MP_MAX_DATASETS; ++d)
        if (ev->ds[d].set && (rc = append_dataset(ev, d))) return rc;
    publish_datasets(ev);
    return MP_OK;
}

// After ev->ds[d] has been (re)set on the host.
static int upload_dataset(Evaluator *ev, int d, bool replaced) {
    const HostDataset &s = ev->ds[d];
    const bool fits = ev->d_ds.p && ev->obs_used + s.g.size() <= ev->d_obs_g.cap && ev->tp_used + s.tile_ptr.size() <= ev->d_tile_ptr.cap;
    if (replaced || !fits) return rebuild_datasets(ev);
    const int rc = append_dataset(ev, d);
    if (rc) return rc;
    publish_datasets(ev);
    return MP_OK;
}

// ---------------------------------------------------------------- what the resident drivers share
// (the ensemble sampler, the differential-evolution optimizer, the nested sampler, the simplex search and the SMC sampler:
// mp_sampler_*, mp_optimizer_*, mp_nested_*, mp_simplex_*, mp_smc_*)
// (declared in mp_host.h, next to the template check_create)

// the bounds box of a driver: finite, lower < upper in every coordinate
int check_box(const char *fn, int ndim, const double *lower, const double *upper) {
    for (int d = 0; d < ndim; ++d)
        if (!(std::isfinite(lower[d]) && std::isfinite(upper[d]) && lower[d] < upper[d]))
            return fail(MP_EINVAL, "%s: bounds of coordinate %d are empty or not finite", fn, d);
    return MP_OK;
}

// every one of the n rows of ndim coordinates lies inside the box (a NaN does not); `what` names the function and the rows
int check_inside(const char *what, const double *rows, size_t n, int ndim, const double *lower, const double *upper) {
    for (size_t i = 0; i < n; ++i)
        for (int d = 0; d < ndim; ++d) {
            const double v = rows[i * ndim + d];
            if (!(v >= lower[d] && v <= upper[d])) return fail(MP_EINVAL, "%s %zu lies outside the box", what, i);
        }
    return MP_OK;
}

// the dataset of every row, ds_id[g] (dataset 0 without ds_id) for the `rows` consecutive rows of group g, uploaded to dst
int upload_ds_rows(int32_t *dst, const int32_t *ds_id, int n_groups, int rows) {
    std::vector<int32_t> ds((size_t)n_groups * rows);
    for (int g = 0; g < n_groups; ++g) std::fill_n(ds.begin() + (size_t)g * rows, rows, ds_id ? ds_id[g] : 0);
    HIP_TRY(hipMemcpy(dst, ds.data(), ds.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    return MP_OK;
}

// *running = the groups whose flag (d_flags[n], read back behind the work on the handle's stream) is 0.  Every driver's flag is
// 0 while its group runs and non-zero once it has ended: converged and stopped become 1, an SMC run's status MP_SMC_DONE,
// MP_SMC_FAILED or MP_SMC_STAGE_LIMIT (1 to 3).
int groups_running(Evaluator *ev, const int32_t *d_flags, int n, int *running) {
    std::vector<int32_t> f((size_t)n);
    HIP_TRY(hipMemcpyAsync(f.data(), d_flags, f.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ev->stream));
    HIP_TRY(hipStreamSynchronize(ev->stream));
    *running = (int)std::count(f.begin(), f.end(), 0);
    return MP_OK;
}

// ---------------------------------------------------------------- the pieces of evaluator_create
// the model configuration and the time grid of mp_create / mp_create_multi
static int check_model_args(const mp_model_cfg *cfg, const double *tgrid, int n_grid) {
    if (!cfg || !tgrid || n_grid < 2)
        return fail(MP_EINVAL, "mp_create: cfg/tgrid NULL or n_grid < 2");
    for (int i = 1; i < n_grid; ++i)
        if (!(tgrid[i] > tgrid[i - 1]) || !std::isfinite(tgrid[i]))
            return fail(MP_EINVAL, "mp_create: tgrid must be finite and strictly increasing (index %d)", i);
    // The integrator is built on a geometric grid (np.logspace), the only kind the reference uses
    // (magnetar/funcs.py:132-137, code/synthetic_datasets/funcs.py:19).
    if (!(tgrid[0] > 0.0))
        return fail(MP_EINVAL, "mp_create: tgrid must be positive");
    // the kernels generate the step end times themselves, t_i = t_0 q^i: the grid has to be geometric to rounding
    const double lnq_check = std::log(tgrid[n_grid - 1] / tgrid[0]) / (double)(n_grid - 1);
    for (int i = 1; i < n_grid; ++i)
        if (std::fabs(tgrid[i] / (tgrid[0] * std::exp((double)i * lnq_check)) - 1.0) > 1.0e-12)
            return fail(MP_EINVAL, "mp_create: tgrid must be log-spaced (np.logspace); it leaves t0*q^i at index %d", i);
    if (!(cfg->inertia_factor > 0) || !(cfg->alpha > 0) || !(cfg->cs7 > 0) || !(cfg->k > 0) ||
        !(cfg->rm_massflow_factor > 0))
        return fail(MP_EINVAL, "mp_create: non-positive model constant in cfg");
    if (!(cfg->sweep_tol >= 0.0) || cfg->sweep_tol > 1.0e-3)
        return fail(MP_EINVAL, "mp_create: cfg.sweep_tol must be 0 (library default) or in (0, 1e-3]");
    if (!(cfg->stride_tol >= 0.0) || cfg->stride_tol > 1.0e-3 ||
        !(cfg->max_stride == 0 || cfg->max_stride == 1 || cfg->max_stride == 2 || cfg->max_stride == 4 ||
          cfg->max_stride == 8))
        return fail(MP_EINVAL, "mp_create: cfg.max_stride must be 0, 1, 2, 4 or 8 and cfg.stride_tol 0 or in (0, 1e-3]");
    if (cfg->dipole_torque != 0 && cfg->dipole_torque != 1)
        return fail(MP_EINVAL, "mp_create: cfg.dipole_torque must be 0 (the packages' dipole torque) or 1 (code/figure_3.py's Bucciantini law)");
    return MP_OK;
}

static void policy_constants(mp::DevShared &s, const mp_model_cfg &cfg) {
    s.sweep_tol = cfg.sweep_tol > 0.0 ? cfg.sweep_tol : MP_SWEEP_TOL_DEFAULT;
    s.stride_tol = cfg.stride_tol > 0.0 ? cfg.stride_tol : MP_STRIDE_TOL_DEFAULT;
    {
        const int ms = cfg.max_stride > 0 ? cfg.max_stride : MP_MAX_STRIDE_DEFAULT;
        s.max_kind = ms == 1 ? 1 : (ms == 2 ? 2 : (ms == 4 ? 3 : 4));
    }
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
}

static void build_tables(double lnq, mp::DevShared &s, std::vector<double> &wtab, size_t &ttab_off) {
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
    wtab.assign((size_t)mp::kWtabSize, 0.0);
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
    ttab_off = wtab.size();
    wtab.resize(ttab_off + (size_t)(mp::kKinds - 1) * mp::kTtabN);
    for (int kind = 1; kind < mp::kKinds; ++kind)
        for (int k = 0; k < mp::kTtabN; ++k) wtab[ttab_off + (size_t)(kind - 1) * mp::kTtabN + k] = std::exp((double)k * s.sk[kind].lnQ);
}

// what mp_destroy does for every evaluator of a handle: the delete runs while its device is current (DevBuf, mp_host.h)
static void evaluator_destroy(Evaluator *ev) {
    DeviceScope scope(ev->device);
    (void)hipDeviceSynchronize();
    if (ev->stream) (void)hipStreamDestroy(ev->stream);
    delete ev;   // (frees the buffers and events, on the evaluator's device)
}

// One evaluator on `device` (negative: the current one).  NULL with the message set on failure; the messages say mp_create,
// the entry point that a caller of mp_create_multi reads them through as well.
static Evaluator *evaluator_create(const mp_model_cfg *cfg, const double *tgrid, int n_grid, int device) {
    if (check_model_args(cfg, tgrid, n_grid)) return nullptr;
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
    Evaluator *ev = new Evaluator();
    ev->device = device;
    DeviceScope scope(device);
    hipDeviceProp_t prop;
    if (!scope.ok || hipStreamCreateWithFlags(&ev->stream, hipStreamNonBlocking) != hipSuccess ||
        hipGetDeviceProperties(&prop, device) != hipSuccess) {
        fail(MP_EHIP, "mp_create: cannot select device %d / create stream", device);
        evaluator_destroy(ev);
        return nullptr;
    }
    ev->tgrid.assign(tgrid, tgrid + n_grid);
    ev->n_tiles = (n_grid - 1 + mp::kTile - 1) / mp::kTile;
    if (ev->d_tgrid.ensure((size_t)n_grid) != MP_OK ||
        hipMemcpy(ev->d_tgrid.p, tgrid, sizeof(double) * (size_t)n_grid, hipMemcpyHostToDevice) != hipSuccess) {
        fail(MP_EHIP, "mp_create: cannot upload the time grid");
        evaluator_destroy(ev);
        return nullptr;
    }
    mp::DevShared &s = ev->sh;
    s.tgrid = ev->d_tgrid.p;
    s.n_grid = n_grid;
    s.n_tiles = ev->n_tiles;
    s.cfg = *cfg;
    s.n_prior = 0;
    s.log_mask = 0;
    mp::star_constants(s, *cfg);
    s.t0 = tgrid[0];
    const double lnq = std::log(tgrid[n_grid - 1] / tgrid[0]) / (double)(n_grid - 1);
    s.lnq8 = lnq / 8.0;
    s.pre_fine = std::min(32, n_grid - 1);                         // oracle/mp_oracle.c MPO_PRE_FINE
    s.n_simd = std::max(1, prop.multiProcessorCount) * 4;         // 4 SIMDs per CU (1 024 on MI355X)
    policy_constants(s, *cfg);
    std::vector<double> wtab;
    size_t ttab_off = 0;
    build_tables(lnq, s, wtab, ttab_off);
    if (ev->d_wtab.ensure(wtab.size()) != MP_OK ||
        hipMemcpy(ev->d_wtab.p, wtab.data(), wtab.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
        fail(MP_EHIP, "mp_create: cannot upload the quadrature tables");
        evaluator_destroy(ev);
        return nullptr;
    }
    s.wtab = ev->d_wtab.p;
    s.ttab = ev->d_wtab.p + ttab_off;
    if (rebuild_datasets(ev) != MP_OK) {
        evaluator_destroy(ev);
        return nullptr;
    }
    return ev;
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

// the handle over one evaluator per listed device
static mp_handle *handle_create(const mp_model_cfg *cfg, const double *tgrid, int n_grid, const int *devices, int n_devices, bool multi) {
    mp_handle *h = new mp_handle();
    h->multi = multi;
    for (int g = 0; g < n_devices; ++g) {
        Evaluator *ev = evaluator_create(cfg, tgrid, n_grid, devices[g]);
        if (!ev) {
            mp_destroy(h);
            return nullptr;
        }
        h->ev.push_back(ev);
    }
    return h;
}

mp_handle *mp_create(const mp_model_cfg *cfg, const double *tgrid, int n_grid, int device) {
    return handle_create(cfg, tgrid, n_grid, &device, 1, false);
}

mp_handle *mp_create_multi(const mp_model_cfg *cfg, const double *tgrid, int n_grid, const int *devices, int n_devices) {
    if (!devices || n_devices < 1 || n_devices > 64) {
        fail(MP_EINVAL, "mp_create_multi: devices NULL or n_devices outside 1..64");
        return nullptr;
    }
    return handle_create(cfg, tgrid, n_grid, devices, n_devices, true);
}

int mp_n_devices(const mp_handle *h) { return h ? (int)h->ev.size() : 0; }

int mp_destroy(mp_handle *h) {
    if (!h) return MP_OK;
    for (Evaluator *ev : h->ev) evaluator_destroy(ev);
    delete h;
    return MP_OK;
}

int mp_set_dataset(mp_handle *h, int ds_id, const double *x, const double *y, const double *yerr, int n_obs) {
    if (!h || !x || !y || !yerr) return fail(MP_EINVAL, "mp_set_dataset: NULL argument");
    if (ds_id < 0 || ds_id >= MP_MAX_DATASETS) return fail(MP_EINVAL, "mp_set_dataset: ds_id %d out of range", ds_id);
    if (n_obs <= 0) return fail(MP_EINVAL, "mp_set_dataset: n_obs must be positive");
    Lock lock(h->mu);
    const std::vector<double> &t = h->first()->tgrid;   // (every evaluator has the same grid: the light curve is digested once)
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
    d.tile_ptr.assign((size_t)h->first()->n_tiles + 1, 0);
    for (int k = 0; k < n_obs; ++k) {
        const int j = order[k];
        int32_t g;
        double dx, idt;
        mp::obs_bracket(t, x[j], g, dx, idt);   // t[g] <= x < t[g+1]; the last point: the last interval
        d.g.push_back(g);
        d.dx.push_back(dx);
        d.idt.push_back(idt);
        d.y.push_back(y[j]);
        d.yerr.push_back(yerr[j]);
        d.tile_ptr[(size_t)(g / mp::kTile) + 1] += 1;
    }
    for (size_t k = 1; k < d.tile_ptr.size(); ++k) d.tile_ptr[k] += d.tile_ptr[k - 1];
    for (Evaluator *ev : h->ev) {
        const bool replaced = ev->ds[ds_id].set;
        ev->ds[ds_id] = d;
        DeviceScope scope(ev->device);
        const int rc = upload_dataset(ev, ds_id, replaced);
        if (rc) return rc;
    }
    return MP_OK;
}

int mp_set_prior(mp_handle *h, const double *lower, const double *upper, int ndim, uint32_t log_mask) {
    if (!h) return fail(MP_EINVAL, "mp_set_prior: NULL handle");
    if (ndim < 0 || ndim > MP_MAX_NDIM) return fail(MP_EINVAL, "mp_set_prior: ndim %d out of range", ndim);
    if (ndim > 0 && (!lower || !upper)) return fail(MP_EINVAL, "mp_set_prior: NULL bounds");
    Lock lock(h->mu);
    for (Evaluator *ev : h->ev) {
        for (int i = 0; i < MP_MAX_NDIM; ++i) {
            ev->sh.lower[i] = i < ndim ? lower[i] : -INFINITY;
            ev->sh.upper[i] = i < ndim ? upper[i] : INFINITY;
        }
        ev->sh.n_prior = ndim;
        ev->sh.log_mask = log_mask;
    }
    return MP_OK;
}

static int check_batch_args(const mp_handle *h, const void *pars, int n, int ndim, const void *lnprob) {
    if (!h || !pars || !lnprob) return fail(MP_EINVAL, "lnprob batch: NULL argument");
    if (n < 0) return fail(MP_EINVAL, "lnprob batch: negative n");
    if (ndim < 6 || ndim > MP_MAX_NDIM) return fail(MP_EINVAL, "lnprob batch: ndim must be 6..9, got %d", ndim);
    if (h->first()->sh.n_ds <= 0) return fail(MP_ESTATE, "lnprob batch: no dataset registered (mp_set_dataset)");
    return MP_OK;
}

int mp_lnprob_batch_dev(mp_handle *h, const double *d_pars, const int32_t *d_ds_id, int n, int ndim,
                        double *d_lnprob, int32_t *d_status, double *d_ltot, void *stream) {
    int rc = check_batch_args(h, d_pars, n, ndim, d_lnprob);
    if (rc) return rc;
    if (h->multi) return fail(MP_ESTATE, "mp_lnprob_batch_dev: device pointers belong to ONE device; a multi-device handle serves the host-buffer entries");
    Evaluator *ev = h->first();
    Lock lock(h->mu);
    if (!d_ds_id && !ev->ds[0].set) return fail(MP_ESTATE, "lnprob batch: ds_id is NULL but dataset 0 is not set");
    DeviceScope scope(ev->device);
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
    return launch_lnprob_ordered(ev, a, (hipStream_t)stream);
}

// An evaluator's block of a host-buffer batch in two halves, so that a handle can have every device's launch in flight before
// it waits for the first: batch_begin stages the rows and enqueues the kernel on the evaluator's stream, batch_end waits and
// hands the results over.  (Caller holds the handle's lock and has validated the arguments.)
static int batch_begin(Evaluator *ev, const double *pars, const int32_t *ds_id, int n, int ndim, double *ltot_out, bool tile_log) {
    int rc;
    DeviceScope scope(ev->device);
    const size_t ng = ev->tgrid.size();
    // One page-locked staging block owned by the evaluator, mapped into the device's address space: [pars n*ndim f64 | ds_id n i32]
    // in, [lnprob n f64 | status n i32 | sweeps n i32 | tiles n i32] out.  The kernel reads a walker's 48 - 72 bytes and writes
    // its 20 bytes IN PLACE over PCIe (round 5): no copy command either way -- one launch and one wait per call where the
    // two asynchronous copies around the kernel cost as much as the kernel itself.
    const size_t in_pars = sizeof(double) * (size_t)n * ndim, in_ids = ds_id ? sizeof(int32_t) * (size_t)n : 0;
    const size_t in_bytes = (in_pars + in_ids + 7) & ~(size_t)7;
    const size_t out_bytes = (sizeof(double) + 4 * sizeof(int32_t)) * (size_t)n;   // lnprob | status | sweeps | tiles (+ pad)
    if ((rc = ev->h_io.ensure(in_bytes + out_bytes)) || (ltot_out && (rc = ev->w_curves.ensure((size_t)n * ng))))
        return rc;
    hipStream_t st = ev->stream;
    std::memcpy(ev->h_io.p, pars, in_pars);
    if (ds_id) std::memcpy(ev->h_io.p + in_pars, ds_id, in_ids);
    unsigned char *d_out = ev->h_io.dev + in_bytes;
    mp::LaunchArgs a{};
    a.pars = (const double *)ev->h_io.dev;
    a.ds_id = ds_id ? (const int32_t *)(ev->h_io.dev + in_pars) : nullptr;
    a.n = n;
    a.ndim = ndim;
    a.physical = 0;
    a.want_chi2 = 1;
    a.lnprob = (double *)d_out;
    a.status = (int32_t *)(d_out + sizeof(double) * (size_t)n);
    a.sweeps = a.status + n;
    a.tiles = a.sweeps + n;
    a.ltot = ltot_out ? ev->w_curves.p : nullptr;   // rows of walkers that fail are NaN-filled by the kernel
    if (tile_log) {
        if ((rc = ev->w_tile_log.ensure((size_t)n * MP_TILE_LOG))) return rc;
        HIP_TRY(hipMemsetAsync(ev->w_tile_log.p, 0xFF, (size_t)n * MP_TILE_LOG * sizeof(int32_t), st));
        a.tile_log = ev->w_tile_log.p;
    }
    if ((rc = launch_lnprob_ordered(ev, a, st))) return rc;
    if (tile_log) {
        ev->last_tile_log.resize((size_t)n * MP_TILE_LOG);
        HIP_TRY(hipMemcpyAsync(ev->last_tile_log.data(), ev->w_tile_log.p, (size_t)n * MP_TILE_LOG * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    } else ev->last_tile_log.clear();
    if (ltot_out)
        HIP_TRY(hipMemcpyAsync(ltot_out, ev->w_curves.p, sizeof(double) * (size_t)n * ng, hipMemcpyDeviceToHost, st));
    ev->pend_n = n;
    ev->pend_in_bytes = in_bytes;
    return MP_OK;
}

// (the block's sweeps and tiles per walker go behind those of the blocks before it)
static int batch_end(Evaluator *ev, double *lnprob_out, int32_t *status_out, std::vector<int32_t> &sweeps_out, std::vector<int32_t> &tiles_out) {
    DeviceScope scope(ev->device);
    const int n = ev->pend_n;
    HIP_TRY(hipStreamSynchronize(ev->stream));
    const unsigned char *h_out = ev->h_io.p + ev->pend_in_bytes;
    std::memcpy(lnprob_out, h_out, sizeof(double) * (size_t)n);
    const int32_t *status = (const int32_t *)(h_out + sizeof(double) * (size_t)n), *sweeps = status + n, *tiles = sweeps + n;
    if (status_out) std::memcpy(status_out, status, sizeof(int32_t) * (size_t)n);
    sweeps_out.insert(sweeps_out.end(), sweeps, sweeps + n);
    tiles_out.insert(tiles_out.end(), tiles, tiles + n);
    ev->last_tot_sweeps = ev->last_tot_tiles = 0.0;
    ev->last_cnt_ok = 0;
    for (int i = 0; i < n; ++i)
        if (status[i] == MP_STATUS_OK) { ev->last_tot_sweeps += sweeps[i]; ev->last_tot_tiles += tiles[i]; ++ev->last_cnt_ok; }
    return MP_OK;
}

int mp_lnprob_batch(mp_handle *h, const double *pars, const int32_t *ds_id, int n, int ndim, double *lnprob_out,
                    int32_t *status_out, double *ltot_out) {
    int rc = check_batch_args(h, pars, n, ndim, lnprob_out);
    if (rc) return rc;
    if (n == 0) return MP_OK;
    Lock lock(h->mu);
    const Evaluator *hd = h->first();     // (every evaluator holds the same datasets)
    if (ds_id) {
        for (int i = 0; i < n; ++i)
            if (ds_id[i] < 0 || ds_id[i] >= MP_MAX_DATASETS || !hd->ds[ds_id[i]].set)
                return fail(MP_EINVAL, "lnprob batch: walker %d refers to unset dataset %d", i, ds_id[i]);
    } else if (!hd->ds[0].set) {
        return fail(MP_ESTATE, "lnprob batch: ds_id is NULL but dataset 0 is not set");
    }
    // Contiguous blocks of ceil(n / G) rows (SURVEY.md 8(e)'s partitioning; one device: the batch is the block), every device's
    // kernel enqueued before the first is waited for; one host thread drives them all (a launch returns in microseconds, the
    // kernels run side by side).
    const int G = (int)h->ev.size(), per = (n + G - 1) / G;
    const size_t ng = hd->tgrid.size();
    int used = 0;
    for (int g = 0; g < G; ++g) {
        const int lo = std::min(g * per, n), cnt = std::min(lo + per, n) - lo;
        if (cnt <= 0) break;
        if ((rc = batch_begin(h->ev[(size_t)g], pars + (size_t)lo * ndim, ds_id ? ds_id + lo : nullptr, cnt, ndim,
                              ltot_out ? ltot_out + (size_t)lo * ng : nullptr, h->tile_log_on))) {
            for (int k = 0; k < used; ++k) (void)hipStreamSynchronize(h->ev[(size_t)k]->stream);   // nothing may still write the caller's buffers
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
        Evaluator *ev = h->ev[(size_t)g];
        const int lo = g * per;
        rc = batch_end(ev, lnprob_out + lo, status_out ? status_out + lo : nullptr, h->last_sweeps, h->last_tiles);
        if (rc && !first_rc) first_rc = rc;
        tot += ev->last_tot_sweeps; tot_tiles += ev->last_tot_tiles; cnt_ok += ev->last_cnt_ok;
    }
    if (first_rc) return first_rc;
    h->last_mean_sweeps = tot_tiles > 0.0 ? tot / tot_tiles : 0.0;
    h->last_mean_tiles = cnt_ok ? tot_tiles / (double)cnt_ok : 0.0;
    return MP_OK;
}

int mp_rhs_batch(mp_handle *h, const double *pars, int ndim, const double *t, const double *y, int n, double *dydt,
                 double *lam) {
    if (!h || !pars || !t || !y || !dydt) return fail(MP_EINVAL, "mp_rhs_batch: NULL argument");
    if (ndim < 6 || ndim > MP_MAX_NDIM) return fail(MP_EINVAL, "mp_rhs_batch: ndim must be 6..9, got %d", ndim);
    if (n < 0) return fail(MP_EINVAL, "mp_rhs_batch: negative n");
    if (n == 0) return MP_OK;
    Evaluator *ev = h->first();
    Held held(h, ev);
    // one device block: [pars n*ndim | t n | y 2n] in, [dydt 2n | lam n] out
    const size_t n_in = (size_t)n * (ndim + 3), n_out = (size_t)n * 3;
    int rc;
    if ((rc = ev->w_curves.ensure(n_in + n_out))) return rc;
    double *d = ev->w_curves.p;
    hipStream_t st = ev->stream;
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
    const int e = mp::launch_rhs(ev->sh, r, st);
    if (e) return launched(e);
    HIP_TRY(hipMemcpyAsync(dydt, r.dydt, sizeof(double) * 2 * (size_t)n, hipMemcpyDeviceToHost, st));
    if (lam) HIP_TRY(hipMemcpyAsync(lam, r.lam, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return MP_OK;
}

int mp_synchronize(mp_handle *h) {
    if (!h) return fail(MP_EINVAL, "mp_synchronize: NULL handle");
    Lock lock(h->mu);
    for (Evaluator *ev : h->ev) {
        DeviceScope scope(ev->device);
        HIP_TRY(hipStreamSynchronize(ev->stream));
    }
    return MP_OK;
}

int mp_device(const mp_handle *h) { return h ? h->first()->device : -1; }
void *mp_stream(const mp_handle *h) { return h && !h->multi ? (void *)h->first()->stream : nullptr; }   // (a multi-device handle has none: NULL)
int mp_n_grid(const mp_handle *h) { return h ? (int)h->first()->tgrid.size() : 0; }
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
    h->tile_log_on = enable != 0;
    return MP_OK;
}
int mp_last_tile_log(const mp_handle *h, int walker, int32_t *out, int n) {
    if (!h || !out || n < 0 || walker < 0) return fail(MP_EINVAL, "mp_last_tile_log: bad argument");
    // the walker's block and its row inside it (contiguous blocks of ceil(n / G) rows of the last batch)
    const int G = (int)h->ev.size(), total = (int)h->last_tiles.size(), per = (total + G - 1) / G;
    if (per <= 0 || walker >= total) return 0;
    const std::vector<int32_t> &log = h->ev[(size_t)(walker / per)]->last_tile_log;
    const size_t off = (size_t)(walker % per) * MP_TILE_LOG;
    if (off + MP_TILE_LOG > log.size()) return 0;
    int m = 0;
    while (m < n && m < MP_TILE_LOG && log[off + m] != -1) { out[m] = log[off + m]; ++m; }
    return m;
}
int mp_last_tiles(const mp_handle *h, int32_t *out, int n) {
    if (!h || !out || n < 0) return fail(MP_EINVAL, "mp_last_tiles: bad argument");
    const int m = std::min<int>(n, (int)h->last_tiles.size());
    std::copy(h->last_tiles.begin(), h->last_tiles.begin() + m, out);
    return m;
}
double mp_sweep_tol(const mp_handle *h) { return h ? h->first()->sh.sweep_tol : 0.0; }
int mp_get_policy(const mp_handle *h, double *out, int n) {
    if (!h || !out || n < 0) return fail(MP_EINVAL, "mp_get_policy: bad argument");
    const mp::DevShared &s = h->first()->sh;
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
int mp_n_simd(const mp_handle *h) { return h ? h->first()->sh.n_simd : 0; }

}  // extern "C"
