// mp_sampler.cpp — the device-resident ensemble sampler (mp_sampler_*): stretch, DE, snooker, KDE, slice, Gaussian and walk moves,
// tempering with a fixed or an adapting ladder, whole-step and walker-sharded driving.  Kernels: mp_kernels.hip, mp_slice.hip for
// the slice move, mp_normal.hip for the Gaussian and walk moves and mp_ladder.hip for the ladder's updates.
#include <memory>
#include <thread>

#include "mp_monitor.h"
#include "mp_normal.h"
#include "mp_slice.h"

struct mp_sampler {
    mp_handle *h = nullptr;         // the lock
    Evaluator *ev = nullptr;        // the device state: the handle's one evaluator
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
        double p0, p1;              // stretch: a; DE: g0 (resolved), s = sigma sqrt(3); snooker: gamma_s; KDE: f (resolved);
                                    // slice: mu0, tune_steps; Gaussian: scale0, tune_steps; walk: s (resolved: 2 .. n_comp)
    };
    std::vector<Move> moves;
    std::vector<double> move_cum;   // cumulative weights, summed in order
    // the slice move (MP_MOVE_SLICE): its per-ensemble state on the device, set up by mp_sampler_set_moves when the table has one
    bool has_slice = false;
    int64_t slice_tune = 0;         // params[1]
    int slice_steps_out = 32, slice_shrink = 64;   // mp_sampler_set_slice_limits
    DevBuf<double> d_slice_mu;      // [n_ensembles]
    DevBuf<int64_t> d_slice_cnt;    // [kSliceCnt][n_ensembles]: nexpand_s, ncontract_s, nexpand, ncontract, nfail, neval, n_tuned
    static constexpr int kSliceCnt = 7;
    // the Gaussian move (MP_MOVE_GAUSSIAN): covariance factor, mode and target of mp_sampler_set_gaussian; its per-ensemble state
    // on the device, set up by mp_sampler_set_moves when the table has one
    bool gauss_set = false, has_gauss = false;
    int gauss_mode = MP_GAUSS_VECTOR;
    double gauss_target = 0.25;
    int64_t gauss_tune = 0;         // params[1]
    DevBuf<double> d_gauss_L;       // [ndim (ndim + 1) / 2]
    DevBuf<double> d_gauss_sigma;   // [n_ensembles]
    DevBuf<int64_t> d_gauss_cnt;    // [kGaussCnt][n_ensembles]: acc_s, n_proposed, n_accepted, n_tuned
    static constexpr int kGaussCnt = 4;
    std::unique_ptr<AcfMonitor> acf;   // the autocorrelation monitor; null: off
    std::unique_ptr<PostMonitor> post; // the posterior monitor; null: off
    std::unique_ptr<ThermoMonitor> thermo;   // the thermodynamic monitor; null: off
    std::unique_ptr<ResMonitor> res;   // the sample reservoir; null: off
    // f(monitor) for every monitor that is on, in the order they are fed, up to the first that fails: its code, else MP_OK
    template <class F>
    int each_monitor(F &&f) const {
        for (ChainMonitor *m : {(ChainMonitor *)acf.get(), (ChainMonitor *)post.get(), (ChainMonitor *)thermo.get(), (ChainMonitor *)res.get()})
            if (int rc = m ? f(*m) : MP_OK) return rc;
        return MP_OK;
    }
    // ladder adaptation (mp_sampler_set_ladder_adaptation; kernels mp_ladder.hip); n_adapt = 0: off, a fixed ladder.  Every step of
    // mp_sampler_run makes one update while ladder_t < n_adapt: update t lies behind step t, so steps >= n_adapt run on the frozen
    // ladder
    int64_t n_adapt = 0, ladder_t = 0;
    double ladder_lag = 0.0, ladder_time = 0.0;
    bool ladder_history = false;
    DevBuf<double> d_gap, d_span, d_ladder_work, d_ladder_hist;
    DevBuf<int64_t> d_swaps_prev, d_ladder_dropped;
};

// the launch arguments of the ladder kernels over the sampler's buffers
static mp::LadderArgs ladder_args(const mp_sampler *s) {
    mp::LadderArgs a{};
    a.beta = s->d_beta.p; a.gap = s->d_gap.p; a.span = s->d_span.p; a.prev = s->d_swaps_prev.p; a.swaps = s->d_swaps.p;
    a.dropped = s->d_ladder_dropped.p; a.work = s->d_ladder_work.p;
    a.history = s->ladder_history ? s->d_ladder_hist.p : nullptr;
    a.n_temps = s->n_temps; a.n_groups = s->n_ensembles / s->n_temps; a.n_walkers = s->n_walkers;
    return a;
}

// Steps per chunk of mp_sampler_run when chain rows go to the device slab: the slab stays below ~256 MB
static size_t slab_chunk_cap(const mp_sampler *s, size_t perm_cap) {
    const size_t row = (size_t)s->n_total * s->ndim;
    return std::max<size_t>(1, std::min<size_t>(perm_cap, (256u << 20) / (row * sizeof(double))));
}
static size_t perm_chunk_cap(const mp_sampler *s) {
    return std::max<size_t>(1, std::min<size_t>((size_t)16 << 20, (size_t)32 * MP_BAD_WINDOW) / (size_t)s->n_total);
}

// The body of the four set functions: with the lock held and the device idle the old monitor goes; if one is asked for (`on`),
// make(the sampler's own chunk cap) puts the new one into `slot` and it is restarted, and whatever fails leaves the monitor off.
template <class M, class Make>
static int set_monitor(mp_sampler *s, std::unique_ptr<M> &slot, bool on, Make &&make) {
    Held held(s->h, s->ev);
    HIP_TRY(hipDeviceSynchronize());
    slot.reset();
    if (!on) return MP_OK;
    int rc = make(slab_chunk_cap(s, perm_chunk_cap(s)));
    if (rc) return rc;
    if ((rc = slot->restart(s->ev->stream))) slot.reset();
    return rc;
}

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
            return s->ev->ds[s->ens_ds[(size_t)x]].g.size() > s->ev->ds[s->ens_ds[(size_t)y]].g.size();
        });
        bool identity = true;
        for (int e = 0; e < s->n_ensembles; ++e) identity = identity && idx[e] == e;
        if (!identity)
            for (int e = 0; e < s->n_ensembles; ++e) g.ens_order |= (uint64_t)idx[e] << (4 * e);
    }
    return g;
}

// the slice move's launch arguments over the sampler's buffers
static mp::SliceArgs slice_args(const mp_sampler *s) {
    const size_t ne = (size_t)s->n_ensembles;
    int64_t *c = s->d_slice_cnt.p;
    mp::SliceArgs sl{};
    sl.mu = s->d_slice_mu.p;
    sl.nexpand_s = c; sl.ncontract_s = c + ne; sl.nexpand = c + 2 * ne; sl.ncontract = c + 3 * ne;
    sl.nfail = c + 4 * ne; sl.neval = c + 5 * ne; sl.n_tuned = c + 6 * ne;
    sl.tune_steps = s->slice_tune;
    sl.max_steps_out = s->slice_steps_out; sl.max_shrink = s->slice_shrink;
    return sl;
}

// the launch arguments of the Gaussian and walk moves over the sampler's buffers (walk_s: the walk move's resolved s, else 0)
static mp::NormalArgs normal_args(const mp_sampler *s, int walk_s) {
    const size_t ne = (size_t)s->n_ensembles;
    int64_t *c = s->d_gauss_cnt.p;
    mp::NormalArgs na{};
    if (s->has_gauss) {
        na.L = s->d_gauss_L.p;
        na.sigma = s->d_gauss_sigma.p;
        na.acc_s = c; na.n_proposed = c + ne; na.n_accepted = c + 2 * ne; na.n_tuned = c + 3 * ne;
    }
    na.tune_steps = s->gauss_tune;
    na.target_accept = s->gauss_target;
    na.mode = s->gauss_mode;
    na.walk_s = walk_s;
    return na;
}

extern "C" {

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
    s->h = h; s->ev = h->first(); s->n_walkers = n_walkers; s->n_ensembles = n_ensembles; s->n_total = n_walkers * n_ensembles;
    s->ndim = ndim; s->target = target; s->seed = seed; s->a = a;
    DeviceScope scope(s->ev->device);
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
    Held held(s->h, s->ev);
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
    DeviceScope scope(s->ev->device);
    std::vector<double> b((size_t)s->n_ensembles);
    for (int e = 0; e < s->n_ensembles; ++e) b[(size_t)e] = betas[e % n_temps];
    const size_t n_pairs = (size_t)(s->n_ensembles / n_temps) * (size_t)(n_temps - 1);
    int rc;
    if ((rc = s->d_beta.ensure(b.size())) || (rc = s->d_swaps.ensure(n_pairs))) return rc;
    HIP_TRY(hipMemcpy(s->d_beta.p, b.data(), b.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(s->d_swaps.p, 0, n_pairs * sizeof(int64_t)));
    s->n_temps = n_temps;
    s->n_adapt = 0;   // a new ladder is a fixed one until mp_sampler_set_ladder_adaptation says otherwise
    s->ladder_t = 0;
    return MP_OK;
}

int mp_sampler_set_ladder_adaptation(mp_sampler *s, int64_t n_adapt, double lag, double time, int keep_history) {
    if (!s) return fail(MP_EINVAL, "mp_sampler_set_ladder_adaptation: NULL sampler");
    Held held(s->h, s->ev);
    if (!s->n_temps) return fail(MP_ESTATE, "mp_sampler_set_ladder_adaptation: call mp_sampler_set_temperatures first");
    if (s->have_state) return fail(MP_ESTATE, "mp_sampler_set_ladder_adaptation: call it before the first mp_sampler_set_positions");
    if (s->n_temps < 3) return fail(MP_EINVAL, "mp_sampler_set_ladder_adaptation: both ends of the ladder stay fixed, so it needs at least 3 temperatures, got %d", s->n_temps);
    if (n_adapt < 1) return fail(MP_EINVAL, "mp_sampler_set_ladder_adaptation: n_adapt must be >= 1, got %lld", (long long)n_adapt);
    if (!std::isfinite(lag) || !(lag > 0.0) || !std::isfinite(time) || !(time > 0.0))
        return fail(MP_EINVAL, "mp_sampler_set_ladder_adaptation: lag and time must be finite and > 0, got %g and %g", lag, time);
    if (keep_history && (double)n_adapt * (double)s->n_ensembles * sizeof(double) > (double)MP_LADDER_MAX_HISTORY_BYTES)
        return fail(MP_EINVAL, "mp_sampler_set_ladder_adaptation: the history of %lld updates of %d ensembles is larger than MP_LADDER_MAX_HISTORY_BYTES = %lld",
                    (long long)n_adapt, s->n_ensembles, (long long)MP_LADDER_MAX_HISTORY_BYTES);
    const size_t n_groups = (size_t)(s->n_ensembles / s->n_temps), n_pairs = n_groups * (size_t)(s->n_temps - 1);
    int rc;
    if ((rc = s->d_gap.ensure(n_pairs)) || (rc = s->d_span.ensure(n_groups)) || (rc = s->d_ladder_work.ensure(2 * n_pairs)) ||
        (rc = s->d_swaps_prev.ensure(n_pairs)) || (rc = s->d_ladder_dropped.ensure(n_groups)) ||
        (keep_history && (rc = s->d_ladder_hist.ensure((size_t)n_adapt * (size_t)s->n_ensembles))))
        return rc;
    s->ladder_history = keep_history != 0;
    HIP_TRY(hipMemsetAsync(s->d_ladder_dropped.p, 0, n_groups * sizeof(int64_t), s->ev->stream));
    if ((rc = launched(mp::launch_ladder_init(ladder_args(s), s->ev->stream)))) return rc;
    HIP_TRY(hipStreamSynchronize(s->ev->stream));
    s->n_adapt = n_adapt; s->ladder_t = 0; s->ladder_lag = lag; s->ladder_time = time;
    return MP_OK;
}

int mp_sampler_get_temperatures(mp_sampler *s, double *betas, int64_t *n_updates, int64_t *n_dropped) {
    if (!s) return fail(MP_EINVAL, "mp_sampler_get_temperatures: NULL sampler");
    Held held(s->h, s->ev);
    if (!s->n_temps) return fail(MP_ESTATE, "mp_sampler_get_temperatures: the sampler is not tempered (mp_sampler_set_temperatures)");
    HIP_TRY(hipDeviceSynchronize());
    const size_t n_groups = (size_t)(s->n_ensembles / s->n_temps);
    if (n_updates) *n_updates = s->ladder_t;
    if (!s->n_adapt) {
        if (n_dropped) std::fill(n_dropped, n_dropped + n_groups, (int64_t)0);
        return read_back(betas, (const double *)s->d_beta.p, (size_t)s->n_ensembles);
    }
    return read_back(betas, (const double *)s->d_beta.p, (size_t)s->n_ensembles, n_dropped, (const int64_t *)s->d_ladder_dropped.p, n_groups);
}

int mp_sampler_get_ladder_history(mp_sampler *s, int group, int64_t first_row, int64_t max_rows, double *betas, int64_t *n_rows) {
    if (!s || first_row < 0 || max_rows < 0 || (max_rows > 0 && !betas)) return fail(MP_EINVAL, "mp_sampler_get_ladder_history: bad argument");
    Held held(s->h, s->ev);
    if (!s->n_adapt || !s->ladder_history)
        return fail(MP_ESTATE, "mp_sampler_get_ladder_history: the sampler keeps no ladder history (mp_sampler_set_ladder_adaptation)");
    const int n_groups = s->n_ensembles / s->n_temps;
    if (group < 0 || group >= n_groups) return fail(MP_EINVAL, "mp_sampler_get_ladder_history: group must be in [0, %d), got %d", n_groups, group);
    HIP_TRY(hipDeviceSynchronize());
    const int64_t rows = std::max<int64_t>(0, std::min<int64_t>(s->ladder_t - first_row, max_rows));
    const size_t w = (size_t)s->n_temps * sizeof(double), pitch = (size_t)s->n_ensembles * sizeof(double);
    if (rows)
        HIP_TRY(hipMemcpy2D(betas, w, s->d_ladder_hist.p + (size_t)first_row * s->n_ensembles + (size_t)group * s->n_temps, pitch, w,
                            (size_t)rows, hipMemcpyDeviceToHost));
    if (n_rows) *n_rows = rows;
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
    int slice_at = -1;   // the table's slice entry
    int gauss_at = -1;   // the table's Gaussian entry
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
        case MP_MOVE_SLICE:
            if (!std::isfinite(p0) || !(p0 > 0.0)) return fail(MP_EINVAL, "mp_sampler_set_moves: slice mu0 must be finite and > 0, got %g", p0);
            if (!(p1 >= 0.0) || !(p1 <= 2147483647.0) || p1 != std::floor(p1))
                return fail(MP_EINVAL, "mp_sampler_set_moves: slice tune_steps must be a whole number in [0, 2^31 - 1], got %g", p1);
            if (n_half < 2) return fail(MP_EINVAL, "mp_sampler_set_moves: the slice move needs n_walkers >= 4 (two partners in the other half)");
            if (slice_at >= 0) return fail(MP_EINVAL, "mp_sampler_set_moves: at most one slice move per table (entries %d and %d)", slice_at, m);
            slice_at = m;
            x.p0 = p0;
            x.p1 = p1;
            break;
        case MP_MOVE_GAUSSIAN:   // (the params first: a bad pair is MP_EINVAL whatever else is wrong)
            if (!std::isfinite(p0) || !(p0 > 0.0)) return fail(MP_EINVAL, "mp_sampler_set_moves: Gaussian scale0 must be finite and > 0, got %g", p0);
            if (!(p1 >= 0.0) || !(p1 <= 2147483647.0) || p1 != std::floor(p1))
                return fail(MP_EINVAL, "mp_sampler_set_moves: Gaussian tune_steps must be a whole number in [0, 2^31 - 1], got %g", p1);
            if (gauss_at >= 0) return fail(MP_EINVAL, "mp_sampler_set_moves: at most one Gaussian move per table (entries %d and %d)", gauss_at, m);
            if (!s->gauss_set) return fail(MP_ESTATE, "mp_sampler_set_moves: the Gaussian move needs a covariance: call mp_sampler_set_gaussian first");
            gauss_at = m;
            x.p0 = p0;
            x.p1 = p1;
            break;
        case MP_MOVE_WALK: {
            const int n_comp = s->n_walkers - n_half;
            if (!(p0 >= 0.0) || !std::isfinite(p0) || p0 != std::floor(p0))
                return fail(MP_EINVAL, "mp_sampler_set_moves: walk s must be 0 (all of the other half) or a whole number >= 2, got %g", p0);
            if (p0 == 1.0) return fail(MP_EINVAL, "mp_sampler_set_moves: walk s must be 0 or >= 2 (one member has no covariance), got 1");
            if (p1 != 0.0) return fail(MP_EINVAL, "mp_sampler_set_moves: walk params[1] must be 0, got %g", p1);
            if (n_half < 2) return fail(MP_EINVAL, "mp_sampler_set_moves: the walk move needs n_walkers >= 4 (two members in the other half)");
            if (p0 > (double)n_comp) return fail(MP_EINVAL, "mp_sampler_set_moves: walk s = %g exceeds the %d walkers of the other half", p0, n_comp);
            if (p0 != 0.0 && p0 != (double)n_comp && p0 > (double)MP_WALK_MAX_S)
                return fail(MP_EINVAL, "mp_sampler_set_moves: walk s must be at most MP_WALK_MAX_S = %d (or 0: all %d of the other half), got %g", MP_WALK_MAX_S, n_comp, p0);
            x.p0 = p0 == 0.0 ? (double)n_comp : p0;
            break;
        }
        default:
            return fail(MP_EINVAL, "mp_sampler_set_moves: unknown move kind %d", (int)kinds[m]);
        }
        mv.push_back(x);
        c += w;
        cum.push_back(c);
    }
    Held held(s->h, s->ev);
    if (slice_at >= 0) {   // the move's state starts over: mu = mu0, no step taken, the counters at zero
        const size_t ne = (size_t)s->n_ensembles;
        int rc;
        if ((rc = s->d_slice_mu.ensure(ne)) || (rc = s->d_slice_cnt.ensure(mp_sampler::kSliceCnt * ne))) return rc;
        HIP_TRY(hipDeviceSynchronize());
        const std::vector<double> mu0(ne, mv[(size_t)slice_at].p0);
        HIP_TRY(hipMemcpy(s->d_slice_mu.p, mu0.data(), ne * sizeof(double), hipMemcpyHostToDevice));
        HIP_TRY(hipMemset(s->d_slice_cnt.p, 0, mp_sampler::kSliceCnt * ne * sizeof(int64_t)));
        s->slice_tune = (int64_t)mv[(size_t)slice_at].p1;
    }
    if (gauss_at >= 0) {   // likewise: sigma = scale0, no update made, the counters at zero
        const size_t ne = (size_t)s->n_ensembles;
        int rc;
        if ((rc = s->d_gauss_sigma.ensure(ne)) || (rc = s->d_gauss_cnt.ensure(mp_sampler::kGaussCnt * ne))) return rc;
        HIP_TRY(hipDeviceSynchronize());
        const std::vector<double> s0(ne, mv[(size_t)gauss_at].p0);
        HIP_TRY(hipMemcpy(s->d_gauss_sigma.p, s0.data(), ne * sizeof(double), hipMemcpyHostToDevice));
        HIP_TRY(hipMemset(s->d_gauss_cnt.p, 0, mp_sampler::kGaussCnt * ne * sizeof(int64_t)));
        s->gauss_tune = (int64_t)mv[(size_t)gauss_at].p1;
    }
    s->has_slice = slice_at >= 0;
    s->has_gauss = gauss_at >= 0;
    s->moves = std::move(mv);
    s->move_cum = std::move(cum);
    return MP_OK;
}

int mp_sampler_set_slice_limits(mp_sampler *s, int max_steps_out, int max_shrink) {
    if (!s) return fail(MP_EINVAL, "mp_sampler_set_slice_limits: NULL sampler");
    if (max_steps_out < 1 || max_steps_out > MP_NEST_MAX_STEPS_OUT)
        return fail(MP_EINVAL, "mp_sampler_set_slice_limits: max_steps_out must be 1 .. %d, got %d", MP_NEST_MAX_STEPS_OUT, max_steps_out);
    if (max_shrink < 1 || max_shrink > MP_SLICE_MAX_SHRINK)
        return fail(MP_EINVAL, "mp_sampler_set_slice_limits: max_shrink must be 1 .. %d, got %d", MP_SLICE_MAX_SHRINK, max_shrink);
    Lock lock(s->h->mu);
    s->slice_steps_out = max_steps_out;
    s->slice_shrink = max_shrink;
    return MP_OK;
}

int mp_sampler_get_slice(mp_sampler *s, double *mu, int64_t *nexpand, int64_t *ncontract, int64_t *nfail, int64_t *neval,
                         int64_t *n_tuned) {
    if (!s) return fail(MP_EINVAL, "mp_sampler_get_slice: NULL sampler");
    Held held(s->h, s->ev);
    if (!s->has_slice) return fail(MP_ESTATE, "mp_sampler_get_slice: the move table has no slice move (mp_sampler_set_moves)");
    HIP_TRY(hipDeviceSynchronize());
    const size_t ne = (size_t)s->n_ensembles;
    const mp::SliceArgs sl = slice_args(s);
    return read_back(mu, (const double *)sl.mu, ne, nexpand, (const int64_t *)sl.nexpand, ne, ncontract, (const int64_t *)sl.ncontract, ne,
                     nfail, (const int64_t *)sl.nfail, ne, neval, (const int64_t *)sl.neval, ne, n_tuned, (const int64_t *)sl.n_tuned, ne);
}

int mp_sampler_set_gaussian(mp_sampler *s, const double *L, int mode, double target_accept) {
    if (!s || !L) return fail(MP_EINVAL, "mp_sampler_set_gaussian: NULL argument");
    if (mode != MP_GAUSS_VECTOR && mode != MP_GAUSS_RANDOM && mode != MP_GAUSS_SEQUENTIAL)
        return fail(MP_EINVAL, "mp_sampler_set_gaussian: mode must be MP_GAUSS_VECTOR, MP_GAUSS_RANDOM or MP_GAUSS_SEQUENTIAL, got %d", mode);
    if (!(target_accept > 0.0) || !(target_accept < 1.0))
        return fail(MP_EINVAL, "mp_sampler_set_gaussian: target_accept must lie in (0, 1), got %g", target_accept);
    const size_t tri = (size_t)s->ndim * (size_t)(s->ndim + 1) / 2;
    for (int a = 0; a < s->ndim; ++a)
        for (int b = 0; b <= a; ++b) {
            const double v = L[(size_t)a * (a + 1) / 2 + b];
            if (!std::isfinite(v)) return fail(MP_EINVAL, "mp_sampler_set_gaussian: L[%d][%d] is not finite", a, b);
            if (a == b && !(v > 0.0)) return fail(MP_EINVAL, "mp_sampler_set_gaussian: the diagonal of L must be > 0, got L[%d][%d] = %g", a, a, v);
            if (a != b && mode != MP_GAUSS_VECTOR && v != 0.0)
                return fail(MP_EINVAL, "mp_sampler_set_gaussian: a single-axis mode needs a diagonal covariance, got L[%d][%d] = %g", a, b, v);
        }
    Held held(s->h, s->ev);
    int rc;
    if ((rc = s->d_gauss_L.ensure(tri))) return rc;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(s->d_gauss_L.p, L, tri * sizeof(double), hipMemcpyHostToDevice));
    s->gauss_set = true;
    s->gauss_mode = mode;
    s->gauss_target = target_accept;
    return MP_OK;
}

int mp_sampler_get_gaussian(mp_sampler *s, double *sigma, int64_t *n_proposed, int64_t *n_accepted, int64_t *n_tuned) {
    if (!s) return fail(MP_EINVAL, "mp_sampler_get_gaussian: NULL sampler");
    Held held(s->h, s->ev);
    if (!s->has_gauss) return fail(MP_ESTATE, "mp_sampler_get_gaussian: the move table has no Gaussian move (mp_sampler_set_moves)");
    HIP_TRY(hipDeviceSynchronize());
    const size_t ne = (size_t)s->n_ensembles;
    const mp::NormalArgs na = normal_args(s, 0);
    return read_back(sigma, (const double *)na.sigma, ne, n_proposed, (const int64_t *)na.n_proposed, ne, n_accepted,
                     (const int64_t *)na.n_accepted, ne, n_tuned, (const int64_t *)na.n_tuned, ne);
}

int mp_sampler_get_swaps(mp_sampler *s, int64_t *n_swaps_accepted) {
    if (!s || !n_swaps_accepted) return fail(MP_EINVAL, "mp_sampler_get_swaps: NULL argument");
    Lock lock(s->h->mu);
    if (!s->n_temps) return fail(MP_ESTATE, "mp_sampler_get_swaps: the sampler is not tempered (mp_sampler_set_temperatures)");
    DeviceScope scope(s->ev->device);
    HIP_TRY(hipDeviceSynchronize());
    const size_t n_pairs = (size_t)(s->n_ensembles / s->n_temps) * (size_t)(s->n_temps - 1);
    HIP_TRY(hipMemcpy(n_swaps_accepted, s->d_swaps.p, n_pairs * sizeof(int64_t), hipMemcpyDeviceToHost));
    return MP_OK;
}

int mp_sampler_set_positions(mp_sampler *s, const double *pos) {
    if (!s || !pos) return fail(MP_EINVAL, "mp_sampler_set_positions: NULL argument");
    Evaluator *ev = s->ev;
    Held held(s->h, ev);
    const size_t nt = (size_t)s->n_total;
    for (size_t i = 0; i < nt * s->ndim; ++i)
        if (!std::isfinite(pos[i])) return fail(MP_EINVAL, "mp_sampler_set_positions: non-finite coordinate");
    HIP_TRY(hipDeviceSynchronize());   // the sharded entry points may have work in flight on a caller's stream
    s->ext_stream_work = false;
    HIP_TRY(hipMemcpyAsync(s->d_pos.p, pos, nt * s->ndim * sizeof(double), hipMemcpyHostToDevice, ev->stream));
    if (s->target == 1) {
        std::vector<double> lp(nt, 0.0);
        for (size_t k = 0; k < nt; ++k)
            for (int i = 0; i < s->ndim; ++i) lp[k] -= 0.5 * pos[k * s->ndim + i] * pos[k * s->ndim + i];
        HIP_TRY(hipMemcpyAsync(s->d_lnprob.p, lp.data(), nt * sizeof(double), hipMemcpyHostToDevice, ev->stream));
        HIP_TRY(hipStreamSynchronize(ev->stream));
    } else {
        mp::LaunchArgs a{};
        a.pars = s->d_pos.p; a.ds_id = s->d_dsid.p; a.n = s->n_total; a.ndim = s->ndim; a.want_chi2 = 1;
        a.lnprob = s->d_lnprob.p; a.status = s->d_status.p;
        const int rc = launch_lnprob_ordered(ev, a, ev->stream);
        if (rc) return rc;
        HIP_TRY(hipStreamSynchronize(ev->stream));
    }
    s->have_state = true;
    return s->each_monitor([&](ChainMonitor &m) { return m.restart(ev->stream); });   // the series is broken
}

// Enqueue step steps_done + row of mp_sampler_run on the handle's stream: split d_perm, chain row `row` of the device slab when
// chain is set, move mv (nullptr: the stretch move of mp_sampler_create).  A whole step per launch (stretch_step_kernel and the
// commit kernel) where `whole` and the move is the stretch move, else two half-step launches (the slice move: of slice_half_kernel,
// with the tune launch behind them; the Gaussian and walk moves: of normal_half_kernel, the Gaussian move with its tune launch); then the swap sweep when tempered, and behind it the ladder's update while it adapts.  fits: a whole step of this sampler fits one launch
// (`whole` is that and mp_sampler_set_whole_step).
static int enqueue_step(mp_sampler *s, const int32_t *d_perm, int row, const mp_sampler::Move *mv, bool chain, bool whole, bool fits) {
    Evaluator *ev = s->ev;
    mp::StretchArgs g = stretch_args(s, d_perm, s->steps_done + (uint64_t)row, 0);
    g.chain = chain ? s->d_chain.p : nullptr;
    g.chain_lnp = chain ? s->d_chain_lnp.p : nullptr;
    g.chain_row = row;
    if (mv) {
        g.move = mv->kind;
        if (mv->kind == MP_MOVE_STRETCH) g.a = mv->p0;
        else if (mv->kind == MP_MOVE_DE) { g.de_g0 = mv->p0; g.de_s = mv->p1; }
        else if (mv->kind == MP_MOVE_SNOOKER) g.gamma_s = mv->p0;
        else if (mv->kind == MP_MOVE_KDE) g.kde_f = mv->p0;
    }
    int e;
    if (g.move == MP_MOVE_SLICE) {
        const mp::SliceArgs sl = slice_args(s);
        e = mp::launch_slice_half(ev->sh, g, sl, ev->stream);
        g.half = 1;
        if (!e) e = mp::launch_slice_half(ev->sh, g, sl, ev->stream);
        if (!e) e = mp::launch_slice_tune(sl, s->n_ensembles, ev->stream);
    } else if (g.move == MP_MOVE_GAUSSIAN || g.move == MP_MOVE_WALK) {
        const mp::NormalArgs na = normal_args(s, g.move == MP_MOVE_WALK ? (int)mv->p0 : 0);
        e = mp::launch_normal_half(ev->sh, g, na, ev->stream);
        g.half = 1;
        if (!e) e = mp::launch_normal_half(ev->sh, g, na, ev->stream);
        if (!e && g.move == MP_MOVE_GAUSSIAN) e = mp::launch_gauss_tune(na, s->n_ensembles, s->n_walkers, ev->stream);
    } else if (whole && g.move == MP_MOVE_STRETCH) {
        g.spec = s->d_spec.p;
        e = mp::launch_stretch_step(ev->sh, g, 3 * g.n_half * g.n_ensembles, ev->stream);
        if (!e) e = mp::launch_stretch_step_commit(g, ev->stream);
    } else {
        // The stretch move by half-step launches of a sampler whose whole step fits (mp_sampler_set_whole_step(0)) is the check of
        // the whole-step launch: it runs the build that launch runs, chosen by 3 x slots, so that the two chains are one bit for
        // bit at every size.  Every other half-step launch is judged by its own size.
        const int n_slots = g.n_half * g.n_ensembles;
        const int variant_blocks = fits && g.move == MP_MOVE_STRETCH ? 3 * n_slots : n_slots;
        e = mp::launch_stretch(ev->sh, g, n_slots, variant_blocks, ev->stream);
        g.half = 1;
        if (!e) e = mp::launch_stretch(ev->sh, g, n_slots, variant_blocks, ev->stream);
    }
    if (!e && s->n_temps) e = mp::launch_stretch_swap(g, s->n_temps, s->d_swaps.p, ev->stream);
    if (!e && s->ladder_t < s->n_adapt) {   // the ladder's update t behind the sweep: the next step reads the new ladder
        mp::LadderArgs la = ladder_args(s);
        la.t = s->ladder_t;
        la.kappa = s->ladder_lag / (s->ladder_time * ((double)s->ladder_t + s->ladder_lag));
        e = mp::launch_ladder_adapt(la, ev->stream);
        if (!e) s->ladder_t += 1;
    }
    if (e) return launched(e);
    return MP_OK;
}

int mp_sampler_run(mp_sampler *s, int n_steps, double *chain, double *chain_lnprob) {
    if (!s || n_steps < 0) return fail(MP_EINVAL, "mp_sampler_run: bad argument");
    if (!s->have_state) return fail(MP_ESTATE, "mp_sampler_run: call mp_sampler_set_positions first");
    if ((chain == nullptr) != (chain_lnprob == nullptr)) return fail(MP_EINVAL, "mp_sampler_run: chain and chain_lnprob go together");
    Evaluator *ev = s->ev;
    Held held(s->h, ev);
    const size_t nt = (size_t)s->n_total, row = nt * s->ndim;
    // chunks of steps so that the device-resident chain slab stays below ~256 MB, the splits below ~64 MB, and the
    // window of failed proposals (drained after every chunk) overflows only if more than 1 in 32 proposals fails
    const size_t perm_cap = perm_chunk_cap(s);
    bool slab = chain != nullptr;   // the monitors read the chain rows from the device slab
    int monitor_cap = std::max(n_steps, 1);
    s->each_monitor([&](ChainMonitor &m) { slab = true; monitor_cap = std::min(monitor_cap, m.chunk_cap); return MP_OK; });
    const int chunk_max = (int)std::min<size_t>((size_t)monitor_cap, slab ? slab_chunk_cap(s, perm_cap) : perm_cap);
    constexpr int kSub = 8;   // steps per batch of splits: the host draws the next batch while the GPU runs this one
    int rc;
    // A whole step per launch (mp_kernels.hip stretch_step_kernel: 3 n/2 evaluations, a third of them speculative) while
    // that beats two half-step launches (mp_device.h stretch_whole_step_fits); larger ensembles fill the device with one half-step
    // at a time.
    const int n_slots = (s->n_walkers / 2) * s->n_ensembles;
    const bool fits = mp::stretch_whole_step_fits(ev->sh, 3 * (long long)n_slots);
    const bool whole = s->whole_step && fits;
    if (whole && (rc = s->d_spec.ensure((size_t)3 * n_slots * (size_t)(s->ndim + mp::kSpecExtra)))) return rc;
    if (s->ext_stream_work) {   // sharded half-steps on a caller's stream may still be updating the state
        HIP_TRY(hipDeviceSynchronize());
        s->ext_stream_work = false;
    }
    for (int done = 0; done < n_steps;) {
        const int chunk = std::min(chunk_max, n_steps - done);
        if ((rc = s->h_perm.ensure((size_t)chunk * nt * sizeof(int32_t))) || (rc = s->d_perm.ensure((size_t)chunk * nt))) return rc;
        int32_t *perm = (int32_t *)s->h_perm.p;
        if (slab) {
            if ((rc = s->d_chain.ensure((size_t)chunk * row)) || (rc = s->d_chain_lnp.ensure((size_t)chunk * nt))) return rc;
        }
        for (int sub = 0; sub < chunk; sub += kSub) {
            const int sub_end = std::min(chunk, sub + kSub);
            draw_splits(s, s->steps_done + (uint64_t)sub, sub_end - sub, perm + (size_t)sub * nt);
            int step_move[kSub];   // with a move table: the move of every step of the batch, drawn next to its splits
            for (int st = sub; st < sub_end; ++st) step_move[st - sub] = draw_move(s, s->steps_done + (uint64_t)st);
            HIP_TRY(hipMemcpyAsync(s->d_perm.p + (size_t)sub * nt, perm + (size_t)sub * nt,
                                   (size_t)(sub_end - sub) * nt * sizeof(int32_t), hipMemcpyHostToDevice, ev->stream));
            for (int st = sub; st < sub_end; ++st) {
                const mp_sampler::Move *mv = s->moves.empty() ? nullptr : &s->moves[(size_t)step_move[st - sub]];
                if ((rc = enqueue_step(s, s->d_perm.p + (size_t)st * nt, st, mv, slab, whole, fits))) return rc;
            }
        }
        const ChainRows rows{s->d_chain.p, s->d_chain_lnp.p, chunk, (int64_t)s->steps_done, s->n_adapt};
        if ((rc = s->each_monitor([&](ChainMonitor &m) { return m.feed(rows, ev->stream); }))) return rc;
        if (chain) {
            HIP_TRY(hipMemcpyAsync(chain + (size_t)done * row, s->d_chain.p, (size_t)chunk * row * sizeof(double), hipMemcpyDeviceToHost, ev->stream));
            HIP_TRY(hipMemcpyAsync(chain_lnprob + (size_t)done * nt, s->d_chain_lnp.p, (size_t)chunk * nt * sizeof(double), hipMemcpyDeviceToHost, ev->stream));
        }
        HIP_TRY(hipStreamSynchronize(ev->stream));
        if ((rc = drain_bad(s))) return rc;
        s->steps_done += (uint64_t)chunk;
        done += chunk;
    }
    return MP_OK;
}

// ---- autocorrelation monitor (mp_monitor.h AcfMonitor)
int mp_sampler_set_autocorr(mp_sampler *s, int max_lag, int64_t discard) {
    const char *fn = "mp_sampler_set_autocorr";
    if (!s) return fail(MP_EINVAL, "%s: NULL sampler", fn);
    const int rc = AcfMonitor::check(fn, max_lag, discard);   // (a bad call leaves the old monitor on)
    if (rc) return rc;
    return set_monitor(s, s->acf, max_lag != 0, [&](size_t cap) {
        return AcfMonitor::make(fn, s->n_walkers, s->n_ensembles, s->ndim, max_lag, discard, cap, &s->acf);
    });
}

int mp_sampler_get_autocorr(mp_sampler *s, double c, double *tau, int32_t *window, int64_t *n_samples) {
    if (!s) return fail(MP_EINVAL, "mp_sampler_get_autocorr: NULL sampler");
    if (!(c > 0.0) || !std::isfinite(c)) return fail(MP_EINVAL, "mp_sampler_get_autocorr: c must be finite and > 0, got %g", c);
    Held held(s->h, s->ev);
    if (n_samples) *n_samples = s->acf ? s->acf->n : 0;
    if (!s->acf) return AcfMonitor::kNames.off("mp_sampler_get_autocorr");
    const int rc = s->acf->finalise("mp_sampler_get_autocorr", c, s->ev->stream);
    return rc ? rc : s->acf->read_tau(tau, window);
}

int mp_sampler_get_acf(mp_sampler *s, int ensemble, int max_rows, double *acf) {
    if (!s || !acf || max_rows < 0) return fail(MP_EINVAL, "mp_sampler_get_acf: bad argument");
    if (ensemble < 0 || ensemble >= s->n_ensembles) return fail(MP_EINVAL, "mp_sampler_get_acf: ensemble must be in [0, %d), got %d", s->n_ensembles, ensemble);
    Held held(s->h, s->ev);
    if (!s->acf) return AcfMonitor::kNames.off("mp_sampler_get_acf");
    const int rc = s->acf->finalise("mp_sampler_get_acf", 5.0, s->ev->stream);
    return rc ? rc : s->acf->read_acf(ensemble, max_rows, acf);
}

int mp_sampler_get_autocorr_sums(mp_sampler *s, int ensemble, double *S, double *T, double *H, double *tail, double *pivot,
                                 int64_t *n_samples) {
    if (!s) return fail(MP_EINVAL, "mp_sampler_get_autocorr_sums: NULL sampler");
    if (ensemble < 0 || ensemble >= s->n_ensembles) return fail(MP_EINVAL, "mp_sampler_get_autocorr_sums: ensemble must be in [0, %d), got %d", s->n_ensembles, ensemble);
    Held held(s->h, s->ev);
    if (!s->acf) return AcfMonitor::kNames.off("mp_sampler_get_autocorr_sums");
    HIP_TRY(hipStreamSynchronize(s->ev->stream));
    return s->acf->read_sums(ensemble, S, T, H, tail, pivot, n_samples);
}

// ---- posterior monitor (mp_monitor.h PostMonitor)
int mp_sampler_set_posterior(mp_sampler *s, int bins1, int bins2, const double *lower, const double *upper, int64_t discard) {
    if (!s) return fail(MP_EINVAL, "mp_sampler_set_posterior: NULL sampler");
    return set_monitor(s, s->post, bins1 != 0, [&](size_t cap) {
        return PostMonitor::make("mp_sampler_set_posterior", s->n_walkers, s->n_ensembles, s->ndim, bins1, bins2, lower, upper, discard, cap, &s->post);
    });
}

// The prologue of the posterior read-outs: the monitor is on, the ensemble exists, and what was fed has been accumulated
static int post_ready(mp_sampler *s, const char *fn, int ensemble) {
    return s->post ? s->post->ready(fn, ensemble, s->ev->stream) : PostMonitor::kNames.off(fn);
}

int mp_sampler_get_posterior_hist1(mp_sampler *s, int ensemble, int64_t *hist1, int64_t *below, int64_t *above,
                                   int64_t *nonfinite, int64_t *n_samples) {
    if (!s) return fail(MP_EINVAL, "mp_sampler_get_posterior_hist1: NULL sampler");
    Held held(s->h, s->ev);
    const int rc = post_ready(s, "mp_sampler_get_posterior_hist1", ensemble);
    return rc ? rc : s->post->read_hist1(ensemble, hist1, below, above, nonfinite, n_samples);
}

int mp_sampler_get_posterior_hist2(mp_sampler *s, int ensemble, int64_t *hist2, int64_t *outside2) {
    if (!s) return fail(MP_EINVAL, "mp_sampler_get_posterior_hist2: NULL sampler");
    Held held(s->h, s->ev);
    const int rc = post_ready(s, "mp_sampler_get_posterior_hist2", ensemble);
    return rc ? rc : s->post->read_hist2("mp_sampler_get_posterior_hist2", ensemble, hist2, outside2);
}

int mp_sampler_get_posterior_moments(mp_sampler *s, int ensemble, double *sum1, double *sum2, double *pivot, int64_t *n_finite) {
    if (!s) return fail(MP_EINVAL, "mp_sampler_get_posterior_moments: NULL sampler");
    Held held(s->h, s->ev);
    const int rc = post_ready(s, "mp_sampler_get_posterior_moments", ensemble);
    return rc ? rc : s->post->read_moments(ensemble, sum1, sum2, pivot, n_finite);
}

int mp_sampler_get_posterior_best(mp_sampler *s, int ensemble, double *x, double *lnprob, int64_t *index) {
    if (!s) return fail(MP_EINVAL, "mp_sampler_get_posterior_best: NULL sampler");
    Held held(s->h, s->ev);
    const int rc = post_ready(s, "mp_sampler_get_posterior_best", ensemble);
    return rc ? rc : s->post->read_best(ensemble, x, lnprob, index);
}

// ---- thermodynamic monitor (mp_monitor.h ThermoMonitor)
int mp_sampler_set_thermo(mp_sampler *s, int64_t discard) {
    if (!s) return fail(MP_EINVAL, "mp_sampler_set_thermo: NULL sampler");
    return set_monitor(s, s->thermo, discard != -1, [&](size_t cap) {
        return ThermoMonitor::make("mp_sampler_set_thermo", s->n_walkers, s->n_ensembles, s->ndim, discard, cap, &s->thermo);
    });
}

int mp_sampler_get_thermo(mp_sampler *s, double *sum_lnl, int64_t *n_finite, int64_t *n_nonfinite, int64_t *n_steps) {
    if (!s) return fail(MP_EINVAL, "mp_sampler_get_thermo: NULL sampler");
    Held held(s->h, s->ev);
    if (!s->thermo) return ThermoMonitor::kNames.off("mp_sampler_get_thermo");
    HIP_TRY(hipStreamSynchronize(s->ev->stream));
    return s->thermo->read(sum_lnl, n_finite, n_nonfinite, n_steps);
}

// ---- sample reservoir (mp_monitor.h ResMonitor)
int mp_sampler_set_reservoir(mp_sampler *s, int size, uint64_t seed, int64_t discard) {
    if (!s) return fail(MP_EINVAL, "mp_sampler_set_reservoir: NULL sampler");
    return set_monitor(s, s->res, size != 0, [&](size_t cap) {
        return ResMonitor::make("mp_sampler_set_reservoir", s->n_walkers, s->n_ensembles, s->ndim, size, seed, discard, cap, &s->res);
    });
}

int mp_sampler_get_reservoir(mp_sampler *s, int ensemble, int max_rows, double *x, double *lnprob, int64_t *step, int32_t *walker,
                             uint64_t *key, int *n_rows, int64_t *n_seen) {
    if (!s) return fail(MP_EINVAL, "mp_sampler_get_reservoir: NULL sampler");
    if (max_rows < 0) return fail(MP_EINVAL, "mp_sampler_get_reservoir: max_rows must be >= 0, got %d", max_rows);
    Held held(s->h, s->ev);
    if (!s->res) return ResMonitor::kNames.off("mp_sampler_get_reservoir");
    const int rc = s->res->ready("mp_sampler_get_reservoir", ensemble, s->ev->stream);
    return rc ? rc : s->res->read(ensemble, max_rows, x, lnprob, step, walker, key, n_rows, n_seen);
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
// a tempered one, one with a move table and one with a monitor on are refused (those run through mp_sampler_run only); otherwise
// the handle's lock and device are held for the call, d_perm is the split of the current step and the sampler notes work on a
// caller's stream.
struct ShardCall {
    Held held;
    const int32_t *d_perm = nullptr;
    int rc = MP_OK;
    ShardCall(mp_sampler *s, const char *fn, void *stream) : held(s->h, s->ev) {
        if (!s->have_state) rc = fail(MP_ESTATE, "%s: call mp_sampler_set_positions first", fn);
        else if (s->n_temps) rc = fail(MP_ESTATE, "%s: a tempered sampler runs on one device only (mp_sampler_run)", fn);
        else if (!s->moves.empty())
            rc = fail(MP_ESTATE, "%s: a sampler with a move table (mp_sampler_set_moves) runs on one device only (mp_sampler_run)", fn);
        else rc = s->each_monitor([&](ChainMonitor &m) { return m.run_only(fn); });   // the first monitor that is on refuses
        if (!rc && !(rc = current_split(s, (hipStream_t)stream, &d_perm))) s->ext_stream_work = true;
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
    const int e = mp::launch_stretch(s->ev->sh, g, slot_hi - slot_lo, slot_hi - slot_lo, stream);   // (a rank's share chooses its own build)
    if (e) return launched(e);
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
    if (e) return launched(e);
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
    const int e = mp::launch_stretch_step(s->ev->sh, g, block_hi - block_lo, stream);
    if (e) return launched(e);
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
    if (e) return launched(e);
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
    Held held(s->h, s->ev);
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
    Held held(s->h, s->ev);
    const size_t nt = (size_t)s->n_total;
    HIP_TRY(hipDeviceSynchronize());
    const int rc = read_back(pos, s->d_pos.p, nt * s->ndim, lnprob, s->d_lnprob.p, nt, n_accepted, s->d_acc.p, nt);
    if (rc) return rc;
    if (steps_done) *steps_done = (int64_t)s->steps_done;
    return MP_OK;
}

}  // extern "C"
