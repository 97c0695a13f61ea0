// mp_smc.cpp — the device-resident tempered SMC sampler (mp_smc_*).  Kernels: mp_smc.hip.
#include "mp_host.h"
#include "mp_smc.h"

struct mp_smc : Resident {
    mp::SmcArgs a{};
    int n_total = 0;                // n_runs * n
    uint32_t stage = 0;             // stages launched since mp_smc_set_particles: stage t reads buffer t & 1 and writes the other
    DevBuf<double> d_x[2], d_lnl[2], d_beta, d_lnz, d_log;
    DevBuf<int32_t> d_st[2], d_acc, d_dsid, d_anc, d_status, d_nstage;
    DevBuf<uint32_t> d_units;
    DevBuf<unsigned long long> d_cum;
    DevBuf<int64_t> d_ncall, d_nacc, d_nfail, d_logcnt;
    DevBuf<double> d_g, d_tlog;     // adaptation: the runs' scale, the tuning log ...
    DevBuf<int32_t> d_rounds, d_moving, d_trounds;   // ... the flags of the current stage and the rounds of every stage
    std::vector<double> g_start;    // g0 per run: what mp_smc_set_particles uploads to g
    double *x[2] = {nullptr, nullptr}, *lnl[2] = {nullptr, nullptr};
    int32_t *st[2] = {nullptr, nullptr};
};

namespace {

constexpr int kSmcChunk = 8;   // stages enqueued between two looks at the runs' status
static_assert(MP_SMC_RUNNING == 0, "groups_running counts the flags that are 0");

// the buffers of stage t (mode 1: of the evaluation of buffer 0 as it is)
void point_at(mp_smc *s, uint32_t t) {
    const int c = (int)(t & 1u);
    s->a.x_cur = s->x[c]; s->a.x_next = s->x[c ^ 1];
    s->a.lnl_cur = s->lnl[c]; s->a.lnl_next = s->lnl[c ^ 1];
    s->a.st_cur = s->st[c]; s->a.st_next = s->st[c ^ 1];
}

}  // namespace

extern "C" {

void *mp_smc_create(mp_handle *h, int n_particles, int n_runs, int ndim, const int32_t *run_ds_id, uint64_t seed,
                    const double *lower, const double *upper, double ess, int walks, double g0, double sigma, int target) {
    return resident_create<mp_smc>(
        h, "mp_smc_create", "the SMC sampler lives on ONE device (a multi-device handle serves host-buffer batches only)",
        ndim, target, "run", n_runs, run_ds_id, 1, lower, upper,
        [&] {
            if (n_particles < MP_SMC_MIN_PARTICLES || n_particles > MP_SMC_MAX_PARTICLES)
                return fail(MP_EINVAL, "mp_smc_create: n_particles must be %d .. %d, got %d", MP_SMC_MIN_PARTICLES, MP_SMC_MAX_PARTICLES, n_particles);
            if (n_runs < 1 || n_runs > MP_MAX_DATASETS) return fail(MP_EINVAL, "mp_smc_create: n_runs must be 1 .. %d", MP_MAX_DATASETS);
            if (target < 0 || target > 2) return fail(MP_EINVAL, "mp_smc_create: target must be 0 (posterior), 1 (unit Gaussian) or 2 (terraced Gaussian)");
            if (!(ess > 0.0 && ess < 1.0)) return fail(MP_EINVAL, "mp_smc_create: ess must lie in (0, 1)");
            if (walks < 1 || walks > MP_SMC_MAX_WALKS) return fail(MP_EINVAL, "mp_smc_create: walks must be 1 .. %d", MP_SMC_MAX_WALKS);
            if (!std::isfinite(g0)) return fail(MP_EINVAL, "mp_smc_create: g0 must be finite (<= 0: the default)");
            if (!(sigma >= 0.0 && sigma < 1.0 / std::sqrt(3.0))) return fail(MP_EINVAL, "mp_smc_create: sigma must lie in [0, 1/sqrt(3))");
            return check_box("mp_smc_create", ndim, lower, upper);
        },
        [&](mp_smc *s, Binder &bind) {
            s->n_total = n_particles * n_runs;
            mp::SmcArgs &a = s->a;
            a.n = n_particles; a.n_runs = n_runs; a.ndim = ndim; a.walks = walks; a.target = target; a.seed = seed;
            a.g0 = g0 > 0.0 ? g0 : 2.38 / std::sqrt(2.0 * ndim);
            a.sig3 = sigma * std::sqrt(3.0);
            a.ess = ess;
            const size_t nt = (size_t)s->n_total, nr = (size_t)n_runs, nl = nr * MP_SMC_MAX_STAGES;
            for (int c = 0; c < 2; ++c) { bind(s->d_x[c], nt * ndim, s->x[c]); bind(s->d_lnl[c], nt, s->lnl[c]); bind(s->d_st[c], nt, s->st[c]); }
            bind(s->d_acc, nt, a.acc); bind(s->d_dsid, nr, a.ds_id); bind(s->d_anc, nt, a.anc); bind(s->d_units, nt, a.units); bind(s->d_cum, nt, a.cum);
            bind(s->d_beta, nr, a.beta); bind(s->d_lnz, nr, a.lnz); bind(s->d_status, nr, a.status); bind(s->d_nstage, nr, a.nstage);
            bind(s->d_ncall, nr, a.ncall); bind(s->d_nacc, nr, a.nacc); bind(s->d_nfail, nr, a.nfail);
            bind(s->d_log, nl * mp::kSmcLogCols, a.log); bind(s->d_logcnt, nl * 2, a.log_cnt);
            bind(s->d_g, nr, a.g); bind(s->d_rounds, nr, a.rounds); bind(s->d_moving, nr, a.moving);
            bind(s->d_trounds, nl, a.tune_rounds); bind(s->d_tlog, nl * mp::kSmcTuneCols, a.tune_log);
            s->g_start.assign(nr, a.g0);
        });
}

int mp_smc_set_adaptive(void *sv, int min_rounds, int max_rounds, double corr, double gain, double accept_target, double g_min,
                        double g_max) {
    mp_smc *s = (mp_smc *)sv;
    if (!s) return fail(MP_EINVAL, "mp_smc_set_adaptive: NULL sampler");
    Held held(s->h, s->ev);
    if (s->have_state) return fail(MP_ESTATE, "mp_smc_set_adaptive: call it before mp_smc_set_particles");
    mp::SmcArgs &a = s->a;
    if (max_rounds == 0) {
        a.adapt_min = a.adapt_max = 0;
        return MP_OK;
    }
    if (max_rounds < 0 || min_rounds < 1 || min_rounds > max_rounds)
        return fail(MP_EINVAL, "mp_smc_set_adaptive: min_rounds must be 1 .. max_rounds (max_rounds = 0: off)");
    if ((long long)a.walks * max_rounds > MP_SMC_MAX_WALKS)
        return fail(MP_EINVAL, "mp_smc_set_adaptive: walks * max_rounds must be <= %d", MP_SMC_MAX_WALKS);
    if (!(corr >= 0.0 && corr < 1.0)) return fail(MP_EINVAL, "mp_smc_set_adaptive: corr must lie in [0, 1)");
    if (!(gain >= 0.0) || !std::isfinite(gain)) return fail(MP_EINVAL, "mp_smc_set_adaptive: gain must be finite and >= 0");
    if (!(accept_target > 0.0 && accept_target < 1.0)) return fail(MP_EINVAL, "mp_smc_set_adaptive: accept_target must lie in (0, 1)");
    if (std::isnan(g_min) || std::isnan(g_max)) return fail(MP_EINVAL, "mp_smc_set_adaptive: g_min and g_max must be finite");
    const double lo = g_min > 0.0 ? g_min : a.g0 / 16.0, hi = g_max > 0.0 ? g_max : 4.0 * a.g0;
    if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo <= a.g0 && a.g0 <= hi))
        return fail(MP_EINVAL, "mp_smc_set_adaptive: need 0 < g_min <= g0 <= g_max, finite (<= 0: g0 / 16 and 4 g0)");
    a.adapt_min = min_rounds; a.adapt_max = max_rounds;
    a.corr = corr; a.gain = gain; a.accept_target = accept_target; a.g_min = lo; a.g_max = hi;
    return MP_OK;
}

int mp_smc_destroy(void *sv) { return resident_destroy((mp_smc *)sv); }

int mp_smc_set_particles(void *sv, const double *particles) {
    mp_smc *s = (mp_smc *)sv;
    if (!s || !particles) return fail(MP_EINVAL, "mp_smc_set_particles: NULL argument");
    Evaluator *ev = s->ev;
    mp::SmcArgs &a = s->a;
    const size_t nt = (size_t)s->n_total, nr = (size_t)a.n_runs;
    int rc = check_inside("mp_smc_set_particles: particle", particles, nt, a.ndim, a.lower, a.upper);
    if (rc) return rc;
    Held held(s->h, ev);
    HIP_TRY(hipMemcpyAsync(s->x[0], particles, nt * a.ndim * sizeof(double), hipMemcpyHostToDevice, ev->stream));
    // (beta and lnz: all bits zero is 0.0)
    if ((rc = zero_async(ev->stream, a.beta, nr, a.lnz, nr, a.status, nr, a.nstage, nr, a.ncall, nr, a.nacc, nr, a.nfail, nr, a.anc, nt)))
        return rc;
    if ((rc = zero_async(ev->stream, a.rounds, nr, a.moving, nr))) return rc;
    HIP_TRY(hipMemcpyAsync(a.g, s->g_start.data(), nr * sizeof(double), hipMemcpyHostToDevice, ev->stream));
    point_at(s, 0);
    a.round = 0;
    a.mode = 1;
    a.stage = 0;
    if ((rc = launched(mp::launch_smc_move(ev->sh, a, ev->stream)))) return rc;
    HIP_TRY(hipStreamSynchronize(ev->stream));
    s->stage = 0;
    s->have_state = true;
    return MP_OK;
}

int mp_smc_run(void *sv, int max_stages, int *n_running) {
    mp_smc *s = (mp_smc *)sv;
    RESIDENT_ENTER(s, max_stages >= 0, "mp_smc_run", "bad argument", "mp_smc_set_particles");
    // Chunks of stages (stage, move, stage, move, ...); a run that stopped inside a chunk ignores the chunk's later launches.
    // Adaptive: a stage is stage, then adapt_max times (move, tune), enqueued without a look: the runs' flags on the device say
    // which of the rounds are theirs.
    return run_chunked(s->ev, s->a.status, s->a.n_runs, kSmcChunk, max_stages, n_running, [&] {
        mp::SmcArgs &a = s->a;
        a.stage = s->stage++;
        a.mode = 0;
        a.round = 0;
        point_at(s, a.stage);
        int e = mp::launch_smc_stage(a, s->ev->stream);
        if (!e) e = mp::launch_smc_move(s->ev->sh, a, s->ev->stream);
        for (int k = 0; !e && k < a.adapt_max; ++k) {
            a.round = k;
            if (k) e = mp::launch_smc_move(s->ev->sh, a, s->ev->stream);
            if (!e) e = mp::launch_smc_tune(a, s->ev->stream);
        }
        return launched(e);
    });
}

int mp_smc_get_state(void *sv, double *x, double *lnl, int32_t *status, int32_t *acc, double *beta, double *lnz, int32_t *nstage,
                     int32_t *run_status, int64_t *ncall, int64_t *nacc, int64_t *nfail) {
    mp_smc *s = (mp_smc *)sv;
    RESIDENT_READ(s, true, "mp_smc_get_state", "NULL sampler", "mp_smc_set_particles");
    const mp::SmcArgs &a = s->a;
    const size_t nt = (size_t)s->n_total, nr = (size_t)a.n_runs, n = (size_t)a.n;
    // a run's particles lie in the buffer its last stage's moves wrote: stage t writes buffer (t + 1) & 1
    std::vector<int32_t> made(nr);
    HIP_TRY(hipMemcpy(made.data(), a.nstage, nr * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (size_t r = 0; r < nr; ++r) {
        const int c = made[r] & 1;
        const int rc = read_back(x ? x + r * n * a.ndim : nullptr, (const double *)s->x[c] + r * n * a.ndim, n * a.ndim,
                                 lnl ? lnl + r * n : nullptr, (const double *)s->lnl[c] + r * n, n,
                                 status ? status + r * n : nullptr, (const int32_t *)s->st[c] + r * n, n);
        if (rc) return rc;
    }
    if (nstage) std::copy(made.begin(), made.end(), nstage);
    return read_back(acc, (const int32_t *)a.acc, nt, beta, (const double *)a.beta, nr, lnz, (const double *)a.lnz, nr,
                     run_status, (const int32_t *)a.status, nr, ncall, (const int64_t *)a.ncall, nr, nacc, (const int64_t *)a.nacc, nr,
                     nfail, (const int64_t *)a.nfail, nr);
}

int mp_smc_get_stages(void *sv, int run, int max_rows, double *beta, double *d, double *ess, double *lnz, double *accept,
                      int64_t *ncall, int *n_rows) {
    mp_smc *s = (mp_smc *)sv;
    RESIDENT_READ(s, run >= 0 && run < s->a.n_runs && max_rows >= 0, "mp_smc_get_stages", "bad argument", "mp_smc_set_particles");
    const mp::SmcArgs &a = s->a;
    int32_t made = 0;
    int64_t tot[2];
    HIP_TRY(hipMemcpy(&made, a.nstage + run, sizeof(int32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&tot[0], a.ncall + run, sizeof(int64_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&tot[1], a.nacc + run, sizeof(int64_t), hipMemcpyDeviceToHost));
    std::vector<double> rows((size_t)made * mp::kSmcLogCols);
    std::vector<int64_t> cnt((size_t)made * 2 + 2);
    if (made) {
        HIP_TRY(hipMemcpy(rows.data(), a.log + (size_t)run * MP_SMC_MAX_STAGES * mp::kSmcLogCols, rows.size() * sizeof(double), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(cnt.data(), a.log_cnt + (size_t)run * MP_SMC_MAX_STAGES * 2, (size_t)made * 2 * sizeof(int64_t), hipMemcpyDeviceToHost));
    }
    cnt[(size_t)made * 2] = tot[0];        // behind the last stage: the totals as they stand
    cnt[(size_t)made * 2 + 1] = tot[1];
    std::vector<int32_t> rounds((size_t)made, 1);   // the rounds of `walks` steps every stage made
    if (made && a.adapt_max)
        HIP_TRY(hipMemcpy(rounds.data(), a.tune_rounds + (size_t)run * MP_SMC_MAX_STAGES, (size_t)made * sizeof(int32_t), hipMemcpyDeviceToHost));
    const int k_end = std::min((int)made, max_rows);
    for (int k = 0; k < k_end; ++k) {
        const double *row = rows.data() + (size_t)k * mp::kSmcLogCols;
        if (beta) beta[k] = row[0];
        if (d) d[k] = row[1];
        if (ess) ess[k] = row[2];
        if (lnz) lnz[k] = row[3];
        if (accept) accept[k] = (double)(cnt[2 * k + 3] - cnt[2 * k + 1]) / ((double)a.n * (double)(a.walks * rounds[k]));
        if (ncall) ncall[k] = cnt[2 * k + 2] - cnt[2 * k];
    }
    if (n_rows) *n_rows = made;
    return MP_OK;
}

int mp_smc_get_tuning(void *sv, int run, int max_rows, int32_t *rounds, double *g, double *rho, int *n_rows) {
    mp_smc *s = (mp_smc *)sv;
    RESIDENT_READ(s, run >= 0 && run < s->a.n_runs && max_rows >= 0, "mp_smc_get_tuning", "bad argument", "mp_smc_set_particles");
    const mp::SmcArgs &a = s->a;
    int32_t made = 0;
    HIP_TRY(hipMemcpy(&made, a.nstage + run, sizeof(int32_t), hipMemcpyDeviceToHost));
    // without adaptation: one round at g0, no rho
    std::vector<int32_t> nr((size_t)made, 1);
    std::vector<double> rows((size_t)made * mp::kSmcTuneCols);
    for (int k = 0; k < made; ++k) { rows[(size_t)k * mp::kSmcTuneCols] = a.g0; rows[(size_t)k * mp::kSmcTuneCols + 1] = NAN; }
    if (made && a.adapt_max) {
        HIP_TRY(hipMemcpy(nr.data(), a.tune_rounds + (size_t)run * MP_SMC_MAX_STAGES, nr.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(rows.data(), a.tune_log + (size_t)run * MP_SMC_MAX_STAGES * mp::kSmcTuneCols, rows.size() * sizeof(double), hipMemcpyDeviceToHost));
    }
    const int k_end = std::min((int)made, max_rows);
    for (int k = 0; k < k_end; ++k) {
        if (rounds) rounds[k] = nr[k];
        if (g) g[k] = rows[(size_t)k * mp::kSmcTuneCols];
        if (rho) rho[k] = rows[(size_t)k * mp::kSmcTuneCols + 1];
    }
    if (n_rows) *n_rows = made;
    return MP_OK;
}

int mp_smc_get_ancestors(void *sv, int32_t *anc) {
    mp_smc *s = (mp_smc *)sv;
    RESIDENT_READ(s, anc, "mp_smc_get_ancestors", "NULL argument", "mp_smc_set_particles");
    return read_back(anc, (const int32_t *)s->a.anc, (size_t)s->n_total);
}

}  // extern "C"
