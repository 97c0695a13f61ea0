// mp_monitor.cpp — the host side of the sampler's autocorrelation, posterior and thermodynamic monitors and of its sample reservoir
// (mp_monitor.h).  Kernels: mp_acf.hip, mp_post.hip, thermo_kernel of mp_ladder.hip, mp_reservoir.hip.
#include "mp_monitor.h"

// ---- what the four share
int MonitorNames::off(const char *fn) const { return fail(MP_ESTATE, "%s: %s is off (%s)", fn, what, setter); }

int ChainMonitor::run_only(const char *fn) const { return fail(MP_ESTATE, "%s: %s (%s) is fed by mp_sampler_run only; turn it off first", fn, names.what, names.setter); }

int ChainMonitor::check_discard(const char *fn, int64_t discard, const char *clause) {
    return discard < 0 ? fail(MP_EINVAL, "%s: discard must be >= 0%s, got %lld", fn, clause, (long long)discard) : MP_OK;
}

int ChainMonitor::ready(const char *fn, int ensemble, hipStream_t st) const {
    if (ensemble < 0 || ensemble >= n_ensembles) return fail(MP_EINVAL, "%s: ensemble must be in [0, %d), got %d", fn, n_ensembles, ensemble);
    HIP_TRY(hipStreamSynchronize(st));
    return MP_OK;
}

// ---- autocorrelation monitor
const MonitorNames AcfMonitor::kNames = {"the autocorrelation monitor", "mp_sampler_set_autocorr"};

int AcfMonitor::check(const char *fn, int max_lag, int64_t discard) {
    if (max_lag < 0 || max_lag > MP_ACF_MAX_LAG) return fail(MP_EINVAL, "%s: max_lag must be in [0, %d] (MP_ACF_MAX_LAG; 0 turns the monitor off), got %d", fn, MP_ACF_MAX_LAG, max_lag);
    return check_discard(fn, discard);
}

int AcfMonitor::make(const char *fn, int n_walkers, int n_ensembles, int ndim, int max_lag, int64_t discard, size_t sampler_cap,
                     std::unique_ptr<AcfMonitor> *out) {
    std::unique_ptr<AcfMonitor> m(new AcfMonitor(kNames, n_walkers, n_ensembles, ndim, discard, sampler_cap));
    const size_t ns = (size_t)m->n_total * ndim;
    const int kp = (max_lag + mp::kAcfLagBlock - 1) / mp::kAcfLagBlock * mp::kAcfLagBlock;
    const size_t ring = (size_t)kp + (size_t)m->chunk_cap;   // the ring holds one chunk behind the kp rows it keeps
    const double bytes = ((double)ring + 3.0 * kp + 2.0) * (double)ns * sizeof(double);   // ring, S, H, rho, T, pivot
    if (bytes > (double)MP_ACF_MAX_BYTES)
        return fail(MP_EINVAL, "%s: max_lag = %d over %zu series needs %.0f bytes of accumulators, more than MP_ACF_MAX_BYTES = %lld: lower max_lag",
                    fn, max_lag, ns, bytes, (long long)MP_ACF_MAX_BYTES);
    m->max_lag = max_lag; m->kp = kp; m->ring_rows = (int)ring;
    const size_t ned = (size_t)n_ensembles * ndim;
    int rc;
    if ((rc = m->hist.ensure(ring * ns)) || (rc = m->S.ensure((size_t)kp * ns)) || (rc = m->H.ensure((size_t)kp * ns)) ||
        (rc = m->rho.ensure((size_t)kp * ns)) || (rc = m->T.ensure(ns)) || (rc = m->pivot.ensure(ns)) ||
        (rc = m->f.ensure(ned * kp)) || (rc = m->tau.ensure(ned)) || (rc = m->window.ensure(ned)))
        return rc;
    *out = std::move(m);
    return MP_OK;
}

mp::AcfArgs AcfMonitor::args(const double *chain) const {
    mp::AcfArgs a{};
    a.chain = chain; a.hist = hist.p; a.S = S.p; a.T = T.p; a.H = H.p; a.pivot = pivot.p;
    a.rho = rho.p; a.f = f.p; a.tau = tau.p; a.window = window.p;
    a.n_series = n_total * ndim; a.n_walkers = n_walkers; a.n_ensembles = n_ensembles; a.ndim = ndim;
    a.kp = kp; a.max_lag = max_lag; a.ring_rows = ring_rows; a.head = head; a.n0 = n;
    return a;
}

int AcfMonitor::restart(hipStream_t st) {
    const size_t ns = (size_t)n_total * ndim;
    HIP_TRY(hipMemsetAsync(hist.p, 0, (size_t)ring_rows * ns * sizeof(double), st));
    HIP_TRY(hipMemsetAsync(S.p, 0, (size_t)kp * ns * sizeof(double), st));
    HIP_TRY(hipMemsetAsync(H.p, 0, (size_t)kp * ns * sizeof(double), st));
    HIP_TRY(hipMemsetAsync(T.p, 0, ns * sizeof(double), st));
    HIP_TRY(hipMemsetAsync(pivot.p, 0, ns * sizeof(double), st));
    head = 0;
    start_over();
    return MP_OK;
}

int AcfMonitor::feed(const ChainRows &c, hipStream_t st) {
    mp::AcfArgs a = args(c.chain);
    a.rows = take(c.rows, &a.first);
    if (a.rows == 0) return MP_OK;
    const int rc = launched(mp::launch_acf_accumulate(a, st));
    if (rc) return rc;
    head = (head + a.rows) % ring_rows;
    n += a.rows;
    return MP_OK;
}

int AcfMonitor::finalise(const char *fn, double c, hipStream_t st) {
    if (n < 2) return fail(MP_ESTATE, "%s: the monitor holds %lld samples, an estimate needs 2 or more", fn, (long long)n);
    mp::AcfArgs a = args(nullptr);
    a.c = c;
    const int rc = launched(mp::launch_acf_finalise(a, st));
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return MP_OK;
}

int AcfMonitor::read_tau(double *tau_out, int32_t *window_out) const {
    const size_t ned = (size_t)n_ensembles * ndim;
    return read_back(tau_out, (const double *)tau.p, ned, window_out, (const int32_t *)window.p, ned);
}

int AcfMonitor::read_acf(int ensemble, int max_rows, double *acf) const {
    const int rows = (int)std::min<int64_t>({(int64_t)max_rows, (int64_t)max_lag, n});
    std::vector<double> fk((size_t)ndim * kp);
    HIP_TRY(hipMemcpy(fk.data(), f.p + (size_t)ensemble * ndim * kp, fk.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int k = 0; k < rows; ++k)
        for (int d = 0; d < ndim; ++d) acf[(size_t)k * ndim + d] = fk[(size_t)d * kp + k];
    return rows;
}

int AcfMonitor::read_sums(int ensemble, double *S_out, double *T_out, double *H_out, double *tail, double *pivot_out,
                          int64_t *n_samples) const {
    const size_t ns = (size_t)n_total * ndim, w = (size_t)n_walkers * ndim, col0 = (size_t)ensemble * w;
    const size_t K = (size_t)max_lag;
    // rows [r0, r0 + rows) of a [.][n_series] device array, the ensemble's columns -> dst[rows][n_walkers][ndim]
    auto cols = [&](double *dst, const double *src, size_t r0, size_t rows) {
        return rows == 0 ? hipSuccess
                         : hipMemcpy2D(dst, w * sizeof(double), src + r0 * ns + col0, ns * sizeof(double), w * sizeof(double), rows, hipMemcpyDeviceToHost);
    };
    if (S_out) HIP_TRY(cols(S_out, S.p, 0, K));
    if (T_out) HIP_TRY(cols(T_out, T.p, 0, 1));
    if (pivot_out) HIP_TRY(cols(pivot_out, pivot.p, 0, 1));
    if (H_out) {
        HIP_TRY(cols(H_out, H.p, 0, K));
        std::vector<double> t(w);
        HIP_TRY(cols(t.data(), T.p, 0, 1));
        for (size_t k = (size_t)std::min<int64_t>(n, (int64_t)K - 1) + 1; k < K; ++k)   // H_k = T once k >= n
            std::memcpy(H_out + k * w, t.data(), w * sizeof(double));
    }
    if (tail) {   // samples n - K .. n - 1: the K ring rows behind the head, zeros before sample 0
        const size_t start = ((size_t)head + (size_t)ring_rows - K) % (size_t)ring_rows;
        const size_t a_rows = std::min(K, (size_t)ring_rows - start);
        HIP_TRY(cols(tail, hist.p, start, a_rows));
        HIP_TRY(cols(tail + a_rows * w, hist.p, 0, K - a_rows));
    }
    if (n_samples) *n_samples = n;
    return MP_OK;
}

// ---- posterior monitor
const MonitorNames PostMonitor::kNames = {"the posterior monitor", "mp_sampler_set_posterior"};

int PostMonitor::make(const char *fn, int n_walkers, int n_ensembles, int ndim, int bins1, int bins2, const double *lower,
                      const double *upper, int64_t discard, size_t sampler_cap, std::unique_ptr<PostMonitor> *out) {
    if (bins1 < 0 || bins1 > MP_POST_MAX_BINS) return fail(MP_EINVAL, "%s: bins1 must be in [0, %d] (MP_POST_MAX_BINS; 0 turns the monitor off), got %d", fn, MP_POST_MAX_BINS, bins1);
    if (bins2 < 0 || bins2 > MP_POST_MAX_BINS2) return fail(MP_EINVAL, "%s: bins2 must be in [0, %d] (MP_POST_MAX_BINS2; 0: no 2-D histograms), got %d", fn, MP_POST_MAX_BINS2, bins2);
    if (int rc = check_discard(fn, discard)) return rc;
    if (!lower || !upper) return fail(MP_EINVAL, "%s: NULL range", fn);
    for (int d = 0; d < ndim; ++d)
        if (!std::isfinite(lower[d]) || !std::isfinite(upper[d]) || !(lower[d] < upper[d]) || !std::isfinite(upper[d] - lower[d]))
            return fail(MP_EINVAL, "%s: range of dimension %d must be finite with lower < upper, got [%g, %g]", fn, d, lower[d], upper[d]);
    if (n_ensembles > 65535) return fail(MP_EINVAL, "%s: at most 65535 ensembles, got %d", fn, n_ensembles);
    std::unique_ptr<PostMonitor> m(new PostMonitor(kNames, n_walkers, n_ensembles, ndim, discard, sampler_cap));
    const size_t ne = (size_t)n_ensembles, nt = (size_t)m->n_total, nd = (size_t)ndim;
    const size_t np = (size_t)mp::post_n_pairs(ndim), nent = (size_t)mp::post_n_entries(ndim);
    const size_t n_h1 = ne * nd * mp::post_stride1(bins1), n_h2 = ne * np * (size_t)bins2 * bins2;
    const double bytes = 8.0 * ((double)n_h1 + (double)n_h2 + (double)(ne * np) + (double)(ne * (nd + 2)) + (double)nt * (double)(nent + 1));
    if (bytes > (double)MP_POST_MAX_BYTES)
        return fail(MP_EINVAL, "%s: bins1 = %d, bins2 = %d over %d ensembles of %d dimensions need %.0f bytes of accumulators, more than MP_POST_MAX_BYTES = %lld: lower the bin counts",
                    fn, bins1, bins2, n_ensembles, ndim, bytes, (long long)MP_POST_MAX_BYTES);
    m->bins1 = bins1; m->bins2 = bins2;
    m->par.resize(5 * nd);
    mp::post_params(m->par.data(), ndim, bins1, bins2, lower, upper);
    int rc;
    if ((rc = m->d_par.ensure(5 * nd)) || (rc = m->hist1.ensure(n_h1)) || (rc = m->hist2.ensure(n_h2)) || (rc = m->outside2.ensure(ne * np)) ||
        (rc = m->mom.ensure(nent * nt)) || (rc = m->nfin.ensure(nt)) || (rc = m->best_x.ensure(ne * nd)) || (rc = m->best_lnp.ensure(ne)) ||
        (rc = m->best_idx.ensure(ne)))
        return rc;
    HIP_TRY(hipMemcpy(m->d_par.p, m->par.data(), 5 * nd * sizeof(double), hipMemcpyHostToDevice));
    *out = std::move(m);
    return MP_OK;
}

mp::PostArgs PostMonitor::args(const double *chain, const double *lnp) const {
    mp::PostArgs a{};
    a.chain = chain; a.lnp = lnp; a.par = d_par.p;
    a.hist1 = hist1.p; a.hist2 = hist2.p; a.outside2 = outside2.p; a.mom = mom.p; a.nfin = nfin.p;
    a.best_x = best_x.p; a.best_lnp = best_lnp.p; a.best_idx = best_idx.p;
    a.n_walkers = n_walkers; a.n_ensembles = n_ensembles; a.n_total = n_total; a.ndim = ndim;
    a.bins1 = bins1; a.bins2 = bins2; a.n0 = n;
    return a;
}

int PostMonitor::restart(hipStream_t st) {
    const size_t ne = (size_t)n_ensembles, nt = (size_t)n_total, nd = (size_t)ndim, np = (size_t)mp::post_n_pairs(ndim);
    HIP_TRY(hipMemsetAsync(hist1.p, 0, ne * nd * mp::post_stride1(bins1) * sizeof(int64_t), st));
    if (bins2 && np) {
        HIP_TRY(hipMemsetAsync(hist2.p, 0, ne * np * (size_t)bins2 * bins2 * sizeof(int64_t), st));
        HIP_TRY(hipMemsetAsync(outside2.p, 0, ne * np * sizeof(int64_t), st));
    }
    HIP_TRY(hipMemsetAsync(mom.p, 0, (size_t)mp::post_n_entries(ndim) * nt * sizeof(double), st));
    HIP_TRY(hipMemsetAsync(nfin.p, 0, nt * sizeof(int64_t), st));
    const int rc = launched(mp::launch_post_reset(args(nullptr, nullptr), st));
    if (rc) return rc;
    start_over();
    return MP_OK;
}

int PostMonitor::feed(const ChainRows &c, hipStream_t st) {
    mp::PostArgs a = args(c.chain, c.lnp);
    a.rows = take(c.rows, &a.first);
    if (a.rows == 0) return MP_OK;
    const int rc = launched(mp::launch_post_accumulate(a, st));
    if (rc) return rc;
    n += a.rows;
    return MP_OK;
}

int PostMonitor::read_hist1(int ensemble, int64_t *hist1_out, int64_t *below, int64_t *above, int64_t *nonfinite,
                            int64_t *n_samples) const {
    const size_t nd = (size_t)ndim, B = (size_t)bins1, stride = (size_t)mp::post_stride1(bins1);
    std::vector<int64_t> h(nd * stride);
    HIP_TRY(hipMemcpy(h.data(), hist1.p + (size_t)ensemble * nd * stride, h.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
    for (size_t d = 0; d < nd; ++d) {
        const int64_t *row = h.data() + d * stride;
        if (hist1_out) std::memcpy(hist1_out + d * B, row, B * sizeof(int64_t));
        if (below) below[d] = row[B];
        if (above) above[d] = row[B + 1];
        if (nonfinite) nonfinite[d] = row[B + 2];
    }
    if (n_samples) *n_samples = n * n_walkers;
    return MP_OK;
}

int PostMonitor::read_hist2(const char *fn, int ensemble, int64_t *hist2_out, int64_t *outside2_out) const {
    if (!bins2) return fail(MP_ESTATE, "%s: the monitor keeps no 2-D histograms (bins2 = 0)", fn);
    const size_t np = (size_t)mp::post_n_pairs(ndim), cells = (size_t)bins2 * bins2;
    if (!np) return MP_OK;
    return read_back(hist2_out, (const int64_t *)hist2.p + (size_t)ensemble * np * cells, np * cells,
                     outside2_out, (const int64_t *)outside2.p + (size_t)ensemble * np, np);
}

int PostMonitor::read_moments(int ensemble, double *sum1, double *sum2, double *pivot, int64_t *n_finite) const {
    const size_t nd = (size_t)ndim, nw = (size_t)n_walkers, nt = (size_t)n_total, nent = (size_t)mp::post_n_entries(ndim);
    // the ensemble's walkers of every entry, summed in walker order from 0.0
    std::vector<double> part(nent * nw), tot(nent);
    HIP_TRY(hipMemcpy2D(part.data(), nw * sizeof(double), mom.p + (size_t)ensemble * nw, nt * sizeof(double), nw * sizeof(double), nent, hipMemcpyDeviceToHost));
    for (size_t k = 0; k < nent; ++k) {
        double t = 0.0;
        for (size_t w = 0; w < nw; ++w) t += part[k * nw + w];
        tot[k] = t;
    }
    if (sum1) std::memcpy(sum1, tot.data(), nd * sizeof(double));
    if (sum2) {
        size_t k = nd;
        for (size_t a = 0; a < nd; ++a)
            for (size_t b = a; b < nd; ++b, ++k) sum2[a * nd + b] = sum2[b * nd + a] = tot[k];
    }
    if (pivot) std::memcpy(pivot, par.data() + 4 * nd, nd * sizeof(double));
    if (n_finite) {
        std::vector<int64_t> cnt(nw);
        HIP_TRY(hipMemcpy(cnt.data(), nfin.p + (size_t)ensemble * nw, nw * sizeof(int64_t), hipMemcpyDeviceToHost));
        *n_finite = std::accumulate(cnt.begin(), cnt.end(), (int64_t)0);
    }
    return MP_OK;
}

int PostMonitor::read_best(int ensemble, double *x, double *lnprob, int64_t *index) const {
    return read_back(x, (const double *)best_x.p + (size_t)ensemble * ndim, (size_t)ndim,
                     lnprob, (const double *)best_lnp.p + ensemble, (size_t)1, index, (const int64_t *)best_idx.p + ensemble, (size_t)1);
}

// ---- thermodynamic monitor
const MonitorNames ThermoMonitor::kNames = {"the thermodynamic monitor", "mp_sampler_set_thermo"};

int ThermoMonitor::make(const char *fn, int n_walkers, int n_ensembles, int ndim, int64_t discard, size_t sampler_cap,
                        std::unique_ptr<ThermoMonitor> *out) {
    if (int rc = check_discard(fn, discard, " (-1 turns the monitor off)")) return rc;
    std::unique_ptr<ThermoMonitor> m(new ThermoMonitor(kNames, n_walkers, n_ensembles, ndim, discard, sampler_cap));
    const size_t ne = (size_t)n_ensembles;
    int rc;
    if ((rc = m->sum.ensure(ne)) || (rc = m->n_finite.ensure(ne)) || (rc = m->n_nonfinite.ensure(ne))) return rc;
    *out = std::move(m);
    return MP_OK;
}

int ThermoMonitor::restart(hipStream_t st) {
    const size_t ne = (size_t)n_ensembles;
    const int rc = zero_async(st, sum.p, ne, n_finite.p, ne, n_nonfinite.p, ne);
    if (rc) return rc;
    start_over();
    return MP_OK;
}

int ThermoMonitor::feed(const ChainRows &c, hipStream_t st) {
    mp::ThermoArgs a{};
    const int chunk = c.rows;
    a.lnp = c.lnp; a.sum = sum.p; a.n_finite = n_finite.p; a.n_nonfinite = n_nonfinite.p;
    a.n_walkers = n_walkers; a.n_ensembles = n_ensembles;
    int first;
    take(chunk, &first);
    // (the steps before the freeze that lie behind the discard are passed over as well)
    a.first = (int)std::min<int64_t>(chunk, std::max<int64_t>(first, c.frozen_from - c.step0));
    a.rows = chunk - a.first;
    if (a.rows == 0) return MP_OK;
    const int rc = launched(mp::launch_thermo(a, st));
    if (rc) return rc;
    n += a.rows;
    return MP_OK;
}

int ThermoMonitor::read(double *sum_out, int64_t *n_finite_out, int64_t *n_nonfinite_out, int64_t *n_steps) const {
    const size_t ne = (size_t)n_ensembles;
    if (n_steps) *n_steps = n;
    return read_back(sum_out, (const double *)sum.p, ne, n_finite_out, (const int64_t *)n_finite.p, ne,
                     n_nonfinite_out, (const int64_t *)n_nonfinite.p, ne);
}

// ---- sample reservoir
const MonitorNames ResMonitor::kNames = {"the sample reservoir", "mp_sampler_set_reservoir"};

int ResMonitor::make(const char *fn, int n_walkers, int n_ensembles, int ndim, int size, uint64_t seed, int64_t discard,
                     size_t sampler_cap, std::unique_ptr<ResMonitor> *out) {
    if (size < 0 || size > MP_RESERVOIR_MAX_ROWS) return fail(MP_EINVAL, "%s: size must be in [0, %d] (MP_RESERVOIR_MAX_ROWS; 0 turns the monitor off), got %d", fn, MP_RESERVOIR_MAX_ROWS, size);
    if (int rc = check_discard(fn, discard)) return rc;
    std::unique_ptr<ResMonitor> m(new ResMonitor(kNames, n_walkers, n_ensembles, ndim, discard, sampler_cap));
    m->size = size; m->seed = seed;
    m->cand_cap = std::max(n_walkers, mp::kResCandCap);   // a slice is one step at least
    const size_t ne = (size_t)n_ensembles, held = ne * (size_t)size, cand = ne * (size_t)m->cand_cap;
    int rc;
    if ((rc = m->key.ensure(held)) || (rc = m->step.ensure(held)) || (rc = m->walker.ensure(held)) || (rc = m->lnp.ensure(held)) ||
        (rc = m->x.ensure(held * ndim)) || (rc = m->meta.ensure(ne * mp::kResMeta)) || (rc = m->cand_key.ensure(cand)) ||
        (rc = m->cand_step.ensure(cand)) || (rc = m->cand_walker.ensure(cand)) || (rc = m->evicted.ensure(cand)) ||
        (rc = m->n_cand.ensure(ne)))
        return rc;
    *out = std::move(m);
    return MP_OK;
}

mp::ResArgs ResMonitor::args(const double *chain, const double *lnp_rows) const {
    mp::ResArgs a{};
    a.chain = chain; a.lnp = lnp_rows;
    a.key = key.p; a.step = step.p; a.walker = walker.p; a.x = x.p; a.held_lnp = lnp.p; a.meta = meta.p;
    a.cand_key = cand_key.p; a.cand_step = cand_step.p; a.cand_walker = cand_walker.p; a.n_cand = n_cand.p; a.evicted = evicted.p;
    a.seed = seed;
    a.n_walkers = n_walkers; a.n_ensembles = n_ensembles; a.n_total = n_total; a.ndim = ndim;
    a.size = size; a.cand_cap = cand_cap;
    return a;
}

int ResMonitor::restart(hipStream_t st) {
    const size_t ne = (size_t)n_ensembles;
    const int rc = zero_async(st, meta.p, ne * mp::kResMeta, n_cand.p, ne);
    if (rc) return rc;
    start_over();
    return MP_OK;
}

int ResMonitor::feed(const ChainRows &c, hipStream_t st) {
    mp::ResArgs a = args(c.chain, c.lnp);
    const int chunk = c.rows;
    int first;
    const int rows = take(chunk, &first);
    if (rows == 0) return MP_OK;
    const int slice = std::max(1, cand_cap / n_walkers);
    for (int r = first; r < chunk; r += slice) {
        a.row0 = r;
        a.rows = std::min(slice, chunk - r);
        a.t0 = c.step0 + r;
        int rc = launched(mp::launch_res_filter(a, st));
        if (!rc) rc = launched(mp::launch_res_merge(a, st));
        if (rc) return rc;
    }
    n += rows;
    return MP_OK;
}

int ResMonitor::read(int ensemble, int max_rows, double *x_out, double *lnprob, int64_t *step_out, int32_t *walker_out,
                     uint64_t *key_out, int *n_rows, int64_t *n_seen) const {
    int64_t m[mp::kResMeta];
    HIP_TRY(hipMemcpy(m, meta.p + (size_t)ensemble * mp::kResMeta, sizeof m, hipMemcpyDeviceToHost));
    const size_t held = (size_t)std::min<int64_t>(m[mp::kResHeld], size), nd = (size_t)ndim, at = (size_t)ensemble * size;
    std::vector<uint64_t> k(held);
    std::vector<int64_t> t(held);
    std::vector<int32_t> w(held);
    std::vector<double> l(held), xs(held * nd);
    int rc = read_back(k.data(), (const uint64_t *)key.p + at, held, t.data(), (const int64_t *)step.p + at, held,
                       w.data(), (const int32_t *)walker.p + at, held, l.data(), (const double *)lnp.p + at, held,
                       xs.data(), (const double *)x.p + at * nd, held * nd);
    if (rc) return rc;
    std::vector<size_t> order(held);
    std::iota(order.begin(), order.end(), (size_t)0);
    std::sort(order.begin(), order.end(), [&](size_t p, size_t q) { return t[p] < t[q] || (t[p] == t[q] && w[p] < w[q]); });
    const size_t rows = std::min(held, (size_t)std::max(max_rows, 0));
    for (size_t i = 0; i < rows; ++i) {
        const size_t j = order[i];
        if (x_out) std::memcpy(x_out + i * nd, xs.data() + j * nd, nd * sizeof(double));
        if (lnprob) lnprob[i] = l[j];
        if (step_out) step_out[i] = t[j];
        if (walker_out) walker_out[i] = w[j];
        if (key_out) key_out[i] = k[j];
    }
    if (n_rows) *n_rows = (int)rows;
    if (n_seen) *n_seen = m[mp::kResSeen];
    return MP_OK;
}
