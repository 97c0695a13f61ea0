// mp_nested.cpp — the device-resident nested sampler (mp_nested_*), random-walk and slice mode.  Kernels: mp_nest.hip.
#include "mp_host.h"

struct mp_nested : Resident {
    mp::NestArgs a{};
    int n_total = 0;                // n_runs * nlive
    int chunk = 0;                  // iterations per chunk (slots of the dead buffers)
    uint32_t iter = 0;              // iterations launched since mp_nested_set_live
    DevBuf<double> d_live, d_lnl, d_lstar, d_dpars, d_dlnl, d_lnx, d_lnz;
    DevBuf<int32_t> d_st, d_acc, d_dsid, d_dslot, d_surv, d_dn, d_stop, d_nit;
    DevBuf<int64_t> d_ncall, d_nacc, d_nzero, d_nexp, d_ncon, d_nfail;
    mp::NestSlice sl{};             // slice mode (sl.slices > 0) from the next iteration on
    std::vector<std::vector<double>> dead_pars, dead_lnl;   // per run, in order
    std::vector<std::vector<int32_t>> dead_n;
};

extern "C" {

mp_nested *mp_nested_create(mp_handle *h, int nlive, int nbatch, int n_runs, int ndim, const int32_t *run_ds_id, uint64_t seed,
                            int walks, double g0, double sigma, double dlogz, const double *lower, const double *upper, int target) {
    return resident_create<mp_nested>(
        h, "mp_nested_create", "the nested sampler lives on ONE device (a multi-device handle serves host-buffer batches only)",
        ndim, target, "run", n_runs, run_ds_id, 1, lower, upper,
        [&] {
            if (nlive < MP_NEST_MIN_LIVE || nlive > MP_NEST_MAX_LIVE) return fail(MP_EINVAL, "mp_nested_create: nlive must be %d .. %d, got %d", MP_NEST_MIN_LIVE, MP_NEST_MAX_LIVE, nlive);
            if (nbatch < 1 || nbatch > nlive / 2) return fail(MP_EINVAL, "mp_nested_create: nbatch must be 1 .. nlive / 2, got %d", nbatch);
            if (n_runs < 1 || n_runs > MP_MAX_DATASETS) return fail(MP_EINVAL, "mp_nested_create: n_runs must be 1 .. %d", MP_MAX_DATASETS);
            if (target != 0 && target != 1) return fail(MP_EINVAL, "mp_nested_create: target must be 0 (posterior) or 1 (unit Gaussian)");
            if (walks < 1 || walks > MP_NEST_MAX_WALKS) return fail(MP_EINVAL, "mp_nested_create: walks must be 1 .. %d", MP_NEST_MAX_WALKS);
            if (!std::isfinite(g0)) return fail(MP_EINVAL, "mp_nested_create: g0 must be finite (<= 0: the default)");
            if (!(sigma >= 0.0 && sigma < 1.0 / std::sqrt(3.0))) return fail(MP_EINVAL, "mp_nested_create: sigma must lie in [0, 1/sqrt(3))");
            if (!(std::isfinite(dlogz) && dlogz > 0.0)) return fail(MP_EINVAL, "mp_nested_create: dlogz must be finite and > 0");
            return check_box("mp_nested_create", ndim, lower, upper);
        },
        [&](mp_nested *ns, Binder &bind) {
            ns->n_total = nlive * n_runs;
            // dead buffers of about 16 MB at most, up to 32 iterations per chunk
            const size_t row = (size_t)n_runs * nbatch * (ndim + 2) * sizeof(double);
            ns->chunk = (int)std::max<size_t>(1, std::min<size_t>(32, (16u << 20) / row));
            mp::NestArgs &a = ns->a;
            a.nlive = nlive; a.nbatch = nbatch; a.n_runs = n_runs; a.ndim = ndim; a.walks = walks; a.target = target; a.seed = seed;
            a.g0 = g0 > 0.0 ? g0 : 2.38 / std::sqrt(2.0 * ndim);
            a.sig3 = sigma * std::sqrt(3.0);
            a.dlogz = dlogz;
            ns->dead_pars.resize(n_runs); ns->dead_lnl.resize(n_runs); ns->dead_n.resize(n_runs);
            const size_t nt = (size_t)ns->n_total, nr = (size_t)n_runs, nk = nr * nbatch, nc = (size_t)ns->chunk * nk;
            bind(ns->d_live, nt * ndim, a.live); bind(ns->d_lnl, nt, a.lnl); bind(ns->d_st, nt, a.st); bind(ns->d_acc, nt, a.acc);
            bind(ns->d_dsid, nr, a.ds_id); bind(ns->d_dslot, nk, a.dead_slot); bind(ns->d_surv, nr * (nlive - nbatch), a.surv);
            bind(ns->d_lstar, nr, a.lstar); bind(ns->d_dpars, nc * ndim, a.dead_pars); bind(ns->d_dlnl, nc, a.dead_lnl); bind(ns->d_dn, nc, a.dead_n);
            bind(ns->d_lnx, nr, a.lnx); bind(ns->d_lnz, nr, a.lnz); bind(ns->d_stop, nr, a.stopped); bind(ns->d_nit, nr, a.nit);
            bind(ns->d_ncall, nr, a.ncall); bind(ns->d_nacc, nr, a.nacc); bind(ns->d_nzero, nr, a.nzero);
            bind(ns->d_nexp, nr, ns->sl.nexpand); bind(ns->d_ncon, nr, ns->sl.ncontract); bind(ns->d_nfail, nr, ns->sl.nfail);
        });
}

int mp_nested_destroy(mp_nested *ns) { return resident_destroy(ns); }

int mp_nested_set_live(mp_nested *ns, const double *live) {
    if (!ns || !live) return fail(MP_EINVAL, "mp_nested_set_live: NULL argument");
    Evaluator *ev = ns->ev;
    mp::NestArgs &a = ns->a;
    const size_t nt = (size_t)ns->n_total, nr = (size_t)a.n_runs;
    int rc = check_inside("mp_nested_set_live: live point", live, nt, a.ndim, a.lower, a.upper);
    if (rc) return rc;
    Held held(ns->h, ev);
    const std::vector<double> zero(nr, 0.0), ninf(nr, -INFINITY);
    HIP_TRY(hipMemcpyAsync(a.live, live, nt * a.ndim * sizeof(double), hipMemcpyHostToDevice, ev->stream));
    HIP_TRY(hipMemcpyAsync(a.lnx, zero.data(), nr * sizeof(double), hipMemcpyHostToDevice, ev->stream));
    HIP_TRY(hipMemcpyAsync(a.lnz, ninf.data(), nr * sizeof(double), hipMemcpyHostToDevice, ev->stream));
    if ((rc = zero_async(ev->stream, a.stopped, nr, a.nit, nr, a.ncall, nr, a.nacc, nr, a.nzero, nr,
                         ns->sl.nexpand, nr, ns->sl.ncontract, nr, ns->sl.nfail, nr)))
        return rc;
    a.mode = 1;
    a.iter = 0;
    if ((rc = launched(mp::launch_nest_walk(ev->sh, a, ev->stream)))) return rc;
    HIP_TRY(hipStreamSynchronize(ev->stream));
    ns->iter = 0;
    for (size_t r = 0; r < nr; ++r) { ns->dead_pars[r].clear(); ns->dead_lnl[r].clear(); ns->dead_n[r].clear(); }
    ns->have_state = true;
    return MP_OK;
}

int mp_nested_run(mp_nested *ns, int max_iterations, int *n_running) {
    RESIDENT_ENTER(ns, max_iterations >= 0, "mp_nested_run", "bad argument", "mp_nested_set_live");
    Evaluator *ev = ns->ev;
    mp::NestArgs &a = ns->a;
    // run_chunked's loop with work of its own around a chunk: chunks of iterations enqueued back to back (select, walk, select,
    // walk, ...; no wait inside a chunk), then a stop check on the live set as it stands and one read-back of the counters and the
    // dead rows, which the host files per run once they have landed; the run ends early once every run stopped.
    const int nr = a.n_runs, K = a.nbatch, nd = a.ndim;
    const size_t per = (size_t)nr * K;
    std::vector<int32_t> nit0((size_t)nr), nit1((size_t)nr);
    std::vector<double> hp, hl;
    std::vector<int32_t> hn;
    int running, rc;
    if ((rc = groups_running(ev, a.stopped, nr, &running))) return rc;
    for (int done = 0; done < max_iterations && running > 0;) {
        const int chunk = std::min(ns->chunk, max_iterations - done);
        HIP_TRY(hipMemcpyAsync(nit0.data(), a.nit, nr * sizeof(int32_t), hipMemcpyDeviceToHost, ev->stream));
        for (int c = 0; c < chunk; ++c) {
            a.slot = c;
            a.iter = ns->iter++;
            a.mode = 0;
            int e = mp::launch_nest_select(a, ev->stream);
            if (!e) e = ns->sl.slices ? mp::launch_nest_slice(ev->sh, a, ns->sl, ev->stream) : mp::launch_nest_walk(ev->sh, a, ev->stream);
            if (e) return launched(e);
        }
        a.mode = 1;
        if ((rc = launched(mp::launch_nest_select(a, ev->stream)))) return rc;
        hp.resize((size_t)chunk * per * nd);
        hl.resize((size_t)chunk * per);
        hn.resize((size_t)chunk * per);
        HIP_TRY(hipMemcpyAsync(hp.data(), a.dead_pars, hp.size() * sizeof(double), hipMemcpyDeviceToHost, ev->stream));
        HIP_TRY(hipMemcpyAsync(hl.data(), a.dead_lnl, hl.size() * sizeof(double), hipMemcpyDeviceToHost, ev->stream));
        HIP_TRY(hipMemcpyAsync(hn.data(), a.dead_n, hn.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ev->stream));
        HIP_TRY(hipMemcpyAsync(nit1.data(), a.nit, nr * sizeof(int32_t), hipMemcpyDeviceToHost, ev->stream));
        if ((rc = groups_running(ev, a.stopped, nr, &running))) return rc;   // (behind the copies above: they have landed)
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
    RESIDENT_READ(ns, true, "mp_nested_get_state", "NULL sampler", "mp_nested_set_live");
    const mp::NestArgs &a = ns->a;
    const size_t nt = (size_t)ns->n_total, nr = (size_t)a.n_runs;
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
    RESIDENT_READ(ns, true, "mp_nested_get_slice_stats", "NULL sampler", "mp_nested_set_live");
    const size_t nr = (size_t)ns->a.n_runs;
    return read_back(nexpand, ns->sl.nexpand, nr, ncontract, ns->sl.ncontract, nr, nfail, ns->sl.nfail, nr);
}

}  // extern "C"
