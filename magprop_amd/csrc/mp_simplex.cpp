// mp_simplex.cpp — the device-resident Nelder-Mead simplex search (mp_simplex_*).  Kernels: mp_nm.hip.
#include "mp_host.h"
#include "mp_nm.h"

struct mp_simplex {
    mp_handle *h = nullptr;         // the lock
    Evaluator *ev = nullptr;        // the device state: the handle's one evaluator
    mp::NmArgs a{};
    bool have_state = false;
    DevBuf<double> d_sim, d_lnp, d_cand, d_cand_lnp;
    DevBuf<int32_t> d_st, d_cand_st, d_dsid, d_stopped, d_nit;
    DevBuf<int64_t> d_nfev, d_outcomes;
};

// one iteration (initial = 0) or the initial evaluation (initial = 1) on the handle's stream: the candidates, then the decision
static int nm_enqueue(mp_simplex *s, int initial) {
    s->a.initial = initial;
    int e = mp::launch_nm_eval(s->ev->sh, s->a, s->ev->stream);
    if (!e) e = mp::launch_nm_decide(s->a, s->ev->stream);
    if (e) return fail(MP_EHIP, "kernel launch failed: %s", hipGetErrorString((hipError_t)e));
    return MP_OK;
}

extern "C" {

void *mp_simplex_create(mp_handle *h, int n_simplex, int ndim, const int32_t *simplex_ds_id, double rho, double chi, double psi,
                        double sigma, double xatol, double fatol, const double *lower, const double *upper, int target) {
    if (!h || !lower || !upper) { fail(MP_EINVAL, "mp_simplex_create: NULL argument"); return nullptr; }
    Lock lock(h->mu);
    const int rc = check_create(h, "mp_simplex_create", "the simplex search lives on ONE device (a multi-device handle serves host-buffer batches only)",
                                ndim, target, "simplex", n_simplex, simplex_ds_id, [&] {
        if (n_simplex < 1 || n_simplex > 1024) return fail(MP_EINVAL, "mp_simplex_create: n_simplex must be 1 .. 1024, got %d", n_simplex);
        if (target < 0 || target > 2) return fail(MP_EINVAL, "mp_simplex_create: target must be 0 (posterior), 1 (unit Gaussian) or 2 (terraced Gaussian)");
        for (const double c : {rho, chi, psi, sigma})
            if (!(std::isfinite(c) && c > 0.0)) return fail(MP_EINVAL, "mp_simplex_create: rho, chi, psi and sigma must be finite and > 0");
        if (!(psi < 1.0 && sigma < 1.0)) return fail(MP_EINVAL, "mp_simplex_create: psi and sigma must lie in (0, 1)");
        if (!(std::isfinite(xatol) && xatol >= 0.0 && std::isfinite(fatol) && fatol >= 0.0)) return fail(MP_EINVAL, "mp_simplex_create: xatol and fatol must be finite and >= 0");
        int rb = check_box("mp_simplex_create", ndim, lower, upper);
        if (rb || target != 0) return rb;
        for (int g = 0; g < n_simplex; ++g) {
            const int d = simplex_ds_id ? simplex_ds_id[g] : 0;
            if (d < 0 || d >= MP_MAX_DATASETS || !h->first()->ds[d].set) return fail(MP_EINVAL, "mp_simplex_create: simplex %d refers to unset dataset %d", g, d);
        }
        return (int)MP_OK;
    });
    if (rc) return nullptr;
    mp_simplex *s = new mp_simplex();
    s->h = h;
    s->ev = h->first();
    mp::NmArgs &a = s->a;
    a.n_simplex = n_simplex; a.ndim = ndim; a.target = target;
    // the coefficients as scipy forms them, every operation rounded on its own
    volatile double rc_ = rho * chi, pr = psi * rho;
    a.ca[0] = 1.0 + rho; a.cb[0] = rho;
    a.ca[1] = 1.0 + rc_; a.cb[1] = rc_;
    a.ca[2] = 1.0 + pr; a.cb[2] = pr;
    a.one_m_psi = 1.0 - psi; a.psi = psi; a.sigma = sigma; a.xatol = xatol; a.fatol = fatol;
    for (int d = 0; d < ndim; ++d) { a.lower[d] = lower[d]; a.upper[d] = upper[d]; }
    DeviceScope scope(s->ev->device);
    const size_t ns = (size_t)n_simplex, nv = ns * (ndim + 1), nc = ns * (ndim + 4);
    Binder bind;
    bind(s->d_sim, nv * ndim, a.sim); bind(s->d_lnp, nv, a.lnp); bind(s->d_st, nv, a.st);
    bind(s->d_cand, nc * ndim, a.cand); bind(s->d_cand_lnp, nc, a.cand_lnp); bind(s->d_cand_st, nc, a.cand_st);
    bind(s->d_dsid, nc, a.ds_id);
    bind(s->d_stopped, ns, a.stopped); bind(s->d_nit, ns, a.nit); bind(s->d_nfev, ns, a.nfev);
    bind(s->d_outcomes, ns * mp::kNmOutcomes, a.outcomes);
    if (bind.rc || upload_ds_rows(s->d_dsid.p, simplex_ds_id, n_simplex, ndim + 4)) {
        fail(MP_EHIP, "mp_simplex_create: device allocation failed");
        mp_simplex_destroy(s);
        return nullptr;
    }
    return s;
}

int mp_simplex_destroy(void *sv) {
    mp_simplex *s = (mp_simplex *)sv;
    if (!s) return MP_OK;
    Held held(s->h, s->ev);
    (void)hipStreamSynchronize(s->ev->stream);
    delete s;
    return MP_OK;
}

int mp_simplex_set_vertices(void *sv, const double *sim) {
    mp_simplex *s = (mp_simplex *)sv;
    if (!s || !sim) return fail(MP_EINVAL, "mp_simplex_set_vertices: NULL argument");
    Evaluator *ev = s->ev;
    const mp::NmArgs &a = s->a;
    const size_t ns = (size_t)a.n_simplex, rows = ns * (a.ndim + 1);
    std::vector<double> v(rows * a.ndim);
    for (size_t i = 0; i < v.size(); ++i) {
        if (!std::isfinite(sim[i])) return fail(MP_EINVAL, "mp_simplex_set_vertices: non-finite coordinate");
        // scipy's rule for a vertex outside the box: reflected at the upper bound into the interior, then clipped
        const double lo = a.lower[i % a.ndim], hi = a.upper[i % a.ndim];
        const double x = sim[i] > hi ? 2.0 * hi - sim[i] : sim[i];
        v[i] = std::min(std::max(x, lo), hi);
    }
    Held held(s->h, ev);
    HIP_TRY(hipMemcpyAsync(a.sim, v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice, ev->stream));
    HIP_TRY(hipMemsetAsync(a.stopped, 0, ns * sizeof(int32_t), ev->stream));
    HIP_TRY(hipMemsetAsync(a.nit, 0, ns * sizeof(int32_t), ev->stream));
    HIP_TRY(hipMemsetAsync(a.nfev, 0, ns * sizeof(int64_t), ev->stream));
    HIP_TRY(hipMemsetAsync(a.outcomes, 0, ns * mp::kNmOutcomes * sizeof(int64_t), ev->stream));
    const int rc = nm_enqueue(s, 1);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(ev->stream));   // (v is pageable: the copy above has left it by now in any case)
    s->have_state = true;
    return MP_OK;
}

int mp_simplex_run(void *sv, int max_iterations, int *n_running) {
    mp_simplex *s = (mp_simplex *)sv;
    if (!s || max_iterations < 0) return fail(MP_EINVAL, "mp_simplex_run: bad argument");
    if (!s->have_state) return fail(MP_ESTATE, "mp_simplex_run: call mp_simplex_set_vertices first");
    Evaluator *ev = s->ev;
    Held held(s->h, ev);
    // Chunks of iterations enqueued back to back (no allocation, no wait inside a chunk); the flags are read back behind each
    // chunk, and the run ends early once every simplex has stopped.  A stopped simplex costs an empty workgroup per candidate
    // and launch, and changes no more: the state does not depend on how a run is split into calls.
    constexpr int kChunk = 16;
    int running, rc;
    if ((rc = groups_running(ev, s->a.stopped, s->a.n_simplex, &running))) return rc;
    for (int done = 0; done < max_iterations && running > 0;) {
        const int chunk = std::min(kChunk, max_iterations - done);
        for (int g = 0; g < chunk; ++g)
            if ((rc = nm_enqueue(s, 0))) return rc;
        if ((rc = groups_running(ev, s->a.stopped, s->a.n_simplex, &running))) return rc;
        done += chunk;
    }
    if (n_running) *n_running = running;
    return MP_OK;
}

int mp_simplex_get_state(void *sv, double *sim, double *lnprob, int32_t *status, int32_t *nit, int32_t *stopped, int64_t *nfev,
                         int64_t *outcomes) {
    mp_simplex *s = (mp_simplex *)sv;
    if (!s) return fail(MP_EINVAL, "mp_simplex_get_state: NULL simplex search");
    if (!s->have_state) return fail(MP_ESTATE, "mp_simplex_get_state: call mp_simplex_set_vertices first");
    Evaluator *ev = s->ev;
    Held held(s->h, ev);
    const mp::NmArgs &a = s->a;
    const size_t ns = (size_t)a.n_simplex, nv = ns * (a.ndim + 1);
    HIP_TRY(hipStreamSynchronize(ev->stream));
    return read_back(sim, (const double *)a.sim, nv * a.ndim, lnprob, (const double *)a.lnp, nv, status, (const int32_t *)a.st, nv,
                     nit, (const int32_t *)a.nit, ns, stopped, (const int32_t *)a.stopped, ns, nfev, (const int64_t *)a.nfev, ns,
                     outcomes, (const int64_t *)a.outcomes, ns * mp::kNmOutcomes);
}

}  // extern "C"
