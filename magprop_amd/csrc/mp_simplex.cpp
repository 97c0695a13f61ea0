// mp_simplex.cpp — the device-resident Nelder-Mead simplex search (mp_simplex_*).  Kernels: mp_nm.hip.
#include "mp_host.h"
#include "mp_nm.h"

struct mp_simplex : Resident {
    mp::NmArgs a{};
    DevBuf<double> d_sim, d_lnp, d_cand, d_cand_lnp;
    DevBuf<int32_t> d_st, d_cand_st, d_dsid, d_stopped, d_nit;
    DevBuf<int64_t> d_nfev, d_outcomes;
};

// one iteration (initial = 0) or the initial evaluation (initial = 1) on the handle's stream: the candidates, then the decision
static int nm_enqueue(mp_simplex *s, int initial) {
    s->a.initial = initial;
    int e = mp::launch_nm_eval(s->ev->sh, s->a, s->ev->stream);
    if (!e) e = mp::launch_nm_decide(s->a, s->ev->stream);
    return launched(e);
}

extern "C" {

void *mp_simplex_create(mp_handle *h, int n_simplex, int ndim, const int32_t *simplex_ds_id, double rho, double chi, double psi,
                        double sigma, double xatol, double fatol, const double *lower, const double *upper, int target) {
    return resident_create<mp_simplex>(
        h, "mp_simplex_create", "the simplex search lives on ONE device (a multi-device handle serves host-buffer batches only)",
        ndim, target, "simplex", n_simplex, simplex_ds_id, ndim + 4, lower, upper,
        [&] {
            if (n_simplex < 1 || n_simplex > 1024) return fail(MP_EINVAL, "mp_simplex_create: n_simplex must be 1 .. 1024, got %d", n_simplex);
            if (target < 0 || target > 2) return fail(MP_EINVAL, "mp_simplex_create: target must be 0 (posterior), 1 (unit Gaussian) or 2 (terraced Gaussian)");
            for (const double c : {rho, chi, psi, sigma})
                if (!(std::isfinite(c) && c > 0.0)) return fail(MP_EINVAL, "mp_simplex_create: rho, chi, psi and sigma must be finite and > 0");
            if (!(psi < 1.0 && sigma < 1.0)) return fail(MP_EINVAL, "mp_simplex_create: psi and sigma must lie in (0, 1)");
            if (!(std::isfinite(xatol) && xatol >= 0.0 && std::isfinite(fatol) && fatol >= 0.0)) return fail(MP_EINVAL, "mp_simplex_create: xatol and fatol must be finite and >= 0");
            return check_box("mp_simplex_create", ndim, lower, upper);
        },
        [&](mp_simplex *s, Binder &bind) {
            mp::NmArgs &a = s->a;
            a.n_simplex = n_simplex; a.ndim = ndim; a.target = target;
            // the coefficients as scipy forms them, every operation rounded on its own
            volatile double rc_ = rho * chi, pr = psi * rho;
            a.ca[0] = 1.0 + rho; a.cb[0] = rho;
            a.ca[1] = 1.0 + rc_; a.cb[1] = rc_;
            a.ca[2] = 1.0 + pr; a.cb[2] = pr;
            a.one_m_psi = 1.0 - psi; a.psi = psi; a.sigma = sigma; a.xatol = xatol; a.fatol = fatol;
            const size_t ns = (size_t)n_simplex, nv = ns * (ndim + 1), nc = ns * (ndim + 4);
            bind(s->d_sim, nv * ndim, a.sim); bind(s->d_lnp, nv, a.lnp); bind(s->d_st, nv, a.st);
            bind(s->d_cand, nc * ndim, a.cand); bind(s->d_cand_lnp, nc, a.cand_lnp); bind(s->d_cand_st, nc, a.cand_st);
            bind(s->d_dsid, nc, a.ds_id);
            bind(s->d_stopped, ns, a.stopped); bind(s->d_nit, ns, a.nit); bind(s->d_nfev, ns, a.nfev);
            bind(s->d_outcomes, ns * mp::kNmOutcomes, a.outcomes);
        });
}

int mp_simplex_destroy(void *sv) { return resident_destroy((mp_simplex *)sv); }

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
    int rc = zero_async(ev->stream, a.stopped, ns, a.nit, ns, a.nfev, ns, a.outcomes, ns * mp::kNmOutcomes);
    if (rc || (rc = nm_enqueue(s, 1))) return rc;
    HIP_TRY(hipStreamSynchronize(ev->stream));   // (v is pageable: the copy above has left it by now in any case)
    s->have_state = true;
    return MP_OK;
}

int mp_simplex_run(void *sv, int max_iterations, int *n_running) {
    mp_simplex *s = (mp_simplex *)sv;
    RESIDENT_ENTER(s, max_iterations >= 0, "mp_simplex_run", "bad argument", "mp_simplex_set_vertices");
    // Chunks of 16 iterations: the run ends early once every simplex has stopped.  A stopped simplex costs an empty workgroup per
    // candidate and launch, and changes no more: the state does not depend on how a run is split into calls.
    return run_chunked(s->ev, s->a.stopped, s->a.n_simplex, 16, max_iterations, n_running, [&] { return nm_enqueue(s, 0); });
}

int mp_simplex_get_state(void *sv, double *sim, double *lnprob, int32_t *status, int32_t *nit, int32_t *stopped, int64_t *nfev,
                         int64_t *outcomes) {
    mp_simplex *s = (mp_simplex *)sv;
    RESIDENT_READ(s, true, "mp_simplex_get_state", "NULL simplex search", "mp_simplex_set_vertices");
    const mp::NmArgs &a = s->a;
    const size_t ns = (size_t)a.n_simplex, nv = ns * (a.ndim + 1);
    return read_back(sim, (const double *)a.sim, nv * a.ndim, lnprob, (const double *)a.lnp, nv, status, (const int32_t *)a.st, nv,
                     nit, (const int32_t *)a.nit, ns, stopped, (const int32_t *)a.stopped, ns, nfev, (const int64_t *)a.nfev, ns,
                     outcomes, (const int64_t *)a.outcomes, ns * mp::kNmOutcomes);
}

}  // extern "C"
