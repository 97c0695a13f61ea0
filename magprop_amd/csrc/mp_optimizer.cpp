// mp_optimizer.cpp — the device-resident differential-evolution optimizer (mp_optimizer_*).  Kernels: mp_opt.hip.
#include "mp_host.h"

struct mp_optimizer : Resident {
    mp::OptArgs a{};                // pointers: cur / next as of the next launch
    int n_total = 0;
    uint32_t gen = 0;               // generations launched so far (0: only the initial evaluation)
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
    int e = mp::launch_opt_trial(o->ev->sh, o->a, o->ev->stream);
    if (!e) e = mp::launch_opt_reduce(o->a, o->ev->stream);
    if (e) return launched(e);
    opt_swap(o);
    return MP_OK;
}

extern "C" {

mp_optimizer *mp_optimizer_create(mp_handle *h, int popsize, int n_pops, int ndim, const int32_t *pop_ds_id, uint64_t seed,
                                  int strategy, double f_lo, double f_hi, double cr, double tol, double atol,
                                  const double *lower, const double *upper, int target) {
    return resident_create<mp_optimizer>(
        h, "mp_optimizer_create", "the optimizer lives on ONE device (a multi-device handle serves host-buffer batches only)",
        ndim, target, "population", n_pops, pop_ds_id, popsize, lower, upper,
        [&] {
            if (popsize < 5 || popsize > 1024) return fail(MP_EINVAL, "mp_optimizer_create: popsize must be 5 .. 1024, got %d", popsize);
            if (n_pops < 1 || n_pops > MP_MAX_DATASETS) return fail(MP_EINVAL, "mp_optimizer_create: n_pops must be 1 .. %d", MP_MAX_DATASETS);
            if (target != 0 && target != 1) return fail(MP_EINVAL, "mp_optimizer_create: target must be 0 (posterior) or 1 (unit Gaussian)");
            if (strategy != MP_DE_BEST1BIN && strategy != MP_DE_RAND1BIN) return fail(MP_EINVAL, "mp_optimizer_create: unknown strategy %d", strategy);
            if (!(f_lo >= 0.0 && f_lo <= f_hi && f_hi < 2.0)) return fail(MP_EINVAL, "mp_optimizer_create: need 0 <= f_lo <= f_hi < 2");
            if (!(cr >= 0.0 && cr <= 1.0)) return fail(MP_EINVAL, "mp_optimizer_create: cr must lie in [0, 1]");
            if (!(std::isfinite(tol) && tol >= 0.0 && std::isfinite(atol) && atol >= 0.0)) return fail(MP_EINVAL, "mp_optimizer_create: tol and atol must be finite and >= 0");
            return check_box("mp_optimizer_create", ndim, lower, upper);
        },
        [&](mp_optimizer *o, Binder &bind) {
            o->n_total = popsize * n_pops;
            mp::OptArgs &a = o->a;
            a.popsize = popsize; a.n_pops = n_pops; a.ndim = ndim; a.strategy = strategy; a.target = target; a.seed = seed;
            a.f_lo = f_lo; a.f_hi = f_hi; a.cr = cr; a.tol = tol; a.atol = atol;
            const size_t nt = (size_t)o->n_total;
            bind(o->d_pop[0], nt * ndim, a.pop_cur); bind(o->d_pop[1], nt * ndim, a.pop_next);
            bind(o->d_lnp[0], nt, a.lnp_cur); bind(o->d_lnp[1], nt, a.lnp_next);
            bind(o->d_st[0], nt, a.st_cur); bind(o->d_st[1], nt, a.st_next);
            bind(o->d_dsid, nt, a.ds_id);
            bind(o->d_best, n_pops, a.best); bind(o->d_conv, n_pops, a.converged); bind(o->d_nit, n_pops, a.nit); bind(o->d_nfev, n_pops, a.nfev);
        });
}

int mp_optimizer_destroy(mp_optimizer *o) { return resident_destroy(o); }

int mp_optimizer_set_population(mp_optimizer *o, const double *pop) {
    if (!o || !pop) return fail(MP_EINVAL, "mp_optimizer_set_population: NULL argument");
    Evaluator *ev = o->ev;
    const size_t nt = (size_t)o->n_total, n_pops = (size_t)o->a.n_pops;
    for (size_t i = 0; i < nt * o->a.ndim; ++i)
        if (!std::isfinite(pop[i])) return fail(MP_EINVAL, "mp_optimizer_set_population: non-finite coordinate");
    Held held(o->h, ev);
    HIP_TRY(hipMemcpyAsync(o->a.pop_cur, pop, nt * o->a.ndim * sizeof(double), hipMemcpyHostToDevice, ev->stream));
    int rc = zero_async(ev->stream, o->a.converged, n_pops, o->a.nit, n_pops, o->a.nfev, n_pops);
    if (rc) return rc;
    o->gen = 0;
    if ((rc = opt_enqueue(o, 0))) return rc;
    HIP_TRY(hipStreamSynchronize(ev->stream));
    o->have_state = true;
    return MP_OK;
}

int mp_optimizer_run(mp_optimizer *o, int max_generations, int *n_running) {
    RESIDENT_ENTER(o, max_generations >= 0, "mp_optimizer_run", "bad argument", "mp_optimizer_set_population");
    // Chunks of 16 generations: the run ends early once every population has converged.  A frozen population costs an empty
    // workgroup per member and launch.
    return run_chunked(o->ev, o->a.converged, o->a.n_pops, 16, max_generations, n_running, [&] {
        ++o->gen;
        return opt_enqueue(o, 1);
    });
}

int mp_optimizer_get_state(mp_optimizer *o, double *pop, double *lnprob, int32_t *status, int32_t *best, int32_t *nit,
                           int32_t *converged, int64_t *nfev) {
    RESIDENT_READ(o, true, "mp_optimizer_get_state", "NULL optimizer", "mp_optimizer_set_population");
    const mp::OptArgs &a = o->a;
    const size_t nt = (size_t)o->n_total, np = (size_t)a.n_pops;
    return read_back(pop, a.pop_cur, nt * a.ndim, lnprob, a.lnp_cur, nt, status, a.st_cur, nt,
                     best, a.best, np, nit, a.nit, np, converged, a.converged, np, nfev, a.nfev, np);
}

}  // extern "C"
