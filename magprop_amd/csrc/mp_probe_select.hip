// mp_probe_select.hip — test infrastructure only: the kernels that decide which values a result is built from
// (band_transpose_kernel, band_select_kernel, nest_select_kernel, opt_reduce_kernel), each behind one extern "C" host function
// mps_* over HOST buffers (tests/test_gpu_select.py, cases of tests/select_cases.py).  Builds into its own libmp_probe_select.so,
// linked from the very objects libmagprop_amd.so is linked from (build/all/mp_band.hip.o, mp_nest.hip.o, mp_opt.hip.o): the kernels
// reached here are the product's compiled code, through the product's launchers.  Nothing here is part of libmagprop_amd.so, of
// include/magprop_amd.h or of the product's ABI.
//
// Every mps_* function allocates on the current device, copies every buffer in (outputs too: the caller fills them with canaries,
// and what the kernel leaves alone comes back as it went), launches, synchronises, copies every buffer back and frees.  It
// returns 0, a hipError_t, or -1 for arguments it refuses: every size the product's own entry points refuse, and NULL pointers.
// Nothing is launched then.
#include <hip/hip_runtime.h>

#include "mp_band.h"
#include "mp_device.h"
#include "mp_probe_bufs.h"

namespace mp {

namespace {

constexpr int kMaxGrid = 1 << 16;     // grid points of a band call (the probe's own cap)
constexpr int kMaxRuns = 64;          // runs / populations of a call (the probe's own cap)
constexpr int kMaxChunk = 64;         // chunk slots of the dead rows (the probe's own cap)
constexpr int kOptMinPop = 5, kOptMaxPop = 1024;   // mp_optimizer_create (include/magprop_amd.h)

bool band_sizes_ok(int n, int n_grid) { return n >= 1 && n <= MP_BAND_MAX_SAMPLES && n_grid >= 1 && n_grid <= kMaxGrid; }

}  // namespace

}  // namespace mp

using namespace mp;

extern "C" {

int mps_band_max_samples(void) { return MP_BAND_MAX_SAMPLES; }
int mps_band_max_q(void) { return MP_BAND_MAX_Q; }
int mps_band_max_grid(void) { return kMaxGrid; }
int mps_nest_min_live(void) { return MP_NEST_MIN_LIVE; }
int mps_nest_max_live(void) { return MP_NEST_MAX_LIVE; }
int mps_opt_min_pop(void) { return kOptMinPop; }
int mps_opt_max_pop(void) { return kOptMaxPop; }
int mps_max_ndim(void) { return MP_MAX_NDIM; }
int mps_max_runs(void) { return kMaxRuns; }
int mps_max_chunk(void) { return kMaxChunk; }

// src[n][n_grid] -> dst[n_grid][n]
int mps_band_transpose(const double *src, double *dst, int n, int n_grid) {
    if (!band_sizes_ok(n, n_grid) || !src || !dst) return -1;
    Bufs B;
    const size_t count = (size_t)n * n_grid;
    const double *s = B.in(src, count);
    double *d = B.io(dst, count);
    int rc = 0;
    if (B.ready()) rc = launch_band_transpose(s, d, n, n_grid, nullptr);
    return B.finish(rc);
}

// cols[n_grid][n], q[nq] -> out[nq][n_grid]
int mps_band_select(const double *cols, int n, int n_grid, const double *q, int nq, double *out) {
    if (!band_sizes_ok(n, n_grid) || nq < 1 || nq > MP_BAND_MAX_Q || !cols || !q || !out) return -1;
    for (int j = 0; j < nq; ++j)
        if (!(q[j] >= 0.0 && q[j] <= 1.0)) return -1;   // (mp_model_band: each finite and in [0, 1])
    BandQ bq{};
    for (int j = 0; j < nq; ++j) bq.q[j] = q[j];
    bq.nq = nq;
    Bufs B;
    const double *c = B.in(cols, (size_t)n * n_grid);
    double *o = B.io(out, (size_t)nq * n_grid);
    int rc = 0;
    if (B.ready()) rc = launch_band_select(c, n, n_grid, bq, o, nullptr);
    return B.finish(rc);
}

// One select launch (mode 0: an iteration; 1: the stop check only) over n_runs live sets.  live[n_runs * nlive][ndim],
// lnl[n_runs * nlive] are read; dead_slot[n_runs][nbatch], surv[n_runs][nlive - nbatch], lstar[n_runs], dead_pars[chunk][n_runs]
// [nbatch][ndim], dead_lnl / dead_n[chunk][n_runs][nbatch], lnx, lnz, stopped, nit [n_runs] go in and come back.
int mps_nest_select(int nlive, int nbatch, int n_runs, int ndim, int mode, int slot, int chunk, double dlogz, const double *live,
                    const double *lnl, int32_t *dead_slot, int32_t *surv, double *lstar, double *dead_pars, double *dead_lnl,
                    int32_t *dead_n, double *lnx, double *lnz, int32_t *stopped, int32_t *nit) {
    if (nlive < MP_NEST_MIN_LIVE || nlive > MP_NEST_MAX_LIVE || nbatch < 1 || nbatch > nlive / 2) return -1;
    if (n_runs < 1 || n_runs > kMaxRuns || ndim < 1 || ndim > MP_MAX_NDIM || (mode != 0 && mode != 1)) return -1;
    if (chunk < 1 || chunk > kMaxChunk || slot < 0 || slot >= chunk) return -1;
    if (!live || !lnl || !dead_slot || !surv || !lstar || !dead_pars || !dead_lnl || !dead_n || !lnx || !lnz || !stopped || !nit) return -1;
    Bufs B;
    const size_t rows = (size_t)n_runs * nlive, drows = (size_t)chunk * n_runs * nbatch;
    NestArgs a{};
    a.live = const_cast<double *>(B.in(live, rows * ndim));   // (the select kernel only reads the live set)
    a.lnl = const_cast<double *>(B.in(lnl, rows));
    a.dead_slot = B.io(dead_slot, (size_t)n_runs * nbatch);
    a.surv = B.io(surv, (size_t)n_runs * (nlive - nbatch));
    a.lstar = B.io(lstar, n_runs);
    a.dead_pars = B.io(dead_pars, drows * ndim);
    a.dead_lnl = B.io(dead_lnl, drows);
    a.dead_n = B.io(dead_n, drows);
    a.lnx = B.io(lnx, n_runs);
    a.lnz = B.io(lnz, n_runs);
    a.stopped = B.io(stopped, n_runs);
    a.nit = B.io(nit, n_runs);
    a.nlive = nlive;
    a.nbatch = nbatch;
    a.n_runs = n_runs;
    a.ndim = ndim;
    a.mode = mode;
    a.slot = slot;
    a.dlogz = dlogz;
    int rc = 0;
    if (B.ready()) rc = launch_nest_select(a, nullptr);
    return B.finish(rc);
}

// One reduce launch (trial 0: behind the initial evaluation; 1: behind a generation) over n_pops populations.  Every buffer goes
// in and comes back: pop_cur / pop_next[n_pops * popsize][ndim], lnp_*, st_*[n_pops * popsize], best, converged, nit, nfev[n_pops].
int mps_opt_reduce(int popsize, int n_pops, int ndim, int trial, double tol, double atol, double *pop_cur, double *pop_next,
                   double *lnp_cur, double *lnp_next, int32_t *st_cur, int32_t *st_next, int32_t *best, int32_t *converged,
                   int32_t *nit, int64_t *nfev) {
    if (popsize < kOptMinPop || popsize > kOptMaxPop || n_pops < 1 || n_pops > kMaxRuns || ndim < 1 || ndim > MP_MAX_NDIM) return -1;
    if (trial != 0 && trial != 1) return -1;
    if (!pop_cur || !pop_next || !lnp_cur || !lnp_next || !st_cur || !st_next || !best || !converged || !nit || !nfev) return -1;
    Bufs B;
    const size_t members = (size_t)n_pops * popsize;
    OptArgs o{};
    o.pop_cur = B.io(pop_cur, members * ndim);
    o.pop_next = B.io(pop_next, members * ndim);
    o.lnp_cur = B.io(lnp_cur, members);
    o.lnp_next = B.io(lnp_next, members);
    o.st_cur = B.io(st_cur, members);
    o.st_next = B.io(st_next, members);
    o.best = B.io(best, n_pops);
    o.converged = B.io(converged, n_pops);
    o.nit = B.io(nit, n_pops);
    o.nfev = B.io(nfev, n_pops);
    o.popsize = popsize;
    o.n_pops = n_pops;
    o.ndim = ndim;
    o.trial = trial;
    o.tol = tol;
    o.atol = atol;
    int rc = 0;
    if (B.ready()) rc = launch_opt_reduce(o, nullptr);
    return B.finish(rc);
}

}  // extern "C"
