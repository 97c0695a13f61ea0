// mp_bridge.cpp — the bridge-sampling evidence estimate of host rows (mp_bridge_logz).  Kernels: mp_bridge.hip; the host-only
// rules (the factor of the proposal, its constant): mp_bridge.h.
//
// One call with no state: the buffers are the call's own and are given back before it returns.  The rows of x_fit and x_est go
// through the device in chunks of kChunkBlocks blocks of MP_BRIDGE_BLOCK rows, so that the blocks of the moments are cut from
// the rows alone whatever the chunk; a, b and the draws stay on the device between the launches.
#include "mp_bridge.h"
#include "mp_host.h"

namespace {

constexpr int64_t kChunkBlocks = 64;   // rows of a chunk: 64 * MP_BRIDGE_BLOCK

int rows_finite(const char *what, const double *rows, int64_t n, int ndim) {
    for (int64_t i = 0; i < n; ++i)
        for (int d = 0; d < ndim; ++d)
            if (!std::isfinite(rows[i * ndim + d])) return fail(MP_EINVAL, "mp_bridge_logz: row %lld of %s is not finite", (long long)i, what);
    return MP_OK;
}

// the checks that need no handle, in the order they fail
int check_bridge_args(const double *x_fit, int64_t n_fit, const double *x_est, const double *lnp_est, int64_t n_est, int ndim,
                      const double *lower, const double *upper, int64_t n_draws, int n_rep, double neff, int max_iter, double tol,
                      int target, const double *out) {
    if (!x_fit || !x_est || !lnp_est || !out) return fail(MP_EINVAL, "mp_bridge_logz: NULL argument");
    if (target < 0 || target > 2) return fail(MP_EINVAL, "mp_bridge_logz: target must be 0, 1 or 2, got %d", target);
    if (ndim < 1 || ndim > MP_MAX_NDIM || (target == 0 && ndim < 6)) return fail(MP_EINVAL, "mp_bridge_logz: bad ndim %d", ndim);
    if (n_fit < ndim + 2) return fail(MP_EINVAL, "mp_bridge_logz: n_fit must be at least ndim + 2 = %d, got %lld", ndim + 2, (long long)n_fit);
    if (n_est < 1 || n_draws < 1) return fail(MP_EINVAL, "mp_bridge_logz: n_est and n_draws must be at least 1");
    if (n_rep < 1 || n_rep > MP_BRIDGE_MAX_REP) return fail(MP_EINVAL, "mp_bridge_logz: n_rep must be 1..%d, got %d", MP_BRIDGE_MAX_REP, n_rep);
    if (n_fit > MP_BRIDGE_MAX_ROWS || n_est > MP_BRIDGE_MAX_ROWS || n_draws > MP_BRIDGE_MAX_ROWS || n_draws * n_rep > MP_BRIDGE_MAX_ROWS)
        return fail(MP_EINVAL, "mp_bridge_logz: n_fit, n_est and n_rep * n_draws must not exceed %lld (MP_BRIDGE_MAX_ROWS)", (long long)MP_BRIDGE_MAX_ROWS);
    if (!(neff > 0.0 && neff <= (double)n_est)) return fail(MP_EINVAL, "mp_bridge_logz: neff must be in (0, n_est], got %g", neff);
    if (!(std::isfinite(tol) && tol >= 0.0)) return fail(MP_EINVAL, "mp_bridge_logz: tol must be finite and >= 0, got %g", tol);
    if (max_iter < 1) return fail(MP_EINVAL, "mp_bridge_logz: max_iter must be at least 1, got %d", max_iter);
    if (!lower != !upper || (target == 0 && !lower)) return fail(MP_EINVAL, "mp_bridge_logz: the box is NULL (allowed for targets 1 and 2, both bounds)");
    int rc;
    if (lower && (rc = check_box("mp_bridge_logz", ndim, lower, upper))) return rc;
    if ((rc = rows_finite("x_fit", x_fit, n_fit, ndim)) || (rc = rows_finite("x_est", x_est, n_est, ndim))) return rc;
    for (int64_t i = 0; i < n_est; ++i)
        if (!std::isfinite(lnp_est[i])) return fail(MP_EINVAL, "mp_bridge_logz: lnp_est[%lld] is not finite", (long long)i);
    return MP_OK;
}

}  // namespace

extern "C" {

int mp_bridge_logz(mp_handle *h, const double *x_fit, int64_t n_fit, const double *x_est, const double *lnp_est, int64_t n_est,
                   int ndim, int ds_id, const double *lower, const double *upper, int64_t n_draws, int n_rep, uint64_t seed,
                   double neff, int max_iter, double tol, int target, double *out, double *moments, double *draws,
                   double *draw_lnp, double *draw_lnq, double *est_lnq) {
    if (!h) return fail(MP_EINVAL, "mp_bridge_logz: NULL argument");
    int rc;
    if ((rc = check_bridge_args(x_fit, n_fit, x_est, lnp_est, n_est, ndim, lower, upper, n_draws, n_rep, neff, max_iter, tol, target, out)))
        return rc;
    if (target == 0 && (ds_id < 0 || ds_id >= MP_MAX_DATASETS)) return fail(MP_EINVAL, "mp_bridge_logz: ds_id %d out of range", ds_id);
    Evaluator *ev = h->first();
    Held held(h, ev);
    const int32_t ds = ds_id;
    if ((rc = check_create(h, "mp_bridge_logz", "the estimate runs on ONE device; a multi-device handle serves the host-buffer batches",
                           ndim, target, "call", 1, &ds, [] { return (int)MP_OK; })))
        return rc;
    hipStream_t st = ev->stream;
    const int nm = mp::bridge_n_moments(ndim);
    const int64_t chunk = kChunkBlocks * MP_BRIDGE_BLOCK, n_blocks = (n_fit + MP_BRIDGE_BLOCK - 1) / MP_BRIDGE_BLOCK;
    const int64_t total = n_draws * n_rep;
    DevBuf<double> d_rows, d_lnp_in, d_part, d_mom, d_draws, d_lnp, d_lnq, d_b, d_a, d_est_lnq, d_out;
    DevBuf<int32_t> d_dsid, d_status;
    if ((rc = d_rows.ensure((size_t)std::min(chunk, std::max(n_fit, n_est)) * ndim)) || (rc = d_lnp_in.ensure((size_t)std::min(chunk, n_est))) ||
        (rc = d_part.ensure((size_t)n_blocks * nm)) || (rc = d_mom.ensure((size_t)nm)) || (rc = d_draws.ensure((size_t)total * ndim)) ||
        (rc = d_lnp.ensure((size_t)total)) || (rc = d_lnq.ensure((size_t)total)) || (rc = d_b.ensure((size_t)total)) ||
        (rc = d_a.ensure((size_t)n_est)) || (rc = d_est_lnq.ensure((size_t)n_est)) || (rc = d_out.ensure((size_t)n_rep * MP_BRIDGE_NOUT)))
        return rc;
    // Everything below enqueues on the evaluator's stream; a failure waits for the stream before the buffers go.
    const auto run = [&]() -> int {
        // 1. the moments of x_fit about its row 0
        for (int64_t lo = 0; lo < n_fit; lo += chunk) {
            const int64_t cnt = std::min(chunk, n_fit - lo);
            HIP_TRY(hipMemcpyAsync(d_rows.p, x_fit + lo * ndim, sizeof(double) * (size_t)cnt * ndim, hipMemcpyHostToDevice, st));
            int e = mp::launch_bridge_moments(d_rows.p, cnt, ndim, x_fit, lo / MP_BRIDGE_BLOCK, d_part.p, (void *)st);
            if (e) return launched(e);
            HIP_TRY(hipStreamSynchronize(st));      // (the next chunk overwrites the rows)
        }
        int e = mp::launch_bridge_combine(d_part.p, n_blocks, ndim, d_mom.p, (void *)st);
        if (e) return launched(e);
        double mom[mp::kBridgeMaxMoments];
        HIP_TRY(hipMemcpyAsync(mom, d_mom.p, sizeof(double) * (size_t)nm, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (moments) std::memcpy(moments, mom, sizeof(double) * (size_t)nm);
        // 2. the proposal
        mp::BridgeGauss g;
        const int bad = mp::bridge_factor(mom, x_fit, n_fit, ndim, g);
        if (bad >= 0)
            return fail(MP_ERANGE, "mp_bridge_logz: the covariance of x_fit is not positive definite at dimension %d (a constant or dependent column)", bad);
        // 3. the draws and their lnprob
        if ((e = mp::launch_bridge_draws(g, seed, n_draws, n_rep, d_draws.p, d_lnq.p, (void *)st))) return launched(e);
        if (target == 0) {
            int r2;
            if ((r2 = d_dsid.ensure((size_t)total)) || (r2 = d_status.ensure((size_t)total)) || (r2 = upload_ds_rows(d_dsid.p, &ds, 1, (int)total)))
                return r2;
            if ((r2 = mp_lnprob_batch_dev(h, d_draws.p, d_dsid.p, (int)total, ndim, d_lnp.p, d_status.p, nullptr, (void *)st))) return r2;
        }
        mp::BridgeBox box{};
        if (lower) {
            box.on = 1;
            for (int d = 0; d < ndim; ++d) { box.lower[d] = lower[d]; box.upper[d] = upper[d]; }
        }
        if ((e = mp::launch_bridge_b(box, target, ndim, d_draws.p, d_lnp.p, d_lnq.p, total, d_b.p, (void *)st))) return launched(e);
        // 4. the proposal density at the estimator rows
        for (int64_t lo = 0; lo < n_est; lo += chunk) {
            const int64_t cnt = std::min(chunk, n_est - lo);
            HIP_TRY(hipMemcpyAsync(d_rows.p, x_est + lo * ndim, sizeof(double) * (size_t)cnt * ndim, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(d_lnp_in.p, lnp_est + lo, sizeof(double) * (size_t)cnt, hipMemcpyHostToDevice, st));
            if ((e = mp::launch_bridge_est(g, d_rows.p, d_lnp_in.p, cnt, d_est_lnq.p + lo, d_a.p + lo, (void *)st))) return launched(e);
            HIP_TRY(hipStreamSynchronize(st));
        }
        // 5. the fixed point
        mp::BridgeFixedArgs f{};
        {
#pragma clang fp contract(off)
            const double dn1 = (double)n_est, dn2 = (double)n_draws, den = neff + dn2;
            f.ln_s1 = std::log(neff / den);
            f.ln_s2 = std::log(dn2 / den);
            f.ln_n1 = std::log(dn1);
            f.ln_n2 = std::log(dn2);
            f.tau = dn1 / neff;
            double lv = 0.0;
            if (lower)
                for (int d = 0; d < ndim; ++d) lv = lv + std::log(upper[d] - lower[d]);
            f.ln_volume = lv;
        }
        f.a = d_a.p;
        f.b = d_b.p;
        f.out = d_out.p;
        f.n1 = n_est;
        f.n2 = n_draws;
        f.tol = tol;
        f.max_iter = max_iter;
        f.n_rep = n_rep;
        if ((e = mp::launch_bridge_fixed(f, (void *)st))) return launched(e);
        HIP_TRY(hipMemcpyAsync(out, d_out.p, sizeof(double) * (size_t)n_rep * MP_BRIDGE_NOUT, hipMemcpyDeviceToHost, st));
        if (draws) HIP_TRY(hipMemcpyAsync(draws, d_draws.p, sizeof(double) * (size_t)total * ndim, hipMemcpyDeviceToHost, st));
        if (draw_lnp) HIP_TRY(hipMemcpyAsync(draw_lnp, d_lnp.p, sizeof(double) * (size_t)total, hipMemcpyDeviceToHost, st));
        if (draw_lnq) HIP_TRY(hipMemcpyAsync(draw_lnq, d_lnq.p, sizeof(double) * (size_t)total, hipMemcpyDeviceToHost, st));
        if (est_lnq) HIP_TRY(hipMemcpyAsync(est_lnq, d_est_lnq.p, sizeof(double) * (size_t)n_est, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return MP_OK;
    };
    rc = run();
    if (rc) (void)hipStreamSynchronize(st);
    return rc;
}

}  // extern "C"
