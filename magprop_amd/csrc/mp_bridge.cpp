// mp_bridge.cpp — the bridge-sampling evidence estimate of host rows (mp_bridge_logz, mp_bridge_logz_warp).  Kernels:
// mp_bridge.hip; the host-only rules (the factor of the proposal, its constant, the constants of the t proposal): mp_bridge.h.
//
// One call with no state: the buffers are the call's own and are given back before it returns.  The rows of x_fit and x_est go
// through the device in chunks of kChunkBlocks blocks of MP_BRIDGE_BLOCK rows, so that the blocks of the moments are cut from
// the rows alone whatever the chunk; a, b and the draws stay on the device between the launches.  Both entries are bridge_run on
// a BridgeCall: the checks, the buffers, the chunks, the moments, the factor and the fixed point are one code; what differs is
// which kernels form the draws, lnq, a and b (mp_bridge_logz keeps its own three).
#include "mp_bridge.h"
#include "mp_host.h"

namespace {

constexpr int64_t kChunkBlocks = 64;   // rows of a chunk: 64 * MP_BRIDGE_BLOCK

int rows_finite(const char *fn, const char *what, const double *rows, int64_t n, int ndim) {
    for (int64_t i = 0; i < n; ++i)
        for (int d = 0; d < ndim; ++d)
            if (!std::isfinite(rows[i * ndim + d])) return fail(MP_EINVAL, "%s: row %lld of %s is not finite", fn, (long long)i, what);
    return MP_OK;
}

// the checks that need no handle, in the order they fail; max_target: 2 for mp_bridge_logz, 4 for mp_bridge_logz_warp
int check_bridge_args(const double *x_fit, int64_t n_fit, const double *x_est, const double *lnp_est, int64_t n_est, int ndim,
                      const double *lower, const double *upper, int64_t n_draws, int n_rep, double neff, int max_iter, double tol,
                      int target, const double *out, int max_target = 2, const char *fn = "mp_bridge_logz") {
    if (!x_fit || !x_est || !lnp_est || !out) return fail(MP_EINVAL, "%s: NULL argument", fn);
    if (target < 0 || target > max_target) return fail(MP_EINVAL, "%s: target must be 0 .. %d, got %d", fn, max_target, target);
    if (ndim < 1 || ndim > MP_MAX_NDIM || (target == 0 && ndim < 6)) return fail(MP_EINVAL, "%s: bad ndim %d", fn, ndim);
    if (n_fit < ndim + 2) return fail(MP_EINVAL, "%s: n_fit must be at least ndim + 2 = %d, got %lld", fn, ndim + 2, (long long)n_fit);
    if (n_est < 1 || n_draws < 1) return fail(MP_EINVAL, "%s: n_est and n_draws must be at least 1", fn);
    if (n_rep < 1 || n_rep > MP_BRIDGE_MAX_REP) return fail(MP_EINVAL, "%s: n_rep must be 1..%d, got %d", fn, MP_BRIDGE_MAX_REP, n_rep);
    if (n_fit > MP_BRIDGE_MAX_ROWS || n_est > MP_BRIDGE_MAX_ROWS || n_draws > MP_BRIDGE_MAX_ROWS || n_draws * n_rep > MP_BRIDGE_MAX_ROWS)
        return fail(MP_EINVAL, "%s: n_fit, n_est and n_rep * n_draws must not exceed %lld (MP_BRIDGE_MAX_ROWS)", fn, (long long)MP_BRIDGE_MAX_ROWS);
    if (!(neff > 0.0 && neff <= (double)n_est)) return fail(MP_EINVAL, "%s: neff must be in (0, n_est], got %g", fn, neff);
    if (!(std::isfinite(tol) && tol >= 0.0)) return fail(MP_EINVAL, "%s: tol must be finite and >= 0, got %g", fn, tol);
    if (max_iter < 1) return fail(MP_EINVAL, "%s: max_iter must be at least 1, got %d", fn, max_iter);
    if (!lower != !upper || (target == 0 && !lower)) return fail(MP_EINVAL, "%s: the box is NULL (allowed for the test targets, both bounds)", fn);
    int rc;
    if (lower && (rc = check_box(fn, ndim, lower, upper))) return rc;
    if ((rc = rows_finite(fn, "x_fit", x_fit, n_fit, ndim)) || (rc = rows_finite(fn, "x_est", x_est, n_est, ndim))) return rc;
    for (int64_t i = 0; i < n_est; ++i)
        if (!std::isfinite(lnp_est[i])) return fail(MP_EINVAL, "%s: lnp_est[%lld] is not finite", fn, (long long)i);
    return MP_OK;
}

// what mp_bridge_logz_warp adds to them (n_draws and n_rep have passed the checks above)
int check_bridge_warp_args(int proposal, int nu, int warp, int64_t n_draws, int n_rep) {
    if (proposal != MP_BRIDGE_NORMAL && proposal != MP_BRIDGE_STUDENT)
        return fail(MP_EINVAL, "mp_bridge_logz_warp: proposal must be MP_BRIDGE_NORMAL (0) or MP_BRIDGE_STUDENT (1), got %d", proposal);
    if (proposal == MP_BRIDGE_STUDENT && (nu < 3 || nu > MP_BRIDGE_MAX_NU))
        return fail(MP_EINVAL, "mp_bridge_logz_warp: nu must be 3..%d, got %d", MP_BRIDGE_MAX_NU, nu);
    if (warp != 0 && warp != 1) return fail(MP_EINVAL, "mp_bridge_logz_warp: warp must be 0 or 1, got %d", warp);
    if (warp && 2 * n_draws * n_rep > MP_BRIDGE_MAX_ROWS)
        return fail(MP_EINVAL, "mp_bridge_logz_warp: with warp, 2 * n_rep * n_draws must not exceed %lld (MP_BRIDGE_MAX_ROWS)", (long long)MP_BRIDGE_MAX_ROWS);
    return MP_OK;
}

// The arguments of either entry, checked.  own_kernels: mp_bridge_logz, whose draws, lnq, a and b come from its own three kernels
// and whose out rows are MP_BRIDGE_NOUT wide; otherwise the kernels of both proposals and out rows of MP_BRIDGE_WARP_NOUT.
struct BridgeCall {
    const char *fn;
    bool own_kernels;
    const double *x_fit;
    int64_t n_fit;
    const double *x_est, *lnp_est;
    int64_t n_est;
    int ndim, ds_id;
    const double *lower, *upper;
    int64_t n_draws;
    int n_rep;
    uint64_t seed;
    double neff;
    int max_iter;
    double tol;
    int target, proposal, nu, warp;
    double *out, *moments, *draws, *draw_lnp, *draw_lnq, *est_lnq;
    double *a_out, *b_out, *draw_mirrors, *est_mirror_lnp, *draw_mirror_lnp;   // mp_bridge_logz_warp's
};

int bridge_run(mp_handle *h, const BridgeCall &c) {
    const int ndim = c.ndim, n_rep = c.n_rep, target = c.target;
    const int64_t n_fit = c.n_fit, n_est = c.n_est, n_draws = c.n_draws;
    const bool warp = c.warp != 0;
    int rc;
    if (target == 0 && (c.ds_id < 0 || c.ds_id >= MP_MAX_DATASETS)) return fail(MP_EINVAL, "%s: ds_id %d out of range", c.fn, c.ds_id);
    Evaluator *ev = h->first();
    Held held(h, ev);
    const int32_t ds = c.ds_id;
    if ((rc = check_create(h, c.fn, "the estimate runs on ONE device; a multi-device handle serves the host-buffer batches",
                           ndim, target, "call", 1, &ds, [] { return (int)MP_OK; })))
        return rc;
    hipStream_t st = ev->stream;
    const int nm = mp::bridge_n_moments(ndim);
    const int64_t chunk = kChunkBlocks * MP_BRIDGE_BLOCK, n_blocks = (n_fit + MP_BRIDGE_BLOCK - 1) / MP_BRIDGE_BLOCK;
    const int64_t total = n_draws * n_rep, est_chunk = std::min(chunk, n_est);
    // with warp the mirrors lie behind the draws: rows total .. 2 total of d_draws, of d_lnp and of the one batch of target 0
    const int64_t evals = warp ? 2 * total : total, batch_rows = warp ? std::max(evals, est_chunk) : evals;
    DevBuf<double> d_rows, d_lnp_in, d_part, d_mom, d_draws, d_lnp, d_lnq, d_b, d_a, d_est_lnq, d_out, d_rows_m, d_est_lnp_m, d_cnt;
    DevBuf<uint8_t> d_flag, d_est_flag;
    DevBuf<int32_t> d_dsid, d_status;
    if ((rc = d_rows.ensure((size_t)std::min(chunk, std::max(n_fit, n_est)) * ndim)) || (rc = d_lnp_in.ensure((size_t)est_chunk)) ||
        (rc = d_part.ensure((size_t)n_blocks * nm)) || (rc = d_mom.ensure((size_t)nm)) || (rc = d_draws.ensure((size_t)evals * ndim)) ||
        (rc = d_lnp.ensure((size_t)evals)) || (rc = d_lnq.ensure((size_t)total)) || (rc = d_b.ensure((size_t)total)) ||
        (rc = d_a.ensure((size_t)n_est)) || (rc = d_est_lnq.ensure((size_t)n_est)) || (rc = d_out.ensure((size_t)n_rep * MP_BRIDGE_NOUT)))
        return rc;
    if (warp && ((rc = d_rows_m.ensure((size_t)est_chunk * ndim)) || (rc = d_est_lnp_m.ensure((size_t)n_est)) ||
                 (rc = d_cnt.ensure((size_t)n_rep + 1)) || (rc = d_flag.ensure((size_t)total)) || (rc = d_est_flag.ensure((size_t)n_est))))
        return rc;
    // Everything below enqueues on the evaluator's stream; a failure waits for the stream before the buffers go.
    const auto run = [&]() -> int {
        // 1. the moments of x_fit about its row 0
        for (int64_t lo = 0; lo < n_fit; lo += chunk) {
            const int64_t cnt = std::min(chunk, n_fit - lo);
            HIP_TRY(hipMemcpyAsync(d_rows.p, c.x_fit + lo * ndim, sizeof(double) * (size_t)cnt * ndim, hipMemcpyHostToDevice, st));
            int e = mp::launch_bridge_moments(d_rows.p, cnt, ndim, c.x_fit, lo / MP_BRIDGE_BLOCK, d_part.p, (void *)st);
            if (e) return launched(e);
            HIP_TRY(hipStreamSynchronize(st));      // (the next chunk overwrites the rows)
        }
        int e = mp::launch_bridge_combine(d_part.p, n_blocks, ndim, d_mom.p, (void *)st);
        if (e) return launched(e);
        double mom[mp::kBridgeMaxMoments];
        HIP_TRY(hipMemcpyAsync(mom, d_mom.p, sizeof(double) * (size_t)nm, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (c.moments) std::memcpy(c.moments, mom, sizeof(double) * (size_t)nm);
        // 2. the proposal
        mp::BridgeGauss g;
        mp::BridgeStudent t{};
        const int bad = mp::bridge_factor(mom, c.x_fit, n_fit, ndim, g);
        if (bad >= 0)
            return fail(MP_ERANGE, "%s: the covariance of x_fit is not positive definite at dimension %d (a constant or dependent column)", c.fn, bad);
        if (c.proposal == MP_BRIDGE_STUDENT) {
            const mp::BridgeGauss gauss = g;
            mp::bridge_student(gauss, c.nu, g, t);
        }
        // 3. the draws and their lnprob
        double *d_mirrors = warp ? d_draws.p + total * ndim : nullptr, *d_lnp_m = warp ? d_lnp.p + total : nullptr;
        if (c.own_kernels) e = mp::launch_bridge_draws(g, c.seed, n_draws, n_rep, d_draws.p, d_lnq.p, (void *)st);
        else e = mp::launch_bridge_draws_warp(g, t, c.seed, n_draws, n_rep, d_draws.p, d_mirrors, d_lnq.p, (void *)st);
        if (e) return launched(e);
        if (target == 0) {
            int r2;
            if ((r2 = d_dsid.ensure((size_t)batch_rows)) || (r2 = d_status.ensure((size_t)batch_rows)) ||
                (r2 = upload_ds_rows(d_dsid.p, &ds, 1, (int)batch_rows)))
                return r2;
            if ((r2 = mp_lnprob_batch_dev(h, d_draws.p, d_dsid.p, (int)evals, ndim, d_lnp.p, d_status.p, nullptr, (void *)st))) return r2;
        }
        mp::BridgeBox box{};
        if (c.lower) {
            box.on = 1;
            for (int d = 0; d < ndim; ++d) { box.lower[d] = c.lower[d]; box.upper[d] = c.upper[d]; }
        }
        if (c.own_kernels) {
            e = mp::launch_bridge_b(box, target, ndim, d_draws.p, d_lnp.p, d_lnq.p, total, d_b.p, (void *)st);
        } else {
            mp::BridgePairArgs p{};
            p.x = d_draws.p; p.xm = d_mirrors; p.lnp = d_lnp.p; p.lnp_m = d_lnp_m; p.lnq = d_lnq.p; p.ab = d_b.p; p.counted_m = d_flag.p;
            p.n = total; p.target = target; p.ndim = ndim; p.given = target == 0; p.test_row = 1;
            e = mp::launch_bridge_pair(box, p, (void *)st);
            if (!e && warp) e = mp::launch_bridge_count(d_flag.p, n_draws, n_rep, d_cnt.p, (void *)st);
        }
        if (e) return launched(e);
        // 4. the proposal density at the estimator rows
        for (int64_t lo = 0; lo < n_est; lo += chunk) {
            const int64_t cnt = std::min(chunk, n_est - lo);
            HIP_TRY(hipMemcpyAsync(d_rows.p, c.x_est + lo * ndim, sizeof(double) * (size_t)cnt * ndim, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(d_lnp_in.p, c.lnp_est + lo, sizeof(double) * (size_t)cnt, hipMemcpyHostToDevice, st));
            if (c.own_kernels) {
                e = mp::launch_bridge_est(g, d_rows.p, d_lnp_in.p, cnt, d_est_lnq.p + lo, d_a.p + lo, (void *)st);
            } else {
                if ((e = mp::launch_bridge_est_warp(g, t, d_rows.p, cnt, d_est_lnq.p + lo, d_rows_m.p, (void *)st))) return launched(e);
                int r2;
                if (warp && target == 0 &&
                    (r2 = mp_lnprob_batch_dev(h, d_rows_m.p, d_dsid.p, (int)cnt, ndim, d_est_lnp_m.p + lo, d_status.p, nullptr, (void *)st)))
                    return r2;
                mp::BridgePairArgs p{};
                p.x = d_rows.p; p.xm = d_rows_m.p; p.lnp = d_lnp_in.p; p.lnp_m = warp ? d_est_lnp_m.p + lo : nullptr; p.lnq = d_est_lnq.p + lo;
                p.ab = d_a.p + lo; p.counted_m = warp ? d_est_flag.p + lo : nullptr;
                p.n = cnt; p.target = target; p.ndim = ndim; p.given = 1; p.test_row = 0;
                e = mp::launch_bridge_pair(box, p, (void *)st);
            }
            if (e) return launched(e);
            HIP_TRY(hipStreamSynchronize(st));
        }
        if (warp && (e = mp::launch_bridge_count(d_est_flag.p, n_est, 1, d_cnt.p + n_rep, (void *)st))) return launched(e);
        // 5. the fixed point
        mp::BridgeFixedArgs f{};
        {
#pragma clang fp contract(off)
            const double dn1 = (double)n_est, dn2 = (double)n_draws, den = c.neff + dn2;
            f.ln_s1 = std::log(c.neff / den);
            f.ln_s2 = std::log(dn2 / den);
            f.ln_n1 = std::log(dn1);
            f.ln_n2 = std::log(dn2);
            f.tau = dn1 / c.neff;
            double lv = 0.0;
            if (c.lower)
                for (int d = 0; d < ndim; ++d) lv = lv + std::log(c.upper[d] - c.lower[d]);
            f.ln_volume = lv;
        }
        f.a = d_a.p;
        f.b = d_b.p;
        f.out = d_out.p;
        f.n1 = n_est;
        f.n2 = n_draws;
        f.tol = c.tol;
        f.max_iter = c.max_iter;
        f.n_rep = n_rep;
        if ((e = mp::launch_bridge_fixed(f, (void *)st))) return launched(e);
        const auto back = [&](double *dst, const double *src, int64_t n) {
            return dst ? hipMemcpyAsync(dst, src, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, st) : hipSuccess;
        };
        std::vector<double> rows12, counts;
        if (c.own_kernels) {
            HIP_TRY(back(c.out, d_out.p, (int64_t)n_rep * MP_BRIDGE_NOUT));
        } else {
            rows12.resize((size_t)n_rep * MP_BRIDGE_NOUT);
            counts.assign((size_t)n_rep + 1, 0.0);
            HIP_TRY(back(rows12.data(), d_out.p, (int64_t)rows12.size()));
            if (warp) HIP_TRY(back(counts.data(), d_cnt.p, (int64_t)counts.size()));
        }
        HIP_TRY(back(c.draws, d_draws.p, total * ndim));
        HIP_TRY(back(c.draw_lnp, d_lnp.p, total));
        HIP_TRY(back(c.draw_lnq, d_lnq.p, total));
        HIP_TRY(back(c.est_lnq, d_est_lnq.p, n_est));
        HIP_TRY(back(c.a_out, d_a.p, n_est));
        HIP_TRY(back(c.b_out, d_b.p, total));
        if (warp) {
            HIP_TRY(back(c.draw_mirrors, d_mirrors, total * ndim));
            HIP_TRY(back(c.draw_mirror_lnp, d_lnp_m, total));
            HIP_TRY(back(c.est_mirror_lnp, d_est_lnp_m.p, n_est));
        }
        HIP_TRY(hipStreamSynchronize(st));
        for (int r = 0; !c.own_kernels && r < n_rep; ++r) {
            double *row = c.out + (size_t)r * MP_BRIDGE_WARP_NOUT;
            std::memcpy(row, rows12.data() + (size_t)r * MP_BRIDGE_NOUT, sizeof(double) * MP_BRIDGE_NOUT);
            row[MP_BRIDGE_EST_MIRRORS] = counts[(size_t)n_rep];
            row[MP_BRIDGE_DRAW_MIRRORS] = counts[(size_t)r];
        }
        return MP_OK;
    };
    rc = run();
    if (rc) (void)hipStreamSynchronize(st);
    return rc;
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
    const BridgeCall c{"mp_bridge_logz", true, x_fit, n_fit, x_est, lnp_est, n_est, ndim, ds_id, lower, upper, n_draws, n_rep, seed, neff,
                       max_iter, tol, target, MP_BRIDGE_NORMAL, 0, 0, out, moments, draws, draw_lnp, draw_lnq, est_lnq,
                       nullptr, nullptr, nullptr, nullptr, nullptr};
    return bridge_run(h, c);
}

int mp_bridge_logz_warp(mp_handle *h, const double *x_fit, int64_t n_fit, const double *x_est, const double *lnp_est, int64_t n_est,
                        int ndim, int ds_id, const double *lower, const double *upper, int64_t n_draws, int n_rep, uint64_t seed,
                        double neff, int max_iter, double tol, int target, int proposal, int nu, int warp, double *out,
                        double *moments, double *draws, double *draw_lnp, double *draw_lnq, double *est_lnq, double *a_out,
                        double *b_out, double *draw_mirrors, double *est_mirror_lnp, double *draw_mirror_lnp) {
    if (!h) return fail(MP_EINVAL, "mp_bridge_logz_warp: NULL argument");
    int rc;
    if ((rc = check_bridge_args(x_fit, n_fit, x_est, lnp_est, n_est, ndim, lower, upper, n_draws, n_rep, neff, max_iter, tol, target, out, 4,
                                "mp_bridge_logz_warp")) ||
        (rc = check_bridge_warp_args(proposal, nu, warp, n_draws, n_rep)))
        return rc;
    const BridgeCall c{"mp_bridge_logz_warp", false, x_fit, n_fit, x_est, lnp_est, n_est, ndim, ds_id, lower, upper, n_draws, n_rep, seed,
                       neff, max_iter, tol, target, proposal, nu, warp, out, moments, draws, draw_lnp, draw_lnq, est_lnq,
                       a_out, b_out, draw_mirrors, est_mirror_lnp, draw_mirror_lnp};
    return bridge_run(h, c);
}

}  // extern "C"
