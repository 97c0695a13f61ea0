// bridge_host_check.cpp — the host-only parts of the bridge-sampling evidence (magprop_amd/csrc/mp_bridge.h bridge_factor,
// mp_bridge.cpp check_bridge_args) under the address and undefined-behaviour sanitizers, on a machine without a GPU: the Cholesky
// rule against a factor multiplied back, on every ndim and on rows whose covariance is singular, and every argument the entry
// refuses before it touches a handle, with arrays of exactly the sizes it may read.  bridge_host_stubs.h compiles mp_bridge.cpp
// itself for the host and stands in for what the library defines elsewhere; no HIP call is made.  From the repository root:
//
//   hipcc -x hip --offload-host-only -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       tools/bridge_host_check.cpp -o /tmp/bridge_host_check && /tmp/bridge_host_check
#include "bridge_host_stubs.h"

static void factor_checks() {
    for (int ndim = 1; ndim <= MP_MAX_NDIM; ++ndim) {
        const int n = 500;
        const std::vector<double> x = rows_of(n, ndim, -1), mom = sums_of(x, n, ndim);
        mp::BridgeGauss g;
        expect(mp::bridge_factor(mom.data(), x.data(), n, ndim, g) == -1, "a full covariance factors");
        double worst = 0.0, c = 0.5 * ndim * 1.8378770664093453;
        for (int a = 0; a < ndim; ++a) {
            c += std::log(g.L[a * (a + 1) / 2 + a]);
            for (int b = 0; b <= a; ++b) {       // L L^T against the covariance the rule states
                double llt = 0.0;
                for (int k = 0; k <= b; ++k) llt += g.L[a * (a + 1) / 2 + k] * g.L[b * (b + 1) / 2 + k];
                const double cov = (mom[ndim + a * (a + 1) / 2 + b] - mom[a] * mom[b] / n) / (n - 1);
                worst = std::max(worst, std::fabs(llt - cov) / (std::fabs(cov) + 1.0));
            }
        }
        expect(worst < 1e-13, "L L^T is the covariance");
        expect(std::fabs(c - g.c) < 1e-12 && g.ndim == ndim, "the constant of ln q");
        if (ndim >= 2) {
            const int col = ndim / 2;
            const std::vector<double> xc = rows_of(n, ndim, col), mc = sums_of(xc, n, ndim);
            expect(mp::bridge_factor(mc.data(), xc.data(), n, ndim, g) == col, "a constant column fails at its dimension");
        }
        std::vector<double> bad = mom;
        bad[0] = std::numeric_limits<double>::quiet_NaN();
        expect(mp::bridge_factor(bad.data(), x.data(), n, ndim, g) == 0, "a NaN sum fails at dimension 0");
    }
}

static void argument_checks() {
    const int nd = 6, n = 16;
    std::vector<double> x = rows_of(n, nd, -1), lnp(n, -1.0), out(MP_BRIDGE_NOUT), lo(nd, -100.0), hi(nd, 100.0);
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const auto call = [&](const double *xf, int64_t n_fit, const double *xe, const double *le, int64_t n_est, int ndim, const double *l,
                          const double *u, int64_t n_draws, int n_rep, double neff, int max_iter, double tol, int target) {
        return check_bridge_args(xf, n_fit, xe, le, n_est, ndim, l, u, n_draws, n_rep, neff, max_iter, tol, target, out.data());
    };
    const double *X = x.data(), *P = lnp.data(), *L = lo.data(), *U = hi.data();
    expect(call(X, n, X, P, n, nd, L, U, 8, 1, 16.0, 10, 1e-8, 0) == MP_OK, "a good call");
    expect(call(X, n, X, P, n, nd, nullptr, nullptr, 8, 64, 0.5, 1, 0.0, 1) == MP_OK, "a good call without a box");
    expect(call(nullptr, n, X, P, n, nd, L, U, 8, 1, 16.0, 10, 1e-8, 0) == MP_EINVAL, "NULL x_fit");
    expect(call(X, n, X, nullptr, n, nd, L, U, 8, 1, 16.0, 10, 1e-8, 0) == MP_EINVAL, "NULL lnp_est");
    expect(call(X, n, X, P, n, nd, L, U, 8, 1, 16.0, 10, 1e-8, 3) == MP_EINVAL, "target 3");
    expect(call(X, n, X, P, n, 5, L, U, 8, 1, 16.0, 10, 1e-8, 0) == MP_EINVAL, "ndim 5 on the posterior");
    expect(call(X, n, X, P, n, 0, nullptr, nullptr, 8, 1, 16.0, 10, 1e-8, 1) == MP_EINVAL, "ndim 0");
    expect(call(X, n, X, P, n, MP_MAX_NDIM + 1, nullptr, nullptr, 8, 1, 16.0, 10, 1e-8, 1) == MP_EINVAL, "ndim 10");
    expect(call(X, nd + 1, X, P, n, nd, L, U, 8, 1, 16.0, 10, 1e-8, 0) == MP_EINVAL, "n_fit = ndim + 1");
    expect(call(X, n, X, P, 0, nd, L, U, 8, 1, 16.0, 10, 1e-8, 0) == MP_EINVAL, "n_est 0");
    expect(call(X, n, X, P, n, nd, L, U, 0, 1, 16.0, 10, 1e-8, 0) == MP_EINVAL, "n_draws 0");
    expect(call(X, n, X, P, n, nd, L, U, 8, 0, 16.0, 10, 1e-8, 0) == MP_EINVAL, "n_rep 0");
    expect(call(X, n, X, P, n, nd, L, U, 8, MP_BRIDGE_MAX_REP + 1, 16.0, 10, 1e-8, 0) == MP_EINVAL, "n_rep 65");
    expect(call(X, n, X, P, n, nd, L, U, (int64_t)MP_BRIDGE_MAX_ROWS + 1, 1, 16.0, 10, 1e-8, 0) == MP_EINVAL, "n_draws above the cap");
    expect(call(X, n, X, P, n, nd, L, U, (int64_t)1 << 62, 64, 16.0, 10, 1e-8, 0) == MP_EINVAL, "a product that would overflow");
    expect(call(X, (int64_t)MP_BRIDGE_MAX_ROWS + 1, X, P, n, nd, L, U, 8, 1, 16.0, 10, 1e-8, 0) == MP_EINVAL, "n_fit above the cap (no row is read)");
    expect(call(X, n, X, P, (int64_t)MP_BRIDGE_MAX_ROWS + 1, nd, L, U, 8, 1, 16.0, 10, 1e-8, 0) == MP_EINVAL, "n_est above the cap");
    for (double neff : {0.0, -1.0, 16.5, nan, inf}) expect(call(X, n, X, P, n, nd, L, U, 8, 1, neff, 10, 1e-8, 0) == MP_EINVAL, "neff outside (0, n_est]");
    for (double tol : {-1e-9, nan, inf}) expect(call(X, n, X, P, n, nd, L, U, 8, 1, 16.0, 10, tol, 0) == MP_EINVAL, "tol not finite or negative");
    expect(call(X, n, X, P, n, nd, L, U, 8, 1, 16.0, 0, 1e-8, 0) == MP_EINVAL, "max_iter 0");
    expect(call(X, n, X, P, n, nd, nullptr, nullptr, 8, 1, 16.0, 10, 1e-8, 0) == MP_EINVAL, "no box on the posterior");
    expect(call(X, n, X, P, n, nd, L, nullptr, 8, 1, 16.0, 10, 1e-8, 1) == MP_EINVAL, "one bound");
    std::vector<double> empty = hi, open = hi;
    empty[3] = lo[3];
    open[2] = inf;
    expect(call(X, n, X, P, n, nd, L, empty.data(), 8, 1, 16.0, 10, 1e-8, 0) == MP_EINVAL, "an empty box");
    expect(call(X, n, X, P, n, nd, L, open.data(), 8, 1, 16.0, 10, 1e-8, 0) == MP_EINVAL, "an infinite box");
    std::vector<double> xb = x, pb = lnp;
    xb[(size_t)(n - 1) * nd + nd - 1] = nan;          // the last element the entry may read
    pb[n - 1] = -inf;
    expect(call(xb.data(), n, X, P, n, nd, L, U, 8, 1, 16.0, 10, 1e-8, 0) == MP_EINVAL && g_msg.find("x_fit") != std::string::npos, "a NaN in x_fit");
    expect(call(X, n, xb.data(), P, n, nd, L, U, 8, 1, 16.0, 10, 1e-8, 0) == MP_EINVAL && g_msg.find("x_est") != std::string::npos, "a NaN in x_est");
    expect(call(X, n, X, pb.data(), n, nd, L, U, 8, 1, 16.0, 10, 1e-8, 0) == MP_EINVAL && g_msg.find("lnp_est[15]") != std::string::npos, "-inf in lnp_est");
    expect(mp_bridge_logz(nullptr, X, n, X, P, n, nd, 0, L, U, 8, 1, 1, 16.0, 10, 1e-8, 0, out.data(), nullptr, nullptr, nullptr, nullptr, nullptr) == MP_EINVAL,
           "a NULL handle");
}

int main() {
    factor_checks();
    argument_checks();
    if (n_failed) { std::printf("%d check(s) failed\n", n_failed); return 1; }
    std::printf("bridge host checks passed\n");
    return 0;
}
