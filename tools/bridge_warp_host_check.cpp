// bridge_warp_host_check.cpp — the host-only parts mp_bridge_logz_warp adds to the bridge-sampling evidence
// (magprop_amd/csrc/mp_bridge.h bridge_student, mp_bridge.cpp check_bridge_warp_args and the wider target range of
// check_bridge_args) under the address and undefined-behaviour sanitizers, on a machine without a GPU: the constants of the t
// proposal against the closed form of the multivariate t density on every ndim and nu, and every argument the new entry refuses
// before it touches a handle.  bridge_host_stubs.h compiles mp_bridge.cpp itself for the host and stands in for what the
// library defines elsewhere; no HIP call is made.  From the repository root:
//
//   hipcc -x hip --offload-host-only -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       tools/bridge_warp_host_check.cpp -o /tmp/bridge_warp_host_check && /tmp/bridge_warp_host_check
#include "bridge_host_stubs.h"

static void student_checks() {
    for (int ndim = 1; ndim <= MP_MAX_NDIM; ++ndim) {
        const int n = 500;
        const std::vector<double> x = rows_of(n, ndim, -1), mom = sums_of(x, n, ndim);
        mp::BridgeGauss g;
        expect(mp::bridge_factor(mom.data(), x.data(), n, ndim, g) == -1, "a full covariance factors");
        for (int nu = 3; nu <= MP_BRIDGE_MAX_NU; ++nu) {
            mp::BridgeGauss gt;
            mp::BridgeStudent t{};
            mp::bridge_student(g, nu, gt, t);
            expect(t.on == 1 && t.n_nu == nu && t.nu == (double)nu && t.h == 0.5 * (nu + ndim) && gt.ndim == ndim, "nu, h and ndim");
            // the covariance of the t proposal, nu / (nu - 2) L_t L_t^T, is that of the Gaussian
            double worst = 0.0, ln_det = 0.0;
            for (int a = 0; a < ndim; ++a) {
                ln_det += std::log(gt.L[a * (a + 1) / 2 + a]);
                expect(gt.m[a] == g.m[a], "the mean is the Gaussian's");
                for (int b = 0; b <= a; ++b) {
                    const double lt = gt.L[a * (a + 1) / 2 + b], l = g.L[a * (a + 1) / 2 + b];
                    worst = std::max(worst, std::fabs(lt * lt * nu / (nu - 2.0) - l * l) / (l * l + 1e-300));
                }
            }
            expect(worst < 1e-14, "L_t L_t^T nu / (nu - 2) is L L^T");
            // -c_t is the log of the density's constant Gamma((nu + d) / 2) / (Gamma(nu / 2) (nu pi)^(d / 2) |L_t|)
            const double want = ln_det + 0.5 * ndim * std::log(nu * 3.141592653589793) + std::lgamma(0.5 * nu) - std::lgamma(0.5 * (nu + ndim));
            expect(std::fabs(gt.c - want) < 1e-12 && std::isfinite(gt.c), "the constant of ln q of the t proposal");
        }
    }
}

static void argument_checks() {
    const int nd = 6, n = 16;
    std::vector<double> x = rows_of(n, nd, -1), lnp(n, -1.0), out(MP_BRIDGE_WARP_NOUT), lo(nd, -100.0), hi(nd, 100.0);
    const double *X = x.data(), *P = lnp.data(), *L = lo.data(), *U = hi.data();
    // the wider target range, under the new entry's name
    for (int target = 0; target <= 4; ++target)
        expect(check_bridge_args(X, n, X, P, n, nd, L, U, 8, 1, 16.0, 10, 1e-8, target, out.data(), 4, "mp_bridge_logz_warp") == MP_OK, "targets 0 .. 4");
    expect(check_bridge_args(X, n, X, P, n, nd, nullptr, nullptr, 8, 1, 16.0, 10, 1e-8, 4, out.data(), 4, "mp_bridge_logz_warp") == MP_OK, "target 4 without a box");
    for (int target : {-1, 5, 1 << 30})
        expect(check_bridge_args(X, n, X, P, n, nd, L, U, 8, 1, 16.0, 10, 1e-8, target, out.data(), 4, "mp_bridge_logz_warp") == MP_EINVAL &&
                   g_msg.find("mp_bridge_logz_warp") != std::string::npos, "target outside 0 .. 4");
    expect(check_bridge_args(X, n, X, P, n, nd, L, U, 8, 1, 16.0, 10, 1e-8, 3, out.data()) == MP_EINVAL && g_msg.find("mp_bridge_logz:") != std::string::npos,
           "target 3 stays refused by mp_bridge_logz");
    // proposal, nu, warp and the rows of a warped call
    const int64_t cap = MP_BRIDGE_MAX_ROWS;
    expect(check_bridge_warp_args(MP_BRIDGE_NORMAL, 0, 0, 8, 1) == MP_OK, "the plain call");
    expect(check_bridge_warp_args(MP_BRIDGE_NORMAL, -7, 1, 8, 1) == MP_OK, "nu is not read for the Gaussian");
    for (int nu : {3, 4, 5, MP_BRIDGE_MAX_NU}) expect(check_bridge_warp_args(MP_BRIDGE_STUDENT, nu, 1, 8, 1) == MP_OK, "nu in 3 .. 32");
    for (int nu : {-1, 0, 2, MP_BRIDGE_MAX_NU + 1, 1 << 30}) expect(check_bridge_warp_args(MP_BRIDGE_STUDENT, nu, 0, 8, 1) == MP_EINVAL, "nu outside 3 .. 32");
    for (int proposal : {-1, 2, 1 << 30}) expect(check_bridge_warp_args(proposal, 5, 0, 8, 1) == MP_EINVAL, "proposal outside 0 .. 1");
    for (int warp : {-1, 2, 1 << 30}) expect(check_bridge_warp_args(MP_BRIDGE_STUDENT, 5, warp, 8, 1) == MP_EINVAL, "warp outside 0 .. 1");
    expect(check_bridge_warp_args(MP_BRIDGE_NORMAL, 0, 1, cap / 2, 1) == MP_OK, "2 n_rep n_draws at the cap");
    expect(check_bridge_warp_args(MP_BRIDGE_NORMAL, 0, 1, cap / 2 + 1, 1) == MP_EINVAL, "2 n_rep n_draws above the cap");
    expect(check_bridge_warp_args(MP_BRIDGE_NORMAL, 0, 1, cap / 64, 33) == MP_EINVAL, "2 n_rep n_draws above the cap over repetitions");
    expect(check_bridge_warp_args(MP_BRIDGE_NORMAL, 0, 0, cap / 2 + 1, 1) == MP_OK, "the cap on warped rows is not read without warp");
    // the entry itself returns before it reads the handle
    mp_handle *no_handle = nullptr;
    expect(mp_bridge_logz_warp(no_handle, X, n, X, P, n, nd, 0, L, U, 8, 1, 1, 16.0, 10, 1e-8, 0, 0, 0, 0, out.data(), nullptr, nullptr, nullptr,
                               nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == MP_EINVAL, "a NULL handle");
    alignas(16) static unsigned char blank[4096];     // no handle: the entry must not get as far as reading it
    mp_handle *unread = reinterpret_cast<mp_handle *>(blank);
    expect(mp_bridge_logz_warp(unread, X, n, X, P, n, nd, 0, L, U, 8, 1, 1, 16.0, 10, 1e-8, 0, 2, 5, 0, out.data(), nullptr, nullptr, nullptr,
                               nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == MP_EINVAL, "proposal 2 through the entry");
    expect(mp_bridge_logz_warp(unread, X, n, X, P, n, nd, 0, L, U, 8, 1, 1, 16.0, 10, 1e-8, 5, 0, 5, 0, out.data(), nullptr, nullptr, nullptr,
                               nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == MP_EINVAL, "target 5 through the entry");
    expect(mp_bridge_logz_warp(unread, X, n, X, P, n, nd, 0, L, U, 8, 1, 1, 16.0, 10, 1e-8, 0, 1, 2, 1, out.data(), nullptr, nullptr, nullptr,
                               nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == MP_EINVAL, "nu 2 through the entry");
}

int main() {
    student_checks();
    argument_checks();
    if (n_failed) { std::printf("%d check(s) failed\n", n_failed); return 1; }
    std::printf("bridge warp host checks passed\n");
    return 0;
}
