// bridge_host_stubs.h — what the host check programs of the bridge-sampling evidence (bridge_host_check.cpp,
// bridge_warp_host_check.cpp) share: mp_bridge.cpp itself, compiled for the host, the `fail` and `check_box` that mp_capi.cpp
// defines in the library, stand-ins for the launchers and the batch entry, none of which the programs reach (no HIP call is made),
// and the bookkeeping of the checks.
#pragma once
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "../magprop_amd/csrc/mp_bridge.cpp"

static std::string g_msg;

int fail(int code, const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_msg = buf;
    return code;
}

int check_box(const char *fn, int ndim, const double *lower, const double *upper) {   // mp_capi.cpp's
    for (int d = 0; d < ndim; ++d)
        if (!(std::isfinite(lower[d]) && std::isfinite(upper[d]) && lower[d] < upper[d]))
            return fail(MP_EINVAL, "%s: bounds of coordinate %d are empty or not finite", fn, d);
    return MP_OK;
}

static int unreachable() { std::abort(); }
int upload_ds_rows(int32_t *, const int32_t *, int, int) { return unreachable(); }
extern "C" int mp_lnprob_batch_dev(mp_handle *, const double *, const int32_t *, int, int, double *, int32_t *, double *, void *) { return unreachable(); }
namespace mp {
int launch_bridge_moments(const double *, int64_t, int, const double *, int64_t, double *, void *) { return unreachable(); }
int launch_bridge_combine(const double *, int64_t, int, double *, void *) { return unreachable(); }
int launch_bridge_draws(const BridgeGauss &, uint64_t, int64_t, int, double *, double *, void *) { return unreachable(); }
int launch_bridge_est(const BridgeGauss &, const double *, const double *, int64_t, double *, double *, void *) { return unreachable(); }
int launch_bridge_b(const BridgeBox &, int, int, const double *, double *, const double *, int64_t, double *, void *) { return unreachable(); }
int launch_bridge_fixed(const BridgeFixedArgs &, void *) { return unreachable(); }
int launch_bridge_draws_warp(const BridgeGauss &, const BridgeStudent &, uint64_t, int64_t, int, double *, double *, double *, void *) { return unreachable(); }
int launch_bridge_est_warp(const BridgeGauss &, const BridgeStudent &, const double *, int64_t, double *, double *, void *) { return unreachable(); }
int launch_bridge_pair(const BridgeBox &, const BridgePairArgs &, void *) { return unreachable(); }
int launch_bridge_count(const uint8_t *, int64_t, int, double *, void *) { return unreachable(); }
}  // namespace mp

static int n_failed = 0;

static void expect(bool ok, const char *what) {
    if (!ok) { std::printf("FAILED: %s (last message: %s)\n", what, g_msg.c_str()); ++n_failed; }
}

// rows x[n][ndim] of a fixed linear generator, mixed so that the covariance is full; their sums about row 0 in plain order
static std::vector<double> rows_of(int n, int ndim, int constant_column) {
    std::vector<double> x((size_t)n * ndim);
    uint64_t s = 12345;
    for (int i = 0; i < n; ++i)
        for (int d = 0; d < ndim; ++d) {
            s = s * 6364136223846793005ull + 1442695040888963407ull;
            const double u = (double)(s >> 11) / 9007199254740992.0 - 0.5;
            x[(size_t)i * ndim + d] = d == constant_column ? 0.5 : (d + 1) * u + (d ? 0.3 * x[(size_t)i * ndim + d - 1] : 0.0) + 7.0 * d;
        }
    return x;
}

static std::vector<double> sums_of(const std::vector<double> &x, int n, int ndim) {
    std::vector<double> mom((size_t)mp::bridge_n_moments(ndim), 0.0);
    for (int i = 0; i < n; ++i)
        for (int a = 0; a < ndim; ++a) {
            const double da = x[(size_t)i * ndim + a] - x[a];
            mom[a] += da;
            for (int b = 0; b <= a; ++b) mom[ndim + a * (a + 1) / 2 + b] += da * (x[(size_t)i * ndim + b] - x[b]);
        }
    return mom;
}
