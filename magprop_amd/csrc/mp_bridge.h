// mp_bridge.h — the bridge-sampling evidence estimate (include/magprop_amd.h mp_bridge_logz, mp_bridge_logz_warp): what
// mp_bridge.cpp passes to the kernels of mp_bridge.hip, and the host-only rules of the call (the Cholesky factor of the proposal,
// the constants formed from it and those of the Student-t proposal), which the kernels take as arguments.  The header states
// every operation; this file names where each one lives.
#pragma once
#include <cmath>

#include "mp_device.h"

namespace mp {

constexpr uint32_t kBridgeCtr = 0x42524700u;                                   // fourth counter word of every normal draw
constexpr uint32_t kBridgeCtrChi = 0x42524701u;                                // ... and of the normals behind a t draw's chi-square
constexpr int kBridgeMaxMoments = MP_MAX_NDIM + MP_MAX_NDIM * (MP_MAX_NDIM + 1) / 2;   // sums of ndim 9: 9 + 45

// the sums of one call over ndim coordinates: [ndim] of (x - pivot), then [ndim (ndim + 1) / 2] of their products, entry
// (a, b <= a) at ndim + a (a + 1) / 2 + b (NormalArgs' packed layout)
MP_HD inline int bridge_n_moments(int ndim) { return ndim + ndim * (ndim + 1) / 2; }

// The Gaussian proposal N(m, L L^T) as the kernels take it, and c = sum ln L_dd + (ndim / 2) ln 2 pi.
struct BridgeGauss {
    double m[MP_MAX_NDIM];
    double L[MP_MAX_NDIM * (MP_MAX_NDIM + 1) / 2];   // lower triangle by rows, entry (a, b <= a) at a (a + 1) / 2 + b
    double c;
    int32_t ndim, pad;
};

struct BridgeBox {
    double lower[MP_MAX_NDIM], upper[MP_MAX_NDIM];
    int32_t on, pad;                                 // 0: no box (targets 1 and 2), every draw is inside
};

// Host: the proposal from the sums mom[bridge_n_moments(ndim)] of n rows about `pivot`.  With s_a and P_ab the sums:
// m_a = pivot_a + s_a / n, S_ab = P_ab - (s_a s_b) / n, C_ab = S_ab / (n - 1), then the lower Cholesky factor by rows:
// for a = 0 .. ndim - 1, for b = 0 .. a: t = C_ab - sum_{k < b, in order} L_ak L_bk (each product and difference rounded on its
// own); b < a: L_ab = t / L_bb; b = a: L_aa = sqrt(t), which must be finite and > 0.  Returns -1, or the first dimension whose
// pivot fails.  c = (sum_a ln L_aa, in order from 0) + (0.5 ndim) 1.8378770664093453 (ln 2 pi), the host's log.
inline int bridge_factor(const double *mom, const double *pivot, int64_t n, int ndim, BridgeGauss &g) {
#pragma clang fp contract(off)
    const double dn = (double)n, dn1 = (double)(n - 1);
    const double *s = mom, *P = mom + ndim;
    g = BridgeGauss{};
    g.ndim = ndim;
    double sum_ln = 0.0;
    for (int a = 0; a < ndim; ++a) {
        g.m[a] = pivot[a] + s[a] / dn;
        for (int b = 0; b <= a; ++b) {
            const double prod = s[a] * s[b];
            const double S = P[a * (a + 1) / 2 + b] - prod / dn;
            double t = S / dn1;
            for (int k = 0; k < b; ++k) {
                const double lk = g.L[a * (a + 1) / 2 + k] * g.L[b * (b + 1) / 2 + k];
                t = t - lk;
            }
            if (b < a) {
                g.L[a * (a + 1) / 2 + b] = t / g.L[b * (b + 1) / 2 + b];
            } else {
                const double r = std::sqrt(t);
                if (!(std::isfinite(r) && r > 0.0)) return a;
                g.L[a * (a + 1) / 2 + a] = r;
                sum_ln = sum_ln + std::log(r);
            }
        }
    }
    const double half_d = 0.5 * (double)ndim;
    g.c = sum_ln + half_d * 1.8378770664093453;
    return -1;
}

// The Student-t proposal of mp_bridge_logz_warp as the kernels take it beside a BridgeGauss that holds L_t and c_t.
struct BridgeStudent {
    double h, nu;                                    // 0.5 (nu + ndim), nu as a double
    int32_t n_nu, on;                                // nu; 0: the proposal is the Gaussian, nothing else here is read
};

// Host: the constants of the t proposal with nu degrees of freedom and the covariance L L^T of g: k = sqrt((nu - 2) / nu),
// L_t,ab = k L_ab, c_t = ((sum_a ln L_t,aa, in order from 0.0) + (0.5 ndim) ln(nu 3.141592653589793)) + lgamma(nu / 2) -
// lgamma((nu + ndim) / 2), h = 0.5 (nu + ndim); the host's sqrt, log and lgamma.  gt: g with L_t for L and c_t for c.
inline void bridge_student(const BridgeGauss &g, int nu, BridgeGauss &gt, BridgeStudent &t) {
#pragma clang fp contract(off)
    const double dn = (double)nu, dd = (double)g.ndim;
    const double k = std::sqrt((dn - 2.0) / dn);
    gt = g;
    double sum_ln = 0.0;
    for (int a = 0; a < g.ndim; ++a) {
        for (int b = 0; b <= a; ++b) gt.L[a * (a + 1) / 2 + b] = k * g.L[a * (a + 1) / 2 + b];
        sum_ln = sum_ln + std::log(gt.L[a * (a + 1) / 2 + a]);
    }
    const double half_d = 0.5 * dd;
    const double ln_nu_pi = std::log(dn * 3.141592653589793);
    const double with_pi = sum_ln + half_d * ln_nu_pi;
    const double with_lg = with_pi + std::lgamma(dn / 2.0);
    gt.c = with_lg - std::lgamma((dn + dd) / 2.0);
    t.h = 0.5 * (dn + dd);
    t.nu = dn;
    t.n_nu = nu;
    t.on = 1;
}

// What the pair kernel takes: the rows and (warp) their mirrors, and what it reads and writes about them.
struct BridgePairArgs {
    const double *x;         // [n][ndim] the rows
    const double *xm;        // [n][ndim] their mirrors; NULL: no warp, ab = lnp - lnq where the row counts
    double *lnp;             // [n] read where `given`, else written (the test targets 1 .. 4)
    double *lnp_m;           // [n] (warp) the mirrors' lnprob: read for target 0, else written
    const double *lnq;       // [n]
    double *ab;              // [n] the log-ratio
    uint8_t *counted_m;      // [n] (warp) 1 where the mirror counts, else 0
    int64_t n;
    int32_t target, ndim;
    int32_t given;           // 1: lnp holds the rows' lnprob (target 0, and the estimator rows of every target)
    int32_t test_row;        // 1: a row outside the box or with a non-finite lnprob does not count (the draws)
};

// What the fixed-point kernel takes beside its arrays; the logs are the host's.
struct BridgeFixedArgs {
    const double *a;         // [n1] a_i = lnp_est_i - lnq_i, all finite; shared by the repetitions
    const double *b;         // [n_rep][n2] b_j = lnp_j - lnq_j, -inf for a draw that does not count
    double *out;             // [n_rep][MP_BRIDGE_NOUT]
    int64_t n1, n2;
    double ln_s1, ln_s2;     // ln(neff / (neff + n2)), ln(n2 / (neff + n2))
    double ln_n1, ln_n2;     // ln n1, ln n2
    double tau;              // n1 / neff
    double ln_volume;
    double tol;
    int32_t max_iter, n_rep;
};

// Every launcher returns hipError_t as int.
// One workgroup of 256 threads per block of MP_BRIDGE_BLOCK rows of x[n][ndim]: part[first_block + block][n_moments] (the rows
// are those of blocks first_block .. of the call); then one thread per sum over part[n_blocks][...] in block order into out.
int launch_bridge_moments(const double *x, int64_t n, int ndim, const double *pivot, int64_t first_block, double *part, void *stream);
int launch_bridge_combine(const double *part, int64_t n_blocks, int ndim, double *out, void *stream);
// one thread per draw j of repetition r: x[r * n_draws + j][ndim] and lnq[r * n_draws + j]
int launch_bridge_draws(const BridgeGauss &g, uint64_t seed, int64_t n_draws, int n_rep, double *x, double *lnq, void *stream);
// one thread per row: lnq[i] of x[i] and (lnp not NULL) a[i] = lnp[i] - lnq[i]
int launch_bridge_est(const BridgeGauss &g, const double *x, const double *lnp, int64_t n, double *lnq, double *a, void *stream);
// one thread per draw: target 1 or 2 writes lnp[i] with point_eval's arithmetic, target 0 reads it; b[i] = lnp[i] - lnq[i] where
// the draw is inside the box and lnp[i] is finite, else -inf
int launch_bridge_b(const BridgeBox &box, int target, int ndim, const double *x, double *lnp, const double *lnq, int64_t n, double *b,
                    void *stream);
int launch_bridge_fixed(const BridgeFixedArgs &f, void *stream);
// mp_bridge_logz_warp's.  One thread per draw: x, lnq and (xm not NULL) the mirror rows xm[r * n_draws + j][ndim], from the Gaussian
// g (t.on = 0) or the t proposal (g holds L_t and c_t)
int launch_bridge_draws_warp(const BridgeGauss &g, const BridgeStudent &t, uint64_t seed, int64_t n_draws, int n_rep, double *x, double *xm,
                             double *lnq, void *stream);
// one thread per estimator row: lnq[i] of x[i] under either proposal and (xm not NULL) the mirror row xm[i][ndim]
int launch_bridge_est_warp(const BridgeGauss &g, const BridgeStudent &t, const double *x, int64_t n, double *lnq, double *xm, void *stream);
// one thread per row: the test targets' lnp of the row and of its mirror, the box, and ab (a of estimator rows, b of draws)
int launch_bridge_pair(const BridgeBox &box, const BridgePairArgs &p, void *stream);
// one workgroup per repetition r: out[r] = the non-zero flags among flag[r * n .. r * n + n), as a double
int launch_bridge_count(const uint8_t *flag, int64_t n, int n_rep, double *out, void *stream);

}  // namespace mp
