// mp_bridge.hip — gfx950 kernels of the bridge-sampling evidence estimate (include/magprop_amd.h mp_bridge_logz states every
// operation; mp_bridge.h the arguments).
//
// bridge_moments_kernel: one workgroup of 256 threads per block of MP_BRIDGE_BLOCK rows: the sums of (x - pivot) and of their
// pairwise products, thread k over rows k, k + 256, ... of the block, then wg_sum; bridge_combine_kernel adds the blocks' partial
// sums in block order, one thread per sum.  The blocks are cut from the rows alone, so the sums do not depend on the launch.
// bridge_draws_kernel: one thread per draw: the normals of its Philox counters, x = m + L z and lnq.
// bridge_est_kernel: one thread per estimator row: forward substitution, lnq and a = lnp - lnq.
// bridge_b_kernel: one thread per draw: the test targets' lnp, the box, and b = lnp - lnq or -inf.
// bridge_fixed_kernel: one workgroup of 256 threads per repetition: the fixed point over a and b, which it only reads (they are
// formed once, by the two kernels above), and the moments of f1 and f2 behind it.
// mp_bridge_logz_warp's: bridge_draws_warp_kernel: one thread per draw from the Gaussian or the Student-t proposal (the chi-square
// loop over Philox pairs has a uniform trip count), with the mirror row beside it; bridge_est_warp_kernel: one thread per
// estimator row: lnq under either proposal and the mirror row; bridge_pair_kernel: one thread per row: the test targets' lnp of
// the row and of its mirror, the box on both, and a or b; bridge_count_kernel: one workgroup per repetition counts the mirrors
// that counted.  mp_bridge_logz keeps the three kernels above; the fixed-point kernel serves both entries as it is.
// Every read of a row-major array by consecutive threads is of consecutive elements (a, b, lnp, lnq) or of consecutive rows of
// ndim doubles; every per-thread array is indexed by unrolled constants, so nothing goes to scratch memory.
#include <hip/hip_runtime.h>

#include "mp_bridge.h"
#include "mp_normal_pair.h"
#include "mp_wg.h"

namespace mp {

namespace {

constexpr int kTri = MP_MAX_NDIM * (MP_MAX_NDIM + 1) / 2;

struct BridgePivot {
    double v[MP_MAX_NDIM];
};

__global__ __launch_bounds__(kWgThreads) void bridge_moments_kernel(const double *x, int64_t n, int ndim, const BridgePivot pv,
                                                                    int64_t first_block, double *part) {
    __shared__ double sh[kWgWaves];
    const int64_t lo = (int64_t)blockIdx.x * MP_BRIDGE_BLOCK;
    const int64_t hi = lo + MP_BRIDGE_BLOCK < n ? lo + MP_BRIDGE_BLOCK : n;
    double s[MP_MAX_NDIM], p[kTri];
#pragma unroll
    for (int a = 0; a < MP_MAX_NDIM; ++a) s[a] = 0.0;
#pragma unroll
    for (int a = 0; a < kTri; ++a) p[a] = 0.0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += kWgThreads) {
        const double *row = x + i * ndim;
        double d[MP_MAX_NDIM];
#pragma unroll
        for (int a = 0; a < MP_MAX_NDIM; ++a) d[a] = a < ndim ? sub_rn(row[a], pv.v[a]) : 0.0;
#pragma unroll
        for (int a = 0; a < MP_MAX_NDIM; ++a) {
            if (a < ndim) {
                s[a] = add_rn(s[a], d[a]);
#pragma unroll
                for (int b = 0; b <= a; ++b) p[a * (a + 1) / 2 + b] = add_rn(p[a * (a + 1) / 2 + b], mul_rn(d[a], d[b]));
            }
        }
    }
    double *out = part + (first_block + blockIdx.x) * bridge_n_moments(ndim);
#pragma unroll
    for (int a = 0; a < MP_MAX_NDIM; ++a) {
        if (a < ndim) {                                              // (uniform: a launch argument)
            const double v = wg_sum(s[a], sh);
            if (threadIdx.x == 0) out[a] = v;
        }
    }
#pragma unroll
    for (int a = 0; a < MP_MAX_NDIM; ++a) {
#pragma unroll
        for (int b = 0; b <= a; ++b) {
            if (a < ndim) {
                const double v = wg_sum(p[a * (a + 1) / 2 + b], sh);
                if (threadIdx.x == 0) out[ndim + a * (a + 1) / 2 + b] = v;
            }
        }
    }
}

__global__ __launch_bounds__(64) void bridge_combine_kernel(const double *part, int64_t n_blocks, int nm, double *out) {
    const int m = (int)threadIdx.x;
    if (m >= nm) return;
    double v = part[m];
    for (int64_t k = 1; k < n_blocks; ++k) v = add_rn(v, part[k * nm + m]);
    out[m] = v;
}

// lnq = -0.5 sum z^2 - c, the squares added in order from dimension 0
MP_DEV double bridge_lnq(const double (&z)[MP_MAX_NDIM + 1], int ndim, double c) {
    double q = 0.0;
#pragma unroll
    for (int a = 0; a < MP_MAX_NDIM; ++a) q = a < ndim ? add_rn(q, mul_rn(z[a], z[a])) : q;
    return sub_rn(mul_rn(-0.5, q), c);
}

__global__ __launch_bounds__(kWgThreads) void bridge_draws_kernel(const BridgeGauss g, uint64_t seed, int64_t n_draws, int n_rep,
                                                                  double *x, double *lnq) {
    const int64_t i = (int64_t)blockIdx.x * kWgThreads + threadIdx.x;
    if (i >= n_draws * n_rep) return;
    const int nd = g.ndim;
    const uint32_t r = (uint32_t)(i / n_draws), j = (uint32_t)(i % n_draws);
    double z[MP_MAX_NDIM + 1];
#pragma unroll
    for (int p = 0; p < (MP_MAX_NDIM + 1) / 2; ++p) {
        z[2 * p] = z[2 * p + 1] = 0.0;
        if (2 * p < nd) {
            uint32_t s4[4];
            philox4x32_10((uint32_t)seed, (uint32_t)(seed >> 32), j, r, (uint32_t)p, kBridgeCtr, s4);
            normal_pair(s4, z[2 * p], z[2 * p + 1]);
        }
    }
    double *row = x + i * nd;
#pragma unroll
    for (int a = 0; a < MP_MAX_NDIM; ++a) {
        if (a < nd) {
            double s = 0.0;
#pragma unroll
            for (int b = 0; b <= a; ++b) s = add_rn(s, mul_rn(g.L[a * (a + 1) / 2 + b], z[b]));
            row[a] = add_rn(g.m[a], s);
        }
    }
    lnq[i] = bridge_lnq(z, nd, g.c);
}

__global__ __launch_bounds__(kWgThreads) void bridge_est_kernel(const BridgeGauss g, const double *x, const double *lnp, int64_t n,
                                                                double *lnq, double *a_out) {
    const int64_t i = (int64_t)blockIdx.x * kWgThreads + threadIdx.x;
    if (i >= n) return;
    const int nd = g.ndim;
    const double *row = x + i * nd;
    double z[MP_MAX_NDIM + 1];
#pragma unroll
    for (int a = 0; a < MP_MAX_NDIM + 1; ++a) z[a] = 0.0;
#pragma unroll
    for (int a = 0; a < MP_MAX_NDIM; ++a) {
        if (a < nd) {
            double t = sub_rn(row[a], g.m[a]);
#pragma unroll
            for (int b = 0; b < a; ++b) t = sub_rn(t, mul_rn(g.L[a * (a + 1) / 2 + b], z[b]));
            z[a] = t / g.L[a * (a + 1) / 2 + a];
        }
    }
    const double q = bridge_lnq(z, nd, g.c);
    lnq[i] = q;
    if (lnp) a_out[i] = sub_rn(lnp[i], q);
}

// The test targets of mp_bridge_logz_warp at a point.  1 and 2: point_eval's arithmetic, as bridge_b_kernel below forms it (that
// kernel, mp_bridge_logz's, stays as compiled); 3 (the split normal) and 4 (the product of t_3 densities) live here alone.
MP_DEV double bridge_test_lnp(int target, const double (&par)[MP_MAX_NDIM], int ndim) {
    double v = 0.0;
    if (target == 3) {
#pragma unroll
        for (int d = 0; d < MP_MAX_NDIM; ++d) {
            const double u = par[d] < 0.0 ? par[d] : mul_rn(0.25, par[d]);
            v = d < ndim ? sub_rn(v, mul_rn(mul_rn(0.5, u), u)) : v;
        }
        return v;
    }
    if (target == 4) {
#pragma unroll
        for (int d = 0; d < MP_MAX_NDIM; ++d)
            v = d < ndim ? sub_rn(v, mul_rn(2.0, log(add_rn(1.0, mul_rn(par[d], par[d]) / 3.0)))) : v;
        return v;
    }
#pragma unroll
    for (int d = 0; d < MP_MAX_NDIM; ++d) v = d < ndim ? sub_rn(v, mul_rn(mul_rn(0.5, par[d]), par[d])) : v;
    if (target == 2) v = sub_rn(v, mul_rn(1.0e-3, floor(mul_rn(37.0, par[0]))));
    return v;
}

MP_DEV bool bridge_inside(const BridgeBox &box, const double (&par)[MP_MAX_NDIM], int ndim) {
    bool inside = true;
    if (box.on) {
#pragma unroll
        for (int d = 0; d < MP_MAX_NDIM; ++d)
            if (d < ndim) inside = inside && par[d] >= box.lower[d] && par[d] <= box.upper[d];
    }
    return inside;
}

__global__ __launch_bounds__(kWgThreads) void bridge_b_kernel(const BridgeBox box, int target, int ndim, const double *x, double *lnp,
                                                              const double *lnq, int64_t n, double *b) {
    const int64_t i = (int64_t)blockIdx.x * kWgThreads + threadIdx.x;
    if (i >= n) return;
    const double *row = x + i * ndim;
    double par[MP_MAX_NDIM];
#pragma unroll
    for (int d = 0; d < MP_MAX_NDIM; ++d) par[d] = d < ndim ? row[d] : 0.0;
    double v;
    if (target != 0) {   // point_eval's test targets
        v = 0.0;
#pragma unroll
        for (int d = 0; d < MP_MAX_NDIM; ++d) v = d < ndim ? sub_rn(v, mul_rn(mul_rn(0.5, par[d]), par[d])) : v;
        if (target == 2) v = sub_rn(v, mul_rn(1.0e-3, floor(mul_rn(37.0, par[0]))));
        lnp[i] = v;
    } else {
        v = lnp[i];
    }
    bool inside = true;
    if (box.on) {
#pragma unroll
        for (int d = 0; d < MP_MAX_NDIM; ++d)
            if (d < ndim) inside = inside && par[d] >= box.lower[d] && par[d] <= box.upper[d];
    }
    b[i] = inside && isfinite(v) ? sub_rn(v, lnq[i]) : -INFINITY;
}

// lse2(u, v) = max + log(1 + exp(min - max))
MP_DEV double lse2(double u, double v) {
    const double mx = fmax(u, v), mn = fmin(u, v);
    return add_rn(mx, log(add_rn(1.0, exp(sub_rn(mn, mx)))));
}

MP_DEV double bridge_f1(double a, double lam, const BridgeFixedArgs &f) {
    return exp(-lse2(sub_rn(add_rn(f.ln_s1, a), lam), f.ln_s2));
}
MP_DEV double bridge_f2(double b, double lam, const BridgeFixedArgs &f) {
    return exp(sub_rn(sub_rn(b, lam), lse2(sub_rn(add_rn(f.ln_s1, b), lam), f.ln_s2)));
}

__global__ __launch_bounds__(kWgThreads) void bridge_fixed_kernel(const BridgeFixedArgs f) {
    __shared__ double shm[kWgWaves], shs[kWgWaves];
    __shared__ uint32_t shc[kWgWaves];
    const int t = (int)threadIdx.x;
    const double *a = f.a, *b = f.b + (int64_t)blockIdx.x * f.n2;
    double *out = f.out + (int64_t)blockIdx.x * MP_BRIDGE_NOUT;
    // the importance-sampling estimate and the draws that count
    uint32_t cnt = 0;
    double m = -INFINITY, s = 0.0;
    for (int64_t j = t; j < f.n2; j += kWgThreads) {
        const double v = b[j];
        cnt += v > -INFINITY ? 1u : 0u;
        lse_add(m, s, v);
    }
    const uint32_t n_finite = wg_count(cnt, shc);
    wg_lse(m, s, shm, shs);
    const double lam0 = sub_rn(add_rn(m, log(s)), f.ln_n2);
    if (n_finite == 0) {   // (uniform)
        if (t == 0) {
            const double nan = __builtin_nan("");
            out[0] = nan; out[1] = nan; out[2] = f.ln_volume; out[3] = nan; out[4] = 0.0; out[5] = (double)MP_BRIDGE_NO_OVERLAP;
            out[6] = 0.0; out[7] = -INFINITY; out[8] = nan; out[9] = nan; out[10] = nan; out[11] = nan;
        }
        return;
    }
    double lam = lam0;
    int niter = 0, status = MP_BRIDGE_ITER_LIMIT;
    while (niter < f.max_iter) {
        const double c2 = add_rn(f.ln_s2, lam);
        double m2 = -INFINITY, s2 = 0.0;
        for (int64_t j = t; j < f.n2; j += kWgThreads) {
            const double v = b[j];
            lse_add(m2, s2, sub_rn(v, lse2(add_rn(f.ln_s1, v), c2)));
        }
        wg_lse(m2, s2, shm, shs);
        double m1 = -INFINITY, s1 = 0.0;
        for (int64_t i = t; i < f.n1; i += kWgThreads) lse_add(m1, s1, -lse2(add_rn(f.ln_s1, a[i]), c2));
        wg_lse(m1, s1, shm, shs);
        const double next = sub_rn(sub_rn(add_rn(m2, log(s2)), f.ln_n2), sub_rn(add_rn(m1, log(s1)), f.ln_n1));
        const double step = fabs(sub_rn(next, lam));
        lam = next;
        ++niter;
        if (step <= f.tol) {   // (uniform: every thread holds the same pair)
            status = MP_BRIDGE_OK;
            break;
        }
    }
    // the moments of f1 and f2 at the result, two passes each
    double acc = 0.0;
    for (int64_t i = t; i < f.n1; i += kWgThreads) acc = add_rn(acc, bridge_f1(a[i], lam, f));
    const double mean1 = wg_sum(acc, shm) / (double)f.n1;
    acc = 0.0;
    for (int64_t i = t; i < f.n1; i += kWgThreads) {
        const double d = sub_rn(bridge_f1(a[i], lam, f), mean1);
        acc = add_rn(acc, mul_rn(d, d));
    }
    const double var1 = wg_sum(acc, shm) / (double)f.n1;
    acc = 0.0;
    for (int64_t j = t; j < f.n2; j += kWgThreads) acc = add_rn(acc, bridge_f2(b[j], lam, f));
    const double mean2 = wg_sum(acc, shm) / (double)f.n2;
    acc = 0.0;
    for (int64_t j = t; j < f.n2; j += kWgThreads) {
        const double d = sub_rn(bridge_f2(b[j], lam, f), mean2);
        acc = add_rn(acc, mul_rn(d, d));
    }
    const double var2 = wg_sum(acc, shm) / (double)f.n2;
    if (t == 0) {
        const double t2 = var2 / mul_rn((double)f.n2, mul_rn(mean2, mean2));
        const double t1 = mul_rn(f.tau, var1 / mul_rn((double)f.n1, mul_rn(mean1, mean1)));
        out[0] = sub_rn(lam, f.ln_volume);
        out[1] = lam;
        out[2] = f.ln_volume;
        out[3] = sqrt(add_rn(t2, t1));
        out[4] = (double)niter;
        out[5] = (double)status;
        out[6] = (double)n_finite;
        out[7] = lam0;
        out[8] = mean1;
        out[9] = var1;
        out[10] = mean2;
        out[11] = var2;
    }
}

// ---------------------------------------------------------------- mp_bridge_logz_warp: both proposals, mirror rows, pairs
// the t density of the scaled residuals xi: lnq = -h log(1 + Q / nu) - c_t, Q = sum xi^2 added in order from dimension 0
MP_DEV double bridge_lnq_t(const double (&xi)[MP_MAX_NDIM + 1], int ndim, const BridgeStudent &t, double c) {
    double q = 0.0;
#pragma unroll
    for (int a = 0; a < MP_MAX_NDIM; ++a) q = a < ndim ? add_rn(q, mul_rn(xi[a], xi[a])) : q;
    return sub_rn(mul_rn(-t.h, log(add_rn(1.0, q / t.nu))), c);
}

__global__ __launch_bounds__(kWgThreads) void bridge_draws_warp_kernel(const BridgeGauss g, const BridgeStudent t, uint64_t seed,
                                                                       int64_t n_draws, int n_rep, double *x, double *xm, double *lnq) {
    const int64_t i = (int64_t)blockIdx.x * kWgThreads + threadIdx.x;
    if (i >= n_draws * n_rep) return;
    const int nd = g.ndim;
    const uint32_t r = (uint32_t)(i / n_draws), j = (uint32_t)(i % n_draws);
    double z[MP_MAX_NDIM + 1];
#pragma unroll
    for (int p = 0; p < (MP_MAX_NDIM + 1) / 2; ++p) {
        z[2 * p] = z[2 * p + 1] = 0.0;
        if (2 * p < nd) {
            uint32_t s4[4];
            philox4x32_10((uint32_t)seed, (uint32_t)(seed >> 32), j, r, (uint32_t)p, kBridgeCtr, s4);
            normal_pair(s4, z[2 * p], z[2 * p + 1]);
        }
    }
    double scale = 1.0;
    if (t.on) {                                                      // (uniform: launch arguments, the trip count too)
        double w = 0.0;
        const int pairs = (t.n_nu + 1) / 2;
        for (int p = 0; p < pairs; ++p) {
            uint32_t s4[4];
            double g0, g1;
            philox4x32_10((uint32_t)seed, (uint32_t)(seed >> 32), j, r, (uint32_t)p, kBridgeCtrChi, s4);
            normal_pair(s4, g0, g1);
            w = add_rn(w, mul_rn(g0, g0));
            if (2 * p + 1 < t.n_nu) w = add_rn(w, mul_rn(g1, g1));   // an odd nu leaves the last pair's second normal
        }
        scale = sqrt(t.nu / w);
    }
    double *row = x + i * nd;
    double *rowm = xm ? xm + i * nd : nullptr;
#pragma unroll
    for (int a = 0; a < MP_MAX_NDIM; ++a) {
        if (a < nd) {
            double s = 0.0;
#pragma unroll
            for (int b = 0; b <= a; ++b) s = add_rn(s, mul_rn(g.L[a * (a + 1) / 2 + b], z[b]));
            const double d = t.on ? mul_rn(scale, s) : s;
            row[a] = add_rn(g.m[a], d);
            if (rowm) rowm[a] = sub_rn(g.m[a], d);
        }
    }
    if (t.on) {
#pragma unroll
        for (int a = 0; a < MP_MAX_NDIM + 1; ++a) z[a] = mul_rn(scale, z[a]);
        lnq[i] = bridge_lnq_t(z, nd, t, g.c);
    } else {
        lnq[i] = bridge_lnq(z, nd, g.c);
    }
}

__global__ __launch_bounds__(kWgThreads) void bridge_est_warp_kernel(const BridgeGauss g, const BridgeStudent t, const double *x,
                                                                     int64_t n, double *lnq, double *xm) {
    const int64_t i = (int64_t)blockIdx.x * kWgThreads + threadIdx.x;
    if (i >= n) return;
    const int nd = g.ndim;
    const double *row = x + i * nd;
    double *rowm = xm ? xm + i * nd : nullptr;
    double z[MP_MAX_NDIM + 1];
#pragma unroll
    for (int a = 0; a < MP_MAX_NDIM + 1; ++a) z[a] = 0.0;
#pragma unroll
    for (int a = 0; a < MP_MAX_NDIM; ++a) {
        if (a < nd) {
            const double d = sub_rn(row[a], g.m[a]);
            if (rowm) rowm[a] = sub_rn(g.m[a], d);
            double s = d;
#pragma unroll
            for (int b = 0; b < a; ++b) s = sub_rn(s, mul_rn(g.L[a * (a + 1) / 2 + b], z[b]));
            z[a] = s / g.L[a * (a + 1) / 2 + a];
        }
    }
    lnq[i] = t.on ? bridge_lnq_t(z, nd, t, g.c) : bridge_lnq(z, nd, g.c);
}

__global__ __launch_bounds__(kWgThreads) void bridge_pair_kernel(const BridgeBox box, const BridgePairArgs p) {
    const int64_t i = (int64_t)blockIdx.x * kWgThreads + threadIdx.x;
    if (i >= p.n) return;
    const int nd = p.ndim;
    const double *row = p.x + i * nd;
    double par[MP_MAX_NDIM];
#pragma unroll
    for (int d = 0; d < MP_MAX_NDIM; ++d) par[d] = d < nd ? row[d] : 0.0;
    double v;
    if (p.given) {
        v = p.lnp[i];
    } else {
        v = bridge_test_lnp(p.target, par, nd);
        p.lnp[i] = v;
    }
    const bool ok = isfinite(v) && (!p.test_row || bridge_inside(box, par, nd));
    const double q = p.lnq[i];
    if (!p.xm) {                                                     // (uniform)
        p.ab[i] = ok ? sub_rn(v, q) : -INFINITY;
        return;
    }
    const double *rowm = p.xm + i * nd;
#pragma unroll
    for (int d = 0; d < MP_MAX_NDIM; ++d) par[d] = d < nd ? rowm[d] : 0.0;
    double vm;
    if (p.target == 0) {
        vm = p.lnp_m[i];
    } else {
        vm = bridge_test_lnp(p.target, par, nd);
        p.lnp_m[i] = vm;
    }
    const bool okm = isfinite(vm) && bridge_inside(box, par, nd);
    p.counted_m[i] = okm ? 1 : 0;
    // the symmetrised density in logs; a point that does not count contributes nothing, and lse2 is formed of two finite values only
    double both = -INFINITY;
    if (ok && okm) both = lse2(v, vm);
    else if (ok) both = v;
    else if (okm) both = vm;
    p.ab[i] = ok || okm ? sub_rn(sub_rn(both, 0.6931471805599453), q) : -INFINITY;
}

__global__ __launch_bounds__(kWgThreads) void bridge_count_kernel(const uint8_t *flag, int64_t n, double *out) {
    __shared__ uint32_t shc[kWgWaves];
    const uint8_t *f = flag + (int64_t)blockIdx.x * n;
    uint32_t cnt = 0;
    for (int64_t j = threadIdx.x; j < n; j += kWgThreads) cnt += f[j] ? 1u : 0u;
    const uint32_t total = wg_count(cnt, shc);
    if (threadIdx.x == 0) out[blockIdx.x] = (double)total;
}

unsigned grid_of(int64_t n) { return (unsigned)((n + kWgThreads - 1) / kWgThreads); }

}  // namespace

int launch_bridge_moments(const double *x, int64_t n, int ndim, const double *pivot, int64_t first_block, double *part, void *stream) {
    if (n <= 0) return 0;
    BridgePivot pv{};
    for (int a = 0; a < ndim; ++a) pv.v[a] = pivot[a];
    const unsigned blocks = (unsigned)((n + MP_BRIDGE_BLOCK - 1) / MP_BRIDGE_BLOCK);
    hipLaunchKernelGGL(bridge_moments_kernel, dim3(blocks), dim3(kWgThreads), 0, (hipStream_t)stream, x, n, ndim, pv, first_block, part);
    return (int)hipGetLastError();
}

int launch_bridge_combine(const double *part, int64_t n_blocks, int ndim, double *out, void *stream) {
    hipLaunchKernelGGL(bridge_combine_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, part, n_blocks, bridge_n_moments(ndim), out);
    return (int)hipGetLastError();
}

int launch_bridge_draws(const BridgeGauss &g, uint64_t seed, int64_t n_draws, int n_rep, double *x, double *lnq, void *stream) {
    hipLaunchKernelGGL(bridge_draws_kernel, dim3(grid_of(n_draws * n_rep)), dim3(kWgThreads), 0, (hipStream_t)stream, g, seed, n_draws,
                       n_rep, x, lnq);
    return (int)hipGetLastError();
}

int launch_bridge_est(const BridgeGauss &g, const double *x, const double *lnp, int64_t n, double *lnq, double *a, void *stream) {
    hipLaunchKernelGGL(bridge_est_kernel, dim3(grid_of(n)), dim3(kWgThreads), 0, (hipStream_t)stream, g, x, lnp, n, lnq, a);
    return (int)hipGetLastError();
}

int launch_bridge_b(const BridgeBox &box, int target, int ndim, const double *x, double *lnp, const double *lnq, int64_t n, double *b,
                    void *stream) {
    hipLaunchKernelGGL(bridge_b_kernel, dim3(grid_of(n)), dim3(kWgThreads), 0, (hipStream_t)stream, box, target, ndim, x, lnp, lnq, n, b);
    return (int)hipGetLastError();
}

int launch_bridge_fixed(const BridgeFixedArgs &f, void *stream) {
    hipLaunchKernelGGL(bridge_fixed_kernel, dim3((unsigned)f.n_rep), dim3(kWgThreads), 0, (hipStream_t)stream, f);
    return (int)hipGetLastError();
}

int launch_bridge_draws_warp(const BridgeGauss &g, const BridgeStudent &t, uint64_t seed, int64_t n_draws, int n_rep, double *x, double *xm,
                             double *lnq, void *stream) {
    hipLaunchKernelGGL(bridge_draws_warp_kernel, dim3(grid_of(n_draws * n_rep)), dim3(kWgThreads), 0, (hipStream_t)stream, g, t, seed,
                       n_draws, n_rep, x, xm, lnq);
    return (int)hipGetLastError();
}

int launch_bridge_est_warp(const BridgeGauss &g, const BridgeStudent &t, const double *x, int64_t n, double *lnq, double *xm, void *stream) {
    hipLaunchKernelGGL(bridge_est_warp_kernel, dim3(grid_of(n)), dim3(kWgThreads), 0, (hipStream_t)stream, g, t, x, n, lnq, xm);
    return (int)hipGetLastError();
}

int launch_bridge_pair(const BridgeBox &box, const BridgePairArgs &p, void *stream) {
    hipLaunchKernelGGL(bridge_pair_kernel, dim3(grid_of(p.n)), dim3(kWgThreads), 0, (hipStream_t)stream, box, p);
    return (int)hipGetLastError();
}

int launch_bridge_count(const uint8_t *flag, int64_t n, int n_rep, double *out, void *stream) {
    hipLaunchKernelGGL(bridge_count_kernel, dim3((unsigned)n_rep), dim3(kWgThreads), 0, (hipStream_t)stream, flag, n, out);
    return (int)hipGetLastError();
}

}  // namespace mp
