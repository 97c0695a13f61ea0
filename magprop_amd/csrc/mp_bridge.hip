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

}  // namespace mp
