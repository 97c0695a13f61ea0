// mp_acf.hip — gfx950 kernels of the sampler's autocorrelation monitor (mp_sampler_set_autocorr; include/magprop_amd.h states
// the definition, mp_acf.h the layout).
//
// Per chunk of mp_sampler_run: acf_ingest_kernel (one lane per series, one strided pass over the chunk's chain rows: y = x - pivot
// into the history ring, T, the head sums H) and acf_accumulate_kernel (one lane per series, kAcfLagBlock lags per workgroup:
// accumulators and the window y_{t-k0} .. y_{t-k0-15} in registers, the window kept by unrolling over the block so that every
// index is a compile-time constant; sequential in t per accumulator, no atomics, no LDS).
// On request: acf_rho_kernel (same shape: the tail sums L_k from the ring, then c_k and rho_k of every series) and
// acf_final_kernel (one workgroup per (ensemble, dimension): the walker mean in walker order parallel over lags, then the running
// sum and the first-index window test in lag order by one lane: at most MP_ACF_MAX_LAG dependent additions, which reproduce
// numpy's cumsum bit for bit).
// Every product and sum is rounded on its own (mp_math.hpp mul_rn / add_rn / sub_rn).
#include <hip/hip_runtime.h>

#include "mp_acf.h"
#include "mp_math.hpp"

namespace mp {

namespace {

constexpr int LB = kAcfLagBlock;

// ring row at offset off from row head, -ring < head + off < 2 ring
MP_DEV int ring_row(int head, int off, int ring) {
    int r = head + off;
    r += r < 0 ? ring : 0;
    r -= r >= ring ? ring : 0;
    return r;
}

__global__ __launch_bounds__(kAcfThreads) void acf_ingest_kernel(AcfArgs a) {
    const int j = blockIdx.x * kAcfThreads + threadIdx.x;
    if (j >= a.n_series) return;
    const size_t ns = (size_t)a.n_series;
    const double *__restrict__ src = a.chain + (size_t)a.first * ns + j;
    double *__restrict__ hist = a.hist + j;
    double *__restrict__ H = a.H + j;
    const double p = a.n0 ? a.pivot[j] : src[0];
    double t = a.n0 ? a.T[j] : 0.0;
    if (!a.n0) a.pivot[j] = p;
    int row = a.head;
#pragma unroll 8
    for (int r = 0; r < a.rows; ++r) {
        const double y = sub_rn(src[(size_t)r * ns], p);
        hist[(size_t)row * ns] = y;
        t = add_rn(t, y);
        const int64_t k = a.n0 + r + 1;          // t is now the sum of samples 0 .. k - 1 = H_k
        if (k < a.kp) H[(size_t)k * ns] = t;
        row = row + 1 == a.ring_rows ? 0 : row + 1;
    }
    a.T[j] = t;
}

// kAcfLagBlock samples tb .. tb + 15 of the chunk into the 16 accumulators of lags k0 .. k0 + 15.  Slot u of the window takes
// y_{t-k0} of sample t = tb + u; lag k0 + i then reads slot (u - i) mod 16, which holds y_{t-k0-i}.
template <bool kGuard>
MP_DEV void acf_group(const AcfArgs &a, const double *__restrict__ hist, size_t ns, int k0, int tb, double (&acc)[LB], double (&w)[LB]) {
#pragma unroll
    for (int u = 0; u < LB; ++u) {
        if (!kGuard || tb + u < a.rows) {
            const double y = hist[(size_t)ring_row(a.head, tb + u, a.ring_rows) * ns];
            w[u] = hist[(size_t)ring_row(a.head, tb + u - k0, a.ring_rows) * ns];
#pragma unroll
            for (int i = 0; i < LB; ++i) acc[i] = add_rn(acc[i], mul_rn(y, w[(u - i + LB) % LB]));
        }
    }
}

__global__ __launch_bounds__(kAcfThreads) void acf_accumulate_kernel(AcfArgs a) {
    const int j = blockIdx.x * kAcfThreads + threadIdx.x;
    if (j >= a.n_series) return;
    const size_t ns = (size_t)a.n_series;
    const int k0 = blockIdx.y * LB;
    const double *__restrict__ hist = a.hist + j;
    double *__restrict__ S = a.S + (size_t)k0 * ns + j;
    double acc[LB], w[LB];
#pragma unroll
    for (int i = 0; i < LB; ++i) acc[i] = S[(size_t)i * ns];
    w[0] = 0.0;
#pragma unroll
    for (int s = 1; s < LB; ++s) w[s] = hist[(size_t)ring_row(a.head, s - LB - k0, a.ring_rows) * ns];   // y_{n0-16+s-k0}
    int tb = 0;
    for (; tb + LB <= a.rows; tb += LB) acf_group<false>(a, hist, ns, k0, tb, acc, w);
    if (tb < a.rows) acf_group<true>(a, hist, ns, k0, tb, acc, w);
#pragma unroll
    for (int i = 0; i < LB; ++i) S[(size_t)i * ns] = acc[i];
}

// c_k = S_k - m (2T - H_k - L_k) + (n - k) m^2
MP_DEV double acf_ck(double S, double T, double H, double L, double m, double nk) {
    const double s = sub_rn(sub_rn(mul_rn(2.0, T), H), L);
    return add_rn(sub_rn(S, mul_rn(m, s)), mul_rn(nk, mul_rn(m, m)));
}

__global__ __launch_bounds__(kAcfThreads) void acf_rho_kernel(AcfArgs a) {
    const int j = blockIdx.x * kAcfThreads + threadIdx.x;
    if (j >= a.n_series) return;
    const size_t ns = (size_t)a.n_series;
    const int k0 = blockIdx.y * LB;
    const int64_t n = a.n0;
    const double *__restrict__ hist = a.hist + j;
    // L_k = sum_{t >= n - k} y_t in increasing t for the block's lags: a.head is the row of sample n, rows before sample 0 hold zeros
    double L[LB];
#pragma unroll
    for (int i = 0; i < LB; ++i) L[i] = 0.0;
    for (int off = -(k0 + LB - 1); off < 0; ++off) {
        const double y = hist[(size_t)ring_row(a.head, off, a.ring_rows) * ns];
#pragma unroll
        for (int i = 0; i < LB; ++i) L[i] = off >= -(k0 + i) ? add_rn(L[i], y) : L[i];
    }
    const double T = a.T[j], m = T / (double)n;
    const double c0 = acf_ck(a.S[j], T, 0.0, 0.0, m, (double)n);
#pragma unroll
    for (int i = 0; i < LB; ++i) {
        const int k = k0 + i;
        double rho = 0.0;
        if (k < n && c0 != 0.0) {
            const double H = a.H[(size_t)k * ns + j];     // (k < n: the ingest kernel has written it)
            rho = acf_ck(a.S[(size_t)k * ns + j], T, H, L[i], m, (double)(n - k)) / c0;
        }
        a.rho[(size_t)k * ns + j] = rho;
    }
}

__global__ __launch_bounds__(kAcfFinalThreads) void acf_final_kernel(AcfArgs a) {
    __shared__ double f[MP_ACF_MAX_LAG];
    const int e = blockIdx.x / a.ndim, d = blockIdx.x % a.ndim;
    const size_t ns = (size_t)a.n_series;
    const int lim = (int)(a.n0 < (int64_t)a.max_lag ? a.n0 : (int64_t)a.max_lag);   // lags 0 .. lim - 1 are known
    const double *__restrict__ rho = a.rho + (size_t)e * a.n_walkers * a.ndim + d;
    for (int k = threadIdx.x; k < lim; k += kAcfFinalThreads) {
        double s = 0.0;
        for (int w = 0; w < a.n_walkers; ++w) s = add_rn(s, rho[(size_t)k * ns + (size_t)w * a.ndim]);
        s = s / (double)a.n_walkers;
        f[k] = s;
        a.f[(size_t)blockIdx.x * a.kp + k] = s;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double cs = 0.0, taus = NAN;
    int window = -1;
    for (int M = 0; M < lim; ++M) {
        cs = add_rn(cs, f[M]);
        taus = sub_rn(mul_rn(2.0, cs), 1.0);
        if (!((double)M < mul_rn(a.c, taus))) {
            window = M;
            break;
        }
    }
    if (window < 0) {
        if (a.n0 <= (int64_t)a.max_lag) window = lim - 1;   // every lag is known: the host estimator's fallback, the last lag
        else taus = NAN;                                     // max_lag was too small: never a truncated sum
    }
    a.tau[blockIdx.x] = taus;
    a.window[blockIdx.x] = window;
}

}  // namespace

int launch_acf_accumulate(const AcfArgs &a, void *stream) {
    if (a.rows <= 0) return 0;
    const unsigned gx = (unsigned)((a.n_series + kAcfThreads - 1) / kAcfThreads);
    hipLaunchKernelGGL(acf_ingest_kernel, dim3(gx), dim3(kAcfThreads), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(acf_accumulate_kernel, dim3(gx, (unsigned)(a.kp / LB)), dim3(kAcfThreads), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int launch_acf_finalise(const AcfArgs &a, void *stream) {
    const unsigned gx = (unsigned)((a.n_series + kAcfThreads - 1) / kAcfThreads);
    hipLaunchKernelGGL(acf_rho_kernel, dim3(gx, (unsigned)(a.kp / LB)), dim3(kAcfThreads), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(acf_final_kernel, dim3((unsigned)(a.n_ensembles * a.ndim)), dim3(kAcfFinalThreads), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

}  // namespace mp
