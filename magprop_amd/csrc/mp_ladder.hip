// mp_ladder.hip — gfx950 kernels of the tempered sampler's ladder adaptation and of the thermodynamic monitor (mp_ladder.h;
// include/magprop_amd.h states the arithmetic of both).
//
// ladder_init_kernel: one workgroup of kWgThreads per group, once when adaptation is switched on: the gaps of ln beta, their sum
// and the swap counters the first update starts from.
// ladder_adapt_kernel: one workgroup per group behind the swap sweep of every adapting step.  The pairs' acceptances, the factors
// exp(kappa (A_i - Abar)) and the new inverse temperatures exp(-cum_i) are spread over the threads; the three sums (Abar, G, cum)
// are formed by thread 0 in index order, so that a restatement with the device's exp reproduces the ladder bit for bit.  An
// update that would leave a gap that is not finite and > 0, or a ladder that is not strictly decreasing, is not taken and counted.
// thermo_kernel: one workgroup per ensemble over the rows of a chunk in step order: the row's sum of the walkers' finite lnprob in
// the order of mp_wg.h, added to the ensemble's running sum with one add per row.
#include <hip/hip_runtime.h>

#include "mp_ladder.h"
#include "mp_wg.h"

namespace mp {

namespace {

__global__ __launch_bounds__(kWgThreads) void ladder_init_kernel(const LadderArgs a) {
    const int grp = (int)blockIdx.x, T = a.n_temps, np = T - 1, tid = (int)threadIdx.x;
    const double *beta = a.beta + (size_t)grp * T;
    for (int i = tid; i < np; i += kWgThreads) {
        const double lb = i == 0 ? 0.0 : log(beta[i]), lb_next = log(beta[i + 1]);   // (beta_0 = 1: lb_0 = 0 exactly)
        a.gap[(size_t)grp * np + i] = sub_rn(lb, lb_next);
        a.prev[(size_t)grp * np + i] = a.swaps[(size_t)grp * np + i];
        if (i == np - 1) a.span[grp] = -lb_next;
    }
}

__global__ __launch_bounds__(kWgThreads) void ladder_adapt_kernel(const LadderArgs a) {
    const int grp = (int)blockIdx.x, T = a.n_temps, np = T - 1, tid = (int)threadIdx.x;
    double *beta = a.beta + (size_t)grp * T, *gap = a.gap + (size_t)grp * np;
    int64_t *prev = a.prev + (size_t)grp * np;
    const int64_t *swaps = a.swaps + (size_t)grp * np;
    double *wa = a.work + (size_t)grp * 2 * np, *wh = wa + np;   // wa: A, then cum, then the new beta; wh: h, then the new gap
    __shared__ double bcast;
    // A_i, and the counters the next update starts from
    for (int i = tid; i < np; i += kWgThreads) {
        const int64_t now = swaps[i];
        wa[i] = (double)(now - prev[i]) / (double)a.n_walkers;
        prev[i] = now;
    }
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int i = 0; i < np; ++i) s = add_rn(s, wa[i]);
        bcast = s / (double)np;
    }
    __syncthreads();
    const double abar = bcast;
    for (int i = tid; i < np; i += kWgThreads) wh[i] = mul_rn(gap[i], exp(mul_rn(a.kappa, sub_rn(wa[i], abar))));
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int i = 0; i < np; ++i) s = add_rn(s, wh[i]);
        bcast = a.span[grp] / s;
    }
    __syncthreads();
    const double c = bcast;
    for (int i = tid; i < np; i += kWgThreads) wh[i] = mul_rn(c, wh[i]);
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int i = 0; i < np; ++i) {
            s = add_rn(s, wh[i]);
            wa[i] = s;
        }
    }
    __syncthreads();
    for (int i = tid; i < np - 1; i += kWgThreads) wa[i] = exp(-wa[i]);   // the new beta_{i + 1}, i = 0 .. T - 3
    __syncthreads();
    // pair i of the new ladder, ends included: its gap finite and > 0, beta_i > beta_{i + 1} (a NaN fails either)
    int bad = 0;
    for (int i = tid; i < np; i += kWgThreads) {
        const double g = wh[i], left = i == 0 ? beta[0] : wa[i - 1], right = i == np - 1 ? beta[T - 1] : wa[i];
        if (!(g > 0.0) || !(g < INFINITY) || !(left > right)) bad = 1;
    }
    bad = __syncthreads_or(bad);
    if (bad) {
        if (tid == 0) a.dropped[grp] += 1;
    } else {
        for (int i = tid; i < np; i += kWgThreads) {
            gap[i] = wh[i];
            if (i < np - 1) beta[i + 1] = wa[i];
        }
    }
    if (a.history) {
        __syncthreads();   // (the writes above are this workgroup's own: visible to it behind the barrier)
        double *row = a.history + ((size_t)a.t * a.n_groups + grp) * T;
        for (int i = tid; i < T; i += kWgThreads) row[i] = beta[i];
    }
}

__global__ __launch_bounds__(kWgThreads) void thermo_kernel(const ThermoArgs a) {
    const int e = (int)blockIdx.x, n = a.n_walkers, tid = (int)threadIdx.x;
    __shared__ double shd[kWgWaves];
    __shared__ uint32_t shc[kWgWaves];
    double sum = a.sum[e];
    int64_t n_fin = a.n_finite[e], n_non = a.n_nonfinite[e];
    for (int r = a.first; r < a.first + a.rows; ++r) {
        const double *lnp = a.lnp + ((size_t)r * a.n_ensembles + e) * n;
        double s = 0.0;
        uint32_t fin = 0;
        for (int i = tid; i < n; i += kWgThreads) {
            const double v = lnp[i];
            if (fabs(v) < INFINITY) {
                s = add_rn(s, v);
                ++fin;
            }
        }
        const double row_sum = wg_sum(s, shd);
        const uint32_t row_fin = wg_count(fin, shc);
        sum = add_rn(sum, row_sum);
        n_fin += row_fin;
        n_non += n - (int)row_fin;
    }
    if (tid == 0) {
        a.sum[e] = sum;
        a.n_finite[e] = n_fin;
        a.n_nonfinite[e] = n_non;
    }
}

}  // namespace

int launch_ladder_init(const LadderArgs &a, void *stream) {
    if (a.n_groups <= 0) return 0;
    hipLaunchKernelGGL(ladder_init_kernel, dim3((unsigned)a.n_groups), dim3(kWgThreads), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int launch_ladder_adapt(const LadderArgs &a, void *stream) {
    if (a.n_groups <= 0) return 0;
    hipLaunchKernelGGL(ladder_adapt_kernel, dim3((unsigned)a.n_groups), dim3(kWgThreads), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int launch_thermo(const ThermoArgs &a, void *stream) {
    if (a.n_ensembles <= 0 || a.rows <= 0) return 0;
    hipLaunchKernelGGL(thermo_kernel, dim3((unsigned)a.n_ensembles), dim3(kWgThreads), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

}  // namespace mp
