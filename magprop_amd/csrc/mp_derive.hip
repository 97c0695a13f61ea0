// mp_derive.hip — gfx950 reduction of the five model curves of every sample to its MP_DERIVED_N derived quantities
// (mp_model_derived, include/magprop_amd.h; the order of the sums is stated in mp_derive.h).
//
// derive_kernel takes one row per workgroup of 256 threads.  Thread k owns segment k of the row's intervals and walks it through
// the LDS staging of mp_segwalk.h (stage, walk: shared with flow_reduce_kernel of mp_flows.hip).  Six passes: Ltot (sums, peak), Ltot again (the crossings need E_tot first; the row is 80 KB and comes from
// L2), Lprop (sum, peak), Ldip (sum), Mdisc and omega (peak).  Maxima: every thread's best in increasing index, then a tree
// under the total order (larger value, then lower index).  The 256 segment totals are added by one lane.  Curves of finished
// rows are finite (the curve kernels fill the rows of the others with NaN; those are not read).
#include <hip/hip_runtime.h>

#include <climits>

#include "mp_derive.h"
#include "mp_segwalk.h"
#include "mp_wg.h"

namespace mp {

namespace {

__global__ __launch_bounds__(kDeriveThreads) void derive_kernel(const DeriveArgs a) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    __shared__ double lc[kSlots], lt[kSlots];
    __shared__ double tot[kDeriveThreads];     // segment totals of the curve being summed; of Ltot then the totals before each segment
    __shared__ double res[MP_DERIVED_N];
    __shared__ double rv[kWaves];
    __shared__ int ri[kWaves];
    const int row = blockIdx.x, tid = threadIdx.x;
    const int G = a.n_grid, seg = derive_seg(G);
    double *out = a.out + (size_t)row * MP_DERIVED_N;
    if (a.status[row] != MP_STATUS_OK) {       // (uniform over the workgroup)
        if (tid < MP_DERIVED_N) out[tid] = __builtin_nan("");
        return;
    }
    const size_t off = (size_t)row * (size_t)G;
    const double *ltot = a.curve[0] + off, *lprop = a.curve[1] + off, *ldip = a.curve[2] + off, *mdisc = a.curve[3] + off,
                 *omega = a.curve[4] + off;
    const double *t = a.tgrid;
    double s;
    Best b;
    int cross[3];

    // Ltot: segment sums and peak
    walk<true, true, false>(ltot, t, G, seg, lc, lt, s, b, 0.0, nullptr, nullptr);
    tot[tid] = s;
    b = wg_best(b, rv, ri);                 // (its barriers order tot[] too)
    if (tid == 0) {
        double e = 0.0;
        for (int k = 0; k < kDeriveThreads; ++k) { const double v = tot[k]; tot[k] = e; e = e + v; }
        res[MP_DERIVED_E_TOT] = e;
        res[MP_DERIVED_L_PEAK] = b.v;
        res[MP_DERIVED_T_PEAK] = t[b.i];
    }
    __syncthreads();
    // Ltot again: the crossings of 10, 50 and 90 % of E_tot
    {
        const double e = res[MP_DERIVED_E_TOT];
        const double thr[3] = {0.1 * e, 0.5 * e, 0.9 * e};
        walk<false, false, true>(ltot, t, G, seg, lc, lt, s, b, tot[tid], thr, cross);
        for (int f = 0; f < 3; ++f) {
            int i = wg_least(cross[f], ri);
            if (i == INT_MAX) i = G - 2;       // never reached (a negative total): the last grid time
            if (e == 0.0) i = 0;
            if (tid == 0) res[MP_DERIVED_T10 + f] = t[i + 1];
        }
    }
    // Lprop: sum and peak
    walk<true, true, false>(lprop, t, G, seg, lc, lt, s, b, 0.0, nullptr, nullptr);
    tot[tid] = s;
    b = wg_best(b, rv, ri);
    if (tid == 0) {
        double e = 0.0;
        for (int k = 0; k < kDeriveThreads; ++k) e = e + tot[k];
        res[MP_DERIVED_E_PROP] = e;
        res[MP_DERIVED_LPROP_PEAK] = b.v;
        res[MP_DERIVED_T_LPROP_PEAK] = t[b.i];
    }
    __syncthreads();
    // Ldip: sum
    walk<true, false, false>(ldip, t, G, seg, lc, lt, s, b, 0.0, nullptr, nullptr);
    tot[tid] = s;
    __syncthreads();
    if (tid == 0) {
        double e = 0.0;
        for (int k = 0; k < kDeriveThreads; ++k) e = e + tot[k];
        res[MP_DERIVED_E_DIP] = e;
    }
    // omega and Mdisc: end value and peak
    walk<false, true, false>(omega, t, G, seg, lc, lt, s, b, 0.0, nullptr, nullptr);
    b = wg_best(b, rv, ri);
    if (tid == 0) {
        res[MP_DERIVED_OMEGA_END] = omega[G - 1];
        res[MP_DERIVED_OMEGA_MAX] = b.v;
        res[MP_DERIVED_T_OMEGA_MAX] = t[b.i];
    }
    walk<false, true, false>(mdisc, t, G, seg, lc, lt, s, b, 0.0, nullptr, nullptr);
    b = wg_best(b, rv, ri);
    if (tid == 0) {
        res[MP_DERIVED_MDISC_END] = mdisc[G - 1];
        res[MP_DERIVED_MDISC_MAX] = b.v;
        res[MP_DERIVED_T_MDISC_MAX] = t[b.i];
    }
    __syncthreads();
    if (tid < MP_DERIVED_N) out[tid] = res[tid];
}

}  // namespace

int launch_derive(const DeriveArgs &a, void *stream) {
    hipLaunchKernelGGL(derive_kernel, dim3((unsigned)a.n), dim3(kDeriveThreads), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

}  // namespace mp
