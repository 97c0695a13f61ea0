// mp_derive.hip — gfx950 reduction of the five model curves of every sample to its MP_DERIVED_N derived quantities
// (mp_model_derived, include/magprop_amd.h; the order of the sums is stated in mp_derive.h).
//
// derive_kernel takes one row per workgroup of 256 threads.  Thread k owns segment k of the row's intervals, so its points are
// contiguous in the row while consecutive lanes are a segment apart.  The row therefore goes through LDS: a window of up to
// kDeriveWindow intervals of EVERY segment (15 points each, the window's last point being the next window's first) is copied
// with consecutive lanes on consecutive points of a segment's stretch, slot k * 15 + r, and every thread then walks its own 15
// slots.  The stride of 15 doubles is odd, so the 64 lanes of a wavefront fall on different banks.  The times go through the
// same staging.  Six passes: Ltot (sums, peak), Ltot again (the crossings need E_tot first; the row is 80 KB and comes from
// L2), Lprop (sum, peak), Ldip (sum), Mdisc and omega (peak).  Maxima: every thread's best in increasing index, then a tree
// under the total order (larger value, then lower index).  The 256 segment totals are added by one lane.  Curves of finished
// rows are finite (the curve kernels fill the rows of the others with NaN; those are not read).
#include <hip/hip_runtime.h>

#include <climits>

#include "mp_derive.h"
#include "mp_wg.h"

namespace mp {

namespace {

constexpr int kStride = kDeriveWindow + 1;              // points of a segment's window, and its LDS stride in doubles
constexpr int kSlots = kDeriveThreads * kStride;
static_assert(kDeriveThreads == kWgThreads, "derive_kernel is one workgroup of mp_wg.h");
constexpr int kWaves = kWgWaves;
using Best = WgBest;   // every thread's best in increasing index, then wg_best's total order (larger value, then lower index)

// window c of every segment of src[0 .. G) into dst[k * kStride + r]: point k seg + c W + r for r <= the window's intervals
__device__ inline void stage(const double *__restrict__ src, double *dst, int G, int seg, int c) {
    const int lim = min(seg - c * kDeriveWindow, kDeriveWindow);
    for (int idx = threadIdx.x; idx < kSlots; idx += kDeriveThreads) {
        const int k = idx / kStride, r = idx - k * kStride;
        const int64_t j = (int64_t)k * seg + (int64_t)c * kDeriveWindow + r;
        if (r <= lim && j < G) dst[idx] = src[j];
    }
}

// One pass of the calling thread over its segment of `row`.  kSum: s becomes the segment's sum of trapezoid terms.  kMax: best
// becomes the first largest value among the segment's points (both ends included: a shared end point loses the tie to its
// lower owner, which is the same point).  kCross: cross[f] becomes the first interval of the segment whose cumulative energy,
// start + the running sum, reaches thr[f] (INT_MAX: none).
template <bool kSum, bool kMax, bool kCross>
__device__ void walk(const double *__restrict__ row, const double *__restrict__ t, int G, int seg, double *lc, double *lt, double &s,
                     Best &best, double start, const double *thr, int *cross) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const int k = threadIdx.x;
    const int64_t first = (int64_t)k * seg;
    const int64_t left = (int64_t)(G - 1) - first;
    const int n_int = left <= 0 ? 0 : (left < seg ? (int)left : seg);   // intervals of this segment
    const int n_win = (seg + kDeriveWindow - 1) / kDeriveWindow;
    const double *mc = lc + k * kStride, *mt = lt + k * kStride;
    s = 0.0;
    best.v = -INFINITY;
    best.i = INT_MAX;
    if (kCross) cross[0] = cross[1] = cross[2] = INT_MAX;
    for (int c = 0; c < n_win; ++c) {
        __syncthreads();                                   // the window before this one has been walked
        stage(row, lc, G, seg, c);
        if (kSum || kCross) stage(t, lt, G, seg, c);
        __syncthreads();
        const int cnt = max(0, min(kDeriveWindow, n_int - c * kDeriveWindow));
        const int i0 = (int)first + c * kDeriveWindow;
        for (int r = 0; r < cnt; ++r) {
            const double a = mc[r], b = mc[r + 1];
            if (kMax) {
                if (c == 0 && r == 0) { best.v = a; best.i = i0; }
                if (b > best.v) { best.v = b; best.i = i0 + r + 1; }
            }
            if (kSum || kCross) {
                const double dt = mt[r + 1] - mt[r];
                const double h = 0.5 * dt;
                const double ab = a + b;
                const double term = h * ab;
                s = s + term;
            }
            if (kCross) {
                const double cum = start + s;
#pragma unroll
                for (int f = 0; f < 3; ++f)
                    if (cross[f] == INT_MAX && cum >= thr[f]) cross[f] = i0 + r;
            }
        }
    }
}

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
