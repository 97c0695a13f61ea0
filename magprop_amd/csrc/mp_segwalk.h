// mp_segwalk.h — the segment walk of the row reductions (derive_kernel of mp_derive.hip, flow_reduce_kernel of mp_flows.hip):
// staging of a row through LDS and one thread's pass over its segment, in the order of sums mp_derive.h states.  Device only:
// included from .hip sources, never from a header a host compiler reads.
//
// One row per workgroup of kDeriveThreads = 256 threads.  Thread k owns segment k of the row's intervals, so its points are
// contiguous in the row while consecutive lanes are a segment apart.  The row therefore goes through LDS: a window of up to
// kDeriveWindow intervals of EVERY segment (15 points each, the window's last point being the next window's first) is copied
// with consecutive lanes on consecutive points of a segment's stretch, slot k * 15 + r, and every thread then walks its own 15
// slots.  The stride of 15 doubles is odd, so the 64 lanes of a wavefront fall on different banks.  The times go through the
// same staging.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>

#include "mp_derive.h"
#include "mp_wg.h"

namespace mp {

namespace {

constexpr int kStride = kDeriveWindow + 1;              // points of a segment's window, and its LDS stride in doubles
constexpr int kSlots = kDeriveThreads * kStride;
static_assert(kDeriveThreads == kWgThreads, "a row reduction is one workgroup of mp_wg.h");
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

}  // namespace

}  // namespace mp
