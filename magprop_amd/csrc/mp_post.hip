// mp_post.hip — gfx950 kernels of the sampler's posterior monitor (mp_sampler_set_posterior; include/magprop_amd.h states the
// definition, mp_post.h the layout).
//
// Per chunk of mp_sampler_run, four kernels read the chunk's rows of the device slab:
//   post_hist1_kernel    one workgroup per (slice of rows, group of dimensions, ensemble).  Its lanes run over the ensemble's
//                        share of every row element by element, so consecutive lanes load consecutive bytes; each element is
//                        binned into the workgroup's private 32-bit histogram in LDS (as many dimensions per group as fit
//                        kPostLdsBytes), and the counters that are not zero are added to the int64 global counters once, when
//                        the workgroup has read its rows.
//   post_hist2_kernel    one workgroup per (slice, pair, ensemble), one lane per (row, walker): consecutive lanes read the two
//                        coordinates of consecutive walkers, so a wavefront covers one contiguous span of the row, which the
//                        other pairs' workgroups find in L2.  Same private histogram and one flush.
//   post_moments_kernel  one lane per (walker, entry), sequential over the rows into the walker's running sum: y = x - pivot,
//                        every difference, product and sum rounded on its own.  The walkers are summed at read-out, on the host.
//   post_best_kernel     one workgroup per ensemble: every lane keeps the best of its samples in increasing index, a tree in
//                        LDS under the same total order (larger lnprob, then lower index) leaves the chunk's best, and lane 0
//                        holds it against the holder.
// Counters are integers, so the order of the LDS and global atomic adds does not matter; there is no floating-point atomic.
// LDS adds of one wavefront to one counter serialise (posterior samples cluster, so that is the usual case).  They are left
// plain: at 64 lanes on one counter a chunk of 64 MB costs every one of the 64 slices some 10^5 LDS cycles, tens of
// microseconds behind 0.2 s of sampling (DESIGN.md section 8 weighs the aggregation of equal bins inside a wavefront).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "mp_math.hpp"
#include "mp_post.h"

namespace mp {

namespace {

// The bin rule: 0 .. B - 1 a bin, B below, B + 1 above, B + 2 not finite
MP_DEV int post_bin(double v, double lo, double hi, double inv, int B) {
    if (!isfinite(v)) return B + 2;
    if (v < lo) return B;
    if (v >= hi) return B + 1;
    const int b = (int)floor(mul_rn(sub_rn(v, lo), inv));
    return b >= B ? B - 1 : b;
}

// rows [r0, r1) of the chunk that slice s of n takes
MP_DEV void slice_rows(int rows, int s, int n, int &r0, int &r1) {
    r0 = (int)((int64_t)rows * s / n);
    r1 = (int)((int64_t)rows * (s + 1) / n);
}

__global__ __launch_bounds__(kPostThreads) void post_hist1_kernel(PostArgs a, int dims_per_group) {
    extern __shared__ uint32_t h[];
    const int e = blockIdx.z, d0 = blockIdx.y * dims_per_group;
    const int nd = min(dims_per_group, a.ndim - d0), stride = a.bins1 + 3, nc = nd * stride;
    for (int k = threadIdx.x; k < nc; k += kPostThreads) h[k] = 0u;
    __syncthreads();
    int r0, r1;
    slice_rows(a.rows, blockIdx.x, gridDim.x, r0, r1);
    const int ew = a.n_walkers * a.ndim;                       // the ensemble's elements of a row
    const size_t row = (size_t)a.n_total * a.ndim;
    const double *__restrict__ src = a.chain + (size_t)(a.first + r0) * row + (size_t)e * ew;
    const int count = (r1 - r0) * ew;                          // (below 2^31: launch_post_accumulate)
    for (int idx = threadIdx.x; idx < count; idx += kPostThreads) {
        const int r = idx / ew, j = idx - r * ew, d = j % a.ndim - d0;
        if ((unsigned)d < (unsigned)nd) {
            const int dd = d + d0;
            const int c = post_bin(src[(size_t)r * row + j], a.par[dd], a.par[a.ndim + dd], a.par[2 * a.ndim + dd], a.bins1);
            atomicAdd(&h[d * stride + c], 1u);
        }
    }
    __syncthreads();
    unsigned long long *dst = (unsigned long long *)a.hist1 + ((size_t)e * a.ndim + d0) * stride;
    for (int k = threadIdx.x; k < nc; k += kPostThreads)
        if (h[k]) atomicAdd(&dst[k], (unsigned long long)h[k]);
}

__global__ __launch_bounds__(kPostThreads) void post_hist2_kernel(PostArgs a) {
    extern __shared__ uint32_t h[];
    const int e = blockIdx.z, B = a.bins2, nc = B * B;
    int pa = 0, pb = blockIdx.y;                               // pair p -> (pa, pb)
    for (int len = a.ndim - 1; pb >= len; pb -= len, --len) ++pa;
    pb += pa + 1;
    for (int k = threadIdx.x; k < nc; k += kPostThreads) h[k] = 0u;
    __syncthreads();
    int r0, r1;
    slice_rows(a.rows, blockIdx.x, gridDim.x, r0, r1);
    const size_t row = (size_t)a.n_total * a.ndim;
    const double *__restrict__ src = a.chain + (size_t)(a.first + r0) * row + (size_t)e * a.n_walkers * a.ndim;
    const double lo_a = a.par[pa], hi_a = a.par[a.ndim + pa], inv_a = a.par[3 * a.ndim + pa];
    const double lo_b = a.par[pb], hi_b = a.par[a.ndim + pb], inv_b = a.par[3 * a.ndim + pb];
    const int count = (r1 - r0) * a.n_walkers;
    unsigned outside = 0u;
    for (int idx = threadIdx.x; idx < count; idx += kPostThreads) {
        const int r = idx / a.n_walkers, w = idx - r * a.n_walkers;
        const double *x = src + (size_t)r * row + (size_t)w * a.ndim;
        const int ba = post_bin(x[pa], lo_a, hi_a, inv_a, B), bb = post_bin(x[pb], lo_b, hi_b, inv_b, B);
        if (ba < B && bb < B) atomicAdd(&h[ba * B + bb], 1u);
        else ++outside;
    }
    __syncthreads();
    const size_t p = (size_t)e * gridDim.y + blockIdx.y;
    unsigned long long *dst = (unsigned long long *)a.hist2 + p * nc;
    for (int k = threadIdx.x; k < nc; k += kPostThreads)
        if (h[k]) atomicAdd(&dst[k], (unsigned long long)h[k]);
    __syncthreads();                                           // the histogram is flushed: its first word now counts the outsiders
    if (threadIdx.x == 0) h[0] = 0u;
    __syncthreads();
    if (outside) atomicAdd(&h[0], outside);
    __syncthreads();
    if (threadIdx.x == 0 && h[0]) atomicAdd((unsigned long long *)a.outside2 + p, (unsigned long long)h[0]);
}

__global__ __launch_bounds__(kPostThreads) void post_moments_kernel(PostArgs a, int n_entries) {
    const int g = blockIdx.x * kPostThreads + threadIdx.x;
    if (g >= n_entries * a.n_total) return;
    const int entry = g / a.n_total, wg = g - entry * a.n_total;
    int ia = entry, ib = -1;                                   // s1[ia], or s2[ia][ib]
    if (entry >= a.ndim) {
        ia = 0;
        ib = entry - a.ndim;
        for (int len = a.ndim; ib >= len; ib -= len, --len) ++ia;
        ib += ia;
    }
    const double pv_a = a.par[4 * a.ndim + ia], pv_b = a.par[4 * a.ndim + (ib < 0 ? ia : ib)];
    const size_t row = (size_t)a.n_total * a.ndim;
    const double *__restrict__ x = a.chain + (size_t)a.first * row + (size_t)wg * a.ndim;
    double acc = a.mom[g];
    int64_t cnt = 0;
    for (int r = 0; r < a.rows; ++r, x += row) {
        bool ok = true;
        for (int d = 0; d < a.ndim; ++d) ok = ok && isfinite(x[d]);
        if (ok) {
            const double ya = sub_rn(x[ia], pv_a);
            acc = add_rn(acc, ib < 0 ? ya : mul_rn(ya, sub_rn(x[ib], pv_b)));
            ++cnt;
        }
    }
    a.mom[g] = acc;
    if (entry == 0) a.nfin[wg] += cnt;
}

// does sample (l, i) take the place of (bl, bi)?  Larger lnprob, or the same with a lower index; a NaN never does
MP_DEV bool post_better(double l, int64_t i, double bl, int64_t bi) { return l > bl || (l == bl && i < bi); }

__global__ __launch_bounds__(kPostBestThreads) void post_best_kernel(PostArgs a) {
    __shared__ double sl[kPostBestThreads];
    __shared__ int si[kPostBestThreads];
    const int e = blockIdx.x, t = threadIdx.x;
    const double *__restrict__ lnp = a.lnp + (size_t)a.first * a.n_total + (size_t)e * a.n_walkers;
    const int count = a.rows * a.n_walkers;                    // sample r * n_walkers + w of the chunk
    double bl = -INFINITY;
    int bi = -1;
    for (int idx = t; idx < count; idx += kPostBestThreads) {
        const int r = idx / a.n_walkers, w = idx - r * a.n_walkers;
        const double l = lnp[(size_t)r * a.n_total + w];
        if (l > bl) { bl = l; bi = idx; }
    }
    sl[t] = bl;
    si[t] = bi;
    __syncthreads();
    for (int s = kPostBestThreads / 2; s > 0; s >>= 1) {
        if (t < s && post_better(sl[t + s], si[t + s], sl[t], si[t])) { sl[t] = sl[t + s]; si[t] = si[t + s]; }
        __syncthreads();
    }
    if (t != 0 || si[0] < 0) return;
    const int64_t gi = a.n0 * a.n_walkers + si[0];
    if (!post_better(sl[0], gi, a.best_lnp[e], a.best_idx[e])) return;
    const int r = si[0] / a.n_walkers, w = si[0] - r * a.n_walkers;
    const double *x = a.chain + ((size_t)(a.first + r) * a.n_total + (size_t)e * a.n_walkers + w) * a.ndim;
    for (int d = 0; d < a.ndim; ++d) a.best_x[(size_t)e * a.ndim + d] = x[d];
    a.best_lnp[e] = sl[0];
    a.best_idx[e] = gi;
}

__global__ __launch_bounds__(kPostThreads) void post_reset_kernel(PostArgs a) {
    const int g = blockIdx.x * kPostThreads + threadIdx.x;
    if (g < a.n_ensembles * a.ndim) a.best_x[g] = NAN;
    if (g < a.n_ensembles) {
        a.best_lnp[g] = -INFINITY;
        a.best_idx[g] = -1;
    }
}

}  // namespace

int launch_post_reset(const PostArgs &a, void *stream) {
    const unsigned gx = (unsigned)((a.n_ensembles * a.ndim + kPostThreads - 1) / kPostThreads);
    hipLaunchKernelGGL(post_reset_kernel, dim3(gx), dim3(kPostThreads), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int launch_post_accumulate(const PostArgs &a, void *stream) {
    if (a.rows <= 0) return 0;
    // the kernels index the elements of a chunk with 32 bits, and the grid's second and third dimensions end at 65 535
    const int ne = post_n_entries(a.ndim);
    if ((int64_t)a.rows * a.n_total * a.ndim >= ((int64_t)1 << 31) || (int64_t)ne * a.n_total >= ((int64_t)1 << 31) || a.n_ensembles > 65535)
        return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    const int64_t samples = (int64_t)a.rows * a.n_walkers;
    const unsigned slices = (unsigned)std::max<int64_t>(1, std::min<int64_t>({(int64_t)kPostMaxSlices, (int64_t)a.rows, (samples + kPostSliceSamples - 1) / kPostSliceSamples}));
    const int per_dim = post_stride1(a.bins1) * (int)sizeof(uint32_t);
    const int dims_per_group = std::min(a.ndim, kPostLdsBytes / per_dim);
    const unsigned groups = (unsigned)((a.ndim + dims_per_group - 1) / dims_per_group);
    hipLaunchKernelGGL(post_hist1_kernel, dim3(slices, groups, (unsigned)a.n_ensembles), dim3(kPostThreads), (size_t)dims_per_group * per_dim, st, a, dims_per_group);
    const int np = post_n_pairs(a.ndim);
    if (a.bins2 > 0 && np > 0)
        hipLaunchKernelGGL(post_hist2_kernel, dim3(slices, (unsigned)np, (unsigned)a.n_ensembles), dim3(kPostThreads), (size_t)a.bins2 * a.bins2 * sizeof(uint32_t), st, a);
    const unsigned gm = (unsigned)(((int64_t)ne * a.n_total + kPostThreads - 1) / kPostThreads);
    hipLaunchKernelGGL(post_moments_kernel, dim3(gm), dim3(kPostThreads), 0, st, a, ne);
    hipLaunchKernelGGL(post_best_kernel, dim3((unsigned)a.n_ensembles), dim3(kPostBestThreads), 0, st, a);
    return (int)hipGetLastError();
}

}  // namespace mp
