// mp_pointwise.hip — gfx950 kernels of the pointwise predictive scores (mp_model_pointwise, include/magprop_amd.h; the cell, the
// tail length and the order of the sums are stated in mp_pointwise.h).
//
// pointwise_cells_kernel turns a chunk's Ltot rows (walker-major [cnt][n_grid], what the curve kernels write) into standardised
// residuals z in the observation-major matrix Z[n_obs][n], through 64 x 64 LDS tiles of stride 65: on the way in a wavefront
// walks one curve row at the observations' grid points, on the way out it stores 64 consecutive samples of one observation.
// pointwise_select_kernel takes one observation per workgroup: the min(T, N_USED)-th largest r = z^2 / 2 by an MSB-first radix
// select over 8-bit digits of band_key(r) (mp_band.h; the column is streamed from memory once per digit: it does not fit LDS at
// 262 144 samples), then the larger values are compacted into LDS, filled up with copies of the cut and sorted (bitonic, at most
// 2 048 slots): wg_tail_select of mp_tail.h, which mp_reweight.hip shares.  pointwise_reduce_kernel takes one observation per workgroup as well: counts, means, the two-pass variance,
// extrema and the log-sum-exp pairs (lse_add, wave_lse, lse_merge of mp_math.hpp), with the select kernel's cut.
#include <hip/hip_runtime.h>

#include "mp_band.h"
#include "mp_math.hpp"
#include "mp_pointwise.h"
#include "mp_tail.h"
#include "mp_wg.h"

namespace mp {

namespace {

static_assert(kPointwiseThreads == kWgThreads, "the select and reduce kernels are one workgroup of mp_wg.h each");
constexpr int kWaves = kWgWaves;

__device__ inline double cell_r(double z) {
#pragma clang fp contract(off)
    const double zz = z * z;
    return 0.5 * zz;
}

__global__ __launch_bounds__(kPointwiseThreads) void pointwise_cells_kernel(const PointwiseCellsArgs a) {
#pragma clang fp contract(off)
    __shared__ double tile[kPointwiseTile][kPointwiseTile + 1];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int j0 = blockIdx.x * kPointwiseTile, s0 = blockIdx.y * kPointwiseTile;
    const int j = j0 + tx;
    const bool have = j < a.d.n_obs;
    int g = 0;
    double dx = 0.0, idt = 0.0, y = 0.0, ye = 1.0;
    if (have) {
        g = min(max(a.d.g[j], 0), a.n_grid - 2);   // (mp_set_dataset keeps g inside the grid: the last point sits in the last interval)
        dx = a.d.dx[j];
        idt = a.d.idt[j];
        y = a.d.y[j];
        ye = a.d.yerr[j];
    }
    for (int r = ty; r < kPointwiseTile; r += kWaves) {
        const int s = s0 + r;
        double z = __builtin_nan("");
        if (have && s < a.cnt && a.status[s] == MP_STATUS_OK) {
            const double *row = a.ltot + (size_t)s * (size_t)a.n_grid;
            const double La = row[g], Lb = row[g + 1];
            const double d = Lb - La;
            const double slope = d * idt;
            const double rise = slope * dx;
            const double mod = rise + La;
            const double res = y - mod;
            z = res / ye;
        }
        tile[r][tx] = z;
    }
    __syncthreads();
    for (int r = ty; r < kPointwiseTile; r += kWaves) {
        const int jj = j0 + r, s = s0 + tx;
        if (jj < a.d.n_obs && s < a.cnt) a.z[(size_t)jj * (size_t)a.n + (size_t)a.lo + (size_t)s] = tile[tx][r];
    }
}

__global__ __launch_bounds__(kPointwiseThreads) void pointwise_select_kernel(const PointwiseColsArgs a) {
    __shared__ WgSelectLds sel;
    __shared__ uint64_t keys[kPointwiseSortCap];
    const int j = blockIdx.x;
    const double *col = a.z + (size_t)j * (size_t)a.n;
    // the candidates are the non-NaN z, their keys band_key(cell_r(z))
    wg_tail_select((int)a.n, sel, keys, a.obs + (size_t)j * MP_POINTWISE_N + MP_POINTWISE_CUT,
                   a.tail ? a.tail + (size_t)j * (size_t)a.tail_stride : nullptr, a.tail_stride, [col](int i, uint64_t &k) {
                       const double z = col[i];
                       k = band_key(cell_r(z));
                       return !__builtin_isnan(z);
                   });
}

__global__ __launch_bounds__(kPointwiseThreads) void pointwise_reduce_kernel(const PointwiseColsArgs a) {
#pragma clang fp contract(off)
    __shared__ double shm[kWaves], shs[kWaves];
    __shared__ uint32_t shc[kWaves];
    const int j = blockIdx.x, tid = threadIdx.x;
    const int n = (int)a.n;
    const double *col = a.z + (size_t)j * (size_t)a.n;
    double *out = a.obs + (size_t)j * MP_POINTWISE_N;
    const double cut = out[MP_POINTWISE_CUT];               // the select kernel's (NaN: no used cell; nothing here writes it)
    double sz = 0.0, sr = 0.0, rmin = INFINITY, rmax = -INFINITY, lm = -INFINITY, ls = 0.0, tm = -INFINITY, ts = 0.0;
    uint32_t cnt = 0, nt = 0;
    for (int i = tid; i < n; i += kPointwiseThreads) {
        const double z = col[i];
        if (__builtin_isnan(z)) continue;
        const double r = cell_r(z);
        ++cnt;
        sz = sz + z;
        sr = sr + r;
        rmin = fmin(rmin, r);
        rmax = fmax(rmax, r);
        lse_add(lm, ls, -r);
        if (r <= cut) {
            ++nt;
            lse_add(tm, ts, r);
        }
    }
    const uint32_t m = wg_count(cnt, shc);
    const uint32_t nontail = wg_count(nt, shc);
    sz = wg_sum(sz, shm);
    sr = wg_sum(sr, shm);
    rmin = wg_min(rmin, shm);
    rmax = wg_max(rmax, shm);
    wg_lse(lm, ls, shm, shs);
    wg_lse(tm, ts, shm, shs);
    const double zmean = sz / (double)m, rmean = sr / (double)m;   // (0 / 0 = NaN without a used cell)
    // second pass: squared deviations of ll = -r from its mean -rmean
    const double mean_ll = -rmean;
    double ss = 0.0;
    for (int i = tid; i < n; i += kPointwiseThreads) {
        const double z = col[i];
        if (__builtin_isnan(z)) continue;
        const double dev = -cell_r(z) - mean_ll;
        const double sq = dev * dev;
        ss = ss + sq;
    }
    ss = wg_sum(ss, shm);
    if (tid == 0) {
        out[MP_POINTWISE_N_USED] = (double)m;
        out[MP_POINTWISE_Z_MEAN] = zmean;
        out[MP_POINTWISE_R_MEAN] = rmean;
        out[MP_POINTWISE_LL_VAR] = m >= 2 ? ss / (double)(m - 1) : __builtin_nan("");
        out[MP_POINTWISE_R_MIN] = m ? rmin : __builtin_nan("");
        out[MP_POINTWISE_R_MAX] = m ? rmax : __builtin_nan("");
        out[MP_POINTWISE_LPPD_M] = lm;
        out[MP_POINTWISE_LPPD_S] = ls;
        out[MP_POINTWISE_NONTAIL_COUNT] = (double)nontail;
        out[MP_POINTWISE_NONTAIL_M] = tm;
        out[MP_POINTWISE_NONTAIL_S] = ts;
    }
}

}  // namespace

int launch_pointwise_cells(const PointwiseCellsArgs &a, void *stream) {
    const dim3 grid((unsigned)((a.d.n_obs + kPointwiseTile - 1) / kPointwiseTile), (unsigned)((a.cnt + kPointwiseTile - 1) / kPointwiseTile));
    hipLaunchKernelGGL(pointwise_cells_kernel, grid, dim3(kPointwiseThreads), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int launch_pointwise_select(const PointwiseColsArgs &a, void *stream) {
    hipLaunchKernelGGL(pointwise_select_kernel, dim3((unsigned)a.n_obs), dim3(kPointwiseThreads), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int launch_pointwise_reduce(const PointwiseColsArgs &a, void *stream) {
    hipLaunchKernelGGL(pointwise_reduce_kernel, dim3((unsigned)a.n_obs), dim3(kPointwiseThreads), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

}  // namespace mp
