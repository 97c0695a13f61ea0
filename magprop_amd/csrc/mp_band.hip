// mp_band.hip — gfx950 reduction of S model light curves to per-grid-point quantiles (mp_model_band, include/magprop_amd.h).
//
// band_transpose_kernel turns one component's curves from walker-major [S][n_grid] (what the curve kernels write) into
// point-major [n_grid][S] through 64 x 64 LDS tiles, so that both its loads and its stores are coalesced.
// band_select_kernel then takes one grid point per workgroup: the S values become order-preserving 64-bit keys in LDS (NaNs
// dropped; S <= MP_BAND_MAX_SAMPLES = 16 384 keys are 128 KiB), every needed order statistic is found by an MSB-first radix
// select over 8-bit digits (256-bin histograms, one per wavefront, merged and scanned once per pass), its upper neighbour by
// one counting pass, and mp_band.h's lerp finishes the quantile.
// band_wselect_kernel is the select of the weighted band (mp_model_band_weighted): the same walk over sums of the rows' integer
// units (64-bit histograms; wg_wradix_select of mp_wg.h), one select per quantile and no interpolation.  The keys sit in LDS at
// their row index, a NaN as the all-ones key; the units stay in global memory, one array shared by every workgroup.
#include <hip/hip_runtime.h>

#include "mp_band.h"
#include "mp_wg.h"

namespace mp {

namespace {

static_assert(kBandThreads == kWgThreads, "the select kernel is one workgroup of mp_wg.h");
constexpr int kWaves = kWgWaves;
// dynamic LDS of the select kernel: the select's words (spare: next_rank's count) | next_rank's minimum | keys[n] u64
struct BandLds {
    WgSelectLds sel;
    unsigned long long above;
    uint32_t pad[6];
};
constexpr int kKeysOffset = sizeof(BandLds);
static_assert(kKeysOffset == 4160, "a multiple of 16, and what the cap of MP_BAND_MAX_SAMPLES keys was sized with");

__global__ __launch_bounds__(kBandThreads) void band_transpose_kernel(const double *__restrict__ src, double *__restrict__ dst,
                                                                      int n, int n_grid) {
    __shared__ double tile[kBandTile][kBandTile + 1];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int g0 = blockIdx.x * kBandTile, s0 = blockIdx.y * kBandTile;
    for (int r = ty; r < kBandTile; r += kWaves) {
        const int s = s0 + r, g = g0 + tx;
        tile[r][tx] = (s < n && g < n_grid) ? src[(size_t)s * n_grid + g] : 0.0;
    }
    __syncthreads();
    for (int r = ty; r < kBandTile; r += kWaves) {
        const int g = g0 + r, s = s0 + tx;
        if (g < n_grid && s < n) dst[(size_t)g * n + s] = tile[tx][r];
    }
}

// The key of rank lo + 1, given the key a of rank lo: a itself if more than lo + 1 keys are <= a, else the least key above a.
__device__ uint64_t next_rank(const uint64_t *keys, int m, int lo, uint64_t a, BandLds &s) {
    uint32_t le = 0;
    uint64_t above = ~0ull;
    for (int i = threadIdx.x; i < m; i += kBandThreads) {
        const uint64_t k = keys[i];
        le += k <= a;
        if (k > a && k < above) above = k;
    }
    for (int d = 32; d >= 1; d >>= 1) {
        le += __shfl_xor(le, d, 64);
        const uint64_t o = __shfl_xor(above, d, 64);
        above = o < above ? o : above;
    }
    if (threadIdx.x == 0) { s.sel.spare = 0; s.above = ~0ull; }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&s.sel.spare, le);
        atomicMin(&s.above, (unsigned long long)above);
    }
    __syncthreads();
    const uint32_t cnt = s.sel.spare;
    const uint64_t res = cnt > (uint32_t)(lo + 1) ? a : (uint64_t)s.above;
    __syncthreads();
    return res;
}

__global__ __launch_bounds__(kBandThreads) void band_select_kernel(const double *__restrict__ cols, int n, int n_grid, const BandQ q,
                                                                   double *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    BandLds &s = *reinterpret_cast<BandLds *>(smem);
    uint64_t *keys = reinterpret_cast<uint64_t *>(smem + kKeysOffset);
    const int g = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double *col = cols + (size_t)g * n;
    if (threadIdx.x == 0) s.sel.count = 0;
    __syncthreads();
    // keys of the non-NaN values, packed (in no particular order: the order statistics do not depend on it)
    for (int base = wave * 64; base < n; base += kBandThreads) {
        const int i = base + lane;
        const double v = i < n ? col[i] : 0.0;
        const bool keep = i < n && !__builtin_isnan(v);
        const uint64_t k = band_key(v);                 // (ahead of the packing step: the select loop below keeps its place in the code)
        const uint32_t slot = wave_pack_slot(keep, &s.sel.count);
        if (keep) keys[slot] = k;
    }
    __syncthreads();
    const int m = (int)s.sel.count;
    __syncthreads();
    for (int j = 0; j < q.nq; ++j) {
        double res;
        if (m == 0) {
            res = __builtin_nan("");
        } else {
            const BandRank rk = band_rank(m, q.q[j]);
            const uint64_t ka = wg_radix_select(m, (uint32_t)rk.lo, s.sel, [keys](int i, uint64_t &k) { k = keys[i]; return true; });
            const uint64_t kb = rk.hi == rk.lo ? ka : next_rank(keys, m, rk.lo, ka, s);
            res = band_lerp(band_value(ka), band_value(kb), rk.gamma);
        }
        if (threadIdx.x == 0) out[(size_t)j * n_grid + g] = res;
    }
}

// dynamic LDS of the weighted select kernel: the select's words | keys[n] u64, unpacked (row i at keys[i])
constexpr int kWKeysOffset = sizeof(WgWSelectLds);
static_assert(kWKeysOffset == 8240 && kWKeysOffset % 16 == 0, "a multiple of 16; with MP_BAND_MAX_SAMPLES keys 139 312 of the CU's 163 840 bytes");
constexpr uint64_t kNoKey = ~0ull;   // what a NaN is stored as: band_key maps no non-NaN double to it

__global__ __launch_bounds__(kBandThreads) void band_wselect_kernel(const double *__restrict__ cols, const uint32_t *__restrict__ units,
                                                                    int n, int n_grid, const BandQ q, double *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    WgWSelectLds &s = *reinterpret_cast<WgWSelectLds *>(smem);
    uint64_t *keys = reinterpret_cast<uint64_t *>(smem + kWKeysOffset);
    const int g = blockIdx.x;
    const double *col = cols + (size_t)g * n;
    // the keys, and W: the units of the rows the column uses
    unsigned long long w = 0;
    for (int i = threadIdx.x; i < n; i += kBandThreads) {
        const double v = col[i];
        const bool used = !__builtin_isnan(v);
        keys[i] = used ? band_key(v) : kNoKey;
        w += used ? units[i] : 0u;
    }
    const uint64_t W = wg_across(wave_all(w, WgAdd()), s.wave, WgAdd());   // (its barriers publish the keys)
    for (int j = 0; j < q.nq; ++j) {
        double res = __builtin_nan("");
        if (W != 0) {
            const uint64_t k = wg_wradix_select(n, band_weight_target(q.q[j], W), s, [keys, units](int i, uint64_t &k, uint32_t &u) {
                k = keys[i];
                u = units[i];
                return k != kNoKey;
            });
            res = band_value(k);
        }
        if (threadIdx.x == 0) out[(size_t)j * n_grid + g] = res;
    }
}

}  // namespace

int launch_band_transpose(const double *src, double *dst, int n, int n_grid, void *stream) {
    const dim3 grid((unsigned)((n_grid + kBandTile - 1) / kBandTile), (unsigned)((n + kBandTile - 1) / kBandTile));
    hipLaunchKernelGGL(band_transpose_kernel, grid, dim3(kBandThreads), 0, (hipStream_t)stream, src, dst, n, n_grid);
    return (int)hipGetLastError();
}

int launch_band_select(const double *cols, int n, int n_grid, const BandQ &q, double *out, void *stream) {
    const size_t lds = (size_t)kKeysOffset + sizeof(uint64_t) * (size_t)n;
    if (lds > 65536) {   // (above 64 KiB of dynamic LDS the kernel has to be allowed it, on the device current now)
        const hipError_t e = hipFuncSetAttribute((const void *)band_select_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(band_select_kernel, dim3((unsigned)n_grid), dim3(kBandThreads), lds, (hipStream_t)stream, cols, n, n_grid, q, out);
    return (int)hipGetLastError();
}

int launch_band_wselect(const double *cols, const uint32_t *units, int n, int n_grid, const BandQ &q, double *out, void *stream) {
    const size_t lds = (size_t)kWKeysOffset + sizeof(uint64_t) * (size_t)n;
    if (lds > 65536) {   // (as above)
        const hipError_t e = hipFuncSetAttribute((const void *)band_wselect_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(band_wselect_kernel, dim3((unsigned)n_grid), dim3(kBandThreads), lds, (hipStream_t)stream, cols, units, n, n_grid, q, out);
    return (int)hipGetLastError();
}

}  // namespace mp
