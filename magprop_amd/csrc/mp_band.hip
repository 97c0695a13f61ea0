// mp_band.hip — gfx950 reduction of S model light curves to per-grid-point quantiles (mp_model_band, include/magprop_amd.h).
//
// band_transpose_kernel turns one component's curves from walker-major [S][n_grid] (what the curve kernels write) into
// point-major [n_grid][S] through 64 x 64 LDS tiles, so that both its loads and its stores are coalesced.
// band_select_kernel then takes one grid point per workgroup: the S values become order-preserving 64-bit keys in LDS (NaNs
// dropped; S <= MP_BAND_MAX_SAMPLES = 16 384 keys are 128 KiB), every needed order statistic is found by an MSB-first radix
// select over 8-bit digits (256-bin histograms, one per wavefront, merged and scanned once per pass), its upper neighbour by
// one counting pass, and mp_band.h's lerp finishes the quantile.
#include <hip/hip_runtime.h>

#include "mp_band.h"

namespace mp {

namespace {

constexpr int kWaves = kBandThreads / 64;
// dynamic LDS of the select kernel: [kWaves][256] u32 histograms | 16 u32 of broadcast words | keys[n] u64
constexpr int kHistBytes = kWaves * 256 * 4;
constexpr int kMiscWords = 16;
constexpr int kKeysOffset = kHistBytes + kMiscWords * 4;   // 4 160: a multiple of 16
enum { kMiscCount = 0, kMiscDigit = 1, kMiscRank = 2, kMiscLe = 3, kMiscWave = 4 /* .. 4 + kWaves */, kMiscMinLo = 8, kMiscMinHi = 9 };

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

// Inclusive sum over the workgroup's 256 threads (one value each); every thread gets its own prefix.  misc[kMiscWave..] is
// scratch.  Ends with a barrier.
__device__ inline uint32_t block_inclusive_scan(uint32_t v, uint32_t *misc) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t u = __shfl_up(v, d, 64);
        if (lane >= d) v += u;
    }
    if (lane == 63) misc[kMiscWave + wave] = v;
    __syncthreads();
    uint32_t before = 0;
    for (int w = 0; w < wave; ++w) before += misc[kMiscWave + w];
    __syncthreads();
    return v + before;
}

// The key of rank r (0-based) among keys[0 .. m).  Every thread returns it.
__device__ uint64_t radix_select(const uint64_t *keys, int m, uint32_t r, uint32_t *hist, uint32_t *misc) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t *my_hist = hist + wave * 256;
    uint64_t prefix = 0, mask = 0;
    for (int shift = 56; shift >= 0; shift -= 8) {
        for (int i = threadIdx.x; i < kWaves * 256; i += kBandThreads) hist[i] = 0;
        __syncthreads();
        for (int base = wave * 64; base < m; base += kBandThreads) {
            const int i = base + lane;
            const uint64_t k = i < m ? keys[i] : 0;
            const bool take = i < m && (k & mask) == prefix;
            const uint32_t bin = (uint32_t)(k >> shift) & 255u;
            const uint64_t act = __ballot(take);
            if (act == 0) continue;
            // most walkers share the leading digits at a grid point: a wavefront whose candidates all fall into one bin adds once
            const int first = __builtin_ctzll(act);
            const uint32_t bin0 = __shfl(bin, first, 64);
            if (__ballot(take && bin == bin0) == act) {
                if (lane == first) atomicAdd(&my_hist[bin0], (uint32_t)__popcll(act));
            } else if (take) {
                atomicAdd(&my_hist[bin], 1u);
            }
        }
        __syncthreads();
        uint32_t c = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) c += hist[w * 256 + threadIdx.x];
        const uint32_t incl = block_inclusive_scan(c, misc);
        const uint32_t excl = incl - c;
        if (excl <= r && r < incl) {
            misc[kMiscDigit] = threadIdx.x;
            misc[kMiscRank] = r - excl;
        }
        __syncthreads();
        prefix |= (uint64_t)misc[kMiscDigit] << shift;
        mask |= (uint64_t)255 << shift;
        r = misc[kMiscRank];
        __syncthreads();
    }
    return prefix;
}

// The key of rank lo + 1, given the key a of rank lo: a itself if more than lo + 1 keys are <= a, else the least key above a.
__device__ uint64_t next_rank(const uint64_t *keys, int m, int lo, uint64_t a, uint32_t *misc) {
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
    if (threadIdx.x == 0) { misc[kMiscLe] = 0; misc[kMiscMinLo] = ~0u; misc[kMiscMinHi] = ~0u; }
    __syncthreads();
    unsigned long long *mn = reinterpret_cast<unsigned long long *>(misc + kMiscMinLo);
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&misc[kMiscLe], le);
        atomicMin(mn, (unsigned long long)above);
    }
    __syncthreads();
    const uint32_t cnt = misc[kMiscLe];
    const uint64_t res = cnt > (uint32_t)(lo + 1) ? a : (uint64_t)*mn;
    __syncthreads();
    return res;
}

__global__ __launch_bounds__(kBandThreads) void band_select_kernel(const double *__restrict__ cols, int n, int n_grid, const BandQ q,
                                                                   double *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t *hist = reinterpret_cast<uint32_t *>(smem);
    uint32_t *misc = reinterpret_cast<uint32_t *>(smem + kHistBytes);
    uint64_t *keys = reinterpret_cast<uint64_t *>(smem + kKeysOffset);
    const int g = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double *col = cols + (size_t)g * n;
    if (threadIdx.x == 0) misc[kMiscCount] = 0;
    __syncthreads();
    // keys of the non-NaN values, packed (in no particular order: the order statistics do not depend on it)
    for (int base = wave * 64; base < n; base += kBandThreads) {
        const int i = base + lane;
        const double v = i < n ? col[i] : 0.0;
        const bool keep = i < n && !__builtin_isnan(v);
        const uint64_t act = __ballot(keep);
        uint32_t at = 0;
        if (lane == 0 && act) at = atomicAdd(&misc[kMiscCount], (uint32_t)__popcll(act));
        at = __shfl(at, 0, 64);
        if (keep) keys[at + __popcll(act & ((1ull << lane) - 1ull))] = band_key(v);
    }
    __syncthreads();
    const int m = (int)misc[kMiscCount];
    __syncthreads();
    for (int j = 0; j < q.nq; ++j) {
        double res;
        if (m == 0) {
            res = __builtin_nan("");
        } else {
            const BandRank rk = band_rank(m, q.q[j]);
            const uint64_t ka = radix_select(keys, m, (uint32_t)rk.lo, hist, misc);
            const uint64_t kb = rk.hi == rk.lo ? ka : next_rank(keys, m, rk.lo, ka, misc);
            res = band_lerp(band_value(ka), band_value(kb), rk.gamma);
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

}  // namespace mp
