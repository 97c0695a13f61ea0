// mp_wg.h — what a workgroup of kWgThreads = 256 threads (four wavefronts of 64) does together in the reductions behind
// mp_model_band, mp_model_derived and mp_model_pointwise (mp_band.hip, mp_derive.hip, mp_pointwise.hip): combinations that
// return one result to every thread, the inclusive scan, the wavefront packing step and the radix select.  Device only: included
// from .hip sources, never from a header a host compiler reads.
//
// Order of every combination, part of the results' definition (mp_pointwise.h, mp_derive.h): inside a wavefront the xor butterfly
// over distances 32, 16, .. 1 (wave_sum and wave_lse of mp_math.hpp where a sum is formed), then the four wavefronts' results
// through LDS in wavefront order starting from wavefront 0's.  Every sum rounds on its own (fp contract off).  Every function
// here is called by all 256 threads and ends with a barrier, so that its LDS may be used again at once.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "mp_math.hpp"

namespace mp {

constexpr int kWgThreads = 256;
constexpr int kWgWaves = kWgThreads / 64;

struct WgAdd {
    template <class T>
    __device__ T operator()(T a, T b) const {
#pragma clang fp contract(off)
        return a + b;
    }
};
struct WgMin {
    __device__ double operator()(double a, double b) const { return fmin(a, b); }
    __device__ int operator()(int a, int b) const { return min(a, b); }
};
struct WgMax {
    __device__ double operator()(double a, double b) const { return fmax(a, b); }
};

// the butterfly over the 64 lanes of a wavefront: every lane ends with the same value
template <class T, class Op>
__device__ inline T wave_all(T v, Op op) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = op(v, __shfl_xor(v, d, 64));
    return v;
}

// the four wavefronts' values v (the same in every lane of a wavefront) combined in wavefront order; sh[kWgWaves] is scratch
template <class T, class Op>
__device__ inline T wg_across(T v, T *sh, Op op) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    T r = sh[0];
#pragma unroll
    for (int w = 1; w < kWgWaves; ++w) r = op(r, sh[w]);
    __syncthreads();
    return r;
}

__device__ inline double wg_sum(double v, double *sh) { return wg_across(wave_sum(v), sh, WgAdd()); }
__device__ inline uint32_t wg_count(uint32_t v, uint32_t *sh) { return wg_across(wave_all(v, WgAdd()), sh, WgAdd()); }
__device__ inline double wg_min(double v, double *sh) { return wg_across(wave_all(v, WgMin()), sh, WgMin()); }
__device__ inline double wg_max(double v, double *sh) { return wg_across(wave_all(v, WgMax()), sh, WgMax()); }
// the least of the workgroup's indices
__device__ inline int wg_least(int v, int *sh) { return wg_across(wave_all(v, WgMin()), sh, WgMin()); }

// the log-sum-exp pair (m, s) over the workgroup (lse_merge of mp_math.hpp)
__device__ inline void wg_lse(double &m, double &s, double *shm, double *shs) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    wave_lse(m, s);
    if (lane == 0) { shm[wave] = m; shs[wave] = s; }
    __syncthreads();
    m = shm[0];
    s = shs[0];
#pragma unroll
    for (int w = 1; w < kWgWaves; ++w) lse_merge(m, s, shm[w], shs[w]);
    __syncthreads();
}

// A candidate for a maximum: value and index, under the total order "larger value, then lower index" (i = INT_MAX: none).
struct WgBest {
    double v;
    int i;
};
__device__ inline bool wg_better(double av, int ai, double bv, int bi) { return av > bv || (av == bv && ai < bi); }

// the best of the workgroup's candidates
__device__ inline WgBest wg_best(WgBest b, double *shv, int *shi) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double ov = __shfl_xor(b.v, d, 64);
        const int oi = __shfl_xor(b.i, d, 64);
        if (wg_better(ov, oi, b.v, b.i)) { b.v = ov; b.i = oi; }
    }
    if (lane == 0) { shv[wave] = b.v; shi[wave] = b.i; }
    __syncthreads();
    WgBest r{shv[0], shi[0]};
#pragma unroll
    for (int w = 1; w < kWgWaves; ++w)
        if (wg_better(shv[w], shi[w], r.v, r.i)) { r.v = shv[w]; r.i = shi[w]; }
    __syncthreads();
    return r;
}

// Inclusive sum over the workgroup's 256 threads (one value each, a 32- or 64-bit count); every thread gets its own prefix.
// sh[kWgWaves] is scratch.
template <class T>
__device__ inline T wg_inclusive_scan(T v, T *sh) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T u = __shfl_up(v, d, 64);
        if (lane >= d) v += u;
    }
    if (lane == 63) sh[wave] = v;
    __syncthreads();
    T before = 0;
    for (int w = 0; w < wave; ++w) before += sh[w];
    __syncthreads();
    return v + before;
}

// The packing step of a whole wavefront: the lanes with `keep` take consecutive slots from *cursor (LDS, advanced once per
// wavefront) in lane order; returns the calling lane's slot (of use where keep).  No barrier: the caller's loop ends with one.
__device__ inline uint32_t wave_pack_slot(bool keep, uint32_t *cursor) {
    const int lane = threadIdx.x & 63;
    const uint64_t act = __ballot(keep);
    uint32_t at = 0;
    if (lane == 0 && act) at = atomicAdd(cursor, (uint32_t)__popcll(act));
    at = __shfl(at, 0, 64);
    return at + (uint32_t)__popcll(act & ((1ull << lane) - 1ull));
}

// LDS of the select: the histograms and the words one thread hands to all
struct WgSelectLds {
    uint32_t hist[kWgWaves * 256];   // one histogram of a digit per wavefront
    uint32_t count;                  // cursor of the caller's packing step
    uint32_t digit, rank;            // of a pass: the digit that holds rank r, and r's rank inside it
    uint32_t spare;                  // the caller's
    uint32_t wave[kWgWaves];         // scratch of the scan; the caller's between selects
};

// The key of rank r (0-based, ascending) among the candidates of elements 0 .. n): key(i, k) says whether element i is one and
// sets k to its 64-bit key.  MSB-first over 8-bit digits; every thread returns the key.  Equal keys are one value, so ties need
// no rule; what orders -0.0, +0.0 and NaNs is the caller's key.
template <class Key>
__device__ uint64_t wg_radix_select(int n, uint32_t r, WgSelectLds &s, Key key) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t *my_hist = s.hist + wave * 256;
    uint64_t prefix = 0, mask = 0;
    for (int shift = 56; shift >= 0; shift -= 8) {
        for (int i = threadIdx.x; i < kWgWaves * 256; i += kWgThreads) s.hist[i] = 0;
        __syncthreads();
        for (int base = wave * 64; base < n; base += kWgThreads) {
            const int i = base + lane;
            uint64_t k = 0;
            const bool cand = i < n && key(i, k);
            const bool take = cand & ((k & mask) == prefix);   // (& : the compare is not worth a branch round it)
            const uint32_t bin = (uint32_t)(k >> shift) & 255u;
            const uint64_t act = __ballot(take);
            if (act == 0) continue;
            // neighbouring elements share their leading digits: a wavefront whose candidates all fall into one bin adds once
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
        for (int w = 0; w < kWgWaves; ++w) c += s.hist[w * 256 + threadIdx.x];
        const uint32_t incl = wg_inclusive_scan(c, s.wave);
        const uint32_t excl = incl - c;
        if (excl <= r && r < incl) {
            s.digit = threadIdx.x;
            s.rank = r - excl;
        }
        __syncthreads();
        prefix |= (uint64_t)s.digit << shift;
        mask |= (uint64_t)255 << shift;
        r = s.rank;
        __syncthreads();
    }
    return prefix;
}

// LDS of the weighted select: 64-bit sums of units where the select above counts candidates (three rows of 2^31 units already
// overflow 32 bits)
struct WgWSelectLds {
    unsigned long long hist[kWgWaves * 256];   // one histogram of a digit per wavefront: the units of the candidates in each bin
    unsigned long long target;                 // of a pass: the target inside the digit taken
    unsigned long long wave[kWgWaves];         // scratch of the scan; the caller's between selects
    uint32_t digit;                            // of a pass: the digit taken
    uint32_t pad;
};

// The least key whose cumulative units, over the candidates of elements 0 .. n) with keys <= it, reach t (1 <= t <= the units of
// all candidates): key(i, k, u) says whether element i is a candidate and sets k to its 64-bit key and u to its units (0: the
// element is there and weighs nothing).  The walk of wg_radix_select over sums of units: per digit the bin with excl < t <= incl
// is taken and t becomes t - excl, so the key returned always belongs to a candidate with units.  Every thread returns the key.
template <class Key>
__device__ uint64_t wg_wradix_select(int n, uint64_t t, WgWSelectLds &s, Key key) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long *my_hist = s.hist + wave * 256;
    uint64_t prefix = 0, mask = 0;
    for (int shift = 56; shift >= 0; shift -= 8) {
        for (int i = threadIdx.x; i < kWgWaves * 256; i += kWgThreads) s.hist[i] = 0;
        __syncthreads();
        // As above, a wavefront whose takers all fall into one bin adds once -- but a sum of units is a butterfly where a count is
        // a popcount, so the lanes keep their own sums for as long as that bin stays the same (held: the bin, or -1; the same in
        // every lane) and the butterfly runs when it changes and behind the last element.  Integer sums: the order is free.
        int held = -1;
        unsigned long long mine = 0;
        const auto flush = [&]() {
            if (held < 0) return;
            const unsigned long long sum = wave_all(mine, WgAdd());
            if (lane == 0) atomicAdd(&my_hist[held], sum);
            mine = 0;
        };
        for (int base = wave * 64; base < n; base += kWgThreads) {
            const int i = base + lane;
            uint64_t k = 0;
            uint32_t u = 0;
            const bool cand = i < n && key(i, k, u);
            const bool take = cand & ((k & mask) == prefix);
            const uint32_t bin = (uint32_t)(k >> shift) & 255u;
            const uint64_t act = __ballot(take);
            if (act == 0) continue;
            const uint32_t bin0 = __shfl(bin, __builtin_ctzll(act), 64);
            if ((act & (act - 1)) != 0 && __ballot(take && bin == bin0) == act) {   // (a single taker adds for itself)
                if ((int)bin0 != held) {
                    flush();
                    held = (int)bin0;
                }
                mine += take ? u : 0u;
            } else if (take) {
                atomicAdd(&my_hist[bin], (unsigned long long)u);
            }
        }
        flush();
        __syncthreads();
        unsigned long long c = 0;
#pragma unroll
        for (int w = 0; w < kWgWaves; ++w) c += s.hist[w * 256 + threadIdx.x];
        const unsigned long long incl = wg_inclusive_scan(c, s.wave);
        const unsigned long long excl = incl - c;
        if (excl < t && t <= incl) {
            s.digit = threadIdx.x;
            s.target = t - excl;
        }
        __syncthreads();
        prefix |= (uint64_t)s.digit << shift;
        mask |= (uint64_t)255 << shift;
        t = s.target;
        __syncthreads();
    }
    return prefix;
}

}  // namespace mp
