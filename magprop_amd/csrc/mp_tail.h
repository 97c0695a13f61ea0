// mp_tail.h — the Pareto tail of one column, what the select kernels of mp_model_pointwise and mp_model_reweight share
// (mp_pointwise.hip, mp_reweight.hip): the cut and the sorted tail row of the candidates of a column, by one workgroup of mp_wg.h.
// Device only: included from .hip sources.
#pragma once
#include "mp_band.h"
#include "mp_pointwise.h"
#include "mp_wg.h"

namespace mp {

// key(i, k) says whether element i of 0 .. n) is a candidate and sets k to its band_key (mp_band.h; the column is streamed
// from memory once per digit of the select: it does not fit LDS at 262 144 samples).  With m candidates, tm = min(T(m), m):
// *cut becomes the tm-th largest value (NaN for m = 0) and tail[0 .. tail_stride), unless nullptr, the tm largest values
// ascending, then NaN.  The larger values are compacted into keys[kPointwiseSortCap] (LDS), filled up with copies of the cut
// and sorted (bitonic).  Called by all 256 threads.
template <class Key>
__device__ inline void wg_tail_select(int n, WgSelectLds &sel, uint64_t *keys, double *cut, double *tail, int tail_stride, Key key) {
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    uint32_t c = 0;
    for (int i = tid; i < n; i += kPointwiseThreads) {
        uint64_t k;
        c += key(i, k);
    }
    const int m = (int)wg_count(c, sel.wave);
    const int tm = min(min(pointwise_tail_len(m), m), kPointwiseMaxTail);   // entries of the tail row (uniform over the workgroup)
    if (m == 0) {
        if (tid == 0) *cut = __builtin_nan("");
        if (tail)
            for (int i = tid; i < tail_stride; i += kPointwiseThreads) tail[i] = __builtin_nan("");
        return;
    }
    // the key of rank m - tm among the candidates' keys
    const uint64_t kc = wg_radix_select(n, (uint32_t)(m - tm), sel, key);
    if (tid == 0) {
        sel.count = 0;
        *cut = band_value(kc);
    }
    __syncthreads();
    // the values above the cut, packed (in no particular order: they are sorted below); fewer than tm by the choice of the cut
    for (int base = wave * 64; base < n; base += kPointwiseThreads) {
        const int i = base + lane;
        uint64_t k = 0;
        const bool keep = i < n && key(i, k) && k > kc;
        const uint32_t slot = wave_pack_slot(keep, &sel.count);
        if (keep && slot < (uint32_t)tm) keys[slot] = k;
    }
    __syncthreads();
    const int above = min((int)sel.count, tm);
    int slots = 1;                                          // the power of two that holds the tm entries
    while (slots < tm) slots <<= 1;
    for (int i = above + tid; i < slots; i += kPointwiseThreads) keys[i] = i < tm ? kc : ~0ull;   // copies of the cut, then padding that sorts last
    __syncthreads();
    for (int k = 2; k <= slots; k <<= 1)
        for (int d = k >> 1; d > 0; d >>= 1) {
            for (int i = tid; i < slots; i += kPointwiseThreads) {
                const int l = i ^ d;
                if (l > i) {
                    const uint64_t x = keys[i], y = keys[l];
                    if (((i & k) == 0) ? x > y : x < y) { keys[i] = y; keys[l] = x; }
                }
            }
            __syncthreads();
        }
    if (tail)
        for (int i = tid; i < tail_stride; i += kPointwiseThreads) tail[i] = i < tm ? band_value(keys[i]) : __builtin_nan("");
}

}  // namespace mp
