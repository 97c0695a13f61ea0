// mp_reservoir.hip — gfx950 kernels of the sampler's sample reservoir (mp_reservoir.h states the rule and the device state).
//
// res_filter_kernel: one thread per (step, walker) of a slice of a chunk, kWgThreads of them per workgroup, the workgroups of one
// ensemble side by side.  A thread forms its sample's key (ten Philox rounds; no memory is read but the ensemble's threshold) and,
// where (key, t, w) is not above the threshold, takes a slot of the ensemble's candidate list: one atomic add per wavefront on the
// list's cursor (wave_pack_slot of mp_wg.h).  Once a reservoir of K is full and m samples were seen, a sample passes with
// probability about K / m, so this kernel is what the monitor costs in the long run.
// res_merge_kernel: one workgroup per ensemble.  No candidate: n_seen moves on and nothing else happens.  Otherwise the cut
// (key, t, w) of rank K - 1 over held and candidates where there are more than K of them: the key by wg_radix_select; where
// more than one entry has that key, t and then w by two more selects among the tied entries (pairs (t, w) are distinct inside an
// ensemble).  Held entries above the cut give up their slots, candidates not above it take those and then the slots behind
// n_held; the order of the slots is free.  Global memory the workgroup wrote is read again only behind a barrier.
#include <hip/hip_runtime.h>

#include "mp_device.h"
#include "mp_reservoir.h"
#include "mp_wg.h"

namespace mp {

namespace {

// (k, t, w) <= (ck, ct, cw) in the order key, then step, then walker
__device__ inline bool res_not_above(uint64_t k, int64_t t, int32_t w, uint64_t ck, int64_t ct, int32_t cw) {
    return k < ck || (k == ck && (t < ct || (t == ct && w <= cw)));
}

__global__ __launch_bounds__(kWgThreads) void res_filter_kernel(const ResArgs a, int blocks_per_ensemble) {
    const int e = (int)(blockIdx.x / (unsigned)blocks_per_ensemble);
    const int i = (int)(blockIdx.x % (unsigned)blocks_per_ensemble) * kWgThreads + (int)threadIdx.x;
    const bool in = i < a.rows * a.n_walkers;
    const int r = i / a.n_walkers, w = i - r * a.n_walkers;
    const int64_t t = a.t0 + r;
    const int64_t *meta = a.meta + (size_t)e * kResMeta;
    uint32_t p[4];
    philox4x32_10((uint32_t)a.seed, (uint32_t)(a.seed >> 32), (uint32_t)(uint64_t)t, (uint32_t)((uint64_t)t >> 32),
                  (uint32_t)(e * a.n_walkers + w), kResCtr, p);
    const uint64_t key = ((uint64_t)p[0] << 32) | p[1];
    const bool pass = in && (meta[kResFull] == 0 ||
                             res_not_above(key, t, w, (uint64_t)meta[kResThrKey], meta[kResThrStep], (int32_t)meta[kResThrWalker]));
    const uint32_t slot = wave_pack_slot(pass, a.n_cand + e);
    if (pass && slot < (uint32_t)a.cand_cap) {
        const size_t at = (size_t)e * a.cand_cap + slot;
        a.cand_key[at] = key;
        a.cand_step[at] = t;
        a.cand_walker[at] = w;
    }
}

__global__ __launch_bounds__(kWgThreads) void res_merge_kernel(const ResArgs a) {
    const int e = (int)blockIdx.x, tid = (int)threadIdx.x, K = a.size, cap = a.cand_cap;
    __shared__ WgSelectLds s;
    __shared__ int64_t tie_step;
    __shared__ int32_t tie_walker;
    int64_t *meta = a.meta + (size_t)e * kResMeta;
    uint64_t *hkey = a.key + (size_t)e * K;
    int64_t *hstep = a.step + (size_t)e * K;
    int32_t *hwalker = a.walker + (size_t)e * K;
    const uint64_t *ckey = a.cand_key + (size_t)e * cap;
    const int64_t *cstep = a.cand_step + (size_t)e * cap;
    const int32_t *cwalker = a.cand_walker + (size_t)e * cap;
    int32_t *evicted = a.evicted + (size_t)e * cap;
    const int H = (int)meta[kResHeld], M = (int)min(a.n_cand[e], (uint32_t)cap), total = H + M;
    const int64_t seen = meta[kResSeen] + (int64_t)a.rows * a.n_walkers;
    if (M == 0) {   // (the same in every thread)
        if (tid == 0) meta[kResSeen] = seen;
        return;
    }
    const auto key_of = [&](int i) { return i < H ? hkey[i] : ckey[i - H]; };
    const auto step_of = [&](int i) { return i < H ? hstep[i] : cstep[i - H]; };
    const auto walker_of = [&](int i) { return i < H ? hwalker[i] : cwalker[i - H]; };
    const bool select = total > K;
    uint64_t cut = 0;
    int64_t cut_t = 0;
    int32_t cut_w = 0;
    if (select) {
        cut = wg_radix_select(total, (uint32_t)(K - 1), s, [&](int i, uint64_t &k) {
            k = key_of(i);
            return true;
        });
        uint32_t less = 0, equal = 0;
        for (int i = tid; i < total; i += kWgThreads) {
            const uint64_t k = key_of(i);
            less += k < cut;
            if (k == cut) {
                ++equal;
                tie_step = step_of(i);   // (of use where one entry has the key: then one thread writes)
                tie_walker = walker_of(i);
            }
        }
        const uint32_t n_less = wg_count(less, s.wave), n_equal = wg_count(equal, s.wave);
        const uint32_t take = (uint32_t)K - n_less;   // of the n_equal tied entries, 1 <= take <= n_equal
        if (n_equal == 1) {
            cut_t = tie_step;
            cut_w = tie_walker;
        } else {
            cut_t = (int64_t)wg_radix_select(total, take - 1u, s, [&](int i, uint64_t &k) {
                k = (uint64_t)step_of(i);
                return key_of(i) == cut;
            });
            uint32_t before = 0;
            for (int i = tid; i < total; i += kWgThreads) before += key_of(i) == cut && step_of(i) < cut_t;
            const uint32_t n_before = wg_count(before, s.wave);
            cut_w = (int32_t)wg_radix_select(total, take - 1u - n_before, s, [&](int i, uint64_t &k) {
                k = (uint64_t)(uint32_t)walker_of(i);
                return key_of(i) == cut && step_of(i) == cut_t;
            });
        }
    }
    if (tid == 0) {
        s.count = 0;   // slots freed
        s.spare = 0;   // candidates placed
    }
    __syncthreads();
    if (select)
        for (int base = 0; base < H; base += kWgThreads) {
            const int i = base + tid;
            const bool out = i < H && !res_not_above(hkey[i], hstep[i], hwalker[i], cut, cut_t, cut_w);
            const uint32_t at = wave_pack_slot(out, &s.count);
            if (out && at < (uint32_t)cap) evicted[at] = i;
        }
    __syncthreads();
    const uint32_t n_evicted = s.count;
    for (int base = 0; base < M; base += kWgThreads) {
        const int j = base + tid;
        const bool win = j < M && (!select || res_not_above(ckey[j], cstep[j], cwalker[j], cut, cut_t, cut_w));
        const uint32_t q = wave_pack_slot(win, &s.spare);
        if (!win) continue;
        const int dst = q < n_evicted ? evicted[q] : H + (int)(q - n_evicted);
        if (dst < 0 || dst >= K) continue;   // (cannot happen: winners = evicted + free slots)
        const int64_t t = cstep[j];
        const int32_t w = cwalker[j];
        const size_t src = (size_t)(a.row0 + (int)(t - a.t0)) * a.n_total + (size_t)e * a.n_walkers + w;
        hkey[dst] = ckey[j];
        hstep[dst] = t;
        hwalker[dst] = w;
        a.held_lnp[(size_t)e * K + dst] = a.lnp[src];
        double *x = a.x + ((size_t)e * K + dst) * a.ndim;
        for (int d = 0; d < a.ndim; ++d) x[d] = a.chain[src * a.ndim + d];
    }
    if (tid == 0) {
        meta[kResSeen] = seen;
        meta[kResHeld] = select ? K : total;
        if (select) {
            meta[kResThrKey] = (int64_t)cut;
            meta[kResThrStep] = cut_t;
            meta[kResThrWalker] = cut_w;
            meta[kResFull] = 1;
        }
        a.n_cand[e] = 0;
    }
}

}  // namespace

int launch_res_filter(const ResArgs &a, void *stream) {
    if (a.n_ensembles <= 0 || a.rows <= 0) return 0;
    const int bpe = (a.rows * a.n_walkers + kWgThreads - 1) / kWgThreads;
    hipLaunchKernelGGL(res_filter_kernel, dim3((unsigned)a.n_ensembles * (unsigned)bpe), dim3(kWgThreads), 0, (hipStream_t)stream, a, bpe);
    return (int)hipGetLastError();
}

int launch_res_merge(const ResArgs &a, void *stream) {
    if (a.n_ensembles <= 0 || a.rows <= 0) return 0;
    hipLaunchKernelGGL(res_merge_kernel, dim3((unsigned)a.n_ensembles), dim3(kWgThreads), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

}  // namespace mp
