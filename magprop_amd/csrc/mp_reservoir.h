// mp_reservoir.h — the sample reservoir of the ensemble sampler (include/magprop_amd.h mp_sampler_set_reservoir): what
// mp_monitor.cpp passes to the two kernels of mp_reservoir.hip, and the rule in words.
//
// The rule.  Every sample (absolute step t of the sampler, walker w of ensemble e) of the monitored steps has the 64-bit key
//     key = (r[0] << 32) | r[1],   r = philox4x32_10(seed_lo, seed_hi, t_lo32, t_hi32, e * n_walkers + w, kResCtr)
// with the monitor's own seed.  The reservoir of size K of ensemble e holds the K samples that are least in the total order
// (key, t, w), all of them while fewer than K were seen.  The keys are independent of the state and of each other, so the held
// set is a uniform random K-subset, without replacement, of the monitored samples; it is a function of the samples alone, not of
// chunks, slices or of how a run was split into calls; and the bottom K of a union is the bottom K of the parts' bottom K, so
// the reservoirs of two runs merge on the host (magprop_amd/reservoir.py).
//
// kResCtr differs from every fourth counter word c3 in use: 0 .. 3 (stretch, DE and snooker draws), kKdeCtr = 0x4B00 .. 0x4B00 +
// MP_MAX_NDIM (KDE move), kSliceMoveCtr = 0x51C00000 .. + 0xFF (slice move), 0x5117 (random splits), 0x30FE (move draw), the
// optimizer's 0xDE00 .. 0xDEFF, the nested sampler's kNestCtr = 0x4E000000 .. and kSliceCtr = 0x4E400000 .. (both below
// 0x4F000000), and the SMC sampler's kSmcCtr = 0x534D0000 .. + 2 MP_SMC_MAX_WALKS + 2.
//
// The device state, per ensemble: the held entries in slots 0 .. n_held) in no particular order (key, step, walker, x[ndim],
// lnprob); the threshold, which is the held set's largest (key, t, w) once a merge has cut the set down to K and "everything
// passes" before that; and a candidate list of cand_cap entries (key, t, w) with its cursor.
// res_filter_kernel forms the key of every sample of a slice of a chunk (arithmetic only: no chain row is read) and appends
// those not above the threshold to the ensemble's candidate list, in free order.  res_merge_kernel, one workgroup per ensemble
// behind it, finds the key of rank K - 1 over held and candidates (wg_radix_select; skipped while the union has <= K members),
// resolves ties at that key by (t, w) ascending, evicts the held entries beyond the cut, copies every winning candidate's row
// and lnprob from the chunk's slab into a freed slot, and writes the new threshold, n_held and n_seen.  A slice holds at most
// cand_cap samples per ensemble (the host slices a chunk into whole steps), so the list cannot overflow.
#pragma once
#include <stdint.h>

namespace mp {

constexpr uint32_t kResCtr = 0x52455300u;   // fourth counter word of the keys ('RES\0')
constexpr int kResCandCap = 32768;          // candidates per ensemble and slice; an ensemble of more walkers gets n_walkers
// int64 words of an ensemble's entry in ResArgs::meta
enum { kResThrKey = 0, kResThrStep, kResThrWalker, kResFull, kResHeld, kResSeen, kResMeta };

struct ResArgs {
    const double *chain;     // [rows of the chunk][n_total][ndim] the chunk's slab (merge only)
    const double *lnp;       // [rows of the chunk][n_total]
    uint64_t *key;           // [n_ensembles][size] the held entries
    int64_t *step;           // [n_ensembles][size]
    int32_t *walker;         // [n_ensembles][size]
    double *x;               // [n_ensembles][size][ndim]
    double *held_lnp;        // [n_ensembles][size]
    int64_t *meta;           // [n_ensembles][kResMeta] threshold (key's bits, t, w), full, n_held, n_seen
    uint64_t *cand_key;      // [n_ensembles][cand_cap] the candidates of the slice
    int64_t *cand_step;      // [n_ensembles][cand_cap]
    int32_t *cand_walker;    // [n_ensembles][cand_cap]
    uint32_t *n_cand;        // [n_ensembles] the lists' cursors; the merge leaves them at 0
    int32_t *evicted;        // [n_ensembles][cand_cap] scratch of the merge: the slots it frees
    uint64_t seed;
    int64_t t0;              // the absolute step of the slice's first row
    int32_t n_walkers, n_ensembles, n_total, ndim;
    int32_t size, cand_cap;
    int32_t row0, rows;      // rows [row0, row0 + rows) of the slab are the slice; rows * n_walkers <= cand_cap
};

// elementwise over the slice's (step, walker, ensemble) triples; return hipError_t as int
int launch_res_filter(const ResArgs &a, void *stream);
// one workgroup per ensemble
int launch_res_merge(const ResArgs &a, void *stream);

}  // namespace mp
