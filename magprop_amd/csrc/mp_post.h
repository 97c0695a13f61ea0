// mp_post.h — the posterior monitor of the device-resident ensemble sampler (mp_sampler_set_posterior, include/magprop_amd.h
// states the definition): launch arguments and accumulator layout of the gfx950 kernels in mp_post.hip.
//
// A chunk is `rows` rows of the sampler's device slab, chain[.][n_total][ndim] and lnp[.][n_total]; row first + r is monitored
// step n0 + r.  Every counter is an int64 in global memory.  Of one ensemble, in this order:
//   hist1[ndim][bins1 + 3]     the bins of a dimension, then its below, above and non-finite counts
//   hist2[npairs][bins2^2]     pair p = (a, b), a < b, in lexicographic order; bin ba * bins2 + bb
//   outside2[npairs]
// The moments are per-walker running sums mom[n_entries][n_total]: entry d < ndim is s1[d], the entries behind them are s2[a][b]
// for a <= b in lexicographic order; nfin[n_total] counts the walker's samples whose coordinates are all finite.
#pragma once
#include <stdint.h>

#include "../../include/magprop_amd.h"

namespace mp {

constexpr int kPostThreads = 256;       // workgroup of the histogram and moment kernels (4 wavefronts)
constexpr int kPostBestThreads = 1024;  // workgroup of the best-sample kernel: one per ensemble
constexpr int kPostLdsBytes = 65536;    // most LDS one workgroup takes for its private histogram
constexpr int kPostMaxSlices = 64;      // most workgroups that share the rows of a chunk (per ensemble and group / pair)
constexpr int kPostSliceSamples = 8192; // samples (row, walker) of a chunk per such workgroup before another one is added

inline int post_n_pairs(int ndim) { return ndim * (ndim - 1) / 2; }
inline int post_n_entries(int ndim) { return ndim + ndim * (ndim + 1) / 2; }
inline int post_stride1(int bins1) { return bins1 + 3; }

// par[5][ndim]: lower, upper, inv1, inv2, pivot, formed once in double as the header states
inline void post_params(double *par, int ndim, int bins1, int bins2, const double *lower, const double *upper) {
    for (int d = 0; d < ndim; ++d) {
        const double w = upper[d] - lower[d];
        par[d] = lower[d];
        par[ndim + d] = upper[d];
        par[2 * ndim + d] = (double)bins1 / w;
        par[3 * ndim + d] = (double)bins2 / w;
        par[4 * ndim + d] = lower[d] + 0.5 * w;
    }
}

struct PostArgs {
    const double *chain;   // [.][n_total][ndim] the chunk's rows of the sampler's device slab
    const double *lnp;     // [.][n_total]
    const double *par;     // [5][ndim] (post_params)
    int64_t *hist1;        // [n_ensembles][ndim][bins1 + 3]
    int64_t *hist2;        // [n_ensembles][npairs][bins2 * bins2]   (bins2 > 0)
    int64_t *outside2;     // [n_ensembles][npairs]
    double *mom;           // [n_entries][n_total]
    int64_t *nfin;         // [n_total]
    double *best_x;        // [n_ensembles][ndim]
    double *best_lnp;      // [n_ensembles]
    int64_t *best_idx;     // [n_ensembles]
    int32_t n_walkers, n_ensembles, n_total, ndim;
    int32_t bins1, bins2;
    int32_t first, rows;   // rows [first, first + rows) of the slab are monitored steps n0 .. n0 + rows - 1
    int64_t n0;            // steps accumulated so far
};

// implemented in mp_post.hip; return hipError_t as int
//   the best-sample holder of every ensemble to "none" (index -1, lnprob -inf, position NaN); the caller zeroes the rest
int launch_post_reset(const PostArgs &a, void *stream);
//   the chunk's rows into every accumulator
int launch_post_accumulate(const PostArgs &a, void *stream);

}  // namespace mp
