// mp_probe_post.hip — test infrastructure only: the kernels of the posterior monitor (post_hist1_kernel, post_hist2_kernel,
// post_moments_kernel, post_best_kernel, post_reset_kernel; mp_post.hip) behind one extern "C" host function over HOST buffers
// (tests/test_gpu_post_kernels.py, cases of tests/post_cases.py).  Builds into its own libmp_probe_post.so, linked from the very
// object libmagprop_amd.so is linked from (build/all/mp_post.hip.o): the kernels reached here are the product's compiled code,
// through the product's launchers launch_post_reset and launch_post_accumulate.  Nothing here is part of libmagprop_amd.so, of
// include/magprop_amd.h or of the product's ABI.
//
// mpq_run_posterior does what post_restart and post_feed of mp_sampler.cpp do, with the chunks in the caller's hands, and
// returns the accumulators as the device holds them (mp_post.h states the layout).  It returns 0, a hipError_t, or -1 for
// arguments it refuses; nothing is launched then.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>

#include "mp_post.h"
#include "mp_probe_bufs.h"

namespace mp {

namespace {

// the probe's own caps
constexpr int kMaxRows = 1 << 17;           // steps of a call
constexpr int kMaxChunks = 1 << 17;
constexpr int kMaxElements = 1 << 22;       // rows * n_total * ndim

}  // namespace

}  // namespace mp

using namespace mp;

extern "C" {

int mpq_threads(void) { return kPostThreads; }
int mpq_max_bins(void) { return MP_POST_MAX_BINS; }
int mpq_max_bins2(void) { return MP_POST_MAX_BINS2; }
int mpq_max_ndim(void) { return MP_MAX_NDIM; }
int mpq_max_rows(void) { return kMaxRows; }
int mpq_max_elements(void) { return kMaxElements; }

// The steps chain[n][n_total][ndim] with lnp[n][n_total] (n_total = n_ensembles * n_walkers) through a monitor of bins1 / bins2
// bins over [lower, upper), in n_chunks chunks of chunk_rows[i] steps (summing to n; 0 allowed).  Chunk i is uploaded as a slab
// of one row of junk (NaN coordinates, +inf lnprob), its rows and one more row of junk, and accumulated with first = 1.
// hist1[n_ensembles][ndim][bins1 + 3], hist2[n_ensembles][npairs][bins2^2], outside2[n_ensembles][npairs],
// mom[n_entries][n_total], nfin[n_total], best_x[n_ensembles][ndim], best_lnp, best_idx[n_ensembles] come back as the device
// holds them (what they held is ignored); hist2 and outside2 may be NULL where bins2 = 0 or ndim = 1.
int mpq_run_posterior(const double *chain, const double *lnp, int n, int n_walkers, int n_ensembles, int ndim, int bins1, int bins2,
                      const double *lower, const double *upper, int n_chunks, const int32_t *chunk_rows, int64_t *hist1,
                      int64_t *hist2, int64_t *outside2, double *mom, int64_t *nfin, double *best_x, double *best_lnp,
                      int64_t *best_idx) {
    if (!chain || !lnp || !lower || !upper || !chunk_rows || !hist1 || !mom || !nfin || !best_x || !best_lnp || !best_idx) return -1;
    if (n_walkers < 2 || (n_walkers & 1) || n_ensembles < 1 || ndim < 1 || ndim > MP_MAX_NDIM) return -1;   // (mp_sampler_create)
    if (bins1 < 1 || bins1 > MP_POST_MAX_BINS || bins2 < 0 || bins2 > MP_POST_MAX_BINS2) return -1;          // (mp_sampler_set_posterior)
    for (int d = 0; d < ndim; ++d)
        if (!std::isfinite(lower[d]) || !std::isfinite(upper[d]) || !(lower[d] < upper[d]) || !std::isfinite(upper[d] - lower[d])) return -1;
    if (n < 1 || n > kMaxRows || n_chunks < 1 || n_chunks > kMaxChunks) return -1;
    if (n_walkers > kMaxElements || n_ensembles > kMaxElements) return -1;
    const int64_t row64 = (int64_t)n_walkers * n_ensembles * ndim;
    if (row64 * ((int64_t)n + 2) > kMaxElements) return -1;
    const int np = post_n_pairs(ndim), nent = post_n_entries(ndim);
    const bool two = bins2 > 0 && np > 0;
    if (two && (!hist2 || !outside2)) return -1;
    int64_t sum = 0;
    int longest = 0;
    for (int i = 0; i < n_chunks; ++i) {
        if (chunk_rows[i] < 0 || chunk_rows[i] > n) return -1;
        sum += chunk_rows[i];
        longest = std::max(longest, chunk_rows[i]);
    }
    if (sum != n) return -1;

    const size_t row = (size_t)row64, nt = (size_t)n_walkers * n_ensembles, ne = (size_t)n_ensembles, nd = (size_t)ndim;
    // junk around a chunk: a NaN coordinate would be counted as non-finite, a +inf lnprob would win
    const double junk = std::numeric_limits<double>::quiet_NaN(), junk_lnp = std::numeric_limits<double>::infinity();
    std::vector<double> slab((size_t)(longest + 2) * row, junk), slab_lnp((size_t)(longest + 2) * nt, junk_lnp), par(5 * nd);
    post_params(par.data(), ndim, bins1, bins2, lower, upper);
    const size_t n_h1 = ne * nd * post_stride1(bins1), n_h2 = two ? ne * np * (size_t)bins2 * bins2 : 0, n_o2 = two ? ne * np : 0;
    Bufs B;
    PostArgs a{};
    double *d_slab = const_cast<double *>(B.in(slab.data(), slab.size()));
    double *d_lnp = const_cast<double *>(B.in(slab_lnp.data(), slab_lnp.size()));
    a.chain = d_slab;
    a.lnp = d_lnp;
    a.par = B.in(par.data(), par.size());
    a.hist1 = B.io(hist1, n_h1);
    a.hist2 = two ? B.io(hist2, n_h2) : nullptr;
    a.outside2 = two ? B.io(outside2, n_o2) : nullptr;
    a.mom = B.io(mom, (size_t)nent * nt);
    a.nfin = B.io(nfin, nt);
    a.best_x = B.io(best_x, ne * nd);
    a.best_lnp = B.io(best_lnp, ne);
    a.best_idx = B.io(best_idx, ne);
    a.n_walkers = n_walkers; a.n_ensembles = n_ensembles; a.n_total = (int32_t)nt; a.ndim = ndim;
    a.bins1 = bins1; a.bins2 = bins2; a.n0 = 0;
    if (!B.ready()) return B.finish(0);
    // post_restart
    hipError_t e = hipMemset(a.hist1, 0, n_h1 * sizeof(int64_t));
    if (e == hipSuccess && two) e = hipMemset(a.hist2, 0, n_h2 * sizeof(int64_t));
    if (e == hipSuccess && two) e = hipMemset(a.outside2, 0, n_o2 * sizeof(int64_t));
    if (e == hipSuccess) e = hipMemset(a.mom, 0, (size_t)nent * nt * sizeof(double));
    if (e == hipSuccess) e = hipMemset(a.nfin, 0, nt * sizeof(int64_t));
    int rc = (int)e;
    if (rc == 0) rc = launch_post_reset(a, nullptr);
    const double *src = chain, *src_lnp = lnp;
    for (int i = 0; i < n_chunks && rc == 0; ++i) {
        // post_feed: the slab of this chunk (the copies wait for the kernels that read the slab before them)
        const int rows = chunk_rows[i];
        std::fill(slab.begin(), slab.end(), junk);
        std::fill(slab_lnp.begin(), slab_lnp.end(), junk_lnp);
        std::copy(src, src + (size_t)rows * row, slab.begin() + row);
        std::copy(src_lnp, src_lnp + (size_t)rows * nt, slab_lnp.begin() + nt);
        src += (size_t)rows * row;
        src_lnp += (size_t)rows * nt;
        rc = (int)hipMemcpy(d_slab, slab.data(), (size_t)(rows + 2) * row * sizeof(double), hipMemcpyHostToDevice);
        if (rc == 0) rc = (int)hipMemcpy(d_lnp, slab_lnp.data(), (size_t)(rows + 2) * nt * sizeof(double), hipMemcpyHostToDevice);
        if (rc) break;
        a.first = 1;
        a.rows = rows;
        rc = launch_post_accumulate(a, nullptr);
        a.n0 += rows;
    }
    return B.finish(rc);
}

}  // extern "C"
