// mp_probe_post.hip — test infrastructure only: the posterior monitor of the sampler, its host unit (PostMonitor, mp_monitor.cpp)
// and its kernels (post_hist1_kernel, post_hist2_kernel, post_moments_kernel, post_best_kernel, post_reset_kernel; mp_post.hip),
// behind one extern "C" host function over HOST buffers (tests/test_gpu_post_kernels.py, cases of tests/post_cases.py).  Builds
// into its own libmp_probe_post.so, linked from the very objects libmagprop_amd.so is linked from (build/all/mp_monitor.cpp.o and
// the kernel objects it calls into): the host functions and the kernels reached here are the product's compiled code.  Nothing
// here is part of libmagprop_amd.so, of include/magprop_amd.h or of the product's ABI.
//
// mpq_run_posterior runs the product's PostMonitor::make, restart and feed, the functions behind mp_sampler_set_posterior and
// mp_sampler_run, with the chunks in the caller's hands, and returns the accumulators as the device holds them (mp_post.h states
// the layout).  It returns 0, a hipError_t, or -1 for arguments it refuses; nothing is allocated or launched then.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>

#include "mp_monitor.h"
#include "mp_probe_bufs.h"

// The monitor reports through fail(), which mp_capi.cpp defines in the product: here the code is all there is to keep
int fail(int code, const char *, ...) { return code; }

namespace mp {

namespace {

// the probe's own caps
constexpr int kMaxRows = 1 << 17;           // steps of a call
constexpr int kMaxChunks = 1 << 17;
constexpr int kMaxElements = 1 << 22;       // rows * n_total * ndim

// a return code of the monitor as this probe returns it: a hipError_t where a HIP call failed, -1 for a refusal
int probe_rc(int rc) {
    if (rc != MP_EHIP) return rc ? -1 : 0;
    const hipError_t e = hipGetLastError();
    return (int)(e != hipSuccess ? e : hipErrorUnknown);
}

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
// of one row of junk (NaN coordinates, +inf lnprob), its rows and one more row of junk, and fed as 1 + chunk_rows[i] rows to a
// monitor that has one step left to pass over.
// hist1[n_ensembles][ndim][bins1 + 3], hist2[n_ensembles][npairs][bins2^2], outside2[n_ensembles][npairs],
// mom[n_entries][n_total], nfin[n_total], best_x[n_ensembles][ndim], best_lnp, best_idx[n_ensembles] go into the monitor's own
// buffers before restart() and come back as the device holds them behind the last launch (restart() leaves nothing of what they
// held); hist2 and outside2 may be NULL where bins2 = 0 or ndim = 1.
int mpq_run_posterior(const double *chain, const double *lnp, int n, int n_walkers, int n_ensembles, int ndim, int bins1, int bins2,
                      const double *lower, const double *upper, int n_chunks, const int32_t *chunk_rows, int64_t *hist1,
                      int64_t *hist2, int64_t *outside2, double *mom, int64_t *nfin, double *best_x, double *best_lnp,
                      int64_t *best_idx) {
    if (!chain || !lnp || !lower || !upper || !chunk_rows || !hist1 || !mom || !nfin || !best_x || !best_lnp || !best_idx) return -1;
    if (n_walkers < 2 || (n_walkers & 1) || n_ensembles < 1 || ndim < 1 || ndim > MP_MAX_NDIM) return -1;   // (mp_sampler_create)
    if (bins1 < 1) return -1;   // (0 turns the sampler's monitor off; PostMonitor::make below checks the other settings)
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

    std::unique_ptr<PostMonitor> m;
    int rc = PostMonitor::make("mpq_run_posterior", n_walkers, n_ensembles, ndim, bins1, bins2, lower, upper, 0, (size_t)longest + 1, &m);
    if (rc) return probe_rc(rc);
    const size_t row = (size_t)row64, nt = (size_t)n_walkers * n_ensembles, ne = (size_t)n_ensembles, nd = (size_t)ndim;
    // junk around a chunk: a NaN coordinate would be counted as non-finite, a +inf lnprob would win
    const double junk = std::numeric_limits<double>::quiet_NaN(), junk_lnp = std::numeric_limits<double>::infinity();
    std::vector<double> slab((size_t)(longest + 2) * row, junk), slab_lnp((size_t)(longest + 2) * nt, junk_lnp);
    Bufs B;
    double *d_slab = const_cast<double *>(B.in(slab.data(), slab.size()));
    double *d_lnp = const_cast<double *>(B.in(slab_lnp.data(), slab_lnp.size()));
    // the caller's bytes into every accumulator of the monitor: whatever restart() leaves of them comes back
    B.adopt(hist1, m->hist1.p, ne * nd * post_stride1(bins1));
    if (two) {
        B.adopt(hist2, m->hist2.p, ne * np * (size_t)bins2 * bins2);
        B.adopt(outside2, m->outside2.p, ne * np);
    }
    B.adopt(mom, m->mom.p, (size_t)nent * nt);
    B.adopt(nfin, m->nfin.p, nt);
    B.adopt(best_x, m->best_x.p, ne * nd);
    B.adopt(best_lnp, m->best_lnp.p, ne);
    B.adopt(best_idx, m->best_idx.p, ne);
    if (!B.ready()) return B.finish(0);
    rc = m->restart(nullptr);
    const double *src = chain, *src_lnp = lnp;
    for (int i = 0; i < n_chunks && rc == 0; ++i) {
        // the slab of this chunk (the copies wait for the kernels that read the slab before them); its junk row in front is the
        // step that feed() passes over
        const int rows = chunk_rows[i];
        std::fill(slab.begin(), slab.end(), junk);
        std::fill(slab_lnp.begin(), slab_lnp.end(), junk_lnp);
        std::copy(src, src + (size_t)rows * row, slab.begin() + row);
        std::copy(src_lnp, src_lnp + (size_t)rows * nt, slab_lnp.begin() + nt);
        src += (size_t)rows * row;
        src_lnp += (size_t)rows * nt;
        if (hipMemcpy(d_slab, slab.data(), (size_t)(rows + 2) * row * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(d_lnp, slab_lnp.data(), (size_t)(rows + 2) * nt * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
            rc = MP_EHIP;
            break;
        }
        m->skip = 1;
        rc = m->feed(ChainRows{d_slab, d_lnp, rows + 1, 0, 0}, nullptr);
    }
    return B.finish(probe_rc(rc));
}

}  // extern "C"
