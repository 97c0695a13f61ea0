// mp_probe_reservoir.hip — test infrastructure only: the sample reservoir of the sampler, its host unit (ResMonitor,
// mp_monitor.cpp) and its kernels (res_filter_kernel, res_merge_kernel; mp_reservoir.hip), behind two extern "C" host functions
// over HOST buffers (tests/test_gpu_reservoir_kernels.py, cases of tests/reservoir_cases.py).  Builds into its own
// libmp_probe_reservoir.so, linked from the very objects libmagprop_amd.so is linked from (build/all/mp_monitor.cpp.o and the
// kernel objects it calls into): the host functions and the kernels reached here are the product's compiled code.  Nothing here
// is part of libmagprop_amd.so, of include/magprop_amd.h or of the product's ABI.
//
// mpr_run_reservoir runs the product's ResMonitor::make, restart, feed and read, the functions behind mp_sampler_set_reservoir,
// mp_sampler_run and mp_sampler_get_reservoir, with the chunks in the caller's hands.  mpr_merge launches res_merge_kernel alone
// over held entries and candidates the caller gives, keys included.  Both return 0, a hipError_t, or -1 for arguments they
// refuse; nothing is allocated or launched then.
#include <hip/hip_runtime.h>

#include <algorithm>
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
constexpr int kMaxEnsembles = 1 << 10;

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

int mpr_cand_cap(void) { return kResCandCap; }
int mpr_max_rows(void) { return MP_RESERVOIR_MAX_ROWS; }
int mpr_meta_words(void) { return kResMeta; }

// The steps chain[n][n_total][ndim] with lnp[n][n_total] (n_total = n_ensembles * n_walkers), the first of them the sampler's
// step `step0`, through a monitor of `size` rows with `seed` and `discard`, in n_chunks chunks of chunk_rows[i] steps (summing to
// n; 0 allowed).  Chunk i is uploaded as a slab of one row of junk (NaN coordinates, +inf lnprob), its rows and one more row of
// junk, and fed as 1 + chunk_rows[i] rows to a monitor that has one step more to pass over.  restart_before >= 0: restart() is
// called once more before chunk restart_before, so that what went in before is dropped and `discard` applies again.
// Comes back, per ensemble, what ResMonitor::read gives: x[n_ensembles][size][ndim], lnprob, step, walker, key
// [n_ensembles][size] (the first n_rows[e] entries of an ensemble's block), n_rows, n_seen [n_ensembles].
int mpr_run_reservoir(const double *chain, const double *lnp, int n, int n_walkers, int n_ensembles, int ndim, int size, uint64_t seed,
                      int64_t discard, int64_t step0, int n_chunks, const int32_t *chunk_rows, int restart_before, double *x,
                      double *lnprob, int64_t *step, int32_t *walker, uint64_t *key, int32_t *n_rows, int64_t *n_seen) {
    if (!chain || !lnp || !chunk_rows || !x || !lnprob || !step || !walker || !key || !n_rows || !n_seen) return -1;
    if (n_walkers < 1 || n_ensembles < 1 ||   // (the monitor takes odd ensembles too, the sampler makes none)
 n_ensembles > kMaxEnsembles || ndim < 1 || ndim > MP_MAX_NDIM) return -1;
    if (size < 1) return -1;   // (0 turns the sampler's monitor off; ResMonitor::make below checks the other settings)
    if (n < 1 || n > kMaxRows || n_chunks < 1 || n_chunks > kMaxChunks || step0 < 1 || restart_before >= n_chunks) return -1;
    if (n_walkers > kMaxElements) return -1;
    const int64_t row64 = (int64_t)n_walkers * n_ensembles * ndim;
    if (row64 * ((int64_t)n + 2) > kMaxElements) return -1;
    int64_t sum = 0;
    int longest = 0;
    for (int i = 0; i < n_chunks; ++i) {
        if (chunk_rows[i] < 0 || chunk_rows[i] > n) return -1;
        sum += chunk_rows[i];
        longest = std::max(longest, chunk_rows[i]);
    }
    if (sum != n) return -1;

    std::unique_ptr<ResMonitor> m;
    int rc = ResMonitor::make("mpr_run_reservoir", n_walkers, n_ensembles, ndim, size, seed, discard, (size_t)longest + 1, &m);
    if (rc) return probe_rc(rc);
    const size_t row = (size_t)row64, nt = (size_t)n_walkers * n_ensembles;
    const double junk = std::numeric_limits<double>::quiet_NaN(), junk_lnp = std::numeric_limits<double>::infinity();
    std::vector<double> slab((size_t)(longest + 2) * row, junk), slab_lnp((size_t)(longest + 2) * nt, junk_lnp);
    Bufs B;
    double *d_slab = const_cast<double *>(B.in(slab.data(), slab.size()));
    double *d_lnp = const_cast<double *>(B.in(slab_lnp.data(), slab_lnp.size()));
    if (!B.ready()) return B.finish(0);
    rc = m->restart(nullptr);
    const double *src = chain, *src_lnp = lnp;
    int64_t t = step0;
    for (int i = 0; i < n_chunks && rc == 0; ++i) {
        if (i == restart_before && (rc = m->restart(nullptr))) break;
        const int rows = chunk_rows[i];
        std::fill(slab.begin(), slab.end(), junk);
        std::fill(slab_lnp.begin(), slab_lnp.end(), junk_lnp);
        std::copy(src, src + (size_t)rows * row, slab.begin() + row);
        std::copy(src_lnp, src_lnp + (size_t)rows * nt, slab_lnp.begin() + nt);
        src += (size_t)rows * row;
        src_lnp += (size_t)rows * nt;
        // (the copies wait for the kernels that read the slab before them)
        if (hipMemcpy(d_slab, slab.data(), (size_t)(rows + 2) * row * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(d_lnp, slab_lnp.data(), (size_t)(rows + 2) * nt * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
            rc = MP_EHIP;
            break;
        }
        m->skip += 1;   // the junk row in front, whose step would be t - 1
        rc = m->feed(ChainRows{d_slab, d_lnp, rows + 1, t - 1, 0}, nullptr);
        t += rows;
    }
    for (int e = 0; e < n_ensembles && rc == 0; ++e) {
        if ((rc = m->ready("mpr_run_reservoir", e, nullptr))) break;
        const size_t at = (size_t)e * size;
        int rows = 0;
        rc = m->read(e, size, x + at * ndim, lnprob + at, step + at, walker + at, key + at, &rows, n_seen + e);
        n_rows[e] = rows;
    }
    return B.finish(probe_rc(rc));
}

// One launch of res_merge_kernel over n_ensembles ensembles: the held entries key, step, walker, lnprob [n_ensembles][size] and
// x[n_ensembles][size][ndim] and meta[n_ensembles][mpr_meta_words()] (threshold key, step, walker; full; n_held; n_seen) go in
// and come back; the candidates cand_key, cand_step, cand_walker [n_ensembles][cand_cap], n_cand[n_ensembles] of them (n_cand
// comes back), refer to the slab chain[n_rows][n_total][ndim], lnp[n_rows][n_total] whose row 0 is step t0; `rows` steps count
// as seen.
int mpr_merge(int n_walkers, int n_ensembles, int ndim, int size, int cand_cap, int n_rows, int64_t t0, int rows, const double *chain,
              const double *lnp, uint64_t *key, int64_t *step, int32_t *walker, double *x, double *lnprob, int64_t *meta,
              const uint64_t *cand_key, const int64_t *cand_step, const int32_t *cand_walker, uint32_t *n_cand) {
    if (!chain || !lnp || !key || !step || !walker || !x || !lnprob || !meta || !cand_key || !cand_step || !cand_walker || !n_cand) return -1;
    if (n_walkers < 1 || n_ensembles < 1 || n_ensembles > kMaxEnsembles || ndim < 1 || ndim > MP_MAX_NDIM) return -1;
    if (size < 1 || size > MP_RESERVOIR_MAX_ROWS || cand_cap < 1 || cand_cap > (1 << 20) || n_rows < 1 || rows < 1 || t0 < 0) return -1;
    if ((int64_t)n_rows * n_walkers * n_ensembles * ndim > kMaxElements) return -1;
    for (int e = 0; e < n_ensembles; ++e) {
        const int64_t held = meta[(size_t)e * kResMeta + kResHeld];
        if (held < 0 || held > size || n_cand[e] > (uint32_t)cand_cap) return -1;
        for (uint32_t j = 0; j < n_cand[e]; ++j) {
            const size_t at = (size_t)e * cand_cap + j;
            if (cand_step[at] < t0 || cand_step[at] >= t0 + n_rows || cand_walker[at] < 0 || cand_walker[at] >= n_walkers) return -1;
        }
    }
    Bufs B;
    const size_t ne = (size_t)n_ensembles, held = ne * size, cand = ne * cand_cap, nt = ne * n_walkers;
    std::vector<int32_t> scratch(cand, -1);
    ResArgs a{};
    a.chain = B.in(chain, (size_t)n_rows * nt * ndim);
    a.lnp = B.in(lnp, (size_t)n_rows * nt);
    a.key = B.io(key, held);
    a.step = B.io(step, held);
    a.walker = B.io(walker, held);
    a.x = B.io(x, held * ndim);
    a.held_lnp = B.io(lnprob, held);
    a.meta = B.io(meta, ne * kResMeta);
    a.cand_key = const_cast<uint64_t *>(B.in(cand_key, cand));
    a.cand_step = const_cast<int64_t *>(B.in(cand_step, cand));
    a.cand_walker = const_cast<int32_t *>(B.in(cand_walker, cand));
    a.n_cand = B.io(n_cand, ne);
    a.evicted = const_cast<int32_t *>(B.in(scratch.data(), cand));
    a.t0 = t0;
    a.n_walkers = n_walkers; a.n_ensembles = n_ensembles; a.n_total = (int)nt; a.ndim = ndim;
    a.size = size; a.cand_cap = cand_cap;
    a.row0 = 0; a.rows = rows;
    int rc = 0;
    if (B.ready()) rc = launch_res_merge(a, nullptr);
    return B.finish(rc);
}

}  // extern "C"
