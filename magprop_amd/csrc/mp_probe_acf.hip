// mp_probe_acf.hip — test infrastructure only: the four kernels of the autocorrelation monitor (acf_ingest_kernel,
// acf_accumulate_kernel, acf_rho_kernel, acf_final_kernel; mp_acf.hip) behind one extern "C" host function over HOST buffers
// (tests/test_gpu_acf_kernels.py, cases of tests/acf_cases.py).  Builds into its own libmp_probe_acf.so, linked from the very
// object libmagprop_amd.so is linked from (build/all/mp_acf.hip.o): the kernels reached here are the product's compiled code,
// through the product's launchers launch_acf_accumulate and launch_acf_finalise.  Nothing here is part of libmagprop_amd.so, of
// include/magprop_amd.h or of the product's ABI.
//
// mpa_run_monitor does what acf_restart, acf_feed and acf_finalise of mp_sampler.cpp do, with the ring, the head, the chunks and
// the values in the caller's hands.  It returns 0, a hipError_t, or -1 for arguments it refuses; nothing is launched then.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>

#include "mp_acf.h"
#include "mp_probe_bufs.h"

namespace mp {

namespace {

// the probe's own caps
constexpr int kMaxSeries = 1024;            // n_walkers * n_ensembles * ndim
constexpr int kMaxRows = 1 << 14;           // samples of a call
constexpr int kMaxChunks = 1 << 14;
constexpr int kMaxLead = 64;                // junk rows in front of a chunk
constexpr int kMaxRing = 1 << 14;           // rows of the ring
constexpr int kMaxRingDoubles = 1 << 22;    // ring_rows * n_series

bool positive_finite(double v) { return v > 0.0 && std::isfinite(v); }

}  // namespace

}  // namespace mp

using namespace mp;

extern "C" {

int mpa_lag_block(void) { return kAcfLagBlock; }
int mpa_threads(void) { return kAcfThreads; }
int mpa_max_lag(void) { return MP_ACF_MAX_LAG; }
int mpa_max_ndim(void) { return MP_MAX_NDIM; }
int mpa_max_series(void) { return kMaxSeries; }
int mpa_max_rows(void) { return kMaxRows; }
int mpa_max_chunks(void) { return kMaxChunks; }
int mpa_max_lead(void) { return kMaxLead; }
int mpa_max_ring(void) { return kMaxRing; }
int mpa_max_ring_doubles(void) { return kMaxRingDoubles; }

// The sequence x[n][n_series] (n_series = n_walkers * n_ensembles * ndim, a chain row of the sampler) through a monitor of max_lag
// lags whose ring has ring_rows rows and starts at row head0, in n_chunks chunks of chunk_rows[i] rows (summing to n; 0 allowed).
// Chunk i is uploaded as a slab of lead[i] rows of NaN, its rows and one more row of NaN, and accumulated with first = lead[i].
// Where finalise_after[i] is not 0 and 2 or more samples are in (acf_finalise refuses fewer), the finalise pair runs behind chunk
// i with the window constant c_mid; behind the last chunk it runs with c.
// hist[ring_rows][ns], S[kp][ns], T[ns], H[kp][ns], pivot[ns] come back as the device holds them (what they held is ignored: they
// start as zeros); rho[kp][ns], f[n_ensembles * ndim][kp], tau and window[n_ensembles * ndim] go in and come back, so that what
// no kernel writes keeps the caller's canary.  kp = max_lag rounded up to a multiple of kAcfLagBlock.
int mpa_run_monitor(const double *x, int n, int n_walkers, int n_ensembles, int ndim, int max_lag, int ring_rows, int head0,
                    int n_chunks, const int32_t *chunk_rows, const int32_t *lead, const int32_t *finalise_after, double c_mid,
                    double c, double *S, double *T, double *H, double *pivot, double *hist, double *rho, double *f, double *tau,
                    int32_t *window) {
    if (!x || !chunk_rows || !lead || !finalise_after || !S || !T || !H || !pivot || !hist || !rho || !f || !tau || !window) return -1;
    if (n_walkers < 2 || (n_walkers & 1) || n_ensembles < 1 || ndim < 1 || ndim > MP_MAX_NDIM) return -1;   // (mp_sampler_create)
    if (n_walkers > kMaxSeries || n_ensembles > kMaxSeries) return -1;
    const int64_t ns64 = (int64_t)n_walkers * n_ensembles * ndim;
    if (ns64 > kMaxSeries) return -1;
    if (max_lag < 1 || max_lag > MP_ACF_MAX_LAG) return -1;
    if (n < 2 || n > kMaxRows || n_chunks < 1 || n_chunks > kMaxChunks) return -1;
    if (!positive_finite(c) || !positive_finite(c_mid)) return -1;
    if (ring_rows < 1 || ring_rows > kMaxRing || (int64_t)ring_rows * ns64 > kMaxRingDoubles) return -1;
    if (head0 < 0 || head0 >= ring_rows) return -1;
    int64_t sum = 0;
    int longest = 0, slab_rows = 0;
    for (int i = 0; i < n_chunks; ++i) {
        if (chunk_rows[i] < 0 || chunk_rows[i] > n || lead[i] < 0 || lead[i] > kMaxLead) return -1;
        sum += chunk_rows[i];
        longest = std::max(longest, chunk_rows[i]);
        slab_rows = std::max(slab_rows, lead[i] + chunk_rows[i] + 1);
    }
    if (sum != n) return -1;
    const int kp = (max_lag + kAcfLagBlock - 1) / kAcfLagBlock * kAcfLagBlock;
    if (ring_rows < kp + longest) return -1;   // (mp_acf.h: below it the kernels' ring offsets are out of range)

    const size_t ns = (size_t)ns64, ned = (size_t)n_ensembles * ndim;
    const double junk = std::numeric_limits<double>::quiet_NaN();
    std::vector<double> slab((size_t)slab_rows * ns, junk);
    Bufs B;
    AcfArgs a{};
    double *d_slab = const_cast<double *>(B.in(slab.data(), slab.size()));
    a.chain = d_slab;
    a.hist = B.io(hist, (size_t)ring_rows * ns);
    a.S = B.io(S, (size_t)kp * ns);
    a.T = B.io(T, ns);
    a.H = B.io(H, (size_t)kp * ns);
    a.pivot = B.io(pivot, ns);
    a.rho = B.io(rho, (size_t)kp * ns);
    a.f = B.io(f, ned * kp);
    a.tau = B.io(tau, ned);
    a.window = B.io(window, ned);
    a.n_series = (int32_t)ns; a.n_walkers = n_walkers; a.n_ensembles = n_ensembles; a.ndim = ndim;
    a.kp = kp; a.max_lag = max_lag; a.ring_rows = ring_rows; a.head = head0; a.n0 = 0;
    if (!B.ready()) return B.finish(0);
    // acf_restart
    hipError_t e = hipMemset(a.hist, 0, (size_t)ring_rows * ns * sizeof(double));
    if (e == hipSuccess) e = hipMemset(a.S, 0, (size_t)kp * ns * sizeof(double));
    if (e == hipSuccess) e = hipMemset(a.H, 0, (size_t)kp * ns * sizeof(double));
    if (e == hipSuccess) e = hipMemset(a.T, 0, ns * sizeof(double));
    if (e == hipSuccess) e = hipMemset(a.pivot, 0, ns * sizeof(double));
    int rc = (int)e;
    const double *src = x;
    for (int i = 0; i < n_chunks && rc == 0; ++i) {
        // acf_feed: the slab of this chunk (the copy waits for the kernels that read the slab before it)
        const int rows = chunk_rows[i], first = lead[i];
        std::fill(slab.begin(), slab.end(), junk);
        std::copy(src, src + (size_t)rows * ns, slab.begin() + (size_t)first * ns);
        src += (size_t)rows * ns;
        rc = (int)hipMemcpy(d_slab, slab.data(), (size_t)(first + rows + 1) * ns * sizeof(double), hipMemcpyHostToDevice);
        if (rc) break;
        a.first = first;
        a.rows = rows;
        rc = launch_acf_accumulate(a, nullptr);
        if (rc) break;
        a.head = (a.head + rows) % ring_rows;
        a.n0 += rows;
        if (finalise_after[i] && a.n0 >= 2) {   // run_mcmc_until's check between two chunks
            a.c = c_mid;
            rc = launch_acf_finalise(a, nullptr);
            if (rc == 0) rc = (int)hipDeviceSynchronize();
        }
    }
    if (rc == 0) {
        a.c = c;
        rc = launch_acf_finalise(a, nullptr);
    }
    return B.finish(rc);
}

}  // extern "C"
