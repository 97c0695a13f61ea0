// mp_probe_acf.hip — test infrastructure only: the autocorrelation monitor of the sampler, its host unit (AcfMonitor, mp_monitor.cpp)
// and its four kernels (acf_ingest_kernel, acf_accumulate_kernel, acf_rho_kernel, acf_final_kernel; mp_acf.hip), behind one
// extern "C" host function over HOST buffers (tests/test_gpu_acf_kernels.py, cases of tests/acf_cases.py).  Builds into its own
// libmp_probe_acf.so, linked from the very objects libmagprop_amd.so is linked from (build/all/mp_monitor.cpp.o and the kernel
// objects it calls into): the host functions and the kernels reached here are the product's compiled code.  Nothing here is part
// of libmagprop_amd.so, of include/magprop_amd.h or of the product's ABI.
//
// mpa_run_monitor runs the product's AcfMonitor::make, restart, feed and finalise, the functions behind mp_sampler_set_autocorr,
// mp_sampler_run and mp_sampler_get_autocorr, with the ring, the head, the chunks and the values in the caller's hands.  It
// returns 0, a hipError_t, or -1 for arguments it refuses; nothing is allocated or launched then.
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
constexpr int kMaxSeries = 1024;            // n_walkers * n_ensembles * ndim
constexpr int kMaxRows = 1 << 14;           // samples of a call
constexpr int kMaxChunks = 1 << 14;
constexpr int kMaxLead = 64;                // junk rows in front of a chunk
constexpr int kMaxRing = 1 << 14;           // rows of the ring
constexpr int kMaxRingDoubles = 1 << 22;    // ring_rows * n_series

constexpr const char *kFn = "mpa_run_monitor";

bool positive_finite(double v) { return v > 0.0 && std::isfinite(v); }

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
// Chunk i is uploaded as a slab of lead[i] rows of NaN, its rows and one more row of NaN, and fed as lead[i] + chunk_rows[i] rows
// to a monitor that has lead[i] steps left to pass over.  Where finalise_after[i] is not 0 and 2 or more samples are in (finalise
// refuses fewer), finalise runs behind chunk i with the window constant c_mid; behind the last chunk it runs with c.
// All nine buffers go into the monitor's own before restart() and come back behind the last launch: hist[ring_rows][ns],
// S[kp][ns], T[ns], H[kp][ns], pivot[ns] start as the zeros of restart() whatever they held; rho[kp][ns],
// f[n_ensembles * ndim][kp], tau and window[n_ensembles * ndim] keep the caller's canary where no kernel writes.
// kp = max_lag rounded up to a multiple of kAcfLagBlock.
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
    // the monitor's ring has kp + chunk_cap rows: the chunk cap that gives the caller's ring (the 64 MB cap lies beyond kMaxRingDoubles)
    std::unique_ptr<AcfMonitor> m;
    int rc = AcfMonitor::make(kFn, n_walkers, n_ensembles, ndim, max_lag, 0, (size_t)(ring_rows - kp), &m);
    if (rc) return probe_rc(rc);
    if (m->ring_rows != ring_rows || m->kp != kp) return -1;
    const double junk = std::numeric_limits<double>::quiet_NaN();
    std::vector<double> slab((size_t)slab_rows * ns, junk);
    Bufs B;
    double *d_slab = const_cast<double *>(B.in(slab.data(), slab.size()));
    // the caller's bytes into every buffer of the monitor: what restart() does not zero and no kernel writes comes back as it went in
    B.adopt(hist, m->hist.p, (size_t)ring_rows * ns);
    B.adopt(S, m->S.p, (size_t)kp * ns);
    B.adopt(T, m->T.p, ns);
    B.adopt(H, m->H.p, (size_t)kp * ns);
    B.adopt(pivot, m->pivot.p, ns);
    B.adopt(rho, m->rho.p, (size_t)kp * ns);
    B.adopt(f, m->f.p, ned * kp);
    B.adopt(tau, m->tau.p, ned);
    B.adopt(window, m->window.p, ned);
    if (!B.ready()) return B.finish(0);
    rc = m->restart(nullptr);
    m->head = head0;
    const double *src = x;
    for (int i = 0; i < n_chunks && rc == 0; ++i) {
        // the slab of this chunk (the copy waits for the kernels that read the slab before it); its junk rows in front are the
        // steps that feed() passes over
        const int rows = chunk_rows[i], first = lead[i];
        std::fill(slab.begin(), slab.end(), junk);
        std::copy(src, src + (size_t)rows * ns, slab.begin() + (size_t)first * ns);
        src += (size_t)rows * ns;
        if (hipMemcpy(d_slab, slab.data(), (size_t)(first + rows + 1) * ns * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
            rc = MP_EHIP;
            break;
        }
        m->skip = first;
        rc = m->feed(ChainRows{d_slab, nullptr, first + rows, 0, 0}, nullptr);
        if (rc == 0 && finalise_after[i] && m->n >= 2) rc = m->finalise(kFn, c_mid, nullptr);   // run_mcmc_until's check between two chunks
    }
    if (rc == 0) rc = m->finalise(kFn, c, nullptr);
    return B.finish(probe_rc(rc));
}

}  // extern "C"
