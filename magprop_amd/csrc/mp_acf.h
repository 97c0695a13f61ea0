// mp_acf.h — the autocorrelation monitor of the device-resident ensemble sampler (mp_sampler_set_autocorr, include/magprop_amd.h
// states the definition): launch arguments of the gfx950 kernels in mp_acf.hip.
//
// A series is one coordinate of one walker: n_series = n_total * ndim of them, the index of a chain row.  Every array below has the
// series index fastest, so a wavefront with one lane per series loads 512 consecutive bytes.  The history is a ring of ring_rows
// rows of y = x - pivot: sample t lives in row (head0 + t) mod ring_rows, rows that no sample has reached yet hold zeros, and
// ring_rows >= kp + (rows of the longest chunk), so the kp samples before a chunk are still there when it is accumulated.
#pragma once
#include <stdint.h>

#include "../../include/magprop_amd.h"

namespace mp {

constexpr int kAcfLagBlock = 16;   // lags per workgroup of the accumulate and rho kernels: accumulators and window in registers
constexpr int kAcfThreads = 256;   // series per workgroup of those kernels (4 wavefronts)
constexpr int kAcfFinalThreads = 1024;

struct AcfArgs {
    const double *chain;   // [.][n_series] the chunk's rows of the sampler's device slab
    double *hist;          // [ring_rows][n_series] ring of y values
    double *S;             // [kp][n_series] S_k = sum_{t >= k} y_t y_{t-k}
    double *T;             // [n_series] sum_t y_t
    double *H;             // [kp][n_series] H_k = sum_{t < k} y_t for k <= n (the running T behind sample k - 1)
    double *pivot;         // [n_series] x_0
    double *rho;           // [kp][n_series] work: rho_k of every series (finalisation)
    double *f;             // [n_ensembles * ndim][kp] walker-mean f_k (finalisation)
    double *tau;           // [n_ensembles * ndim]
    int32_t *window;       // [n_ensembles * ndim]
    int32_t n_series, n_walkers, n_ensembles, ndim;
    int32_t kp;            // max_lag rounded up to a multiple of kAcfLagBlock
    int32_t max_lag;
    int32_t ring_rows;
    int32_t head;          // ring row of sample n0
    int32_t first, rows;   // rows [first, first + rows) of `chain` are samples n0 .. n0 + rows - 1
    int64_t n0;            // samples accumulated so far
    double c;              // window constant (finalisation)
};

// implemented in mp_acf.hip; return hipError_t as int
//   ingest: the chunk's rows into the ring, T, H and (at n0 == 0) the pivot; then accumulate: S over the new samples
int launch_acf_accumulate(const AcfArgs &a, void *stream);
//   rho_k of every series from the n0 samples so far, then per (ensemble, dimension) the walker mean, the window and tau
int launch_acf_finalise(const AcfArgs &a, void *stream);

}  // namespace mp
