// mp_pointwise.h — pointwise predictive scores of model samples (mp_model_pointwise; include/magprop_amd.h states the definition
// and the columns MP_POINTWISE_*): what the gfx950 kernels (mp_pointwise.hip), the host driver (mp_summaries.cpp), the probe and a
// host test share -- the tail-length rule, the tile and workgroup sizes, the arguments and the launchers.
//
// Cell (s, j): La, Lb the Ltot row of sample s at grid points g_j, g_j + 1; mod = ((Lb - La) * idt_j) * dx_j + La; z = (y_j -
// mod) / ye_j; r = 0.5 * (z * z); ll = -r.  Every operation rounds on its own (no FMA contraction).  A sample whose status is
// not MP_STATUS_OK gives NaN cells; the used cells of an observation are its non-NaN ones.
//
// Order of every sum over the used cells of an observation (a function of the cells and of their sample indices only): thread k
// of kPointwiseThreads = 256 takes the cells of samples k, k + 256, ... in increasing index (NaN cells skipped) from the empty
// sum, and the 256 partial results are combined as mp_wg.h combines a workgroup's (wg_sum, wg_lse: the xor butterfly of
// mp_math.hpp inside a wavefront, distances 32, 16, .. 1, then the four wavefronts in wavefront order starting from wavefront
// 0's result).  Minima, maxima and counts do not depend on an order.  tests/pointwise_restated.py is the same order in numpy.
#pragma once
#include <stdint.h>

#include "../../include/magprop_amd.h"

#if defined(__HIP__) || defined(__HIPCC__)
#define MP_POINTWISE_HD __host__ __device__
#else
#define MP_POINTWISE_HD
#endif

namespace mp {

constexpr int kPointwiseThreads = 256;   // one workgroup of the select and reduce kernels per observation (mp_wg.h kWgThreads)
constexpr int kPointwiseTile = 64;       // cells kernel: tiles of 64 samples x 64 observations
constexpr int kPointwiseMaxTail = 1537;  // pointwise_tail_len(MP_POINTWISE_MAX_SAMPLES)
constexpr int kPointwiseSortCap = 2048;  // slots of the select kernel's LDS sort: the power of two above kPointwiseMaxTail

// T(n) = M + 1, M = ceil(min(n / 5, 3 sqrt(n))) in integers: min((n + 4) / 5, the least m with m * m >= 9 n).  The M largest
// importance ratios of an observation are its Pareto tail (Vehtari, Simpson, Gelman, Yao & Gabry 2024), the value below them
// is the cut.  0 for n < 1.
MP_POINTWISE_HD inline int pointwise_tail_len(int64_t n) {
    if (n < 1) return 0;
    const int64_t a = (n + 4) / 5;
    // the least m with m * m >= 9 n, below a: a bisection over [1, a] (a * a >= 9 n or the minimum is a anyway)
    int64_t lo = 1, hi = a;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (mid * mid >= 9 * n) hi = mid;
        else lo = mid + 1;
    }
    return (int)lo + 1;
}

struct PointwiseData {       // one dataset as mp_set_dataset digested it (observations sorted by time)
    const int32_t *g;        // [n_obs] grid interval of every observation, 0 <= g <= n_grid - 2
    const double *dx, *idt;  // [n_obs] x - t[g]; 1 / (t[g + 1] - t[g])
    const double *y, *yerr;  // [n_obs]
    int32_t n_obs;
};

struct PointwiseCellsArgs {
    const double *ltot;      // [cnt][n_grid]: the chunk's Ltot rows, walker-major as the curve kernels write them
    const int32_t *status;   // [cnt]: a row whose status is not MP_STATUS_OK gives NaN cells (its curve is not read)
    PointwiseData d;
    double *z;               // [n_obs][n]: observation-major cell matrix; the chunk writes columns [lo, lo + cnt)
    int64_t n, lo;
    int32_t cnt, n_grid;
};

struct PointwiseColsArgs {
    const double *z;         // [n_obs][n]
    double *obs;             // [n_obs][MP_POINTWISE_N]: the select kernel writes CUT, the reduce kernel reads it and writes the rest
    double *tail;            // [n_obs][tail_stride] (select kernel; may be nullptr: not written)
    int64_t n;
    int32_t n_obs, tail_stride;
};

// implemented in mp_pointwise.hip; return hipError_t as int
int launch_pointwise_cells(const PointwiseCellsArgs &a, void *stream);
int launch_pointwise_select(const PointwiseColsArgs &a, void *stream);
int launch_pointwise_reduce(const PointwiseColsArgs &a, void *stream);

}  // namespace mp
