// mp_derive.h — energy budgets and light-curve landmarks of model samples (mp_model_derived; include/magprop_amd.h states the
// definition and the columns MP_DERIVED_*): what the gfx950 reduction kernel (mp_derive.hip), the host driver (mp_summaries.cpp) and a
// host test share -- the segment rule of the summation order, the workgroup size and the launcher.
//
// Order of every sum (a function of the row's curves and of G = n_grid only): the G - 1 intervals are cut into kDeriveThreads =
// 256 contiguous segments of derive_seg(G) = ceil((G - 1) / 256) intervals, segment k holding intervals [k seg, min((k + 1) seg,
// G - 1)) (the last ones may be short or empty).  Inside a segment the terms 0.5 * dt_i * (L_i + L_{i+1}) are added in increasing
// i from 0.0; the 256 segment totals are added in segment order from 0.0 (an empty segment adds 0.0).  The cumulative energy up
// to t_{i+1} is the total of the segments before i's plus the running sum of its segment.  Every product and sum rounds on its
// own: no FMA contraction, no floating-point atomic.  A maximum is the first largest value: every segment's in increasing i, then
// the segments' under wg_best of mp_wg.h (larger value, then lower index).  tests/derive_restated.py is the same order in numpy.
#pragma once
#include <stdint.h>

#include "../../include/magprop_amd.h"

#if defined(__HIP__) || defined(__HIPCC__)
#define MP_DERIVE_HD __host__ __device__
#else
#define MP_DERIVE_HD
#endif

namespace mp {

constexpr int kDeriveThreads = 256;   // one workgroup per row; thread k walks segment k (mp_wg.h kWgThreads)
constexpr int kDeriveWindow = 14;     // intervals of every segment staged in LDS at a time (15 points: an odd stride in doubles)

// intervals per segment
MP_DERIVE_HD inline int derive_seg(int n_grid) { return (n_grid - 1 + kDeriveThreads - 1) / kDeriveThreads; }

struct DeriveArgs {
    const double *curve[5];   // [n][n_grid] each, walker-major as the curve kernels write them: Ltot, Lprop, Ldip, Mdisc, omega
    const int32_t *status;    // [n]: a row whose status is not MP_STATUS_OK gets MP_DERIVED_N NaNs (its curves are not read)
    const double *tgrid;      // [n_grid]
    double *out;              // [n][MP_DERIVED_N]
    int32_t n, n_grid;
};

// implemented in mp_derive.hip; returns hipError_t as int
int launch_derive(const DeriveArgs &a, void *stream);

}  // namespace mp
