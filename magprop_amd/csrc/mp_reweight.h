// mp_reweight.h — importance reweighting of model samples to other error models and data subsets (mp_model_reweight;
// include/magprop_amd.h states the term, the row sum and the columns MP_REWEIGHT_*): what the gfx950 kernels (mp_reweight.hip),
// the host driver (mp_summaries.cpp), the probe and a host check share -- the judgement of the alternatives and of the
// observation weights, the group and workgroup sizes, the arguments and the launchers.
//
// Term (s, j, k): mod and res = y_j - mod as in mp_pointwise.h; se = scale_k * ye_j, a = se * se, jm = jitter_k * mod, b = jm *
// jm, var = a + b, q = (res * res) / var, g = 0.5 * log(var); Gaussian t = -(0.5 * q + g), Student-t t = -((0.5 * (nu_k + 1)) *
// log1p(q / nu_k) + g); t_0 the Gaussian term of scale 1 and jitter 0; d = w_kj * t - t_0 (w_kj == 0: d = -t_0).  Every
// operation rounds on its own (no FMA contraction).  Row sum: lane l of the row's wavefront adds d of observations l, l + 64, ..
// in increasing order from 0.0, wave_sum (mp_math.hpp) combines the 64 partial sums.  The columns are reduced per alternative in
// the order mp_pointwise.h states, the values ordered by band_key (mp_band.h).  tests/reweight_restated.py is the same in numpy.
#pragma once
#include <stdint.h>

#include <cmath>

#include "mp_pointwise.h"

namespace mp {

constexpr int kReweightThreads = 256;   // one workgroup of the select and reduce kernels per alternative (mp_wg.h kWgThreads)
constexpr int kReweightGroup = 8;       // rows kernel: alternatives whose terms are formed side by side (no sum depends on it)

// The first alternative that mp_model_reweight refuses, or -1: a kind other than MP_REWEIGHT_GAUSS or MP_REWEIGHT_STUDENT, a
// scale not finite or not > 0, a jitter not finite or < 0, for a Student-t a nu not finite or not > 0.  alt[n_alt][3]: scale,
// jitter, nu.
inline int reweight_bad_alternative(int n_alt, const int32_t *kind, const double *alt) {
    for (int k = 0; k < n_alt; ++k) {
        const double scale = alt[3 * k], jitter = alt[3 * k + 1], nu = alt[3 * k + 2];
        if (kind[k] != MP_REWEIGHT_GAUSS && kind[k] != MP_REWEIGHT_STUDENT) return k;
        if (!std::isfinite(scale) || !(scale > 0.0)) return k;
        if (!std::isfinite(jitter) || !(jitter >= 0.0)) return k;
        if (kind[k] == MP_REWEIGHT_STUDENT && (!std::isfinite(nu) || !(nu > 0.0))) return k;
    }
    return -1;
}

// The first observation weight that mp_model_reweight refuses (not finite, or < 0), or -1.
inline int64_t reweight_bad_weight(const double *obs_w, int64_t count) {
    for (int64_t i = 0; i < count; ++i)
        if (!std::isfinite(obs_w[i]) || !(obs_w[i] >= 0.0)) return i;
    return -1;
}

struct ReweightRowsArgs {
    const double *ltot;      // [cnt][n_grid]: the chunk's Ltot rows, walker-major as the curve kernels write them
    const int32_t *status;   // [cnt]: a row whose status is not MP_STATUS_OK gives NaN in every alternative (its curve is not read)
    PointwiseData d;
    const int32_t *kind;     // [n_alt]
    const double *alt;       // [n_alt][3]: scale, jitter, nu
    const double *obs_w;     // [n_alt][n_obs], or nullptr: every weight 1
    double *lw;              // [n_alt][n]: alternative-major; the chunk writes columns [lo, lo + cnt)
    int64_t n, lo;
    int32_t cnt, n_grid, n_alt;
};

struct ReweightColsArgs {
    const double *lw;        // [n_alt][n]
    double *out;             // [n_alt][MP_REWEIGHT_N]: the select kernel writes CUT, the reduce kernel reads it and writes the rest
    double *tail;            // [n_alt][tail_stride] (select kernel; may be nullptr: not written)
    int64_t n;
    int32_t n_alt, tail_stride;
};

// implemented in mp_reweight.hip; return hipError_t as int
int launch_reweight_rows(const ReweightRowsArgs &a, void *stream);
int launch_reweight_select(const ReweightColsArgs &a, void *stream);
int launch_reweight_reduce(const ReweightColsArgs &a, void *stream);

}  // namespace mp
