// mp_band.h — posterior-predictive light-curve bands (mp_model_band): the per-grid-point quantile rule shared by the gfx950
// reduction kernels (mp_band.hip) and a host build of the same functions (tests/test_band_cpu.py compiles this header with g++
// and holds it against np.nanquantile bit for bit).
//
// The rule is numpy's method "linear" after the NaNs are dropped (numpy/lib/_function_base_impl.py _quantile, _get_indexes,
// _get_gamma, _lerp): m finite-or-infinite values, h = (m - 1) q, lo = floor(h), hi = lo + 1; h >= m - 1 takes the last value
// twice with gamma = h - (-1) (numpy's index -1); gamma = h - lo otherwise; result = b - (b - a)(1 - gamma) for gamma >= 0.5,
// else a + (b - a) gamma.  Every operation rounds on its own: no FMA contraction.
//
// The weighted band (mp_model_band_weighted) interpolates nothing: the rows' weights become integer units once
// (band_weight_units), every sum of units is exact, and a quantile is the least value whose cumulative units reach
// band_weight_target (tests/test_wband_cpu.py compiles both with g++ and holds them against tests/wband_restated.py bit for bit).
#pragma once
#include <stdint.h>

#include "../../include/magprop_amd.h"

#if defined(__HIP__) || defined(__HIPCC__)
#define MP_BAND_HD __host__ __device__
#else
#define MP_BAND_HD
#endif

namespace mp {

constexpr int kBandThreads = 256;   // one workgroup of the select kernel per (component, grid point) (mp_wg.h kWgThreads)
constexpr int kBandTile = 64;       // transpose tiles: 64 walkers x 64 grid points

// Order-preserving map of a (non-NaN) double to an unsigned key: negative values have every bit flipped, the others only the
// sign bit.  Keys compare as the values do, with -0.0 just below +0.0 (the only equal values whose keys differ).
MP_BAND_HD inline uint64_t band_key(double v) {
    const uint64_t b = __builtin_bit_cast(uint64_t, v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
MP_BAND_HD inline double band_value(uint64_t k) {
    return __builtin_bit_cast(double, (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k);
}

struct BandRank {
    int lo, hi;      // order statistics (0-based ranks among the m non-NaN values) that enter the lerp
    double gamma;    // weight of the upper one
};

// The ranks and weight of quantile q (0 <= q <= 1) of m >= 1 values, as numpy computes them.
MP_BAND_HD inline BandRank band_rank(int m, double q) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double h = (double)(m - 1) * q;
    BandRank r;
    if (h >= (double)(m - 1)) {                 // numpy: previous = next = -1 (the last value), gamma = h - (-1)
        r.lo = r.hi = m - 1;
        r.gamma = h - (-1.0);
    } else {
        const double f = __builtin_floor(h);
        r.lo = (int)f;
        r.hi = r.lo + 1;
        r.gamma = h - (double)r.lo;             // (the integer index, converted: -0.0 - 0 stays -0.0 as in numpy)
    }
    return r;
}

// numpy's _lerp(a, b, gamma), every step rounded.
MP_BAND_HD inline double band_lerp(double a, double b, double gamma) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double d = b - a;
    if (gamma >= 0.5) {
        const double t = d * (1.0 - gamma);
        return b - t;
    }
    const double t = d * gamma;
    return a + t;
}

// The weights of the weighted band in integer units: u_i = floor((w_i / wmax) * 2^31), wmax the largest weight.  The division
// rounds once, the product with 2^31 and the floor are exact; the heaviest row has exactly kBandUnitMax units and a row below
// 2^-31 of it none.  false (and units_out undefined) unless every weight is finite and >= 0 and at least one is > 0.  Host only.
constexpr uint32_t kBandUnitMax = 0x80000000u;
inline bool band_weight_units(const double *w, int n, uint32_t *units_out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double wmax = 0.0;
    for (int i = 0; i < n; ++i) {
        if (!(w[i] >= 0.0 && w[i] <= 1.7976931348623157e308)) return false;   // (NaN, negative, infinite)
        if (w[i] > wmax) wmax = w[i];
    }
    if (!(wmax > 0.0)) return false;
    for (int i = 0; i < n; ++i) {
        const double ratio = w[i] / wmax;
        units_out[i] = (uint32_t)__builtin_floor(ratio * 2147483648.0);
    }
    return true;
}

// The cumulative units quantile q (0 <= q <= 1) has to reach, of W >= 1 units in all (W < 2^53, so that (double)W is exact):
// ceil(q W) with the product rounded once, clamped to [1, W].  q = 0 answers the least value that carries weight.
MP_BAND_HD inline uint64_t band_weight_target(double q, uint64_t W) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double t = __builtin_ceil(q * (double)W);
    if (!(t >= 1.0)) return 1;
    if (t >= (double)W) return W;
    return (uint64_t)t;
}

// Arguments of the select kernel: quantiles of one component, column-major curves in, [nq][n_grid] out.
struct BandQ {
    double q[MP_BAND_MAX_Q];
    int32_t nq;
};

// implemented in mp_band.hip; return hipError_t as int
//   src[n][n_grid] (walker-major, as the curve kernels write it) -> dst[n_grid][n]
int launch_band_transpose(const double *src, double *dst, int n, int n_grid, void *stream);
//   cols[n_grid][n] -> out[nq][n_grid]: per grid point np.nanquantile(cols[g], q) (all NaN: NaN)
int launch_band_select(const double *cols, int n, int n_grid, const BandQ &q, double *out, void *stream);
//   cols[n_grid][n], units[n] (each <= kBandUnitMax) -> out[nq][n_grid]: per grid point the weighted quantiles of the column's
//   non-NaN values under the rows' units (no unit on them: NaN)
int launch_band_wselect(const double *cols, const uint32_t *units, int n, int n_grid, const BandQ &q, double *out, void *stream);

}  // namespace mp
