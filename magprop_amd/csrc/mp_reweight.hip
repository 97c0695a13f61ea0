// mp_reweight.hip — gfx950 kernels of the importance reweighting (mp_model_reweight, include/magprop_amd.h; the term, the row sum
// and the order of the column sums are stated in mp_reweight.h).
//
// reweight_rows_kernel turns a chunk's Ltot rows (walker-major [cnt][n_grid], what the curve kernels write) into the rows' log
// weights lw[n_alt][n]: one wavefront, a workgroup of its own, per row.  A lane walks the observations l, l + 64, ...; mod, res
// and the base term of an observation are formed once and serve every alternative.  The alternatives are taken in groups of
// kReweightGroup whose terms are formed side by side in registers (fp64 log and log1p bind the kernel: the group is what a lane
// has in flight at one wavefront per SIMD), and their running sums wait in the lane's own LDS column between observations.
// reweight_select_kernel and reweight_reduce_kernel take one alternative per workgroup, as the pointwise pair takes an
// observation (wg_tail_select of mp_tail.h with lw itself as the key; counts, sums, extrema and log-sum-exp pairs of mp_wg.h).
#include <hip/hip_runtime.h>

#include "mp_band.h"
#include "mp_math.hpp"
#include "mp_reweight.h"
#include "mp_tail.h"
#include "mp_wg.h"

namespace mp {

namespace {

static_assert(kReweightThreads == kWgThreads && kReweightThreads == kPointwiseThreads, "the select and reduce kernels are one workgroup of mp_wg.h each");
static_assert(MP_REWEIGHT_MAX_ALT % kReweightGroup == 0, "whole groups");
constexpr int kWaves = kWgWaves;
constexpr int kG = kReweightGroup;

// g = 0.5 * log(var) and q = rr / var of one term
__device__ inline void term_var(double scale, double jitter, double ye, double mod, double rr, double &q, double &g) {
#pragma clang fp contract(off)
    const double se = scale * ye;
    const double a = se * se;
    const double jm = jitter * mod;
    const double b = jm * jm;
    const double var = a + b;
    q = rr / var;
    g = 0.5 * log(var);
}

__device__ inline double term_gauss(double q, double g) {
#pragma clang fp contract(off)
    const double h = 0.5 * q;
    const double s = h + g;
    return -s;
}

__device__ inline double term_student(double q, double g, double nu) {
#pragma clang fp contract(off)
    const double u = q / nu;
    const double hn = nu + 1.0;
    const double c = 0.5 * hn;
    const double p = c * log1p(u);
    const double s = p + g;
    return -s;
}

__global__ __launch_bounds__(64) void reweight_rows_kernel(const ReweightRowsArgs a) {
#pragma clang fp contract(off)
    __shared__ double acc[MP_REWEIGHT_MAX_ALT][64];          // the lane's running sums, one column per lane
    const int lane = threadIdx.x, s = blockIdx.x;
    if (s >= a.cnt) return;
    const size_t at = (size_t)a.lo + (size_t)s;
    if (a.status[s] != MP_STATUS_OK) {
        for (int k = lane; k < a.n_alt; k += 64) a.lw[(size_t)k * (size_t)a.n + at] = __builtin_nan("");
        return;
    }
    const int groups = (a.n_alt + kG - 1) / kG;
    for (int k = 0; k < groups * kG; ++k) acc[k][lane] = 0.0;
    const double *row = a.ltot + (size_t)s * (size_t)a.n_grid;
    for (int j = lane; j < a.d.n_obs; j += 64) {
        const int g = min(max(a.d.g[j], 0), a.n_grid - 2);   // (mp_set_dataset keeps g inside the grid: the last point sits in the last interval)
        const double dx = a.d.dx[j], idt = a.d.idt[j], y = a.d.y[j], ye = a.d.yerr[j];
        const double La = row[g], Lb = row[g + 1];
        const double dl = Lb - La;
        const double slope = dl * idt;
        const double rise = slope * dx;
        const double mod = rise + La;
        const double res = y - mod;
        const double rr = res * res;
        double q0, g0;
        term_var(1.0, 0.0, ye, mod, rr, q0, g0);
        const double t0 = term_gauss(q0, g0);
        for (int grp = 0; grp < groups; ++grp) {
            const int k0 = grp * kG;
            double q[kG], gg[kG], nu[kG], w[kG];
            bool student[kG], any_student = false;
#pragma unroll
            for (int i = 0; i < kG; ++i) {
                const int k = min(k0 + i, a.n_alt - 1);      // (a last group is filled up with its last alternative; those sums are not stored)
                student[i] = a.kind[k] == MP_REWEIGHT_STUDENT;
                any_student |= student[i];
                nu[i] = a.alt[3 * k + 2];
                w[i] = a.obs_w ? a.obs_w[(size_t)k * (size_t)a.d.n_obs + (size_t)j] : 1.0;
                term_var(a.alt[3 * k], a.alt[3 * k + 1], ye, mod, rr, q[i], gg[i]);
            }
            double ts[kG];
            if (any_student) {                               // (uniform over the wavefront: the table is)
#pragma unroll
                for (int i = 0; i < kG; ++i) ts[i] = term_student(q[i], gg[i], nu[i]);
            }
#pragma unroll
            for (int i = 0; i < kG; ++i) {
                const double t = student[i] ? ts[i] : term_gauss(q[i], gg[i]);
                const double wt = w[i] * t;
                const double d = w[i] == 0.0 ? -t0 : wt - t0;
                acc[k0 + i][lane] = acc[k0 + i][lane] + d;
            }
        }
    }
    for (int k = 0; k < a.n_alt; ++k) {
        const double v = wave_sum(acc[k][lane]);
        if (lane == 0) a.lw[(size_t)k * (size_t)a.n + at] = v;
    }
}

__global__ __launch_bounds__(kReweightThreads) void reweight_select_kernel(const ReweightColsArgs a) {
    __shared__ WgSelectLds sel;
    __shared__ uint64_t keys[kPointwiseSortCap];
    const int k = blockIdx.x;
    const double *col = a.lw + (size_t)k * (size_t)a.n;
    wg_tail_select((int)a.n, sel, keys, a.out + (size_t)k * MP_REWEIGHT_N + MP_REWEIGHT_CUT,
                   a.tail ? a.tail + (size_t)k * (size_t)a.tail_stride : nullptr, a.tail_stride, [col](int i, uint64_t &key) {
                       const double v = col[i];
                       key = band_key(v);
                       return !__builtin_isnan(v);
                   });
}

struct KeyMin {
    __device__ uint64_t operator()(uint64_t x, uint64_t y) const { return x < y ? x : y; }
};
struct KeyMax {
    __device__ uint64_t operator()(uint64_t x, uint64_t y) const { return x > y ? x : y; }
};

__global__ __launch_bounds__(kReweightThreads) void reweight_reduce_kernel(const ReweightColsArgs a) {
#pragma clang fp contract(off)
    __shared__ double shm[kWaves], shs[kWaves];
    __shared__ uint32_t shc[kWaves];
    __shared__ uint64_t shk[kWaves];
    const int k = blockIdx.x, tid = threadIdx.x;
    const int n = (int)a.n;
    const double *col = a.lw + (size_t)k * (size_t)a.n;
    double *out = a.out + (size_t)k * MP_REWEIGHT_N;
    const double cut = out[MP_REWEIGHT_CUT];                 // the select kernel's (NaN: no used cell; nothing here writes it)
    const uint64_t kcut = band_key(cut);
    double sum = 0.0, m1 = -INFINITY, s1 = 0.0, m2 = -INFINITY, s2 = 0.0, tm = -INFINITY, ts = 0.0;
    uint64_t kmin = ~0ull, kmax = 0ull;                      // extrema by key: -0.0 sits below +0.0 whatever the order
    uint32_t cnt = 0, nt = 0;
    for (int i = tid; i < n; i += kReweightThreads) {
        const double v = col[i];
        if (__builtin_isnan(v)) continue;
        const uint64_t key = band_key(v);
        ++cnt;
        sum = sum + v;
        kmin = key < kmin ? key : kmin;
        kmax = key > kmax ? key : kmax;
        lse_add(m1, s1, v);
        lse_add(m2, s2, 2.0 * v);
        if (key <= kcut) {
            ++nt;
            lse_add(tm, ts, v);
        }
    }
    const uint32_t m = wg_count(cnt, shc);
    const uint32_t nontail = wg_count(nt, shc);
    sum = wg_sum(sum, shm);
    kmin = wg_across(wave_all(kmin, KeyMin()), shk, KeyMin());
    kmax = wg_across(wave_all(kmax, KeyMax()), shk, KeyMax());
    wg_lse(m1, s1, shm, shs);
    wg_lse(m2, s2, shm, shs);
    wg_lse(tm, ts, shm, shs);
    if (tid == 0) {
        out[MP_REWEIGHT_N_USED] = (double)m;
        out[MP_REWEIGHT_LW_MEAN] = sum / (double)m;          // (0 / 0 = NaN without a used cell)
        out[MP_REWEIGHT_LW_MIN] = m ? band_value(kmin) : __builtin_nan("");
        out[MP_REWEIGHT_LW_MAX] = m ? band_value(kmax) : __builtin_nan("");
        out[MP_REWEIGHT_LSE1_M] = m1;
        out[MP_REWEIGHT_LSE1_S] = s1;
        out[MP_REWEIGHT_LSE2_M] = m2;
        out[MP_REWEIGHT_LSE2_S] = s2;
        out[MP_REWEIGHT_NONTAIL_COUNT] = (double)nontail;
        out[MP_REWEIGHT_NONTAIL_M] = tm;
        out[MP_REWEIGHT_NONTAIL_S] = ts;
    }
}

}  // namespace

int launch_reweight_rows(const ReweightRowsArgs &a, void *stream) {
    hipLaunchKernelGGL(reweight_rows_kernel, dim3((unsigned)a.cnt), dim3(64), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int launch_reweight_select(const ReweightColsArgs &a, void *stream) {
    hipLaunchKernelGGL(reweight_select_kernel, dim3((unsigned)a.n_alt), dim3(kReweightThreads), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int launch_reweight_reduce(const ReweightColsArgs &a, void *stream) {
    hipLaunchKernelGGL(reweight_reduce_kernel, dim3((unsigned)a.n_alt), dim3(kReweightThreads), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

}  // namespace mp
