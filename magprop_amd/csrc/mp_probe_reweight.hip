// mp_probe_reweight.hip — test infrastructure only: the three kernels of the importance reweighting (mp_reweight.hip) behind
// extern "C" host functions over HOST buffers, and the device runtime's double-precision log, log1p and exp, one value per lane,
// behind mpr_libm, which the restatement takes where a device value is compared bit for bit (tests/test_gpu_reweight_kernels.py,
// tests/test_gpu_reweight.py; cases of tests/reweight_cases.py).  Builds into its own libmp_probe_reweight.so, linked from the very
// object libmagprop_amd.so is linked from (build/all/mp_reweight.hip.o): the kernels reached here are the product's compiled
// code, through the product's launchers.  Nothing here is part of libmagprop_amd.so, of include/magprop_amd.h or of the
// product's ABI.
//
// Each function does what mp_model_reweight (mp_summaries.cpp) does with its launches, with the buffers in the caller's hands.
// It returns 0, a hipError_t, or -1 for arguments it refuses; nothing is launched then.
#include <hip/hip_runtime.h>

#include "mp_probe_bufs.h"
#include "mp_reweight.h"

namespace mp {

namespace {

// the probe's own caps
constexpr int kMaxRows = 8192;
constexpr int kMaxObs = 4096;
constexpr int kMaxGrid = 1 << 16;
constexpr int64_t kMaxElements = 1 << 24;   // cnt * n_grid
constexpr int kMaxN = 1 << 20;              // values of an mpr_libm call

__global__ void __launch_bounds__(64) reweight_libm_kernel(int func, const double *x, double *y, int n) {
    const long i = (long)blockIdx.x * 64 + threadIdx.x;
    if (i >= (long)n) return;
    y[i] = func == 0 ? log(x[i]) : func == 1 ? log1p(x[i]) : exp(x[i]);
}

}  // namespace

}  // namespace mp

using namespace mp;

extern "C" {

int mpr_group(void) { return kReweightGroup; }
int mpr_threads(void) { return kReweightThreads; }
int mpr_columns(void) { return MP_REWEIGHT_N; }
int mpr_max_alt(void) { return MP_REWEIGHT_MAX_ALT; }
int mpr_max_rows(void) { return kMaxRows; }
int mpr_max_obs(void) { return kMaxObs; }

// y[i] = f(x[i]), func: 0 log, 1 log1p, 2 exp; 1 <= n <= 1 << 20
int mpr_libm(int func, const double *x, double *y, int n) {
    if (func < 0 || func > 2 || n < 1 || n > kMaxN || !x || !y) return -1;
    Bufs B;
    const double *dx = B.in(x, n);
    double *dy = B.io(y, n);
    if (B.ready()) reweight_libm_kernel<<<dim3((n + 63) / 64), dim3(64)>>>(func, dx, dy, n);
    return B.finish((int)hipGetLastError());
}

// ltot[cnt][n_grid], status[cnt], the dataset tables [n_obs], kind[n_alt], alt[n_alt][3], obs_w[n_alt][n_obs] (may be NULL) ->
// columns [lo, lo + cnt) of lw[n_alt][n] (the others are left as they are)
int mpr_rows(const double *ltot, const int32_t *status, const int32_t *g, const double *dx, const double *idt, const double *y,
             const double *yerr, int cnt, int n_grid, int n_obs, int n_alt, const int32_t *kind, const double *alt,
             const double *obs_w, int64_t n, int64_t lo, double *lw) {
    if (!ltot || !status || !g || !dx || !idt || !y || !yerr || !kind || !alt || !lw) return -1;
    if (cnt < 1 || cnt > kMaxRows || n_grid < 2 || n_grid > kMaxGrid || (int64_t)cnt * n_grid > kMaxElements) return -1;
    if (n_obs < 1 || n_obs > kMaxObs || n < 1 || n > kMaxRows || lo < 0 || lo + cnt > n) return -1;
    if (n_alt < 1 || n_alt > MP_REWEIGHT_MAX_ALT || reweight_bad_alternative(n_alt, kind, alt) >= 0) return -1;
    if (obs_w && reweight_bad_weight(obs_w, (int64_t)n_alt * n_obs) >= 0) return -1;
    for (int j = 0; j < n_obs; ++j)
        if (g[j] < 0 || g[j] > n_grid - 2) return -1;
    Bufs B;
    ReweightRowsArgs a{};
    a.ltot = B.in(ltot, (size_t)cnt * (size_t)n_grid);
    a.status = B.in(status, (size_t)cnt);
    a.d.g = B.in(g, (size_t)n_obs);
    a.d.dx = B.in(dx, (size_t)n_obs);
    a.d.idt = B.in(idt, (size_t)n_obs);
    a.d.y = B.in(y, (size_t)n_obs);
    a.d.yerr = B.in(yerr, (size_t)n_obs);
    a.d.n_obs = n_obs;
    a.kind = B.in(kind, (size_t)n_alt);
    a.alt = B.in(alt, (size_t)n_alt * 3);
    a.obs_w = obs_w ? B.in(obs_w, (size_t)n_alt * (size_t)n_obs) : nullptr;
    a.lw = B.io(lw, (size_t)n_alt * (size_t)n);
    a.n = n;
    a.lo = lo;
    a.cnt = cnt;
    a.n_grid = n_grid;
    a.n_alt = n_alt;
    if (!B.ready()) return B.finish(0);
    return B.finish(launch_reweight_rows(a, nullptr));
}

// lw[n_alt][n] -> out[n_alt][MP_REWEIGHT_N] (select, then reduce) and tail[n_alt][tail_stride] (may be NULL)
int mpr_cols(const double *lw, int64_t n, int n_alt, int tail_stride, double *out, double *tail) {
    if (!lw || !out || n < 1 || n > kMaxRows || n_alt < 1 || n_alt > MP_REWEIGHT_MAX_ALT) return -1;
    if (tail_stride < pointwise_tail_len(n) || tail_stride > 2 * kPointwiseSortCap) return -1;
    Bufs B;
    ReweightColsArgs a{};
    a.lw = B.in(lw, (size_t)n_alt * (size_t)n);
    a.out = B.io(out, (size_t)n_alt * MP_REWEIGHT_N);
    a.tail = tail ? B.io(tail, (size_t)n_alt * (size_t)tail_stride) : nullptr;
    a.n = n;
    a.n_alt = n_alt;
    a.tail_stride = tail_stride;
    if (!B.ready()) return B.finish(0);
    int rc = launch_reweight_select(a, nullptr);
    if (!rc) rc = launch_reweight_reduce(a, nullptr);
    return B.finish(rc);
}

}  // extern "C"
