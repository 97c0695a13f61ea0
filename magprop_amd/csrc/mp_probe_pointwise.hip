// mp_probe_pointwise.hip — test infrastructure only: the three kernels of the pointwise scores (mp_pointwise.hip) behind extern "C"
// host functions over HOST buffers (tests/test_gpu_pointwise_kernels.py, cases of tests/pointwise_cases.py).  Builds into its own
// libmp_probe_pointwise.so, linked from the very object libmagprop_amd.so is linked from (build/all/mp_pointwise.hip.o): the
// kernels reached here are the product's compiled code, through the product's launchers.  Nothing here is part of
// libmagprop_amd.so, of include/magprop_amd.h or of the product's ABI.
//
// Each function does what mp_model_pointwise (mp_summaries.cpp) does with one launch, with the buffers in the caller's hands.  It
// returns 0, a hipError_t, or -1 for arguments it refuses; nothing is launched then.
#include <hip/hip_runtime.h>

#include "mp_pointwise.h"
#include "mp_probe_bufs.h"

namespace mp {

namespace {

// the probe's own caps
constexpr int kMaxRows = 8192;
constexpr int kMaxObs = 4096;
constexpr int kMaxGrid = 1 << 16;
constexpr int64_t kMaxElements = 1 << 24;   // cnt * n_grid, n * n_obs

bool cols_ok(const double *z, const double *obs, int64_t n, int n_obs, int tail_stride) {
    return z && obs && n >= 1 && n <= kMaxRows && n_obs >= 1 && n_obs <= kMaxObs && n * n_obs <= kMaxElements &&
           tail_stride >= pointwise_tail_len(n) && tail_stride <= 2 * kPointwiseSortCap;
}

}  // namespace

}  // namespace mp

using namespace mp;

extern "C" {

int mpw_threads(void) { return kPointwiseThreads; }
int mpw_tile(void) { return kPointwiseTile; }
int mpw_columns(void) { return MP_POINTWISE_N; }
int mpw_max_tail(void) { return kPointwiseMaxTail; }
int mpw_sort_cap(void) { return kPointwiseSortCap; }
int mpw_tail_len(int64_t n) { return pointwise_tail_len(n); }
int mpw_max_rows(void) { return kMaxRows; }
int mpw_max_obs(void) { return kMaxObs; }

// ltot[cnt][n_grid], status[cnt], the dataset tables [n_obs] -> columns [lo, lo + cnt) of z[n_obs][n] (the others are left as they are)
int mpw_cells(const double *ltot, const int32_t *status, const int32_t *g, const double *dx, const double *idt, const double *y,
              const double *yerr, int cnt, int n_grid, int n_obs, int64_t n, int64_t lo, double *z) {
    if (!ltot || !status || !g || !dx || !idt || !y || !yerr || !z) return -1;
    if (cnt < 1 || cnt > kMaxRows || n_grid < 2 || n_grid > kMaxGrid || (int64_t)cnt * n_grid > kMaxElements) return -1;
    if (n_obs < 1 || n_obs > kMaxObs || n < 1 || n > kMaxRows || lo < 0 || lo + cnt > n || n * n_obs > kMaxElements) return -1;
    for (int j = 0; j < n_obs; ++j)
        if (g[j] < 0 || g[j] > n_grid - 2) return -1;
    Bufs B;
    PointwiseCellsArgs a{};
    a.ltot = B.in(ltot, (size_t)cnt * (size_t)n_grid);
    a.status = B.in(status, (size_t)cnt);
    a.d.g = B.in(g, (size_t)n_obs);
    a.d.dx = B.in(dx, (size_t)n_obs);
    a.d.idt = B.in(idt, (size_t)n_obs);
    a.d.y = B.in(y, (size_t)n_obs);
    a.d.yerr = B.in(yerr, (size_t)n_obs);
    a.d.n_obs = n_obs;
    a.z = B.io(z, (size_t)n_obs * (size_t)n);
    a.n = n;
    a.lo = lo;
    a.cnt = cnt;
    a.n_grid = n_grid;
    if (!B.ready()) return B.finish(0);
    return B.finish(launch_pointwise_cells(a, nullptr));
}

// z[n_obs][n] -> obs[n_obs][MP_POINTWISE_N] column CUT (the others are left as they are), tail[n_obs][tail_stride] (may be NULL)
int mpw_select(const double *z, int64_t n, int n_obs, int tail_stride, double *obs, double *tail) {
    if (!cols_ok(z, obs, n, n_obs, tail_stride)) return -1;
    Bufs B;
    PointwiseColsArgs a{};
    a.z = B.in(z, (size_t)n_obs * (size_t)n);
    a.obs = B.io(obs, (size_t)n_obs * MP_POINTWISE_N);
    a.tail = tail ? B.io(tail, (size_t)n_obs * (size_t)tail_stride) : nullptr;
    a.n = n;
    a.n_obs = n_obs;
    a.tail_stride = tail_stride;
    if (!B.ready()) return B.finish(0);
    return B.finish(launch_pointwise_select(a, nullptr));
}

// z[n_obs][n] and column CUT of obs[n_obs][MP_POINTWISE_N] -> the other columns of obs
int mpw_reduce(const double *z, int64_t n, int n_obs, double *obs) {
    if (!cols_ok(z, obs, n, n_obs, pointwise_tail_len(n))) return -1;
    Bufs B;
    PointwiseColsArgs a{};
    a.z = B.in(z, (size_t)n_obs * (size_t)n);
    a.obs = B.io(obs, (size_t)n_obs * MP_POINTWISE_N);
    a.tail = nullptr;
    a.n = n;
    a.n_obs = n_obs;
    a.tail_stride = pointwise_tail_len(n);
    if (!B.ready()) return B.finish(0);
    return B.finish(launch_pointwise_reduce(a, nullptr));
}

}  // extern "C"
