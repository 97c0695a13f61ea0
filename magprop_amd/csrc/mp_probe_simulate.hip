// mp_probe_simulate.hip — test infrastructure only: the cells kernel of the simulated light curves (mp_simulate.hip) alone, over
// caller-given curves and bracket tables, behind the extern "C" host functions mpm_* over HOST buffers
// (tests/test_gpu_simulate_kernels.py, cases of tests/simulate_cases.py).  Builds into its own libmp_probe_simulate.so, linked
// from the very object libmagprop_amd.so is linked from (build/all/mp_simulate.hip.o): the kernel reached here is the product's
// compiled code, through the product's launcher.  Nothing here is part of libmagprop_amd.so, of include/magprop_amd.h or of the
// product's ABI.
//
// mpm_cells does what mp_simulate (mp_summaries.cpp) does with one chunk behind its curve launch, with the buffers in the
// caller's hands; mpm_bracket is the host's bracket rule.  They return 0, a hipError_t, or -1 for arguments they refuse; nothing
// is launched then.
#include <hip/hip_runtime.h>

#include "mp_probe_bufs.h"
#include "mp_simulate.h"

namespace mp {

namespace {

// the probe's own caps
constexpr int kMaxRows = 8192;
constexpr int kMaxObs = 4096;
constexpr int kMaxGrid = 1 << 16;
constexpr int64_t kMaxElements = 1 << 24;   // cnt * n_grid, cnt * n_obs

}  // namespace

}  // namespace mp

using namespace mp;

extern "C" {

int mpm_threads(void) { return kSimThreads; }
uint32_t mpm_counter(void) { return kSimCtr; }

// sim_bracket of x[n] on the grid t[n_grid] (strictly increasing; every x inside it): g[n], dx[n], idt[n]
int mpm_bracket(const double *t, int n_grid, const double *x, int64_t n, int32_t *g, double *dx, double *idt) {
    if (!t || !x || !g || !dx || !idt || n_grid < 2 || n_grid > kMaxGrid || n < 1 || n > kMaxElements) return -1;
    for (int i = 1; i < n_grid; ++i)
        if (!(t[i] > t[i - 1])) return -1;
    const std::vector<double> grid(t, t + n_grid);
    for (int64_t i = 0; i < n; ++i) {
        if (!(x[i] >= grid.front()) || !(x[i] <= grid.back())) return -1;
        sim_bracket(grid, x[i], g[i], dx[i], idt[i]);
    }
    return 0;
}

// ltot[cnt][n_grid], status[cnt], the bracket tables and yerr (NULL: frac_err) [tab_rows][n_obs], tab_rows 1 or cnt -> y, ye, mod,
// z [cnt][n_obs] (each may be NULL) and zero_err[cnt] (may be NULL; marks are added to what it holds)
int mpm_cells(const double *ltot, const int32_t *status, const int32_t *g, const double *dx, const double *idt, const double *yerr,
              double frac_err, uint64_t seed, int64_t row0, int cnt, int n_obs, int n_grid, int tab_rows, double *y, double *ye,
              double *mod, double *z, int32_t *zero_err) {
    if (!ltot || !status || !g || !dx || !idt) return -1;
    if (cnt < 1 || cnt > kMaxRows || n_grid < 2 || n_grid > kMaxGrid || (int64_t)cnt * n_grid > kMaxElements) return -1;
    if (n_obs < 1 || n_obs > kMaxObs || (int64_t)cnt * n_obs > kMaxElements || row0 < 0 || (tab_rows != 1 && tab_rows != cnt)) return -1;
    const size_t tab = (size_t)tab_rows * (size_t)n_obs, cells = (size_t)cnt * (size_t)n_obs;
    for (size_t j = 0; j < tab; ++j)
        if (g[j] < 0 || g[j] > n_grid - 1 || (g[j] == n_grid - 1 && dx[j] != 0.0)) return -1;
    Bufs B;
    SimCellsArgs a{};
    a.ltot = B.in(ltot, (size_t)cnt * (size_t)n_grid);
    a.status = B.in(status, (size_t)cnt);
    a.g = B.in(g, tab);
    a.dx = B.in(dx, tab);
    a.idt = B.in(idt, tab);
    a.yerr = yerr ? B.in(yerr, tab) : nullptr;
    a.frac_err = frac_err;
    a.seed = seed;
    a.row0 = row0;
    a.y = y ? B.io(y, cells) : nullptr;
    a.ye = ye ? B.io(ye, cells) : nullptr;
    a.mod = mod ? B.io(mod, cells) : nullptr;
    a.z = z ? B.io(z, cells) : nullptr;
    a.zero_err = zero_err ? B.io(zero_err, (size_t)cnt) : nullptr;
    a.cnt = cnt;
    a.n_obs = n_obs;
    a.n_grid = n_grid;
    a.tab_rows = tab_rows;
    if (!B.ready()) return B.finish(0);
    return B.finish(launch_simulate_cells(a, nullptr));
}

}  // extern "C"
