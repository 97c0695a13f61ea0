// mp_probe_ladder.hip — test infrastructure only: the kernels of the ladder adaptation (ladder_init_kernel, ladder_adapt_kernel)
// and of the thermodynamic monitor (thermo_kernel) one launch at a time behind the extern "C" host functions mpt_init, mpt_adapt
// and mpt_thermo over HOST buffers, and the device runtime's double-precision exp and log, one value per lane, behind mpt_libm,
// which the restated rule takes where a device value is compared bit for bit (tests/test_gpu_ladder_kernels.py,
// tests/test_gpu_ladder.py).  Builds into its own libmp_probe_ladder.so, linked from the very object libmagprop_amd.so is linked
// from (build/all/mp_ladder.hip.o): the kernels reached here are the product's compiled code, through the product's launchers.
// Nothing here is part of libmagprop_amd.so, of include/magprop_amd.h or of the product's ABI.
//
// Every function allocates on the current device, copies every buffer in (outputs too: what a kernel leaves alone comes back as
// it went), launches, synchronises, copies every buffer back and frees.  They return 0, a hipError_t, or -1 for arguments they
// refuse (nothing is launched then).
#include <hip/hip_runtime.h>

#include "mp_ladder.h"
#include "mp_probe_bufs.h"

namespace mp {

namespace {

constexpr int kMaxN = 1 << 20;        // values of an mpt_libm call
constexpr int kMaxTemps = 1 << 16;    // the probe's own caps
constexpr int kMaxGroups = 1 << 10;
constexpr int kMaxRows = 1 << 12;

__global__ void __launch_bounds__(64) ladder_libm_kernel(int func, const double *x, double *y, int n) {
    const long i = (long)blockIdx.x * 64 + threadIdx.x;
    if (i >= (long)n) return;
    y[i] = func == 0 ? exp(x[i]) : log(x[i]);
}

bool shape_ok(int n_temps, int n_groups, int n_walkers) {
    return n_temps >= 3 && n_temps <= kMaxTemps && n_groups >= 1 && n_groups <= kMaxGroups && n_walkers >= 1;
}

}  // namespace

}  // namespace mp

using namespace mp;

extern "C" {

// y[i] = f(x[i]), func: 0 exp, 1 log; 1 <= n <= 1 << 20
int mpt_libm(int func, const double *x, double *y, int n) {
    if (func < 0 || func > 1 || n < 1 || n > kMaxN || !x || !y) return -1;
    Bufs B;
    const double *dx = B.in(x, n);
    double *dy = B.io(y, n);
    if (B.ready()) ladder_libm_kernel<<<dim3((n + 63) / 64), dim3(64)>>>(func, dx, dy, n);
    return B.finish((int)hipGetLastError());
}

// The init launch over n_groups ladders beta[n_groups][n_temps] and swap counts swaps[n_groups][n_temps - 1]: gap, prev
// [n_groups][n_temps - 1] and span[n_groups] come back.
int mpt_init(int n_temps, int n_groups, const double *beta, const int64_t *swaps, double *gap, double *span, int64_t *prev) {
    if (!shape_ok(n_temps, n_groups, 1) || !beta || !swaps || !gap || !span || !prev) return -1;
    Bufs B;
    const size_t np = (size_t)n_groups * (n_temps - 1);
    LadderArgs a{};
    a.beta = const_cast<double *>(B.in(beta, (size_t)n_groups * n_temps));   // (the init kernel only reads the ladder)
    a.swaps = B.in(swaps, np);
    a.gap = B.io(gap, np);
    a.span = B.io(span, n_groups);
    a.prev = B.io(prev, np);
    a.n_temps = n_temps; a.n_groups = n_groups; a.n_walkers = 1;
    int rc = 0;
    if (B.ready()) rc = launch_ladder_init(a, nullptr);
    return B.finish(rc);
}

// One update launch: beta[n_groups][n_temps], gap, prev [n_groups][n_temps - 1] and dropped[n_groups] go in and come back;
// span[n_groups] and swaps[n_groups][n_temps - 1] are read; history (NULL: none) is one row [n_groups][n_temps], written as row 0.
int mpt_adapt(int n_temps, int n_groups, int n_walkers, double kappa, const double *span, const int64_t *swaps, double *beta,
              double *gap, int64_t *prev, int64_t *dropped, double *history) {
    if (!shape_ok(n_temps, n_groups, n_walkers) || !span || !swaps || !beta || !gap || !prev || !dropped) return -1;
    Bufs B;
    const size_t np = (size_t)n_groups * (n_temps - 1), nb = (size_t)n_groups * n_temps;
    std::vector<double> work(2 * np, 0.0);
    LadderArgs a{};
    a.span = const_cast<double *>(B.in(span, n_groups));
    a.swaps = B.in(swaps, np);
    a.beta = B.io(beta, nb);
    a.gap = B.io(gap, np);
    a.prev = B.io(prev, np);
    a.dropped = B.io(dropped, n_groups);
    a.work = const_cast<double *>(B.in(work.data(), 2 * np));
    a.history = history ? B.io(history, nb) : nullptr;
    a.n_temps = n_temps; a.n_groups = n_groups; a.n_walkers = n_walkers;
    a.t = 0;
    a.kappa = kappa;
    int rc = 0;
    if (B.ready()) rc = launch_ladder_adapt(a, nullptr);
    return B.finish(rc);
}

// One thermo launch over lnp[n_rows][n_ensembles][n_walkers], rows [first, first + rows): sum, n_finite, n_nonfinite [n_ensembles]
// go in and come back.
int mpt_thermo(int n_walkers, int n_ensembles, int n_rows, int first, int rows, const double *lnp, double *sum, int64_t *n_finite,
               int64_t *n_nonfinite) {
    if (n_walkers < 1 || n_ensembles < 1 || n_ensembles > kMaxTemps || n_rows < 1 || n_rows > kMaxRows) return -1;
    if (first < 0 || rows < 0 || first + rows > n_rows || !lnp || !sum || !n_finite || !n_nonfinite) return -1;
    if ((size_t)n_walkers * n_ensembles * n_rows > ((size_t)1 << 26)) return -1;
    Bufs B;
    ThermoArgs a{};
    a.lnp = B.in(lnp, (size_t)n_rows * n_ensembles * n_walkers);
    a.sum = B.io(sum, n_ensembles);
    a.n_finite = B.io(n_finite, n_ensembles);
    a.n_nonfinite = B.io(n_nonfinite, n_ensembles);
    a.n_walkers = n_walkers; a.n_ensembles = n_ensembles; a.first = first; a.rows = rows;
    int rc = 0;
    if (B.ready()) rc = launch_thermo(a, nullptr);
    return B.finish(rc);
}

}  // extern "C"
