// mp_probe_derive.hip — test infrastructure only: the derived-quantity kernel (derive_kernel; mp_derive.hip) behind one extern "C"
// host function over HOST buffers (tests/test_gpu_derive_kernels.py, cases of tests/derive_cases.py).  Builds into its own
// libmp_probe_derive.so, linked from the very object libmagprop_amd.so is linked from (build/all/mp_derive.hip.o): the kernel
// reached here is the product's compiled code, through the product's launcher launch_derive.  Nothing here is part of
// libmagprop_amd.so, of include/magprop_amd.h or of the product's ABI.
//
// mpd_run_derive does what the chunk loop of mp_model_derived (mp_summaries.cpp) does behind the curve launch, with the curves in the
// caller's hands.  It returns 0, a hipError_t, or -1 for arguments it refuses; nothing is launched then.
#include <hip/hip_runtime.h>

#include "mp_derive.h"
#include "mp_probe_bufs.h"

namespace mp {

namespace {

// the probe's own caps
constexpr int kMaxRows = 4096;
constexpr int kMaxGrid = 1 << 20;
constexpr int64_t kMaxElements = 1 << 24;   // n * n_grid

}  // namespace

}  // namespace mp

using namespace mp;

extern "C" {

int mpd_threads(void) { return kDeriveThreads; }
int mpd_window(void) { return kDeriveWindow; }
int mpd_seg(int n_grid) { return derive_seg(n_grid); }
int mpd_columns(void) { return MP_DERIVED_N; }
int mpd_max_rows(void) { return kMaxRows; }
int mpd_max_grid(void) { return kMaxGrid; }

// curves[5][n][n_grid] (Ltot, Lprop, Ldip, Mdisc, omega), status[n], tgrid[n_grid] -> out[n][MP_DERIVED_N] (what it held is ignored)
int mpd_run_derive(const double *curves, const int32_t *status, const double *tgrid, int n, int n_grid, double *out) {
    if (!curves || !status || !tgrid || !out) return -1;
    if (n < 1 || n > kMaxRows || n_grid < 2 || n_grid > kMaxGrid || (int64_t)n * n_grid > kMaxElements) return -1;
    const size_t rows = (size_t)n * (size_t)n_grid;
    Bufs B;
    DeriveArgs a{};
    const double *d = B.in(curves, 5 * rows);
    for (int c = 0; c < 5; ++c) a.curve[c] = d ? d + (size_t)c * rows : nullptr;
    a.status = B.in(status, (size_t)n);
    a.tgrid = B.in(tgrid, (size_t)n_grid);
    a.out = B.io(out, (size_t)n * MP_DERIVED_N);
    a.n = n;
    a.n_grid = n_grid;
    if (!B.ready()) return B.finish(0);
    return B.finish(launch_derive(a, nullptr));
}

}  // extern "C"
