// mp_probe_wselect.hip — test infrastructure only: the weighted select of the band (band_wselect_kernel) behind one extern "C"
// host function over HOST buffers (tests/test_gpu_wband_kernels.py, cases of tests/wband_cases.py).  Builds into its own
// libmp_probe_wselect.so, linked from the very object libmagprop_amd.so is linked from (build/all/mp_band.hip.o): the kernel
// reached here is the product's compiled code, through the product's launcher.  Nothing here is part of libmagprop_amd.so, of
// include/magprop_amd.h or of the product's ABI.
//
// mpv_wselect allocates on the current device, copies every buffer in (the output too: the caller fills it with canaries, and
// what the kernel leaves alone comes back as it went), launches, synchronises, copies the output back and frees.  It returns 0, a
// hipError_t, or -1 for arguments it refuses: every size mp_model_band_weighted refuses, a unit above 2^31 and NULL pointers.
// Nothing is launched then.
#include <hip/hip_runtime.h>

#include "mp_band.h"
#include "mp_probe_bufs.h"

using namespace mp;

extern "C" {

int mpv_max_grid(void) { return 1 << 16; }   // grid points of a call (the probe's own cap)

// cols[n_grid][n], units[n], q[nq] -> out[nq][n_grid]
int mpv_wselect(const double *cols, const uint32_t *units, int n, int n_grid, const double *q, int nq, double *out) {
    if (n < 1 || n > MP_BAND_MAX_SAMPLES || n_grid < 1 || n_grid > mpv_max_grid() || nq < 1 || nq > MP_BAND_MAX_Q) return -1;
    if (!cols || !units || !q || !out) return -1;
    for (int j = 0; j < nq; ++j)
        if (!(q[j] >= 0.0 && q[j] <= 1.0)) return -1;   // (mp_model_band_weighted: each finite and in [0, 1])
    for (int i = 0; i < n; ++i)
        if (units[i] > kBandUnitMax) return -1;         // (the sum over n rows has to stay below 2^46)
    BandQ bq{};
    for (int j = 0; j < nq; ++j) bq.q[j] = q[j];
    bq.nq = nq;
    Bufs B;
    const double *c = B.in(cols, (size_t)n * n_grid);
    const uint32_t *u = B.in(units, (size_t)n);
    double *o = B.io(out, (size_t)nq * n_grid);
    int rc = 0;
    if (B.ready()) rc = launch_band_wselect(c, u, n, n_grid, bq, o, nullptr);
    return B.finish(rc);
}

}  // extern "C"
