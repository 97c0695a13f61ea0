// mp_probe_libm.hip — test infrastructure only: the device runtime's double-precision log, cos, sin and sqrt, one value per
// lane, behind the extern "C" host function mpl_libm (tests/test_gpu_sampler_posterior.py).  The sampler's kernels call these
// functions for ln u, the stretch move's ln z and the normals of the KDE move, and numpy's miss them by an ulp now and then: the
// restated draw takes the device's where a device value is compared bit for bit.  Builds into its own libmp_probe_libm.so;
// nothing here is part of libmagprop_amd.so, of include/magprop_amd.h or of the product's ABI.
//
// mpl_libm takes HOST pointers, allocates, copies, launches, synchronises and frees on the current device and returns 0, a
// hipError_t, or -1 for arguments it refuses (nothing is launched then).
#include <hip/hip_runtime.h>

#include "mp_probe_bufs.h"

namespace mp {

namespace {

constexpr int kMaxN = 1 << 20;

__global__ void __launch_bounds__(64) libm_kernel(int func, const double *x, double *y, int n) {
    const long i = (long)blockIdx.x * 64 + threadIdx.x;
    if (i >= (long)n) return;
    const double v = x[i];
    y[i] = func == 0 ? log(v) : (func == 1 ? cos(v) : (func == 2 ? sin(v) : sqrt(v)));
}

}  // namespace

}  // namespace mp

using namespace mp;

extern "C" {

// y[i] = f(x[i]), func: 0 log, 1 cos, 2 sin, 3 sqrt; 1 <= n <= 1 << 20
int mpl_libm(int func, const double *x, double *y, int n) {
    if (func < 0 || func > 3 || n < 1 || n > kMaxN || !x || !y) return -1;
    Bufs B;
    const double *dx = B.in(x, n);
    double *dy = B.io(y, n);
    if (B.ready()) libm_kernel<<<dim3((n + 63) / 64), dim3(64)>>>(func, dx, dy, n);
    return B.finish((int)hipGetLastError());
}

}  // extern "C"
