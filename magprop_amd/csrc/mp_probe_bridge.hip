// mp_probe_bridge.hip — test infrastructure only: the fixed-point kernel of the bridge-sampling evidence (bridge_fixed_kernel)
// alone, and its moments kernels (bridge_moments_kernel, bridge_combine_kernel) alone, on caller-given arrays behind the extern
// "C" host functions mpb_fixed and mpb_moments over HOST buffers (tests/test_gpu_bridge_kernels.py).  Builds into its own
// libmp_probe_bridge.so, linked from the very object libmagprop_amd.so is linked from (build/all/mp_bridge.hip.o): the kernels
// reached here are the product's compiled code, through the product's launchers.  Nothing here is part of libmagprop_amd.so, of
// include/magprop_amd.h or of the product's ABI.
//
// Every function allocates on the current device, copies every buffer in (outputs too), launches, synchronises, copies every
// buffer back and frees.  They return 0, a hipError_t, or -1 for arguments they refuse (nothing is launched then).
#include <hip/hip_runtime.h>

#include "mp_bridge.h"
#include "mp_probe_bufs.h"

namespace mp {

namespace {

constexpr int64_t kMaxRows = 1 << 22;   // the probe's own cap on every array

}  // namespace

}  // namespace mp

using namespace mp;

extern "C" {

// The fixed point over a[n1] and b[n_rep][n2] with the host's constants as the caller formed them: out[n_rep][MP_BRIDGE_NOUT].
int mpb_fixed(const double *a, int64_t n1, const double *b, int64_t n2, int n_rep, double ln_s1, double ln_s2, double ln_n1,
              double ln_n2, double tau, double ln_volume, int max_iter, double tol, double *out) {
    if (!a || !b || !out || n1 < 1 || n2 < 1 || n1 > kMaxRows || n_rep < 1 || n_rep > MP_BRIDGE_MAX_REP || n2 * n_rep > kMaxRows || max_iter < 1)
        return -1;
    Bufs B;
    BridgeFixedArgs f{};
    f.a = B.in(a, (size_t)n1);
    f.b = B.in(b, (size_t)n2 * n_rep);
    f.out = B.io(out, (size_t)n_rep * MP_BRIDGE_NOUT);
    f.n1 = n1; f.n2 = n2;
    f.ln_s1 = ln_s1; f.ln_s2 = ln_s2; f.ln_n1 = ln_n1; f.ln_n2 = ln_n2;
    f.tau = tau; f.ln_volume = ln_volume; f.tol = tol;
    f.max_iter = max_iter; f.n_rep = n_rep;
    int rc = 0;
    if (B.ready()) rc = launch_bridge_fixed(f, nullptr);
    return B.finish(rc);
}

// The sums of x[n][ndim] about pivot[ndim], launched in chunks of chunk_blocks blocks of MP_BRIDGE_BLOCK rows (the way
// mp_bridge_logz moves the rows; any chunk_blocks >= 1 gives the same bits): out[ndim + ndim (ndim + 1) / 2].
int mpb_moments(const double *x, int64_t n, int ndim, const double *pivot, int64_t chunk_blocks, double *out) {
    if (!x || !pivot || !out || n < 1 || n > kMaxRows || ndim < 1 || ndim > MP_MAX_NDIM || chunk_blocks < 1) return -1;
    Bufs B;
    const int nm = bridge_n_moments(ndim);
    const int64_t n_blocks = (n + MP_BRIDGE_BLOCK - 1) / MP_BRIDGE_BLOCK, chunk = chunk_blocks * MP_BRIDGE_BLOCK;
    std::vector<double> zero((size_t)n_blocks * nm, 0.0);
    const double *dx = B.in(x, (size_t)n * ndim);
    double *part = const_cast<double *>(B.in(zero.data(), zero.size()));
    double *dout = B.io(out, (size_t)nm);
    int rc = 0;
    for (int64_t lo = 0; B.ready() && !rc && lo < n; lo += chunk)
        rc = launch_bridge_moments(dx + lo * ndim, n - lo < chunk ? n - lo : chunk, ndim, pivot, lo / MP_BRIDGE_BLOCK, part, nullptr);
    if (B.ready() && !rc) rc = launch_bridge_combine(part, n_blocks, ndim, dout, nullptr);
    return B.finish(rc);
}

}  // extern "C"
