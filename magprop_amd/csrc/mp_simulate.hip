// mp_simulate.hip — gfx950 kernel of the simulated light curves (mp_simulate, include/magprop_amd.h; the cell is stated in
// mp_simulate.h).
//
// simulate_cells_kernel is elementwise over a chunk's rows x pairs of observations: thread k of the launch takes pair k % npairs
// (observations 2 p and 2 p + 1) of row k / npairs, so consecutive threads read consecutive entries of the bracket tables and
// write consecutive cells of a row, and one Philox draw serves both observations of a pair.  The two curve reads per observation
// are gathers inside one Ltot row.  No LDS, no scratch memory, no atomic: the zero-error mark of a row is a plain store of 1 by
// every thread that finds one.
#include <hip/hip_runtime.h>

#include "mp_device.h"
#include "mp_normal_pair.h"
#include "mp_simulate.h"

namespace mp {

namespace {

__global__ __launch_bounds__(kSimThreads) void simulate_cells_kernel(const SimCellsArgs a) {
#pragma clang fp contract(off)
    const int npairs = (a.n_obs + 1) >> 1;
    const int64_t k = (int64_t)blockIdx.x * kSimThreads + threadIdx.x;
    if (k >= (int64_t)a.cnt * npairs) return;
    const int s = (int)(k / npairs), p = (int)(k % npairs);
    const bool ok = a.status[s] == MP_STATUS_OK;
    const size_t tab = (a.tab_rows > 1 ? (size_t)s : 0) * (size_t)a.n_obs, cell = (size_t)s * (size_t)a.n_obs;
    double n2[2] = {0.0, 0.0};
    if (ok && (a.y || a.z)) {
        const uint64_t i = (uint64_t)(a.row0 + s);
        uint32_t s4[4];
        philox4x32_10((uint32_t)a.seed, (uint32_t)(a.seed >> 32), (uint32_t)i, (uint32_t)p, 0u, kSimCtr, s4);
        normal_pair(s4, n2[0], n2[1]);
    }
    bool zero = false;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int j = 2 * p + h;
        if (j >= a.n_obs) break;
        double mod = __builtin_nan(""), ye = mod, z = mod, y = mod;
        if (ok) {
            const int g = min(max(a.g[tab + j], 0), a.n_grid - 1);
            const double dx = a.dx[tab + j];
            const double *row = a.ltot + (size_t)s * (size_t)a.n_grid;
            const double La = row[g];
            mod = La;
            if (dx != 0.0 && g < a.n_grid - 1) {   // off a knot: the interval's other end is read
                const double Lb = row[g + 1];
                const double d = Lb - La;
                const double slope = d * a.idt[tab + j];
                const double rise = slope * dx;
                mod = rise + La;
            }
            ye = a.yerr ? a.yerr[tab + j] : a.frac_err * fabs(mod);
            zero = zero || ye == 0.0;
            z = n2[h];
            const double noise = ye * z;
            y = mod + noise;
        }
        if (a.mod) a.mod[cell + j] = mod;
        if (a.ye) a.ye[cell + j] = ye;
        if (a.z) a.z[cell + j] = z;
        if (a.y) a.y[cell + j] = y;
    }
    if (zero && a.zero_err) a.zero_err[s] = 1;
}

}  // namespace

int launch_simulate_cells(const SimCellsArgs &a, void *stream) {
    const int64_t threads = (int64_t)a.cnt * ((a.n_obs + 1) / 2);
    hipLaunchKernelGGL(simulate_cells_kernel, dim3((unsigned)((threads + kSimThreads - 1) / kSimThreads)), dim3(kSimThreads), 0,
                       (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

}  // namespace mp
