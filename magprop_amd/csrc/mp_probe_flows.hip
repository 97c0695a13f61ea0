// mp_probe_flows.hip — test infrastructure only: the two kernels of the radii, mass flows and torques (flow_cells_kernel,
// flow_reduce_kernel; mp_flows.hip) behind extern "C" host functions over HOST buffers (tests/test_gpu_flows_kernels.py, cases of
// tests/flows_cases.py).  Builds into its own libmp_probe_flows.so, linked from the very object libmagprop_amd.so is linked from
// (build/all/mp_flows.hip.o): the kernels reached here are the product's compiled code, through the product's launchers.
// Nothing here is part of libmagprop_amd.so, of include/magprop_amd.h or of the product's ABI.
//
// mpf_cells does what the chunk loop of mp_model_flows (mp_summaries.cpp) does behind the curve launch, with the states in the
// caller's hands: every state has its own time, the parameter rows are physical, and the star constants come from the caller's
// mp_model_cfg by the function evaluator_create uses.  mpf_reduce is the reduction launch on caller-given cell curves.  Both
// return 0, a hipError_t, or -1 for arguments they refuse; nothing is launched then.
#include <hip/hip_runtime.h>

#include "mp_flows.h"
#include "mp_probe_bufs.h"

namespace mp {

namespace {

// the probe's own caps
constexpr int kMaxRows = 4096;
constexpr int kMaxGrid = 1 << 20;
constexpr int64_t kMaxElements = 1 << 22;   // rows * n_grid

bool sizes_ok(int rows, int n_grid, int min_grid) {
    return rows >= 1 && rows <= kMaxRows && n_grid >= min_grid && n_grid <= kMaxGrid && (int64_t)rows * n_grid <= kMaxElements;
}

}  // namespace

}  // namespace mp

using namespace mp;

extern "C" {

int mpf_threads(void) { return kFlowThreads; }
int mpf_lane(void) { return kFlowLane; }
int mpf_window(void) { return kDeriveWindow; }
int mpf_seg(int n_grid) { return derive_seg(n_grid); }
int mpf_curves(void) { return MP_FLOW_NCURVES; }
int mpf_columns(void) { return MP_FLOW_N; }
unsigned mpf_reduce_mask(void) { return kFlowReduceMask; }
int mpf_max_rows(void) { return kMaxRows; }

// t, mdisc, omega [rows][n_grid]; pars[rows][ndim] physical; status[rows] -> cells[popcount(mask)][rows][n_grid] in the order of
// the mask's bits (what it held is kept where the kernel writes nothing)
int mpf_cells(const mp_model_cfg *cfg, const double *t, const double *mdisc, const double *omega, const double *pars,
              const int32_t *status, int rows, int n_grid, int ndim, uint32_t mask, double *cells) {
    if (!cfg || !t || !mdisc || !omega || !pars || !status || !cells) return -1;
    if (!sizes_ok(rows, n_grid, 1) || ndim < 6 || ndim > MP_MAX_NDIM || mask == 0 || (mask & ~kFlowAllMask)) return -1;
    const size_t cnt = (size_t)rows * (size_t)n_grid;
    DevShared sh{};
    sh.cfg = *cfg;
    star_constants(sh, *cfg);
    Bufs B;
    FlowCellsArgs a{};
    a.t = B.in(t, cnt);
    a.t_row_stride = n_grid;
    a.mdisc = B.in(mdisc, cnt);
    a.omega = B.in(omega, cnt);
    a.pars = B.in(pars, (size_t)rows * ndim);
    a.status = B.in(status, (size_t)rows);
    double *d = B.io(cells, (size_t)__builtin_popcount(mask) * cnt);
    for (int c = 0, k = 0; c < MP_FLOW_NCURVES; ++c)
        if (mask & (1u << c)) a.cell[c] = d ? d + (size_t)k++ * cnt : nullptr;
    a.rows = rows;
    a.n_grid = n_grid;
    a.ndim = ndim;
    a.physical = 1;
    if (!B.ready()) return B.finish(0);
    return B.finish(launch_flow_cells(sh, a, nullptr));
}

// cells[MP_FLOW_NCURVES][rows][n_grid] (the curves outside mpf_reduce_mask() are not read), status[rows], tgrid[n_grid] ->
// out[rows][MP_FLOW_N] (what it held is ignored)
int mpf_reduce(const double *cells, const int32_t *status, const double *tgrid, int rows, int n_grid, double *out) {
    if (!cells || !status || !tgrid || !out) return -1;
    if (!sizes_ok(rows, n_grid, 2)) return -1;
    const size_t cnt = (size_t)rows * (size_t)n_grid;
    Bufs B;
    FlowReduceArgs a{};
    const double *d = B.in(cells, (size_t)MP_FLOW_NCURVES * cnt);
    for (int c = 0; c < MP_FLOW_NCURVES; ++c) a.cell[c] = d ? d + (size_t)c * cnt : nullptr;
    a.status = B.in(status, (size_t)rows);
    a.tgrid = B.in(tgrid, (size_t)n_grid);
    a.out = B.io(out, (size_t)rows * MP_FLOW_N);
    a.rows = rows;
    a.n_grid = n_grid;
    if (!B.ready()) return B.finish(0);
    return B.finish(launch_flow_reduce(a, nullptr));
}

}  // extern "C"
