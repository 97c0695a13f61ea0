// mp_flows.h — radii, mass flows and torques of model samples (mp_model_flows, mp_model_flow_band; include/magprop_amd.h states the
// curves MP_FLOW_CURVE_* and the columns MP_FLOW_*): what the gfx950 kernels (mp_flows.hip), the host driver (mp_summaries.cpp) and a
// host test share -- the launch arguments and the launchers.
//
// flow_cells_kernel turns the (Mdisc, omega) rows of a chunk, as the curve kernels leave them, into up to MP_FLOW_NCURVES cell
// curves with the device functions the right-hand side is built from (walker_setup, disc_point, flow_state with cfg.n_ode,
// mdot_fb of mp_eval.hpp).  flow_reduce_kernel reduces the cell curves of every row to MP_FLOW_N columns.  Its sums follow
// mp_derive.h's segment rule (256 contiguous segments of derive_seg(G) intervals, terms in increasing index, segment totals in
// segment order, no FMA contraction, no floating-point atomic; stage and walk of mp_segwalk.h); its counts are integers and
// its extrema and first / last indices are taken under total orders (wg_best, wg_least of mp_wg.h), so neither depends on the
// order in which the points are visited.  tests/flows_restated.py is both kernels in numpy.
#pragma once
#include <stdint.h>

#include "mp_derive.h"
#include "mp_device.h"

namespace mp {

constexpr int kFlowThreads = kDeriveThreads;   // both kernels: workgroups of 256
constexpr int kFlowLane = 2;                   // grid points of a lane of flow_cells_kernel (one 16-byte access per curve)
// the curves flow_reduce_kernel reads
constexpr uint32_t kFlowReduceMask = (1u << MP_FLOW_CURVE_RM) | (1u << MP_FLOW_CURVE_FASTNESS) | (1u << MP_FLOW_CURVE_MDOT_PROP) |
                                     (1u << MP_FLOW_CURVE_MDOT_ACC) | (1u << MP_FLOW_CURVE_MDOT_FB) | (1u << MP_FLOW_CURVE_N_ACC) |
                                     (1u << MP_FLOW_CURVE_N_DIP) | (1u << MP_FLOW_CURVE_BRANCH);
constexpr uint32_t kFlowAllMask = (1u << MP_FLOW_NCURVES) - 1u;

struct FlowCellsArgs {
    const double *mdisc, *omega;   // [rows][n_grid] each: the states (the curve kernels' Mdisc and omega of a chunk)
    const double *t;               // the time of grid point g of row r: t[r * t_row_stride + g] (t_row_stride = 0: the grid)
    const double *pars;            // [rows][ndim]
    const int32_t *status;         // [rows]: a row whose status is not MP_STATUS_OK gets NaN cells (its states are not read)
    double *cell[MP_FLOW_NCURVES]; // [rows][n_grid] each; nullptr: not written
    int64_t t_row_stride;
    int32_t rows, n_grid, ndim, physical;
};

struct FlowReduceArgs {
    const double *cell[MP_FLOW_NCURVES];   // [rows][n_grid] each; the curves of kFlowReduceMask are read
    const int32_t *status;                 // [rows]: a row whose status is not MP_STATUS_OK gets MP_FLOW_N NaNs
    const double *tgrid;                   // [n_grid]
    double *out;                           // [rows][MP_FLOW_N]
    int32_t rows, n_grid;
};

// implemented in mp_flows.hip; return hipError_t as int
int launch_flow_cells(const DevShared &sh, const FlowCellsArgs &a, void *stream);
int launch_flow_reduce(const FlowReduceArgs &a, void *stream);

}  // namespace mp
