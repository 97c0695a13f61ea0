// mp_simulate.h — simulated light curves of parameter rows (mp_simulate; include/magprop_amd.h states every operation): what the
// gfx950 kernel (mp_simulate.hip), the host drivers (mp_summaries.cpp; mp_capi.cpp for the bracket), the probe and a host check
// share -- the bracket of an observed time, the arguments and the launcher.  No HIP type: a plain host compiler reads it.
//
// Cell (i, j), i the row's index in the call: La = L[g], and off a knot Lb = L[g + 1]; mod = La where dx == 0, otherwise
// ((Lb - La) * idt) * dx + La; ye = the given error or frac_err * |mod|; z the normal of Philox (seed; i, j / 2, 0, kSimCtr)
// through normal_pair (mp_normal_pair.h), its first for even j and its second for odd j; y = mod + ye * z.  Every operation
// rounds on its own (no FMA contraction).  A row whose status is not MP_STATUS_OK gives NaN cells.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/magprop_amd.h"

namespace mp {

constexpr uint32_t kSimCtr = 0x53494D00u;   // fourth counter word of every noise draw ('SIM\0')
constexpr int kSimThreads = 256;            // one thread per pair of observations of a row

// The bracket of an observed time x on the grid t (strictly increasing, two points or more; t[0] <= x <= t.back(), which the
// caller has checked): the interval g with t[g] <= x < t[g + 1], the last point in the last interval (g = n - 2, as np.interp
// places it), dx = x - t[g] and idt = 1 / (t[g + 1] - t[g]).  What mp_set_dataset keeps of an observation.
inline void obs_bracket(const std::vector<double> &t, double x, int32_t &g, double &dx, double &idt) {
    const int n = (int)t.size();
    g = (int32_t)std::min(std::max((int)(std::upper_bound(t.begin(), t.end(), x) - t.begin()) - 1, 0), n - 2);
    dx = x - t[(size_t)g];
    idt = 1.0 / (t[(size_t)g + 1] - t[(size_t)g]);
}

// The bracket mp_simulate takes: obs_bracket, but the last grid point sits ON its knot (g = n - 1, the largest index with
// t[g] <= x; dx = 0, idt = 0), so that every grid time reads its own curve value and nothing else.
inline void sim_bracket(const std::vector<double> &t, double x, int32_t &g, double &dx, double &idt) {
    obs_bracket(t, x, g, dx, idt);
    if (x == t.back()) {
        g = (int32_t)t.size() - 1;
        dx = 0.0;
        idt = 0.0;
    }
}

struct SimCellsArgs {
    const double *ltot;      // [cnt][n_grid]: the chunk's Ltot rows, walker-major as the curve kernels write them
    const int32_t *status;   // [cnt]: a row whose status is not MP_STATUS_OK gives NaN cells (its curve is not read)
    const int32_t *g;        // [tab_rows][n_obs] sim_bracket of every time; tab_rows = 1 (shared by the rows) or cnt
    const double *dx, *idt;  // likewise
    const double *yerr;      // likewise, or nullptr: frac_err * |mod|
    double frac_err;
    uint64_t seed;
    int64_t row0;            // index in the call of the chunk's first row: row s draws with counter word row0 + s
    double *y, *ye, *mod, *z;   // [cnt][n_obs] each; any may be nullptr: not written
    int32_t *zero_err;       // [cnt]: set to 1 for a row with a cell whose error is 0 (never cleared here; may be nullptr)
    int32_t cnt, n_obs, n_grid, tab_rows;
};

// implemented in mp_simulate.hip; returns hipError_t as int
int launch_simulate_cells(const SimCellsArgs &a, void *stream);

}  // namespace mp
