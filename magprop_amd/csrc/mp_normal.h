// mp_normal.h — the Gaussian (Metropolis) and walk moves of the device-resident sampler (include/magprop_amd.h MP_MOVE_GAUSSIAN,
// MP_MOVE_WALK): what mp_sampler.cpp passes to the kernels of mp_normal.hip beside StretchArgs, which the other moves' kernels
// keep as it is.
#pragma once
#include "mp_device.h"

namespace mp {

// g.move says which of the two moves a launch proposes.  The Gaussian move's per-ensemble state is device memory [n_ensembles];
// the walk move has no state.
struct NormalArgs {
    const double *L;         // Gaussian: Cholesky factor of the covariance, lower triangle by rows, entry (a, b <= a) at a (a + 1) / 2 + b
    double *sigma;           // Gaussian: the scale of every ensemble; tuned by gauss_tune_kernel
    int64_t *acc_s;          // this step's accepted proposals: what the tune rule reads (and zeroes)
    int64_t *n_proposed;     // totals since mp_sampler_set_moves: proposals made, ...
    int64_t *n_accepted;     // ... proposals accepted, ...
    int64_t *n_tuned;        // ... tuning updates made; sigma is tuned while this is below tune_steps
    int64_t tune_steps;
    double target_accept;
    int32_t mode;            // MP_GAUSS_VECTOR, MP_GAUSS_RANDOM or MP_GAUSS_SEQUENTIAL
    int32_t walk_s;          // walk: members of the other half behind a proposal (resolved: 2 .. n_comp)
};

// One workgroup per slot of the active half of every ensemble (g.n_half * g.n_ensembles of them, on the builds of
// launch_point_kernel for that count); then one thread per ensemble (Gaussian steps only).  Return hipError_t as int.
int launch_normal_half(const DevShared &sh, const StretchArgs &g, const NormalArgs &na, void *stream);
int launch_gauss_tune(const NormalArgs &na, int n_ensembles, int n_walkers, void *stream);

}  // namespace mp
