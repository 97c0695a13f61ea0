// mp_slice.h — the ensemble slice-sampling move of the device-resident sampler (include/magprop_amd.h MP_MOVE_SLICE): what
// mp_sampler.cpp passes to the kernels of mp_slice.hip beside StretchArgs, which the other moves' kernels keep as it is.
#pragma once
#include "mp_device.h"

namespace mp {

// Per-ensemble state of the move, all device memory [n_ensembles], and the limits of a slice.
struct SliceArgs {
    double *mu;              // the scale of the initial interval, in units of the direction; tuned by slice_tune_kernel
    int64_t *nexpand_s;      // this step's stepping-out steps and rejected shrink points: what the tune rule reads (and zeroes)
    int64_t *ncontract_s;
    int64_t *nexpand;        // totals since mp_sampler_set_moves: stepping-out steps taken, ...
    int64_t *ncontract;      // ... shrink points rejected, ...
    int64_t *nfail;          // ... slices that ended where they started (shrink cap, or a zero direction), ...
    int64_t *neval;          // ... points evaluated, ...
    int64_t *n_tuned;        // ... slice steps taken; mu is tuned while this is below tune_steps
    int64_t tune_steps;
    int32_t max_steps_out;   // Neal's stepping-out budget m
    int32_t max_shrink;      // shrink points per slice before it counts as failed
};

// One workgroup per slot of the active half of every ensemble (g.n_half * g.n_ensembles of them, on the builds of
// launch_point_kernel for that count); then one thread per ensemble.  Return hipError_t as int.
int launch_slice_half(const DevShared &sh, const StretchArgs &g, const SliceArgs &sl, void *stream);
int launch_slice_tune(const SliceArgs &sl, int n_ensembles, void *stream);

}  // namespace mp
