// mp_ladder.h — the tempered sampler's ladder adaptation (include/magprop_amd.h mp_sampler_set_ladder_adaptation) and the
// per-temperature sums of lnL behind mp_sampler_get_thermo: what mp_sampler.cpp and mp_monitor.cpp pass to the three kernels of
// mp_ladder.hip.  A group is n_temps consecutive ensembles; its ladder beta[group * n_temps + i] keeps both ends and moves the
// gaps g_i = ln beta_i - ln beta_{i+1} of ln beta, whose sum L = -ln beta_{T-1} is fixed.
#pragma once
#include <stdint.h>

namespace mp {

struct LadderArgs {
    double *beta;            // [n_groups][n_temps] the ladders the sampler's kernels read; entries 1 .. n_temps - 2 are written
    double *gap;             // [n_groups][n_temps - 1] g_i
    double *span;            // [n_groups] L
    int64_t *prev;           // [n_groups][n_temps - 1] the pair's accepted swaps at the last update
    const int64_t *swaps;    // [n_groups][n_temps - 1] the pair's accepted swaps now (the swap sweep's counters)
    int64_t *dropped;        // [n_groups] updates not taken
    double *work;            // [n_groups][2][n_temps - 1] scratch of an update
    double *history;         // [n_adapt][n_groups][n_temps] the ladders after every update, or NULL
    int32_t n_temps, n_groups, n_walkers, pad;
    int64_t t;               // the update's index (the row of history it writes)
    double kappa;            // the update's rate, formed on the host
};

struct ThermoArgs {
    const double *lnp;       // [rows of the chunk][n_ensembles][n_walkers] the chunk's stored lnprob
    double *sum;             // [n_ensembles] sum of the finite lnprob
    int64_t *n_finite;       // [n_ensembles]
    int64_t *n_nonfinite;    // [n_ensembles]
    int32_t n_walkers, n_ensembles;
    int32_t first, rows;     // rows [first, first + rows) of the chunk go in
};

// one workgroup per group; return hipError_t as int
int launch_ladder_init(const LadderArgs &a, void *stream);
int launch_ladder_adapt(const LadderArgs &a, void *stream);
// one workgroup per ensemble, the chunk's rows in step order
int launch_thermo(const ThermoArgs &a, void *stream);

}  // namespace mp
