// mp_smc.h — the tempered sequential Monte Carlo sampler (include/magprop_amd.h mp_smc_*): what mp_smc.cpp passes to the three
// kernels of mp_smc.hip.  Particle j of run r is row r * n + j of either particle buffer; a stage reads one buffer (cur) and its
// moves write the other (next), so no workgroup reads what another one writes.  With adaptation on (adapt_max > 0) the moves of
// a stage are rounds of `walks` steps: round 0 as before, round k >= 1 continues slot j in place from its own row of next, and
// the tune kernel behind every round decides per run whether another one follows (rounds, moving) and sets the run's scale g.
#pragma once
#include "mp_device.h"

namespace mp {

constexpr uint32_t kSmcCtr = 0x534D0000u;   // fourth counter word: 0x534D0000 the stage's offset, + 2 t + 1 and + 2 t + 2 step t
constexpr int kSmcLogCols = 4;              // a stage's row of the log: beta, d, ESS(d), ln Z
constexpr int kSmcTuneCols = 2;             // a stage's row of the tuning log: g, rho

struct SmcArgs {
    double *x_cur, *x_next;          // [n_runs * n][ndim]
    double *lnl_cur, *lnl_next;      // [n_runs * n] the untempered lnprob (NaN stored as -inf)
    int32_t *st_cur, *st_next;       // [n_runs * n] status of every particle (MP_STATUS_*)
    int32_t *acc;                    // [n_runs * n] accepted steps of the slot's last move
    const int32_t *ds_id;            // [n_runs] dataset of every run
    int32_t *anc;                    // [n_runs * n] the last stage's ancestors (indices inside the run)
    uint32_t *units;                 // [n_runs * n] the last stage's integer weights
    unsigned long long *cum;         // [n_runs * n] their cumulative sums
    double *beta;                    // [n_runs]
    double *lnz;                     // [n_runs]
    int32_t *status;                 // [n_runs] MP_SMC_RUNNING, _DONE, _FAILED, _STAGE_LIMIT
    int32_t *nstage;                 // [n_runs] stages made
    int64_t *ncall;                  // [n_runs] evaluations (those of mp_smc_set_particles included)
    int64_t *nacc;                   // [n_runs] accepted steps
    int64_t *nfail;                  // [n_runs] evaluations whose model failed (status not MP_STATUS_OK)
    double *log;                     // [n_runs][MP_SMC_MAX_STAGES][kSmcLogCols]
    int64_t *log_cnt;                // [n_runs][MP_SMC_MAX_STAGES][2]: ncall and nacc as the stage found them
    double lower[MP_MAX_NDIM], upper[MP_MAX_NDIM];   // the prior box (sampler coordinates)
    int32_t n, n_runs, ndim;
    int32_t walks;                   // Metropolis steps per move
    int32_t target;                  // 0: posterior, 1 and 2: point_eval's test targets
    int32_t mode;                    // move: 0 a stage's moves, 1 evaluate x_cur as it is
    uint32_t stage;                  // the stage's index (the Philox counter): stage t makes a run's nstage t + 1
    uint32_t pad;
    uint64_t seed;
    double g0, sig3, ess;            // sig3 = sigma sqrt(3); ess: the target fraction of the finite particles
    // adaptation (mp_smc_set_adaptive); adapt_max = 0: off, nothing below is read or written
    double *g;                       // [n_runs] the run's scale: what its moves read where the others read g0
    int32_t *rounds;                 // [n_runs] rounds made in the run's current stage (the stage kernel resets it)
    int32_t *moving;                 // [n_runs] 1: the stage's moves go on (set by the stage kernel, cleared by the round that stops)
    int32_t *tune_rounds;            // [n_runs][MP_SMC_MAX_STAGES] rounds the stage made
    double *tune_log;                // [n_runs][MP_SMC_MAX_STAGES][kSmcTuneCols] the g its moves used, rho at the stop
    double *rho_d;                   // [n_runs][ndim] the last tune launch's rho of every dimension, or NULL (the probe's)
    int32_t adapt_min, adapt_max;    // rounds of a stage: at least, at most
    int32_t round;                   // the launch's round (move and tune): it acts on the runs whose rounds equals it
    int32_t pad2;
    double corr, gain, accept_target, g_min, g_max;
};

// one workgroup per run (reweight, next beta, ln Z, ancestors), then one per particle (the tempered walk of the slot; mode 1: one
// evaluation of the particle as it is); return hipError_t as int
int launch_smc_stage(const SmcArgs &a, void *stream);
int launch_smc_move(const DevShared &sh, const SmcArgs &a, void *stream);
// one workgroup per run behind round a.round of an adaptive stage: rho, the decision, and at the stop the tuning row and the next g
int launch_smc_tune(const SmcArgs &a, void *stream);

}  // namespace mp
