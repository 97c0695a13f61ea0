// mp_probe_smc.hip — test infrastructure only: the stage kernel of the SMC sampler (smc_stage_kernel) behind the extern "C" host
// function mpz_stage over HOST buffers, its tune kernel (smc_tune_kernel) behind mpz_tune, and the device runtime's double-precision exp, one value per lane, behind mpz_exp, which
// the restated stage takes where a device value is compared bit for bit (tests/test_gpu_smc_kernels.py, tests/test_gpu_smc.py).
// Builds into its own libmp_probe_smc.so, linked from the very object libmagprop_amd.so is linked from (build/all/mp_smc.hip.o):
// the kernel reached here is the product's compiled code, through the product's launcher.  Nothing here is part of
// libmagprop_amd.so, of include/magprop_amd.h or of the product's ABI.
//
// Both functions allocate on the current device, copy every buffer in (outputs too: the caller fills them with canaries, and what
// the kernel leaves alone comes back as it went), launch, synchronise, copy every buffer back and free.  They return 0, a
// hipError_t, or -1 for arguments they refuse: every size mp_smc_create refuses, and NULL pointers.  Nothing is launched then.
#include <hip/hip_runtime.h>

#include "mp_probe_bufs.h"
#include "mp_smc.h"

namespace mp {

namespace {

constexpr int kMaxRuns = 64;       // runs of a call (MP_MAX_DATASETS)
constexpr int kMaxN = 1 << 20;     // values of an mpz_exp call (the probe's own cap)

__global__ void __launch_bounds__(64) exp_kernel(const double *x, double *y, int n) {
    const long i = (long)blockIdx.x * 64 + threadIdx.x;
    if (i >= (long)n) return;
    y[i] = exp(x[i]);
}

}  // namespace

}  // namespace mp

using namespace mp;

extern "C" {

int mpz_min_particles(void) { return MP_SMC_MIN_PARTICLES; }
int mpz_max_particles(void) { return MP_SMC_MAX_PARTICLES; }
int mpz_max_stages(void) { return MP_SMC_MAX_STAGES; }
int mpz_max_runs(void) { return kMaxRuns; }

// y[i] = exp(x[i]); 1 <= n <= 1 << 20
int mpz_exp(const double *x, double *y, int n) {
    if (n < 1 || n > kMaxN || !x || !y) return -1;
    Bufs B;
    const double *dx = B.in(x, n);
    double *dy = B.io(y, n);
    if (B.ready()) exp_kernel<<<dim3((n + 63) / 64), dim3(64)>>>(dx, dy, n);
    return B.finish((int)hipGetLastError());
}

// One stage launch (stage index `stage`) over n_runs runs of n particles.  lnl[n_runs * n] is read; anc, units [n_runs * n], cum
// [n_runs * n] (64-bit), beta, lnz, status, nstage, ncall, nacc [n_runs], log[n_runs][MP_SMC_MAX_STAGES][4] and
// log_cnt[n_runs][MP_SMC_MAX_STAGES][2] go in and come back.
int mpz_stage(int n, int n_runs, uint64_t seed, uint32_t stage, double ess, const double *lnl, int32_t *anc, uint32_t *units,
              uint64_t *cum, double *beta, double *lnz, int32_t *status, int32_t *nstage, int64_t *ncall, int64_t *nacc, double *log,
              int64_t *log_cnt) {
    if (n < MP_SMC_MIN_PARTICLES || n > MP_SMC_MAX_PARTICLES || n_runs < 1 || n_runs > kMaxRuns || !(ess > 0.0 && ess < 1.0)) return -1;
    if (!lnl || !anc || !units || !cum || !beta || !lnz || !status || !nstage || !ncall || !nacc || !log || !log_cnt) return -1;
    for (int r = 0; r < n_runs; ++r)
        if (nstage[r] < 0 || nstage[r] > MP_SMC_MAX_STAGES) return -1;   // (the row of the log the stage would write)
    Bufs B;
    const size_t rows = (size_t)n_runs * n, lrows = (size_t)n_runs * MP_SMC_MAX_STAGES;
    SmcArgs a{};
    a.lnl_cur = const_cast<double *>(B.in(lnl, rows));   // (the stage kernel only reads the particles' lnl)
    a.anc = B.io(anc, rows);
    a.units = B.io(units, rows);
    a.cum = reinterpret_cast<unsigned long long *>(B.io(cum, rows));
    a.beta = B.io(beta, n_runs);
    a.lnz = B.io(lnz, n_runs);
    a.status = B.io(status, n_runs);
    a.nstage = B.io(nstage, n_runs);
    a.ncall = B.io(ncall, n_runs);
    a.nacc = B.io(nacc, n_runs);
    a.log = B.io(log, lrows * kSmcLogCols);
    a.log_cnt = B.io(log_cnt, lrows * 2);
    a.n = n;
    a.n_runs = n_runs;
    a.seed = seed;
    a.stage = stage;
    a.ess = ess;
    int rc = 0;
    if (B.ready()) rc = launch_smc_stage(a, nullptr);
    return B.finish(rc);
}

// One tune launch (round `round` of a stage of `walks` steps per round) over n_runs runs of n slots in ndim dimensions.
// start[n_runs * n][ndim] (where every slot started: the launch reads it through the identity genealogy), now[n_runs * n][ndim]
// and acc[n_runs * n] are read; g, rounds, moving [n_runs] go in and come back (a run takes part while moving = 1 and rounds =
// round); rho_d[n_runs][ndim], tune_rounds[n_runs] and tune_log[n_runs][2] (g used, rho: the row of stage 0) come back as the
// launch left them.  set[7] = corr, gain, accept_target, g_min, g_max, min_rounds, max_rounds.
int mpz_tune(int n, int n_runs, int ndim, int walks, int round, const double *set, const double *start, const double *now,
             const int32_t *acc, double *g, int32_t *rounds, int32_t *moving, double *rho_d, int32_t *tune_rounds, double *tune_log) {
    if (n < MP_SMC_MIN_PARTICLES || n > MP_SMC_MAX_PARTICLES || n_runs < 1 || n_runs > kMaxRuns || ndim < 1 || ndim > MP_MAX_NDIM) return -1;
    if (!set || !start || !now || !acc || !g || !rounds || !moving || !rho_d || !tune_rounds || !tune_log) return -1;
    const int min_rounds = (int)set[5], max_rounds = (int)set[6];
    if (walks < 1 || min_rounds < 1 || min_rounds > max_rounds || (long long)walks * max_rounds > MP_SMC_MAX_WALKS) return -1;
    if (round < 0 || round >= max_rounds) return -1;
    Bufs B;
    const size_t rows = (size_t)n_runs * n;
    std::vector<int32_t> ident(rows), one(n_runs, 1);
    for (size_t i = 0; i < rows; ++i) ident[i] = (int32_t)(i % (size_t)n);
    // every run's stage 0 is made: the row of the tuning log a run writes is row r * MP_SMC_MAX_STAGES
    std::vector<int32_t> tr((size_t)n_runs * MP_SMC_MAX_STAGES);
    std::vector<double> tl((size_t)n_runs * MP_SMC_MAX_STAGES * kSmcTuneCols);
    for (int r = 0; r < n_runs; ++r) {
        tr[(size_t)r * MP_SMC_MAX_STAGES] = tune_rounds[r];
        for (int c = 0; c < kSmcTuneCols; ++c) tl[(size_t)r * MP_SMC_MAX_STAGES * kSmcTuneCols + c] = tune_log[r * kSmcTuneCols + c];
    }
    SmcArgs a{};
    a.x_cur = const_cast<double *>(B.in(start, rows * ndim));
    a.x_next = const_cast<double *>(B.in(now, rows * ndim));
    a.acc = const_cast<int32_t *>(B.in(acc, rows));
    a.anc = const_cast<int32_t *>(B.in(ident.data(), rows));
    a.nstage = const_cast<int32_t *>(B.in(one.data(), n_runs));
    a.g = B.io(g, n_runs);
    a.rounds = B.io(rounds, n_runs);
    a.moving = B.io(moving, n_runs);
    a.rho_d = B.io(rho_d, (size_t)n_runs * ndim);
    a.tune_rounds = B.io(tr.data(), tr.size());
    a.tune_log = B.io(tl.data(), tl.size());
    a.n = n; a.n_runs = n_runs; a.ndim = ndim; a.walks = walks; a.stage = 0; a.round = round;
    a.corr = set[0]; a.gain = set[1]; a.accept_target = set[2]; a.g_min = set[3]; a.g_max = set[4];
    a.adapt_min = min_rounds; a.adapt_max = max_rounds;
    int rc = 0;
    if (B.ready()) rc = launch_smc_tune(a, nullptr);
    rc = B.finish(rc);
    for (int r = 0; r < n_runs; ++r) {
        tune_rounds[r] = tr[(size_t)r * MP_SMC_MAX_STAGES];
        for (int c = 0; c < kSmcTuneCols; ++c) tune_log[r * kSmcTuneCols + c] = tl[(size_t)r * MP_SMC_MAX_STAGES * kSmcTuneCols + c];
    }
    return rc;
}

}  // extern "C"
