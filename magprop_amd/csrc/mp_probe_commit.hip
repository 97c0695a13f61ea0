// mp_probe_commit.hip — test infrastructure only: the sampler's deciding kernels (stretch_step_commit_kernel<TEMPERED>,
// stretch_apply_kernel, stretch_swap_kernel, order_kernel; mp_kernels.hip) one launch at a time behind extern "C" host functions
// over HOST buffers (tests/test_gpu_commit_kernels.py, cases of tests/commit_cases.py).  Builds into its own
// libmp_probe_commit.so, linked from the very object libmagprop_amd.so is linked from (build/all/mp_kernels.hip.o): the kernels
// reached here are the product's compiled code, through the product's launchers launch_stretch_step_commit, launch_stretch_apply,
// launch_stretch_swap and launch_order.  Nothing here is part of libmagprop_amd.so, of include/magprop_amd.h or of the
// product's ABI.
//
// Every mpc_* function fills a StretchArgs (mpc_order: a DevShared) from plain arguments, uploads, launches once, synchronises
// and returns the writable buffers as the device holds them.  It returns 0, a hipError_t, or -1 for arguments it refuses;
// nothing is launched then.  Refused: the sizes mp_sampler_create and the launchers refuse, and every index a kernel would
// address memory with -- an entry of perm outside [0, n_walkers), a partner slot of spec outside [0, n_half), a chain_row outside
// [0, n_rows), an ens_order that is no permutation of the ensembles -- so that no case can make a kernel leave its buffers.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "mp_device.h"
#include "mp_probe_bufs.h"

namespace mp {

namespace {

// the probe's own caps
constexpr int kMaxWalkers = 1 << 12;        // per ensemble
constexpr int kMaxEnsembles = 1 << 10;
constexpr int kMaxTotal = 1 << 16;          // walkers of all ensembles
constexpr int kMaxRows = 16;                // rows of a chain buffer
constexpr int kMaxBadCap = 1 << 16;
constexpr int kMaxOrderN = 1 << 20;
constexpr int kMaxDatasets = 1 << 12;

// the state of a sampler and where its chain row goes
struct State {
    double *pos, *lnprob;
    int64_t *n_accepted;
    const int32_t *perm;
    int n_walkers, n_ensembles, ndim;
    double *chain, *chain_lnp;
    int chain_row, n_rows;
};

bool state_ok(const State &s) {
    if (!s.pos || !s.lnprob || !s.n_accepted || !s.perm) return false;
    if (s.n_walkers < 2 || (s.n_walkers & 1) || s.n_walkers > kMaxWalkers) return false;              // (mp_sampler_create)
    if (s.n_ensembles < 1 || s.n_ensembles > kMaxEnsembles || s.ndim < 1 || s.ndim > MP_MAX_NDIM) return false;
    if ((int64_t)s.n_walkers * s.n_ensembles > kMaxTotal) return false;
    const size_t nt = (size_t)s.n_walkers * s.n_ensembles;
    for (size_t i = 0; i < nt; ++i)
        if (s.perm[i] < 0 || s.perm[i] >= s.n_walkers) return false;
    if (s.chain) {
        if (!s.chain_lnp || s.n_rows < 1 || s.n_rows > kMaxRows || s.chain_row < 0 || s.chain_row >= s.n_rows) return false;
    } else if (s.chain_lnp) {
        return false;
    }
    return true;
}

// the device copies of the state, and the part of a StretchArgs every kernel here reads
StretchArgs upload(Bufs &B, const State &s) {
    const size_t nt = (size_t)s.n_walkers * s.n_ensembles, nd = (size_t)s.ndim;
    StretchArgs g{};
    g.pos = B.io(s.pos, nt * nd);
    g.lnprob = B.io(s.lnprob, nt);
    g.n_accepted = B.io(s.n_accepted, nt);
    g.perm = B.in(s.perm, nt);
    if (s.chain) {
        g.chain = B.io(s.chain, (size_t)s.n_rows * nt * nd);
        g.chain_lnp = B.io(s.chain_lnp, (size_t)s.n_rows * nt);
        g.chain_row = s.chain_row;
    }
    g.n_walkers = s.n_walkers; g.n_half = s.n_walkers / 2; g.n_ensembles = s.n_ensembles;
    g.n_total = (int32_t)nt; g.ndim = s.ndim; g.target = 1; g.a = 2.0;
    return g;
}

// bad_log[bad_cap + 1][ndim]: the rows of the log and a guard row behind them, which travels back with them
bool bad_ok(const double *bad_log, const uint32_t *bad_count, int bad_cap) {
    return bad_count && bad_cap >= 0 && bad_cap <= kMaxBadCap;
}
void upload_bad(Bufs &B, StretchArgs &g, double *bad_log, uint32_t *bad_count, int bad_cap) {
    g.bad_log = bad_log ? B.io(bad_log, ((size_t)bad_cap + 1) * (size_t)g.ndim) : nullptr;
    g.bad_count = B.io(bad_count, 1);
    g.bad_cap = (uint32_t)bad_cap;
}

}  // namespace

}  // namespace mp

using namespace mp;

extern "C" {

int mpc_max_ndim(void) { return MP_MAX_NDIM; }
int mpc_spec_extra(void) { return kSpecExtra; }
int mpc_max_walkers(void) { return kMaxWalkers; }
int mpc_max_ensembles(void) { return kMaxEnsembles; }
int mpc_max_total(void) { return kMaxTotal; }
int mpc_max_rows(void) { return kMaxRows; }
int mpc_max_bad_cap(void) { return kMaxBadCap; }
int mpc_max_order_n(void) { return kMaxOrderN; }
int mpc_max_datasets(void) { return kMaxDatasets; }

// The decisions of a whole step (stretch_step_commit_kernel; the TEMPERED build where beta is given) from the outcome rows
// spec[3][n_half * n_ensembles][ndim + kSpecExtra].  pos[n_total][ndim], lnprob[n_total], n_accepted[n_total],
// perm[n_ensembles][n_walkers]; chain[n_rows][n_total][ndim] with chain_lnp[n_rows][n_total], or both NULL; beta[n_ensembles] or
// NULL; bad_log[bad_cap + 1][ndim] (the last row a guard) or NULL, bad_count[1].
int mpc_commit(double *pos, double *lnprob, int64_t *n_accepted, const int32_t *perm, const double *spec, int n_walkers,
               int n_ensembles, int ndim, double *chain, double *chain_lnp, int chain_row, int n_rows, const double *beta,
               double *bad_log, uint32_t *bad_count, int bad_cap) {
    const State s{pos, lnprob, n_accepted, perm, n_walkers, n_ensembles, ndim, chain, chain_lnp, chain_row, n_rows};
    if (!state_ok(s) || !spec || !bad_ok(bad_log, bad_count, bad_cap)) return -1;
    const int n_half = n_walkers / 2, R = ndim + kSpecExtra;
    const size_t n_slots = (size_t)n_half * n_ensembles;
    for (size_t b = 0; b < 3 * n_slots; ++b) {   // the partner's slot of every row
        const double jc = spec[b * R + ndim + 5];
        if (!(jc >= 0.0) || !(jc < (double)n_half) || jc != std::floor(jc)) return -1;
    }
    Bufs B;
    StretchArgs g = upload(B, s);
    g.spec = const_cast<double *>(B.in(spec, 3 * n_slots * R));
    g.beta = beta ? B.in(beta, (size_t)n_ensembles) : nullptr;
    upload_bad(B, g, bad_log, bad_count, bad_cap);
    if (!B.ready()) return B.finish(0);
    return B.finish(launch_stretch_step_commit(g, nullptr));
}

// The commit of one half-step (stretch_apply_kernel) from the gathered rows upd[n_half * n_ensembles][ndim + 3]; row gs belongs
// to slot gs % n_half of the ensemble at position gs / n_half of ens_order (0: the ensembles as they are numbered).
int mpc_apply(double *pos, double *lnprob, int64_t *n_accepted, const int32_t *perm, const double *upd, int n_walkers,
              int n_ensembles, int ndim, int half, uint64_t ens_order, double *chain, double *chain_lnp, int chain_row, int n_rows,
              double *bad_log, uint32_t *bad_count, int bad_cap) {
    const State s{pos, lnprob, n_accepted, perm, n_walkers, n_ensembles, ndim, chain, chain_lnp, chain_row, n_rows};
    if (!state_ok(s) || !upd || (half != 0 && half != 1) || !bad_ok(bad_log, bad_count, bad_cap)) return -1;
    if (ens_order) {   // (mp_sampler.cpp: at most 16 ensembles, four bits each, a permutation)
        if (n_ensembles > 16) return -1;
        unsigned seen = 0;
        for (int p = 0; p < n_ensembles; ++p) {
            const unsigned e = (unsigned)((ens_order >> (4 * p)) & 15u);
            if ((int)e >= n_ensembles || (seen >> e & 1u)) return -1;
            seen |= 1u << e;
        }
        if (n_ensembles < 16 && (ens_order >> (4 * n_ensembles))) return -1;
    }
    Bufs B;
    StretchArgs g = upload(B, s);
    g.upd = const_cast<double *>(B.in(upd, (size_t)(n_walkers / 2) * n_ensembles * (ndim + 3)));
    g.half = half;
    g.ens_order = ens_order;
    upload_bad(B, g, bad_log, bad_count, bad_cap);
    if (!B.ready()) return B.finish(0);
    return B.finish(launch_stretch_apply(g, nullptr));
}

// The swap sweep of a tempered step (stretch_swap_kernel): beta[n_ensembles], n_ensembles / n_temps groups;
// n_swaps[n_groups][n_temps - 1] is added to.
int mpc_swap(double *pos, double *lnprob, int64_t *n_accepted, const int32_t *perm, const double *beta, int n_walkers,
             int n_ensembles, int ndim, int n_temps, uint64_t seed, uint32_t step, int64_t *n_swaps, double *chain,
             double *chain_lnp, int chain_row, int n_rows) {
    const State s{pos, lnprob, n_accepted, perm, n_walkers, n_ensembles, ndim, chain, chain_lnp, chain_row, n_rows};
    if (!state_ok(s) || !beta || !n_swaps) return -1;
    if (n_temps < 2 || n_ensembles % n_temps) return -1;   // (launch_stretch_swap, mp_sampler_set_temperatures)
    Bufs B;
    StretchArgs g = upload(B, s);
    g.beta = B.in(beta, (size_t)n_ensembles);
    g.seed = seed;
    g.step = step;
    int64_t *d_swaps = B.io(n_swaps, (size_t)(n_ensembles / n_temps) * (n_temps - 1));
    if (!B.ready()) return B.finish(0);
    return B.finish(launch_stretch_swap(g, n_temps, d_swaps, nullptr));
}

// The launch order of a mixed-length batch (order_kernel): n_obs[n_ds] the lengths of the registered light curves, ds_id[n] any
// integers (an id outside [0, n_ds) counts as length 0), order[n].  order_class reads ds, n_ds and ds[d].n_obs only: the rest
// of the DevShared is zero, and n_ds = 0 gives ds = nullptr.
int mpc_order(const int32_t *n_obs, int n_ds, const int32_t *ds_id, int n, int32_t *order) {
    if (!ds_id || !order || n < 1 || n > kMaxOrderN || n_ds < 0 || n_ds > kMaxDatasets || (n_ds > 0 && !n_obs)) return -1;
    std::vector<DsDesc> ds((size_t)n_ds);
    for (int d = 0; d < n_ds; ++d) {
        std::memset(&ds[(size_t)d], 0, sizeof(DsDesc));
        ds[(size_t)d].n_obs = n_obs[d];
    }
    Bufs B;
    DevShared sh;
    std::memset(&sh, 0, sizeof sh);
    sh.ds = n_ds ? B.in(ds.data(), ds.size()) : nullptr;
    sh.n_ds = n_ds;
    const int32_t *d_id = B.in(ds_id, (size_t)n);
    int32_t *d_order = B.io(order, (size_t)n);
    if (!B.ready()) return B.finish(0);
    return B.finish(launch_order(sh, d_id, n, d_order, nullptr));
}

}  // extern "C"
