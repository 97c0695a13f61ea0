// mp_monitor.h — the four chain monitors of the ensemble sampler as a host unit of their own (mp_monitor.cpp): the autocorrelation
// monitor (mp_sampler_set_autocorr; kernels mp_acf.hip), the posterior monitor (mp_sampler_set_posterior; kernels mp_post.hip),
// the thermodynamic monitor (mp_sampler_set_thermo; thermo_kernel of mp_ladder.hip) and the sample reservoir
// (mp_sampler_set_reservoir; kernels mp_reservoir.hip).
//
// Internal, like mp_host.h.  A monitor knows the shape of the chain, the device rows it is fed and a stream, and nothing of the
// sampler: mp_sampler.cpp holds one of each behind its entry points and restarts, feeds and refuses through ChainMonitor, and
// the probe libraries mp_probe_acf.hip, mp_probe_post.hip and mp_probe_reservoir.hip drive the same functions over crafted
// chains.  A function that reports an error names the entry point `fn`.
#pragma once
#include <memory>

#include "mp_acf.h"
#include "mp_host.h"
#include "mp_ladder.h"
#include "mp_post.h"
#include "mp_reservoir.h"

#pragma GCC visibility push(hidden)

// What a monitor type is called in messages and the entry point that turns it on and off (every type states its own as kNames);
// off(): MP_ESTATE "<fn>: <what> is off (<setter>)", the answer of a read-out while the sampler holds no such monitor
struct MonitorNames { const char *what, *setter; int off(const char *fn) const; };

// What a chunk of mp_sampler_run offers the monitors: `rows` steps chain[rows][n_total][ndim] with their lnp[rows][n_total] on
// the device, the first of them step `step0`; frozen_from is the first step on the ladder's final state (0: a fixed ladder)
struct ChainRows { const double *chain, *lnp; int rows; int64_t step0, frozen_from; };

// What every monitor keeps, the shape of the chain and the count of the steps that went in, and what the sampler does to a
// monitor without knowing which one it is: restart, feed, run_only.
struct ChainMonitor {
    const MonitorNames &names;
    int n_walkers = 0, n_ensembles = 0, n_total = 0, ndim = 0;
    int chunk_cap = 0;              // most steps per chunk of mp_sampler_run while the monitor is on
    int64_t n = 0;                  // steps accumulated
    int64_t discard = 0, skip = 0;  // steps to pass over after a (re)start; how many of them are left
    ChainMonitor(const MonitorNames &names, int n_walkers, int n_ensembles, int ndim, int64_t discard, size_t sampler_cap)
        : names(names), n_walkers(n_walkers), n_ensembles(n_ensembles), n_total(n_walkers * n_ensembles), ndim(ndim),
          chunk_cap((int)capped(sampler_cap)), discard(discard) {}
    virtual ~ChainMonitor() = default;
    // chunks of at most 64 MB of chain rows while a monitor is on, and no longer than the sampler's own chunks (sampler_cap)
    size_t capped(size_t sampler_cap) const {
        return std::max<size_t>(1, std::min<size_t>(sampler_cap, ((size_t)64 << 20) / ((size_t)n_total * ndim * sizeof(double))));
    }
    void start_over() { n = 0; skip = discard; }
    // Of a chunk of `chunk` steps, the rows that go in: rows [first, first + rows), behind the steps still to be passed over
    int take(int chunk, int *first) {
        *first = (int)std::min<int64_t>(skip, chunk);
        skip -= *first;
        return chunk - *first;
    }
    // Empty the monitor: nothing accumulated, `discard` steps from now.  A chunk into the monitor: every monitor reads the fields
    // of ChainRows that it needs.  Both stream-ordered.
    virtual int restart(hipStream_t st) = 0;
    virtual int feed(const ChainRows &c, hipStream_t st) = 0;
    int run_only(const char *fn) const;   // MP_ESTATE: the walker-sharded entry point `fn` does not feed the monitor
    // The prologue of a read-out by ensemble: the ensemble exists, and what was fed has been accumulated
    int ready(const char *fn, int ensemble, hipStream_t st) const;
    // the check of a `discard` argument; `clause` goes behind "must be >= 0"
    static int check_discard(const char *fn, int64_t discard, const char *clause = "");
};

// Accumulators and the history ring of mp_acf.h, fed once per chunk of mp_sampler_run from the device slab of chain rows.
struct AcfMonitor : ChainMonitor {
    int max_lag = 0, kp = 0;        // lags asked for; rounded up to the kernels' lag block
    int ring_rows = 0, head = 0;    // the ring: kp + chunk_cap rows; row of the next sample
    DevBuf<double> hist, S, T, H, pivot, rho, f, tau;
    DevBuf<int32_t> window;
    using ChainMonitor::ChainMonitor;
    static const MonitorNames kNames;

    static int check(const char *fn, int max_lag, int64_t discard);   // max_lag = 0, which turns the monitor off, passes
    // A monitor of max_lag >= 1 checked lags with its buffers, within MP_ACF_MAX_BYTES; restart() comes next
    static int make(const char *fn, int n_walkers, int n_ensembles, int ndim, int max_lag, int64_t discard, size_t sampler_cap,
                    std::unique_ptr<AcfMonitor> *out);
    int restart(hipStream_t st) override;
    // The rows c.chain[rows][n_series] of a chunk into the monitor (stream-ordered)
    int feed(const ChainRows &c, hipStream_t st) override;
    // rho, the walker means, windows and taus of the samples so far into the monitor's buffers; waits for them
    int finalise(const char *fn, double c, hipStream_t st);
    // read-outs behind mp_sampler_get_autocorr, _get_acf (after finalise) and _get_autocorr_sums (after a wait for the stream)
    int read_tau(double *tau_out, int32_t *window_out) const;
    int read_acf(int ensemble, int max_rows, double *acf) const;   // the rows written
    int read_sums(int ensemble, double *S_out, double *T_out, double *H_out, double *tail, double *pivot_out, int64_t *n_samples) const;

private:
    mp::AcfArgs args(const double *chain) const;
};

// The counters, running sums and best-sample holders of mp_post.h, fed once per chunk of mp_sampler_run from the device slab of
// chain rows and their lnprob.
struct PostMonitor : ChainMonitor {
    int bins1 = 0, bins2 = 0;
    std::vector<double> par;        // [5][ndim] lower, upper, inv1, inv2, pivot (mp::post_params)
    DevBuf<double> d_par, mom, best_x, best_lnp;
    DevBuf<int64_t> hist1, hist2, outside2, nfin, best_idx;
    using ChainMonitor::ChainMonitor;
    static const MonitorNames kNames;

    // A monitor of bins1 != 0 bins with its buffers, after the checks of bins1, bins2, discard, the range, the ensemble count and
    // MP_POST_MAX_BYTES in this order; restart() comes next
    static int make(const char *fn, int n_walkers, int n_ensembles, int ndim, int bins1, int bins2, const double *lower,
                    const double *upper, int64_t discard, size_t sampler_cap, std::unique_ptr<PostMonitor> *out);
    // Empty the monitor (stream-ordered): no sample, best = none, `discard` steps from now.
    int restart(hipStream_t st) override;
    // The rows c.chain[rows][n_total][ndim] and c.lnp[rows][n_total] of a chunk into the monitor (stream-ordered)
    int feed(const ChainRows &c, hipStream_t st) override;
    // read-outs behind mp_sampler_get_posterior_hist1, _hist2, _moments and _best (after ready)
    int read_hist1(int ensemble, int64_t *hist1_out, int64_t *below, int64_t *above, int64_t *nonfinite, int64_t *n_samples) const;
    int read_hist2(const char *fn, int ensemble, int64_t *hist2_out, int64_t *outside2_out) const;
    int read_moments(int ensemble, double *sum1, double *sum2, double *pivot, int64_t *n_finite) const;
    int read_best(int ensemble, double *x, double *lnprob, int64_t *index) const;

private:
    mp::PostArgs args(const double *chain, const double *lnp) const;
};

// Per ensemble the sum of the finite stored lnprob and the counts of finite and non-finite cells (mp_ladder.h ThermoArgs), fed once
// per chunk of mp_sampler_run from the device slab's lnprob rows: what thermodynamic integration needs of a run.
struct ThermoMonitor : ChainMonitor {
    DevBuf<double> sum;
    DevBuf<int64_t> n_finite, n_nonfinite;
    using ChainMonitor::ChainMonitor;
    static const MonitorNames kNames;

    // A monitor with its buffers, after the check of discard; restart() comes next
    static int make(const char *fn, int n_walkers, int n_ensembles, int ndim, int64_t discard, size_t sampler_cap,
                    std::unique_ptr<ThermoMonitor> *out);
    int restart(hipStream_t st) override;
    // The rows c.lnp[rows][n_total] of a chunk whose first row is step c.step0 into the monitor (stream-ordered): those behind the
    // steps still to be passed over, and of them the steps >= c.frozen_from
    int feed(const ChainRows &c, hipStream_t st) override;
    // read-out behind mp_sampler_get_thermo (after a wait for the stream)
    int read(double *sum_out, int64_t *n_finite_out, int64_t *n_nonfinite_out, int64_t *n_steps) const;
};

// A uniform random subset of `size` of the monitored samples per ensemble with their lnprob, step, walker and key (mp_reservoir.h
// states the rule), fed once per chunk of mp_sampler_run from the device slab of chain rows and their lnprob.
struct ResMonitor : ChainMonitor {
    int size = 0, cand_cap = 0;     // K; candidates per ensemble and slice of a chunk
    uint64_t seed = 0;
    DevBuf<uint64_t> key, cand_key;
    DevBuf<int64_t> step, cand_step, meta;
    DevBuf<int32_t> walker, cand_walker, evicted;
    DevBuf<uint32_t> n_cand;
    DevBuf<double> x, lnp;
    using ChainMonitor::ChainMonitor;
    static const MonitorNames kNames;

    // A monitor of size != 0 rows per ensemble with its buffers, after the checks of size and discard in this order; restart()
    // comes next
    static int make(const char *fn, int n_walkers, int n_ensembles, int ndim, int size, uint64_t seed, int64_t discard,
                    size_t sampler_cap, std::unique_ptr<ResMonitor> *out);
    // Empty the monitor (stream-ordered): nothing held, nothing seen, everything passes, `discard` steps from now.
    int restart(hipStream_t st) override;
    // The rows c.chain[rows][n_total][ndim] and c.lnp[rows][n_total] of a chunk whose first row is step c.step0 into the monitor
    // (stream-ordered), in slices of whole steps of at most cand_cap samples per ensemble
    int feed(const ChainRows &c, hipStream_t st) override;
    // read-out behind mp_sampler_get_reservoir (after ready): the first max_rows held rows in the order (step, walker)
    int read(int ensemble, int max_rows, double *x_out, double *lnprob, int64_t *step_out, int32_t *walker_out, uint64_t *key_out,
             int *n_rows, int64_t *n_seen) const;
    // the launch arguments over the monitor's buffers (the probe's merge entry fills the slice in itself)
    mp::ResArgs args(const double *chain, const double *lnp) const;
};

#pragma GCC visibility pop
