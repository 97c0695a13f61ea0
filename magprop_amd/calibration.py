"""Injection-recovery studies (simulation-based calibration; Talts et al. 2018, Cook, Gelman & Rubin 2006): if the truth were
theta, with these observing times and errors, what would this pipeline recover?  Truths are drawn from the prior, a light curve is
simulated for each on the device (mp_simulate), every light curve is fitted by an ensemble of its own (up to MP_MAX_DATASETS
ensembles per launch), and the fits are held against the truths: for a calibrated pipeline the probability integral transform
(PIT) u = P(theta < truth | data) of every parameter is uniform over the datasets.

Host only (numpy and scipy.stats).  ``injection_study`` ties the device pieces together; the summary functions below it are plain
functions of arrays."""
from dataclasses import dataclass, field

import numpy as np

from . import _capi, engine
from . import moves as _moves

BALL = 1.0e-4     # the walkers start in the reference's ball around the truth (synth_mcmc.py:172-176)
HIST_BINS = 4096  # bins per dimension of the posterior monitor's histograms over the prior box (_capi.POST_MAX_BINS)


# ---------------------------------------------------------------- summary functions
def pit_from_samples(samples, truth):
    """u = the fraction of posterior samples below the truth, per parameter: samples (n, ndim) and truth (ndim,), or samples
    (n_datasets, n, ndim) and truth (n_datasets, ndim).  Resolution 1 / n."""
    s, t = np.asarray(samples, dtype=np.float64), np.asarray(truth, dtype=np.float64)
    if s.ndim == 1:
        s = s[:, None]
    return np.mean(s < np.expand_dims(np.atleast_1d(t), -2), axis=-2)


def pit_from_histogram(hist1, below, above, lower, upper, truth):
    """(u, resolution) per parameter from 1-D histograms hist1 (ndim, bins) over [lower, upper) with the counts below and above
    the range (EnsembleSampler.get_posterior): u = (samples in the bins under the truth's + the fraction of the truth's bin that
    lies under the truth, by linear interpolation) / N.  The samples of the truth's own bin are the only ones whose side is not
    known, so u differs from pit_from_samples of the same samples by at most resolution = (count of the truth's bin) / N.  A
    truth outside the range: u is NaN and the resolution the mass on that side."""
    h = np.atleast_2d(np.asarray(hist1, dtype=np.float64))
    ndim, bins = h.shape
    lo, hi, bl, ab, t = (np.broadcast_to(np.asarray(v, dtype=np.float64), (ndim,)) for v in (lower, upper, below, above, truth))
    u, res = np.full(ndim, np.nan), np.full(ndim, np.nan)
    for d in range(ndim):
        n = bl[d] + h[d].sum() + ab[d]
        if n == 0:
            continue
        if not lo[d] <= t[d] < hi[d]:
            res[d] = (bl[d] if t[d] < lo[d] else ab[d]) / n
            continue
        pos = (t[d] - lo[d]) / (hi[d] - lo[d]) * bins
        k = min(int(pos), bins - 1)
        u[d] = (bl[d] + h[d, :k].sum() + (pos - k) * h[d, k]) / n
        res[d] = h[d, k] / n
    return u, res


def _columns(pit):
    p = np.asarray(pit, dtype=np.float64)
    return p[:, None] if p.ndim == 1 else p


def coverage(pit, levels=(0.68, 0.95)):
    """How often the central credible interval of every level held the truth: per level a dict with "level", "n" (datasets with
    a finite PIT, per parameter), "count" and "observed" = count / n per parameter (the truth is inside the central interval of
    mass `level` when |u - 1/2| <= level / 2), "expected": the central 95 % binomial interval of the fraction under calibration
    (lower, upper per parameter), and "inside": whether observed lies in it."""
    from scipy import stats
    p = _columns(pit)
    ok = np.isfinite(p)
    n = ok.sum(axis=0)
    out = []
    for level in levels:
        inside = ok & (np.abs(np.where(ok, p, 0.5) - 0.5) <= 0.5 * level + 1.0e-12)
        count = inside.sum(axis=0)
        lo, hi = stats.binom.interval(0.95, np.maximum(n, 1), level)
        with np.errstate(invalid="ignore", divide="ignore"):
            obs, exp = count / n, (lo / n, hi / n)
        out.append({"level": float(level), "n": n, "count": count, "observed": obs, "expected": exp,
                    "inside": (count >= lo) & (count <= hi)})
    return out


def uniformity(pit):
    """(statistic, pvalue) per parameter of the Kolmogorov-Smirnov test of the PIT values against the uniform law (the exact
    two-sided distribution, scipy.stats.kstest); NaN values are left out.  A small p-value says the fits are not calibrated: too
    narrow or too wide posteriors pile the PIT up at the ends or in the middle, a bias piles it up on one side."""
    from scipy import stats
    p = _columns(pit)
    stat, pv = np.full(p.shape[1], np.nan), np.full(p.shape[1], np.nan)
    for d in range(p.shape[1]):
        u = p[np.isfinite(p[:, d]), d]
        if u.size:
            r = stats.kstest(u, "uniform")
            stat[d], pv[d] = r.statistic, r.pvalue
    return stat, pv


def rank_histogram(pit, bins=10):
    """(counts (ndim, bins), (lower, upper)): the PIT values of every parameter in `bins` equal bins of [0, 1] (u = 1 goes into
    the last) and the central 99 % binomial interval of a bin's count under calibration (per parameter)."""
    from scipy import stats
    p = _columns(pit)
    counts = np.zeros((p.shape[1], int(bins)), dtype=np.int64)
    n = np.zeros(p.shape[1], dtype=np.int64)
    for d in range(p.shape[1]):
        u = p[np.isfinite(p[:, d]), d]
        n[d] = u.size
        counts[d] = np.bincount(np.minimum((u * bins).astype(np.int64), int(bins) - 1), minlength=int(bins))
    return counts, stats.binom.interval(0.99, np.maximum(n, 1), 1.0 / int(bins))


def summarize(pit, zscore=None, contraction=None, levels=(0.68, 0.95), alpha=0.001):
    """The calibration summary of a study: {"n", "ks", "ks_pvalue", "ks_critical" (the 1 - alpha quantile of the exact KS law for
    n values, per parameter), "calibrated" (ks < ks_critical), "coverage", "rank_histogram"}; with the z-scores (mean - truth) /
    sd also "z_mean", "z_sd", with the contractions their "contraction_median"."""
    from scipy import stats
    p = _columns(pit)
    n = np.isfinite(p).sum(axis=0)
    ks, pv = uniformity(p)
    crit = stats.kstwo.ppf(1.0 - alpha, np.maximum(n, 1))
    out = {"n": n, "ks": ks, "ks_pvalue": pv, "ks_critical": crit, "calibrated": ks < crit, "coverage": coverage(p, levels),
           "rank_histogram": rank_histogram(p)[0]}
    if zscore is not None:
        z = _columns(zscore)
        out["z_mean"], out["z_sd"] = np.nanmean(z, axis=0), np.nanstd(z, axis=0, ddof=1)
    if contraction is not None:
        out["contraction_median"] = np.nanmedian(_columns(contraction), axis=0)
    return out


# ---------------------------------------------------------------- the study
@dataclass
class InjectionResult:
    """What injection_study returns.  Arrays are per dataset (n_datasets, ...) in the order of the truths; a dataset that was left
    out has NaN rows and an entry in `left_out`."""
    truths: np.ndarray            # (n_datasets, ndim) sampler coordinates
    x: np.ndarray                 # (n_obs,) or (n_datasets, n_obs)
    y: np.ndarray                 # (n_datasets, n_obs)
    yerr: np.ndarray
    model: np.ndarray
    status: np.ndarray            # (n_datasets,) of the simulation (_capi.STATUS_*)
    pit: np.ndarray               # (n_datasets, ndim): from the stored chain with store=True, else from the histograms
    pit_hist: np.ndarray          # (n_datasets, ndim) from the posterior monitor's histograms
    pit_resolution: np.ndarray    # (n_datasets, ndim) of pit_hist: the mass of the truth's bin
    zscore: np.ndarray            # (mean - truth) / sd
    contraction: np.ndarray       # 1 - var_post / var_prior
    mean: np.ndarray
    sd: np.ndarray
    tau: np.ndarray               # (n_datasets, ndim) integrated autocorrelation times of the device monitor
    converged: np.ndarray         # (n_datasets,) bool: the dataset's ensemble met emcee's stopping rule within max_steps
    acceptance: np.ndarray        # (n_datasets,) mean acceptance fraction of the ensemble
    n_samples: np.ndarray         # (n_datasets,) posterior samples behind the summaries (steps x walkers)
    steps: np.ndarray             # (n_datasets,) steps the dataset's batch ran
    redrawn: int = 0              # truths drawn again because their model failed
    left_out: list = field(default_factory=list)   # [{"dataset", "reason"}]: never silently dropped
    chains: list = None           # store=True: per batch the chain (steps, datasets x nwalkers, ndim), burn-in included
    tau_history: list = field(default_factory=list)   # per batch [(samples, tau (datasets, ndim)), ...] of run_mcmc_until's checks
    discard: int = 0

    def summarize(self, **kw):
        """summarize() of the datasets that were fitted and whose batch converged."""
        use = self.converged & np.all(np.isfinite(self.pit), axis=1)
        return summarize(self.pit[use], self.zscore[use], self.contraction[use], **kw)


def _generate(variant, GRBtype, truths, x, n_obs, frac_err, yerr, seed, device):
    if variant == "synth":
        from . import synth
        return synth.generate_data(truths, None, n_obs, frac_err, seed, x, yerr, device=device)
    from . import mcmc_eqns
    return mcmc_eqns.generate_data(truths, GRBtype, x, n_obs, frac_err, seed, yerr, device=device)


def injection_study(x=None, n_obs=50, frac_err=0.25, yerr=None, truths=None, n_datasets=32, centre=None, spread=None, nwalkers=32,
                    variant="synth", GRBtype=None, moves=None, max_steps=4000, check_every=200, discard=None, seed=0, store=False,
                    ndim=6, device=-1):
    """Simulate n_datasets light curves from known truths, fit each with an ensemble of its own, and hold the fits against the
    truths.

    Truths (sampler coordinates): given as (n_datasets, ndim); or drawn uniformly from the prior box of `variant`; or, with
    centre and spread, uniformly from centre +- spread clipped to the box -- the fit's prior is then that smaller box, so that
    the generating law and the prior agree.  A drawn truth whose model fails is drawn again: the fit's prior is the box
    restricted to the parameters whose model succeeds (everything else has lnprob = -inf), so the generating law has to be
    restricted in the same way.  Given truths are never replaced; one that fails is left out and reported.
    Datasets: generate_data on all truths in one call (x, n_obs, frac_err, yerr as there; dataset i's noise depends on seed and
    i), fitted in batches of at most MP_MAX_DATASETS by one EnsembleSampler(datasets=[...]) per batch.
    Fit: walkers start in a ball of 1e-4 around the truth (the reference's start), moves default to [(KDEMove(), 0.8), (DEMove(),
    0.2)], run_mcmc_until(max_steps, check_every, per_ensemble=True) with the autocorrelation and posterior monitors on, both from
    `discard` steps on (None: max_steps // 8): every dataset's ensemble has to meet emcee's stopping rule (50 tau < samples, tau
    settled to 1 %) at one of the checks, and the batch runs until all have or max_steps are done.  store=False leaves no chain on the host: PIT, mean and sd come from the posterior monitor
    (HIST_BINS bins per dimension over the prior box, linear inside the truth's bin: good to the mass of that bin, which
    pit_resolution reports per value).  store=True keeps the chain and takes PIT, mean and sd from its steps behind `discard`.
    Returns an InjectionResult."""
    from .ensemble import EnsembleSampler
    lo, hi, _ = engine.prior_box(variant, ndim, strict=True)
    rng = np.random.default_rng(seed)
    if centre is not None:
        c, s = np.asarray(centre, dtype=np.float64), np.broadcast_to(np.asarray(spread, dtype=np.float64), (ndim,))
        lo, hi = np.maximum(lo, c - s), np.minimum(hi, c + s)
        if np.any(lo >= hi):
            raise ValueError("centre +- spread leaves no room inside the prior box")
    given = truths is not None
    if given:
        truths = np.array(truths, dtype=np.float64, ndmin=2)
        if truths.shape[1] != ndim:
            raise ValueError(f"truths must be (n_datasets, {ndim}), got {truths.shape}")
    else:
        truths = rng.uniform(lo, hi, (int(n_datasets), ndim))
    n = truths.shape[0]
    data = _generate(variant, GRBtype, truths, x, n_obs, frac_err, yerr, seed, device)
    redrawn = 0
    while not given:
        failed = np.nonzero((data["status"] != _capi.STATUS_OK) & (data["status"] != _capi.STATUS_ZEROERR))[0]
        if failed.size == 0:
            break
        if redrawn > 100 * n:
            raise RuntimeError("the model fails almost everywhere in the box the truths are drawn from")
        truths[failed] = rng.uniform(lo, hi, (failed.size, ndim))
        redrawn += failed.size
        data = _generate(variant, GRBtype, truths, data["x"], n_obs, frac_err, yerr, seed, device)   # (the same times; index i keeps its noise)
    xs = data["x"]
    nan = lambda *shape: np.full(shape, np.nan)   # noqa: E731
    res = InjectionResult(truths=truths, x=xs, y=data["y"], yerr=data["yerr"], model=data["model"], status=data["status"],
                          pit=nan(n, ndim), pit_hist=nan(n, ndim), pit_resolution=nan(n, ndim), zscore=nan(n, ndim),
                          contraction=nan(n, ndim), mean=nan(n, ndim), sd=nan(n, ndim), tau=nan(n, ndim),
                          converged=np.zeros(n, dtype=bool), acceptance=nan(n), n_samples=np.zeros(n, dtype=np.int64),
                          steps=np.zeros(n, dtype=np.int64), redrawn=redrawn, chains=[] if store else None)
    for i in np.nonzero(data["status"] != _capi.STATUS_OK)[0]:
        why = "a simulated error is 0" if data["status"][i] == _capi.STATUS_ZEROERR else f"the truth's model failed (status {data['status'][i]})"
        res.left_out.append({"dataset": int(i), "reason": why})
    fit = np.nonzero(data["status"] == _capi.STATUS_OK)[0]
    discard = int(max_steps) // 8 if discard is None else int(discard)
    res.discard = discard
    var_prior = (hi - lo) ** 2 / 12.0
    table = [(_moves.KDEMove(), 0.8), (_moves.DEMove(), 0.2)] if moves is None else moves
    for b0 in range(0, fit.size, _capi.MAX_DATASETS):
        ids = fit[b0:b0 + _capi.MAX_DATASETS]
        sets = [(xs if xs.ndim == 1 else xs[i], data["y"][i], data["yerr"][i]) for i in ids]
        es = EnsembleSampler(nwalkers, ndim, variant=variant, GRBtype=GRBtype, datasets=sets, lower=lo, upper=hi, moves=table,
                             seed=int(seed) + 1 + b0, device=device)
        try:
            pos = np.repeat(truths[ids], nwalkers, axis=0) + BALL * rng.standard_normal((ids.size * nwalkers, ndim))
            es.monitor_autocorr(discard=discard)
            es.monitor_posterior(bins=HIST_BINS, bins2=0, discard=discard)
            es.run_mcmc_until(pos, max_steps, check_every=check_every, store=store, per_ensemble=True)
            tau = np.atleast_2d(es.get_autocorr_device(wait=True)[0])
            acc = es.acceptance_fraction.reshape(ids.size, nwalkers).mean(axis=1)
            chain = es.get_chain() if store else None
            for k, i in enumerate(ids):
                post = es.get_posterior(ensemble=k)
                u, r = pit_from_histogram(post["hist1"], post["below"], post["above"], lo, hi, truths[i])
                res.pit_hist[i], res.pit_resolution[i] = u, r
                mean, sd, cnt = post["mean"], np.sqrt(np.diag(post["cov"])), post["n"]
                res.pit[i] = u
                if store:
                    rows = chain[discard:, k * nwalkers:(k + 1) * nwalkers].reshape(-1, ndim)
                    if len(rows) > 1:
                        res.pit[i], mean, sd, cnt = pit_from_samples(rows, truths[i]), rows.mean(axis=0), rows.std(axis=0, ddof=1), len(rows)
                res.mean[i], res.sd[i], res.n_samples[i] = mean, sd, cnt
                with np.errstate(invalid="ignore", divide="ignore"):
                    res.zscore[i] = (mean - truths[i]) / sd
                    res.contraction[i] = 1.0 - sd ** 2 / var_prior
                res.tau[i], res.converged[i], res.acceptance[i], res.steps[i] = tau[k], es.converged_ensembles[k], acc[k], es.iteration
            res.tau_history.append([(int(m), np.atleast_2d(t)) for m, t in es.tau_history])
            if store:
                res.chains.append(chain)
            if not es.converged:
                late = [int(i) for k, i in enumerate(ids) if not es.converged_ensembles[k]]
                res.left_out.append({"dataset": late, "reason": f"not converged within {int(max_steps)} steps (the batch ran to the end)"})
        finally:
            es.close()
    return res
