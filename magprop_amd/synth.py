"""Posterior of the synthetic-dataset variant, signatures of ``code/synthetic_datasets/mcmc_eqns.py``.

``lnlike(pars, x, y, yerr)`` (:5-25), ``lnprior(pars)`` (:28-49), ``lnprob(pars, x, y, yerr, fbad)``
(:52-81) — the callable ``synth_mcmc.py:180-185`` hands to ``emcee.EnsembleSampler``.  ``pars`` may be
2-D ``(n_walkers, 6)`` (emcee ``vectorize=True``): one kernel launch for the whole batch.
"""
import contextlib

import numpy as np

from . import _capi, engine, summaries

PRIOR_UPPER = np.array([10.0, 10.0, -2.0, np.log10(2000.0), 2.0, 3.0])   # :40
PRIOR_LOWER = np.array([1.0e-3, 0.69, -6.0, np.log10(50.0), -2.0, -1.0])  # :41
LOG_MASK = 0b111100                                                       # arr[2:] = 10**arr[2:]  (:16-17)


_cfg_cache = {}


def _cfg():
    """The synthetic variant's model configuration (one object per pair of solver defaults in force: building the ctypes
    structure and its cache key costs more than the rest of a call's Python)."""
    key = (_capi.DEFAULT_SWEEP_TOL, _capi.DEFAULT_MAX_STRIDE)
    c = _cfg_cache.get(key)
    if c is None:
        c = _cfg_cache[key] = _capi.cfg_synth()
        c._mp_key = engine._cfg_key(c)
    return c


def _evaluate(pars, x, y, yerr, lower, upper, device=-1, want_status=False):
    p = np.asarray(pars, dtype=np.float64)
    scalar = p.ndim == 1
    p2 = np.atleast_2d(p)
    if p2.shape[1] != 6:
        raise ValueError("pars must have 6 entries: B, P, log10 MdiscI, log10 RdiscI, log10 epsilon, log10 delta")
    eng = engine.acquire(_cfg(), None, device)      # (what `with engine.use(...)` does, without the generator: this is the hot entry)
    try:
        slot = eng.dataset_slot(x, y, yerr)
        eng.set_prior(lower, upper, LOG_MASK)
        out, st = eng.handle.lnprob_batch(p2, ds_id=slot, want_status=True)
    finally:
        engine.release(eng)
    if scalar:
        return (float(out[0]), int(st[0])) if want_status else float(out[0])
    return (out, st) if want_status else out


def lnlike(pars, x, y, yerr, device=-1):
    return _evaluate(pars, x, y, yerr, None, None, device)


def lnprior(pars):
    p = np.asarray(pars, dtype=np.float64)
    inside = np.all(p <= PRIOR_UPPER, axis=-1) & np.all(p >= PRIOR_LOWER, axis=-1)
    if p.ndim == 1:
        return 0.0 if inside else -np.inf
    return np.where(inside, 0.0, -np.inf)


def lnprob(pars, x, y, yerr, fbad=None, device=-1):
    """Parameter sets inside the prior whose likelihood is not finite are appended to ``fbad`` (:72-79)."""
    out, st = _evaluate(pars, x, y, yerr, PRIOR_LOWER, PRIOR_UPPER, device, want_status=True)
    if fbad is not None:
        bad = np.atleast_1d(st)
        rows = np.atleast_2d(np.asarray(pars, dtype=np.float64))[(bad == _capi.STATUS_FLAG) |
                                                                (bad == _capi.STATUS_NONFINITE)]
        if len(rows):
            with open(fbad, "a") as f:
                for r in rows:
                    f.write(", ".join(f"{v}" for v in r) + "\n")
    return out


def _source(device, x=None, y=None, yerr=None):
    """Source of magprop_amd.summaries: the cached engine of the synthetic variant on `device` under the synthetic prior, held for
    the duration of a summary, with the light curve (x, y, yerr) registered when one is given."""
    @contextlib.contextmanager
    def enter(ndim):
        with engine.use(_cfg(), None, device) as eng:
            slot = 0 if x is None else eng.dataset_slot(x, y, yerr)
            eng.set_prior(PRIOR_LOWER, PRIOR_UPPER, LOG_MASK)
            yield eng.handle, slot, None if x is None else engine._as_f64(x)
    return enter


# the four canonical parameter sets of code/synthetic_datasets/generate_data.py:10-15, physical as the reference writes them
GRBS = {"Humped": (1.0, 5.0, 1.0e-3, 100.0, 0.1, 1.0), "Classic": (1.0, 5.0, 1.0e-3, 1000.0, 0.1, 1.0),
        "Sloped": (1.0, 1.0, 1.0e-3, 100.0, 10.0, 10.0), "Stuttering": (1.0, 5.0, 1.0e-5, 100.0, 0.1, 100.0)}


def generate_data(pars=None, grb=None, n_obs=50, frac_err=0.25, seed=0, x=None, yerr=None, physical=False, device=-1):
    """A synthetic light curve from known parameters, the recipe of code/synthetic_datasets/generate_data.py:61-67 on the device
    (mp_simulate): the model at n_obs grid points drawn with replacement and sorted (numpy.random.default_rng(seed)), yerr =
    frac_err * |model|, Gaussian noise.  grb: one of GRBS by name (its physical parameters, as the reference takes them); or
    pars (6,) / (n, 6) for n datasets at once, in sampler coordinates (physical=True: physical ones).  x: observed times
    instead of the draw, anywhere inside the grid, (n_obs,) or (n, n_obs); yerr: absolute errors of x's shape instead of
    frac_err.  Returns {"x", "y", "yerr", "model", "z", "status", "n_ok"}; dataset i's noise depends on seed and i alone.  A row
    whose model failed, or with a zero error (_capi.STATUS_ZEROERR), is all NaN."""
    if (pars is None) == (grb is None):
        raise ValueError("give either pars or grb")
    if grb is not None:
        if grb not in GRBS:
            raise ValueError(f"grb must be one of {', '.join(GRBS)}, got {grb!r}")
        pars, physical = np.array(GRBS[grb]), True
    return summaries.simulate(_source(device), pars, x, n_obs, frac_err, seed, yerr, physical, width=6)


def model_band(samples, q=(0.025, 0.5, 0.975), components=("Ltot",), device=-1, weights=None):
    """Posterior-predictive band of the synthetic model: per point of the grid logspace(0, 6, 10001), the quantiles q of the
    light curves of `samples` (rows in sampler coordinates, as a chain stores them; rows outside the prior or whose model
    failed are left out, as np.nanquantile leaves out NaN).  The reference's plot_synth.py:143-206 takes percentiles of the
    parameters and draws one curve at their medians instead.  Returns {"t": tarr, "Ltot": (nq, n_grid), ..., "n_used": rows
    that entered}; a grid point no row reached is NaN.  weights (one per row, finite and >= 0): the quantiles of the weighted
    empirical distribution of the curves (mp_model_band_weighted, no interpolation), and "n_eff", Kish's effective sample size
    of the rows that entered."""
    return summaries.band(_source(device), samples, q, components, weights, width=6)


def model_derived(samples, q=(0.16, 0.5, 0.84), weights=None, device=-1):
    """Energy budgets and light-curve landmarks of the synthetic model of every row of `samples` (sampler coordinates, as a
    chain stores them; any number of rows), on the grid logspace(0, 6, 10001): radiated energy and its dipole / propeller
    split, peaks, the times by which 10, 50 and 90 % of the energy is out, spin-up and disc mass (magprop_amd.derived.NAMES).
    Returns {"values": (n, 16) with rows outside the prior or whose model failed all NaN, "status": (n,), "n_used": rows that
    finished, "summary": derived.summarize(values, q, weights)}."""
    return summaries.derived(_source(device), samples, q, weights, width=6)


def model_flows(rows, curves=(), q=(0.16, 0.5, 0.84), weights=None, device=-1):
    """Mass budget, angular-momentum budget and propeller / accretor regime of the synthetic model of every row of `rows`
    (sampler coordinates, as a chain stores them; any number of rows), on the grid logspace(0, 6, 10001): what
    magprop_amd.flows.NAMES lists, from the radii, mass-flow rates and torques of the integrated system (mp_model_flows; the
    quantities code/figure_3.py:202-286 recovers and code/figure_4.py:139-175 plots).  Returns {"values": (n, 16) with rows
    outside the prior or whose model failed all NaN, "status": (n,), "n_used", "summary": flows.summarize(values, q, weights)}
    and, per name of flows.CURVES in `curves`, that cell curve (n, n_grid) in cgs, with "t" the grid."""
    return summaries.flows(_source(device), rows, q, weights, curves, width=6)


def model_flow_band(samples, q=(0.025, 0.5, 0.975), curves=("fastness",), device=-1, weights=None):
    """Bands of the cell curves of model_flows over `samples` (sampler coordinates; up to _capi.BAND_MAX_SAMPLES rows): per grid
    point, the quantiles q of every curve named in `curves` (flows.CURVES without "branch") over the rows that finished, as
    model_band gives them for the luminosities (mp_model_flow_band).  Returns {"t", name: (nq, n_grid), "n_used"}; with
    weights also "n_eff"."""
    return summaries.flow_band(_source(device), samples, q, curves, weights, width=6)


def model_pointwise(samples, x, y, yerr, device=-1, cells=False):
    """Pointwise predictive scores of the synthetic model on the light curve (x, y, yerr): per observation, in the order of x,
    PSIS-LOO with its Pareto-k diagnostic and WAIC over the rows of `samples` (sampler coordinates, as a chain stores them;
    equally weighted: resample a nested run's rows first; up to pointwise.MAX_SAMPLES rows).  The reductions over the samples
    run on the device (mp_model_pointwise), the scores on the host (magprop_amd.pointwise).  Returns {"obs": (n_obs, 12) the
    table of pointwise.NAMES, "tail", "status": (n,), "n_used": rows that finished, "loo": pointwise.psis_loo, "waic":
    pointwise.waic, "summary": pointwise.summarize}; cells=True adds "z": (n_obs, n), the standardised residuals.  The
    log-likelihood is the unnormalised lnlike term; pointwise.normalisation(yerr) per point normalises it."""
    return summaries.pointwise(_source(device, x, y, yerr), samples, cells, width=6)


def model_reweight(samples, x, y, yerr, alternatives, device=-1):
    """Importance reweighting of a fit of the synthetic model on the light curve (x, y, yerr) to other error models and data
    subsets: per row of `samples` (sampler coordinates, as a chain stores them; up to pointwise.MAX_SAMPLES rows) and per
    alternative (magprop_amd.reweight.gaussian / student_t, one or up to 64), the log importance weight that carries the chain
    from lnlike = -0.5 chi^2 to the alternative likelihood, summed on the device (mp_model_reweight); per-observation weights
    and leave_out masks are in the order of x.  Returns {"lw": (n_alt, n), "table": (n_alt, 12) of reweight.NAMES, "tail",
    "status": (n,), "n_used", "n_eff", "khat", "log_evidence_ratio", "log_evidence_ratio_err": (n_alt,)};
    reweight.weights(lw, k) are the weights the weights= arguments of model_band, model_derived and model_flows take."""
    return summaries.reweight(_source(device, x, y, yerr), samples, alternatives, width=6)
