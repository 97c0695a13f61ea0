"""Posterior of the library variant, signatures of ``magnetar/mcmc_eqns.py``.

``lnlike(pars, data, GRBtype)`` (:6-37), ``lnprior(pars, custom_lims=None)`` (:40-84),
``lnprob(pars, data, GRBtype, custom_lims=None)`` (:87-119).  ``pars`` may also be 2-D
``(n_walkers, ndim)``: the whole batch is one kernel launch (emcee ``vectorize=True``).

Reference quirk Q1: the reference's ``lnprob`` checks a log-space prior box
(``mcmc_limits.csv`` rows 3-6) but hands the same numbers to ``model_lc`` un-exponentiated.  Here
``lnprob`` implements the documented intent — parameters 3-6 are log10 in sampler coordinates and are
un-logged before the model — while ``lnlike`` keeps the reference behaviour (physical parameters).
"""
import contextlib
import os

import numpy as np

from . import _capi, engine, summaries

# Default prior box: the values of the reference's magnetar/mcmc_limits.csv:2-10 (rows B, P, log_MdiscI, log_RdiscI,
# log_epsilon, log_delta, dipeff, propeff, f_beam), kept in code so that nothing depends on the working directory
# (the reference re-reads a cwd-relative CSV on every call, magnetar/mcmc_eqns.py:55).
DEFAULT_LIMITS_LOWER = np.array([1.0e-3, 0.69, -3.0, np.log10(50.0), -1.0, -5.0, 0.01, 0.01, 1.0])
DEFAULT_LIMITS_UPPER = np.array([10.0, 10.0, -1.0, np.log10(2000.0), 3.0, np.log10(50.0), 1.0, 1.0, 600.0])
_limits_cache = {}
LIB_LOG_MASK = 0b111100


def _read_limits(path):
    """rows `pars,lower,upper`; cached per (path, mtime) — the reference re-reads it on every call (:55)."""
    try:
        key = (path, os.path.getmtime(path))
    except OSError:
        raise ValueError("Please provide a valid file path.")
    hit = _limits_cache.get(key)
    if hit is None:
        import pandas as pd
        try:
            lims = pd.read_csv(path, index_col="pars")
        except ValueError:
            raise ValueError("Please provide a valid file path.")
        hit = (lims["lower"].values.astype(float), lims["upper"].values.astype(float))
        _limits_cache[key] = hit
    return hit


def _bounds(ndim, custom_lims=None):
    lo, hi = (DEFAULT_LIMITS_LOWER, DEFAULT_LIMITS_UPPER) if custom_lims is None else _read_limits(custom_lims)
    if ndim == 7:  # :64-75: the 7th parameter is f_beam, the last row
        return np.append(lo[:6], lo[-1]), np.append(hi[:6], hi[-1])
    return lo[:ndim].copy(), hi[:ndim].copy()


def _columns(data):
    return (np.asarray(data["t"], dtype=np.float64), np.asarray(data["Lum50"], dtype=np.float64),
            np.asarray(data["Lum50err"], dtype=np.float64))


def _evaluate(pars, data, GRBtype, lower, upper, log_mask, device=-1, want_status=False):
    p = np.asarray(pars, dtype=np.float64)
    scalar = p.ndim == 1
    p2 = np.atleast_2d(p)
    if not 6 <= p2.shape[1] <= 9:
        raise ValueError("pars must have 6, 7, 8 or 9 entries")
    x, y, yerr = _columns(data)
    with engine.use(_capi.cfg_lib(), GRBtype, device) as eng:
        slot = eng.dataset_slot(x, y, yerr)
        eng.set_prior(lower, upper, log_mask)
        out, st = eng.handle.lnprob_batch(p2, ds_id=slot, want_status=True)
    if want_status:
        return (float(out[0]) if scalar else out), st
    return float(out[0]) if scalar else out


def lnlike(pars, data, GRBtype, device=-1, reference_quirk=False):
    """-0.5*chi^2 of model_lc against data (physical parameters; 6/7/8/9-parameter dispatch of :22-34).
    A failed integration gives -inf.  The reference has no branch for it: its ``model_lc`` returns the string 'flag'
    and ``ydata - 'flag'`` raises (:37); ``reference_quirk=True`` raises the same TypeError."""
    out, st = _evaluate(pars, data, GRBtype, None, None, 0, device, want_status=True)
    if reference_quirk and np.any(st == _capi.STATUS_FLAG):
        raise TypeError("unsupported operand type(s) for -: 'float' and 'str'  (model_lc returned 'flag', "
                        "magnetar/mcmc_eqns.py:37)")
    return out


def lnprior(pars, custom_lims=None):
    p = np.asarray(pars, dtype=np.float64)
    lo, hi = _bounds(p.shape[-1], custom_lims)
    inside = np.all(p >= lo, axis=-1) & np.all(p <= hi, axis=-1)
    if p.ndim == 1:
        return 0.0 if inside else -np.inf
    return np.where(inside, 0.0, -np.inf)


def lnprob(pars, data, GRBtype, custom_lims=None, device=-1, reference_quirk=False):
    """Default: the documented intent (module docstring) — box prior in sampler coordinates, parameters
    3-6 un-logged before the model.  ``reference_quirk=True`` evaluates what the reference's code literally does: the
    same box test, then the SAME numbers handed to ``model_lc`` un-exponentiated (:108-113), so a point inside the
    log-space box reaches the model with e.g. MdiscI = -2.5; the model state goes non-finite and the result is -inf
    (:115-116) wherever the reference would return -inf or NaN."""
    p = np.asarray(pars, dtype=np.float64)
    lo, hi = _bounds(p.shape[-1], custom_lims)
    return _evaluate(p, data, GRBtype, lo, hi, 0 if reference_quirk else LIB_LOG_MASK, device)


def _source(GRBtype, custom_lims, device, data=None):
    """Source of magprop_amd.summaries: the cached engine of the library variant on the grid of ``GRBtype`` and `device`, under the
    prior box ``lnprob`` uses for rows of ndim parameters, held for the duration of a summary, with the light curve ``data``
    registered when one is given."""
    @contextlib.contextmanager
    def enter(ndim):
        lo, hi = _bounds(ndim, custom_lims)
        x, y, yerr = (None, None, None) if data is None else _columns(data)
        with engine.use(_capi.cfg_lib(), GRBtype, device) as eng:
            slot = 0 if data is None else eng.dataset_slot(x, y, yerr)
            eng.set_prior(lo, hi, LIB_LOG_MASK)
            yield eng.handle, slot, x
    return enter


def generate_data(pars, GRBtype, times=None, n_obs=50, frac_err=0.25, seed=0, yerr=None, custom_lims=None, physical=False, device=-1):
    """Synthetic light curves of the library model from known parameters on the grid of ``GRBtype`` ("L" or "S"): pars (ndim,) or
    (n, ndim), 6..9 parameters in the sampler coordinates of ``lnprob`` (physical=True: physical ones, as ``lnlike`` takes
    them), observed at ``times`` ((n_obs,) or (n, n_obs); None: n_obs grid points drawn as ``synth.generate_data`` draws them)
    with errors yerr or frac_err * |model| and Gaussian noise (mp_simulate).  Returns what ``synth.generate_data`` returns."""
    return summaries.simulate(_source(GRBtype, custom_lims, device), pars, times, n_obs, frac_err, seed, yerr, physical, width=(6, 9))


def model_band(samples, GRBtype, custom_lims=None, q=(0.025, 0.5, 0.975), components=("Ltot",), weights=None, device=-1):
    """Posterior-predictive band of the library model: per point of the grid of ``GRBtype``, the quantiles q of the light
    curves of the rows of `samples` (n, 6..9) in the sampler coordinates of ``lnprob`` (rows outside the prior or whose model
    failed are left out).  With weights (one per row, finite and >= 0) the quantiles of the weighted empirical distribution of
    the curves, without interpolation (mp_model_band_weighted).  Returns what ``synth.model_band`` returns."""
    return summaries.band(_source(GRBtype, custom_lims, device), samples, q, components, weights, width=(6, 9))


def model_derived(samples, GRBtype, custom_lims=None, q=(0.16, 0.5, 0.84), weights=None, device=-1):
    """Energy budgets and light-curve landmarks of the library model of every row of `samples` (n, 6..9) in the sampler
    coordinates of ``lnprob`` (box prior of ``custom_lims``, parameters 3-6 un-logged before the model), on the grid of
    ``GRBtype``: what magprop_amd.derived.NAMES lists.  Returns {"values": (n, 16) with rows outside the prior or whose model
    failed all NaN, "status", "n_used", "summary": derived.summarize(values, q, weights)}."""
    return summaries.derived(_source(GRBtype, custom_lims, device), samples, q, weights, width=(6, 9))


def model_flows(rows, GRBtype, custom_lims=None, curves=(), q=(0.16, 0.5, 0.84), weights=None, device=-1):
    """Mass budget, angular-momentum budget and propeller / accretor regime of the library model of every row of `rows`
    (n, 6..9) in the sampler coordinates of ``lnprob``, on the grid of ``GRBtype``: what magprop_amd.flows.NAMES lists (the
    quantities code/figure_4.py:139-175 plots for every burst type, reduced per sample).  Returns what ``synth.model_flows``
    returns."""
    return summaries.flows(_source(GRBtype, custom_lims, device), rows, q, weights, curves, width=(6, 9))


def model_pointwise(samples, data, GRBtype, custom_lims=None, device=-1, cells=False):
    """Pointwise predictive scores of the library model on the light curve ``data`` (columns t, Lum50, Lum50err): per
    observation, in the order of data["t"], PSIS-LOO with its Pareto-k diagnostic and WAIC over the rows of `samples` (n, 6..9)
    in the sampler coordinates of ``lnprob`` (equally weighted; up to pointwise.MAX_SAMPLES rows).  What
    ``synth.model_pointwise`` returns; two models fitted to the same ``data`` (6 against 7 parameters, say) are held against
    each other with pointwise.compare(a["loo"], b["loo"])."""
    return summaries.pointwise(_source(GRBtype, custom_lims, device, data), samples, cells, width=(6, 9))


def model_reweight(samples, data, GRBtype, alternatives, custom_lims=None, device=-1):
    """Importance reweighting of a fit of the library model on the light curve ``data`` (columns t, Lum50, Lum50err) to other
    error models and data subsets, over the rows of `samples` (n, 6..9) in the sampler coordinates of ``lnprob``; per-observation
    weights and leave_out masks are in the order of data["t"].  What ``synth.model_reweight`` returns."""
    return summaries.reweight(_source(GRBtype, custom_lims, device, data), samples, alternatives, width=(6, 9))
