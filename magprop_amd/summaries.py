"""The summaries of model curves over a set of parameter rows, each one path from the rows to the result: the light-curve band,
the derived quantities, the flows, the flow band, the pointwise scores, the importance reweighting and the simulated light
curves.

Every front end (synth, mcmc_eqns, EnsembleSampler, NestedSampler) hands its rows and the request to one function here, together
with its *source*: a function of the rows' width that returns a context manager yielding (handle, dataset slot, times) -- the
Handle to evaluate on, held for the duration of the call, and for the pointwise scores the slot of the light curve and the times x
it was registered with.  ``on`` is the source of a handle that is open already.  Each function validates the request before the
source is entered (a bad request touches no device), calls the Handle and assembles the dict the front end returns.  `width`: the
number of parameters the rows must have (a number, or a (least, most) pair); None: whatever the source's handle takes.
"""
import contextlib

import numpy as np

from . import _capi
from . import derived as _derived
from . import flows as _flows
from . import pointwise as _pointwise
from . import reweight as _reweight


def on(handle, ds_id=0, x=None):
    """The source of an open handle (a sampler's own), with dataset ds_id registered under the times x."""
    return lambda ndim: contextlib.nullcontext((handle, ds_id, x))


def _rows(samples, width, cap=False):
    """samples as contiguous float64 rows (n, width); cap: no more than a band takes (_capi.band_rows)."""
    p = np.ascontiguousarray(samples, dtype=np.float64)
    lo, hi = width if np.ndim(width) else (width, width)
    if p.ndim != 2 or (width is not None and not lo <= p.shape[1] <= hi):
        raise ValueError(f"samples must be 2-D (n, {'ndim' if width is None else lo if lo == hi else f'{lo}..{hi}'}), got shape {p.shape}")
    return _capi.band_rows(p) if cap else p


def _band(method, source, samples, q, names, weights, width, extra):
    """{"t": grid, name: (nq, n_grid) per name, "n_used": rows that entered} of Handle.`method`(rows, q, names); with weights (one
    per row: the weighted band) also "n_eff", Kish's effective sample size of the rows that finished; then the entries of extra."""
    p = _rows(samples, width, cap=True)
    w = None if weights is None else _capi.band_weights(weights, p.shape[0])
    with source(p.shape[1]) as (handle, _, _):
        band, st, used = getattr(handle, method)(p, q, names, weights=w)
        out = {"t": handle.tgrid.copy()}
    out.update({c: band[k] for k, c in enumerate(names)})
    out["n_used"] = used
    if w is not None:
        out["n_eff"] = _capi.kish_n_eff(w, st)
    out.update(extra)
    return out


def band(source, samples, q, components, weights=None, width=None, extra=()):
    """The light-curve band (Handle.model_band) of the components named, in the order Ltot, Lprop, Ldip."""
    qa, _, names = _capi.band_args(q, components)
    return _band("model_band", source, samples, qa, names, weights, width, extra)


def flow_band(source, samples, q, curves, weights=None, width=None, extra=()):
    """The band of the cell curves named (Handle.model_flow_band), in the order of flows.CURVES."""
    qa, _, _ = _capi.band_args(q, "Ltot")
    _, names = _capi.flow_curve_args(curves, band=True)
    return _band("model_flow_band", source, samples, qa, names, weights, width, extra)


def derived(source, samples, q, weights=None, width=None):
    """{"values", "status", "n_used", "summary"} of Handle.model_derived(rows) and derived.summarize(values, q, weights)."""
    p = _rows(samples, width)
    with source(p.shape[1]) as (handle, _, _):
        values, status, used = handle.model_derived(p)
    return {"values": values, "status": status, "n_used": used, "summary": _derived.summarize(values, q, weights)}


def flows(source, samples, q, weights=None, curves=(), width=None):
    """{"values", "status", "n_used", "summary"} of Handle.model_flows(rows) and flows.summarize(values, q, weights); with curves
    also "t" and {name: (n, n_grid)} per named cell curve, in the order of flows.CURVES."""
    _, names = _capi.flow_curve_args(curves)
    p = _rows(samples, width)
    with source(p.shape[1]) as (handle, _, _):
        values, cells, status, used = handle.model_flows(p, curves=curves)
        t = handle.tgrid.copy()
    out = {"values": values, "status": status, "n_used": used, "summary": _flows.summarize(values, q, weights)}
    if cells is not None:
        out["t"] = t
        out.update({c: cells[:, k] for k, c in enumerate(names)})
    return out


def simulate(source, pars, x=None, n_obs=50, frac_err=0.25, seed=0, yerr=None, physical=False, width=None):
    """{"x", "y", "yerr", "model", "z", "status", "n_ok"} of Handle.simulate(rows, x): noisy light curves of the rows.  pars (ndim,)
    gives 1-D arrays, pars (n, ndim) arrays (n, n_obs) with "x" (n_obs,) when the rows share their times.  x=None is the
    reference's recipe (code/synthetic_datasets/generate_data.py:61-67): n_obs indices of the handle's grid drawn with
    replacement from numpy.random.default_rng(seed) and sorted, shared by the rows; the noise comes from the device's own
    generator under the same seed."""
    single = np.ndim(pars) == 1
    p = _rows(np.atleast_2d(np.asarray(pars, dtype=np.float64)), width)
    if x is None and int(n_obs) < 1:
        raise ValueError(f"n_obs must be at least 1, got {n_obs}")
    with source(p.shape[1]) as (handle, _, _):
        if x is None:
            t = handle.tgrid
            x = t[np.sort(np.random.default_rng(seed).integers(0, t.size, size=int(n_obs)))]
        xa = np.asarray(x, dtype=np.float64)
        out = handle.simulate(p, xa, yerr=yerr, frac_err=frac_err, seed=seed, physical=physical)
    out["x"] = xa.copy()
    if single:
        out.update({k: out[k][0] for k in ("y", "yerr", "model", "z")}, x=xa.reshape(-1), status=int(out["status"][0]))
    return out


def pointwise(source, samples, cells=False, width=None):
    """{"obs", "tail", "status", "n_used", "loo", "waic", "summary"} (and "z" with cells=True) of Handle.model_pointwise(rows,
    ds_id) and the scores of magprop_amd.pointwise.  The library keeps a dataset's observations in ascending time (stable); with
    the times x of the source, every per-point array is returned in the caller's order of x."""
    p = _rows(samples, width)
    with source(p.shape[1]) as (handle, ds_id, x):
        res = handle.model_pointwise(p, ds_id=ds_id, cells=cells)
    obs, tail, status, used = res[:4]
    z = res[4] if cells else None
    if x is not None:
        order = np.argsort(np.asarray(x, dtype=np.float64), kind="stable")
        if order.size != obs.shape[0]:
            raise ValueError(f"x has {order.size} points, the dataset {obs.shape[0]}")
        back = np.empty_like(order)
        back[order] = np.arange(order.size)
        obs, tail = obs[back], tail[back]
        z = None if z is None else z[back]
    loo, w = _pointwise.psis_loo(obs, tail), _pointwise.waic(obs)
    out = {"obs": obs, "tail": tail, "status": status, "n_used": used, "loo": loo, "waic": w, "summary": _pointwise.summarize({**w, **loo})}
    if cells:
        out["z"] = z
    return out


def reweight(source, samples, alternatives, width=None):
    """{"lw", "table", "tail", "status", "n_used", "n_eff", "khat", "log_evidence_ratio", "log_evidence_ratio_err"} of
    Handle.model_reweight(rows, ...) under the alternatives (magprop_amd.reweight.gaussian / student_t, one or a sequence) and
    the host functions of magprop_amd.reweight: lw (n_alt, n) the log importance weights, one row of the table and of the tail
    per alternative.  Per-observation weights and leave_out masks are in the caller's order of the source's times x; the
    library keeps a dataset's observations in ascending time (stable) and gets them in that order."""
    p = _rows(samples, width)
    alts = _reweight._list(alternatives)
    with source(p.shape[1]) as (handle, ds_id, x):
        n_obs = handle.dataset_size(ds_id) if x is None else int(np.size(x))
        order = None if x is None else np.argsort(np.asarray(x, dtype=np.float64), kind="stable")
        kind, alt, obs_w = _reweight.pack(alts, n_obs, order)
        lw, table, tail, status, used = handle.model_reweight(p, kind, alt, obs_w, ds_id=ds_id)
    ratio, err = _reweight.log_evidence_ratio(table, alts, n_obs)
    return {"lw": lw, "table": table, "tail": tail, "status": status, "n_used": used, "n_eff": _reweight.n_eff(table),
            "khat": _reweight.psis(table, tail)["khat"], "log_evidence_ratio": ratio, "log_evidence_ratio_err": err}
