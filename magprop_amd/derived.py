"""Derived quantities of model samples: names, units helpers and summaries of the table mp_model_derived returns.

Host only.  The table itself comes from the device (``Handle.model_derived``: one row per sample, the columns of
include/magprop_amd.h MP_DERIVED_*): radiated energy and its split between the propeller and dipole channels, peak
luminosities and their times, the times by which 10, 50 and 90 % of the energy is out, and the spin and disc-mass landmarks
of the trajectory.  Energies are in 1e50 erg, luminosities in 1e50 erg/s, times in s, omega in rad/s, disc masses in g.
"""
import numpy as np

# column names in the order of include/magprop_amd.h MP_DERIVED_* (tests/test_derived_cpu.py holds the two together)
NAMES = ("E_tot", "E_prop", "E_dip", "L_peak", "t_peak", "Lprop_peak", "t_Lprop_peak", "t10", "t50", "t90", "omega_end",
         "omega_max", "t_omega_max", "Mdisc_end", "Mdisc_max", "t_Mdisc_max")

M_STAR = 1.4 * 1.99e33   # g (magnetar/funcs.py:7-13, as magprop_amd/csrc/mp_capi.cpp star_constants)
R_STAR = 1.0e6           # cm


def as_dict(values):
    """{name: column} of a table (n, 16) (views of it), or {name: value} of one row (16,)."""
    v = np.asarray(values)
    if v.shape[-1] != len(NAMES):
        raise ValueError(f"a derived table has {len(NAMES)} columns, got shape {v.shape}")
    return {name: v[..., k] for k, name in enumerate(NAMES)}


def spin_period_ms(omega):
    """Spin period in milliseconds of an angular frequency in rad/s (the inverse of magnetar/funcs.py:17-29 init_conds)."""
    return 2.0e3 * np.pi / np.asarray(omega, dtype=np.float64)


def rotational_energy(omega, cfg):
    """0.5 I omega^2 in 1e50 erg, I = cfg.inertia_factor M R^2 the moment of inertia of the model configuration: the reservoir
    the radiated energy E_tot is held against."""
    inertia = float(cfg.inertia_factor) * M_STAR * R_STAR * R_STAR
    return 0.5 * inertia * np.asarray(omega, dtype=np.float64) ** 2 / 1.0e50


def weighted_quantile(x, q, w):
    """Quantiles q of the weighted empirical distribution of x (1-D, no NaN; weights w >= 0, not all zero): the least x whose
    cumulative weight, in sorted order, reaches q times the total.  Rows of weight 0 are no part of the distribution (q = 0
    answers the least x that carries weight)."""
    keep = w > 0.0
    x, w = x[keep], w[keep]
    order = np.argsort(x, kind="stable")
    xs, cw = x[order], np.cumsum(w[order])
    idx = np.searchsorted(cw, np.asarray(q, dtype=np.float64) * cw[-1], side="left")
    return xs[np.minimum(idx, xs.size - 1)]


def summarize(values, q=(0.16, 0.5, 0.84), weights=None):
    """Quantiles q of every column over the finished rows of a table (n, 16): {"q": q, name: (nq,) per column, "n_used": rows
    that entered}.  Without weights np.nanquantile; with weights (n,) the weighted empirical distribution function
    (weighted_quantile), so that a nested sampler's weighted samples are summarised without resampling.  No row finished, or
    no weight on those that did: NaN."""
    v = np.asarray(values, dtype=np.float64)
    if v.ndim != 2 or v.shape[1] != len(NAMES):
        raise ValueError(f"values must be 2-D (n, {len(NAMES)}), got shape {v.shape}")
    qa = np.atleast_1d(np.asarray(q, dtype=np.float64))
    if qa.ndim != 1 or qa.size < 1 or not np.all((qa >= 0.0) & (qa <= 1.0)):
        raise ValueError("every quantile in q must be finite and in [0, 1]")
    ok = ~np.isnan(v).any(axis=1)
    out = {"q": qa.copy(), "n_used": int(ok.sum())}
    if weights is None:
        cols = np.full((qa.size, len(NAMES)), np.nan) if not ok.any() else np.nanquantile(v[ok], qa, axis=0)
    else:
        w = np.asarray(weights, dtype=np.float64)
        if w.shape != (v.shape[0],) or not np.all(np.isfinite(w)) or np.any(w < 0.0):
            raise ValueError(f"weights must be finite, >= 0 and of shape ({v.shape[0]},)")
        w = w[ok]
        if not ok.any() or not w.sum() > 0.0:
            cols = np.full((qa.size, len(NAMES)), np.nan)
        else:
            cols = np.stack([weighted_quantile(v[ok, k], qa, w) for k in range(len(NAMES))], axis=1)
    out.update({name: cols[:, k] for k, name in enumerate(NAMES)})
    return out
