"""Radii, mass flows and torques of model samples: names, summaries and budgets of the table mp_model_flows returns.

Host only.  The table itself comes from the device (``Handle.model_flows``: one row per sample, the columns of
include/magprop_amd.h MP_FLOW_*): the mass that fell back, was propelled away and was accreted, the angular momentum the star
gained by accretion and lost to the dipole, the largest and the final fastness, how many grid points the sample spends on the
propeller side and when, how often it changes sides, and the smallest Alfven radius.  The cell curves behind it (``CURVES``,
include/magprop_amd.h MP_FLOW_CURVE_*) are what code/figure_3.py:202-286 recovers from its integrations and
code/figure_4.py:139-175 plots.  Masses are in g, angular momenta in g cm^2 / s, radii in cm, times in s.
"""
import numpy as np

from . import _capi, derived

# column names in the order of include/magprop_amd.h MP_FLOW_* (tests/test_flows_cases_cpu.py holds the two together)
NAMES = ("M_fb", "M_prop", "M_acc", "J_acc", "J_dip", "w_max", "t_w_max", "w_end", "n_prop", "t_prop_first", "t_prop_last",
         "n_switch", "n_capped", "n_inside", "Rm_min", "t_Rm_min")
# cell curves in the order of their mask bits MP_FLOW_CURVE_*
CURVES = _capi.FLOW_CURVES

M_SOL = 1.99e33          # g (magnetar/funcs.py:7-13)


def as_dict(values):
    """{name: column} of a table (n, 16) (views of it), or {name: value} of one row (16,)."""
    v = np.asarray(values)
    if v.shape[-1] != len(NAMES):
        raise ValueError(f"a flows table has {len(NAMES)} columns, got shape {v.shape}")
    return {name: v[..., k] for k, name in enumerate(NAMES)}


def summarize(table, q=(0.16, 0.5, 0.84), weights=None):
    """Quantiles q of every column over the finished rows of a table (n, 16), by derived.summarize's rules: {"q": q, name:
    (nq,) per column, "n_used": rows that entered}.  A finished row is one whose budgets are numbers (t_prop_first and
    t_prop_last are NaN for a sample that never propels: such a row stays in, and those two columns are summarised over the
    rows that have them).  Without weights np.nanquantile; with weights (n,) the weighted empirical distribution function
    (derived.weighted_quantile).  No row finished, or no weight on those that did: NaN."""
    v = np.asarray(table, dtype=np.float64)
    if v.ndim != 2 or v.shape[1] != len(NAMES):
        raise ValueError(f"table must be 2-D (n, {len(NAMES)}), got shape {v.shape}")
    qa = np.atleast_1d(np.asarray(q, dtype=np.float64))
    if qa.ndim != 1 or qa.size < 1 or not np.all((qa >= 0.0) & (qa <= 1.0)):
        raise ValueError("every quantile in q must be finite and in [0, 1]")
    ok = ~np.isnan(v[:, 0])
    out = {"q": qa.copy(), "n_used": int(ok.sum())}
    w = None
    if weights is not None:
        w = np.asarray(weights, dtype=np.float64)
        if w.shape != (v.shape[0],) or not np.all(np.isfinite(w)) or np.any(w < 0.0):
            raise ValueError(f"weights must be finite, >= 0 and of shape ({v.shape[0]},)")
    for k, name in enumerate(NAMES):
        have = ok & ~np.isnan(v[:, k])
        if not have.any() or (w is not None and not w[have].sum() > 0.0):
            out[name] = np.full(qa.size, np.nan)
        elif w is None:
            out[name] = np.nanquantile(v[have, k], qa)
        else:
            out[name] = derived.weighted_quantile(v[have, k], qa, w[have])
    return out


def ejected_fraction(table):
    """M_prop / (M_prop + M_acc): the share of the mass that left the disc inwards which the propeller threw out."""
    d = as_dict(np.asarray(table, dtype=np.float64))
    return d["M_prop"] / (d["M_prop"] + d["M_acc"])


def propeller_fraction(table, n_grid):
    """n_prop / n_grid: the share of the grid points (equal steps in log t) a sample spends on the propeller side, w >= 1."""
    return as_dict(np.asarray(table, dtype=np.float64))["n_prop"] / float(n_grid)


def budgets(table, derived_table, pars, cfg):
    """The two closure residuals of a flows table against the trajectory's own end points (a derived table of the same rows:
    Mdisc_end, omega_end) and initial conditions (pars: PHYSICAL rows B, P [ms], MdiscI [Msol], ...; cfg: the model
    configuration, for the moment of inertia):
      mass      |(Mdisc_end - Mdisc_0) - (M_fb - M_prop - M_acc)| / (M_fb + M_prop + M_acc)
      momentum  |I (omega_end - omega_0) - (J_acc + J_dip)| / (|J_acc| + |J_dip|)
    Both are the quadrature error of the trapezoid on the grid (plus the integrator's): {"mass": (n,), "momentum": (n,)}."""
    f = as_dict(np.asarray(table, dtype=np.float64))
    d = derived.as_dict(np.asarray(derived_table, dtype=np.float64))
    p = np.atleast_2d(np.asarray(pars, dtype=np.float64))
    mdisc0 = p[:, 2] * M_SOL
    omega0 = (2.0 * np.pi) / (1.0e-3 * p[:, 1])
    inertia = float(cfg.inertia_factor) * derived.M_STAR * derived.R_STAR * derived.R_STAR
    mass = np.abs((d["Mdisc_end"] - mdisc0) - (f["M_fb"] - f["M_prop"] - f["M_acc"])) / (f["M_fb"] + f["M_prop"] + f["M_acc"])
    mom = np.abs(inertia * (d["omega_end"] - omega0) - (f["J_acc"] + f["J_dip"])) / (np.abs(f["J_acc"]) + np.abs(f["J_dip"]))
    return {"mass": mass, "momentum": mom}
