"""Importance reweighting of a fit to other error models and data subsets: the alternatives mp_model_reweight takes, and what
follows on the host from the table it returns -- the Bayes factor between the error models, Kish's effective sample size, the
Pareto-k diagnostic, normalised weights for the ``weights=`` arguments of the summaries, and the sensitivity of the parameters.

Host only (numpy, math and the generalised-Pareto fit of magprop_amd.pointwise).  The log weights come from the device
(``Handle.model_reweight``: lw[n_alt, n], one row of the columns of include/magprop_amd.h MP_REWEIGHT_* per alternative and
the row of its largest lw).  The chain was sampled under lnlike = -0.5 chi^2 with the light curve's own yerr, every observation
counted once: the base.  An alternative is a Gaussian or Student-t error law with ``scale`` x yerr and a model scatter of
``jitter`` x model added in quadrature, with a weight per observation (``weights=``, ``leave_out=``, ``power=``): lw of a sample
is the alternative's log-likelihood minus the base's, without the constants of the densities, which ``shape_constant`` holds.

References: Vehtari, Simpson, Gelman, Yao & Gabry (2024), JMLR 25(72); Kallioinen, Paananen, Buerkner & Vehtari (2023),
Statistics and Computing 34, 57 (power-scaling sensitivity); Kish (1965).
"""
import math
from typing import NamedTuple, Optional

import numpy as np
from scipy.special import logsumexp

from . import pointwise as _pointwise

# column names in the order of include/magprop_amd.h MP_REWEIGHT_* (tests/test_reweight_cpu.py holds the two together)
NAMES = ("n_used", "lw_mean", "lw_min", "lw_max", "lse1_m", "lse1_s", "lse2_m", "lse2_s", "cut", "nontail_count", "nontail_m",
         "nontail_s")
N_USED, LW_MEAN, LW_MIN, LW_MAX, LSE1_M, LSE1_S, LSE2_M, LSE2_S, CUT, NONTAIL_COUNT, NONTAIL_M, NONTAIL_S = range(12)
GAUSS, STUDENT, MAX_ALT = 0, 1, 64         # MP_REWEIGHT_GAUSS, MP_REWEIGHT_STUDENT, MP_REWEIGHT_MAX_ALT
KHAT_BAD, MIN_TAIL = _pointwise.KHAT_BAD, _pointwise.MIN_TAIL


class Alternative(NamedTuple):
    """One alternative likelihood (made by ``gaussian`` and ``student_t``)."""
    kind: int
    scale: float
    jitter: float
    nu: float
    weights: Optional[np.ndarray]           # per observation, in the caller's order of x; None: 1 each
    leave_out: Optional[np.ndarray]         # a boolean mask or indices of observations whose weight is 0
    power: Optional[float]                  # every weight times this


def _alternative(kind, scale, jitter, nu, weights, leave_out, power):
    scale, jitter, nu = float(scale), float(jitter), float(nu)
    if not (math.isfinite(scale) and scale > 0.0):
        raise ValueError(f"scale must be finite and > 0, got {scale!r}")
    if not (math.isfinite(jitter) and jitter >= 0.0):
        raise ValueError(f"jitter must be finite and >= 0, got {jitter!r}")
    if kind == STUDENT and not (math.isfinite(nu) and nu > 0.0):
        raise ValueError(f"nu must be finite and > 0, got {nu!r}")
    if weights is not None:
        weights = np.asarray(weights, dtype=np.float64)
        if weights.ndim != 1 or not np.all(np.isfinite(weights)) or np.any(weights < 0.0):
            raise ValueError("weights must be 1-D, finite and >= 0")
    if leave_out is not None:
        leave_out = np.asarray(leave_out)
        if leave_out.size == 0 and leave_out.ndim == 1:
            leave_out = leave_out.astype(np.intp)             # (an empty list of indices: nothing is left out)
        if leave_out.ndim != 1 or leave_out.dtype.kind not in "biu":
            raise ValueError("leave_out must be a 1-D boolean mask or 1-D indices")
    if power is not None:
        power = float(power)
        if not (math.isfinite(power) and power >= 0.0):
            raise ValueError(f"power must be finite and >= 0, got {power!r}")
    return Alternative(kind, scale, jitter, nu, weights, leave_out, power)


def gaussian(scale=1.0, jitter=0.0, weights=None, leave_out=None, power=None):
    """A Gaussian error law of standard deviation sqrt((scale yerr)^2 + (jitter model)^2)."""
    return _alternative(GAUSS, scale, jitter, 0.0, weights, leave_out, power)


def student_t(nu, scale=1.0, jitter=0.0, weights=None, leave_out=None, power=None):
    """A Student-t error law with nu degrees of freedom and the Gaussian's scale parameter."""
    return _alternative(STUDENT, scale, jitter, nu, weights, leave_out, power)


def _list(alternatives):
    alts = [alternatives] if isinstance(alternatives, Alternative) else list(alternatives)
    if not 1 <= len(alts) <= MAX_ALT or not all(isinstance(a, Alternative) for a in alts):
        raise ValueError(f"1 to {MAX_ALT} (MP_REWEIGHT_MAX_ALT) alternatives made by gaussian() or student_t() expected")
    return alts


def observation_weights(alt, n_obs):
    """The weights (n_obs,) of the observations under alt, in the caller's order; None: every weight 1."""
    if alt.weights is None and alt.leave_out is None and alt.power is None:
        return None
    n_obs = int(n_obs)
    w = np.ones(n_obs) if alt.weights is None else alt.weights.copy()
    if w.shape != (n_obs,):
        raise ValueError(f"weights must be of shape ({n_obs},), one per observation, got {w.shape}")
    if alt.leave_out is not None:
        if alt.leave_out.dtype.kind == "b" and alt.leave_out.shape != (n_obs,):
            raise ValueError(f"a leave_out mask must be of shape ({n_obs},), got {alt.leave_out.shape}")
        w[alt.leave_out] = 0.0                                # (an index out of range raises)
    if alt.power is not None:
        w = w * alt.power
    return w


def total_weight(alt, n_obs):
    w = observation_weights(alt, n_obs)
    return float(n_obs) if w is None else float(np.sum(w))


def pack(alternatives, n_obs, order=None):
    """(kind int32 [n_alt], alt float64 [n_alt, 3], obs_w float64 [n_alt, n_obs] or None) as mp_model_reweight takes them;
    order: the permutation that takes the caller's observations to the library's (ascending time, stable)."""
    alts = _list(alternatives)
    kind = np.array([a.kind for a in alts], dtype=np.int32)
    table = np.ascontiguousarray([[a.scale, a.jitter, a.nu] for a in alts], dtype=np.float64)
    ws = [observation_weights(a, n_obs) for a in alts]
    if all(w is None for w in ws):
        return kind, table, None
    obs_w = np.ascontiguousarray([np.ones(int(n_obs)) if w is None else w for w in ws], dtype=np.float64)
    return kind, table, obs_w if order is None else np.ascontiguousarray(obs_w[:, order])


def shape_constant(alt, W):
    """The normalising constant per observation of alt's density (what lw leaves out) times the total weight W: Gaussian
    -0.5 ln 2 pi, Student-t lgamma((nu + 1) / 2) - lgamma(nu / 2) - 0.5 ln(nu pi)."""
    if alt.kind == GAUSS:
        c = -0.5 * math.log(2.0 * math.pi)
    else:
        c = math.lgamma(0.5 * (alt.nu + 1.0)) - math.lgamma(0.5 * alt.nu) - 0.5 * math.log(alt.nu * math.pi)
    return c * float(W)


def _table(table):
    t = np.atleast_2d(np.asarray(table, dtype=np.float64))
    if t.ndim != 2 or t.shape[1] != len(NAMES):
        raise ValueError(f"a reweight table has {len(NAMES)} columns, got shape {t.shape}")
    return t


def as_dict(table):
    """{name: column} of a table (n_alt, 12) (views of it)."""
    t = _table(table)
    return {name: t[:, k] for k, name in enumerate(NAMES)}


def log_mean_weight(table):
    """ln mean exp(lw) per alternative: LSE1_M + ln LSE1_S - ln N_USED (NaN without a sample)."""
    t = _table(table)
    with np.errstate(divide="ignore", invalid="ignore"):
        return t[:, LSE1_M] + np.log(t[:, LSE1_S]) - np.log(t[:, N_USED])


def n_eff(table):
    """Kish's effective sample size (sum w)^2 / sum w^2 of the weights exp(lw), per alternative."""
    t = _table(table)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.exp(2.0 * (t[:, LSE1_M] + np.log(t[:, LSE1_S])) - (t[:, LSE2_M] + np.log(t[:, LSE2_S])))


def log_evidence_ratio(table, alternatives, n_obs):
    """(ln Z_k - ln Z_0, its standard error) per alternative: the log Bayes factor of the alternative against the base, both
    likelihoods normalised densities.  ln mean exp(lw) plus the constants lw leaves out (shape_constant of the alternative
    over its total weight, minus the base's over n_obs observations); the error is the delta method's for independent
    samples, sqrt(1 / n_eff - 1 / N_USED)."""
    t = _table(table)
    alts = _list(alternatives)
    if len(alts) != t.shape[0]:
        raise ValueError(f"{len(alts)} alternatives but a table of {t.shape[0]} rows")
    base = shape_constant(gaussian(), n_obs)
    const = np.array([shape_constant(a, total_weight(a, n_obs)) - base for a in alts])
    with np.errstate(divide="ignore", invalid="ignore"):
        # 1 / n_eff - 1 / n = (n sum w^2 / (sum w)^2 - 1) / n, the bracket through expm1: exactly 0 for equal weights
        l1, l2 = t[:, LSE1_M] + np.log(t[:, LSE1_S]), t[:, LSE2_M] + np.log(t[:, LSE2_S])
        err = np.sqrt(np.maximum(np.expm1(np.log(t[:, N_USED]) + l2 - 2.0 * l1), 0.0) / t[:, N_USED])
    return log_mean_weight(t) + const, err


def psis(table, tail):
    """{"khat", "log_mean_weight"} per alternative: the shape of the generalised Pareto distribution fitted to the M = T - 1
    largest weights exp(lw) (above KHAT_BAD = 0.7 the reweighting is not reliable; inf: fewer than MIN_TAIL values above the cut,
    nothing fitted) and ln mean exp(lw) with those weights replaced by the fit's expected order statistics, truncated at the
    largest raw weight (Vehtari et al. 2024)."""
    t = _table(table)
    tl = np.atleast_2d(np.asarray(tail, dtype=np.float64))
    if tl.shape[0] != t.shape[0]:
        raise ValueError(f"tail must be 2-D ({t.shape[0]}, T), got shape {tl.shape}")
    khat, lmw = np.full(t.shape[0], np.nan), np.full(t.shape[0], np.nan)
    for k, row in enumerate(t):
        n = row[N_USED]
        if not n >= 1:
            continue
        top = row[LW_MAX]
        if not np.isfinite(top):                               # every weight 0, or an infinite one
            khat[k], lmw[k] = np.inf, top
            continue
        n_above = int(n - row[NONTAIL_COUNT])
        held = int(np.sum(~np.isnan(tl[k])))
        if n_above > held:
            raise ValueError(f"alternative {k}: {n_above} samples lie above the cut but its tail row holds {held}")
        lw = tl[k, held - n_above:held] - top                  # log weights of the tail, the largest at 0
        khat[k] = np.inf
        if lw.size >= MIN_TAIL:
            c = np.exp(row[CUT] - top)
            x = np.exp(lw) - c
            if x[0] > 0.0 and np.isfinite(x[-1]):
                kk, sigma = _pointwise.gpdfit(x)
                if np.isfinite(kk):
                    khat[k] = kk
                    p = (np.arange(lw.size, dtype=np.float64) + 0.5) / lw.size
                    with np.errstate(divide="ignore"):
                        lw = np.minimum(np.log(_pointwise.gpdinv(p, kk, sigma) + c), 0.0)
        with np.errstate(divide="ignore"):
            nontail = row[NONTAIL_M] + np.log(row[NONTAIL_S])
        lmw[k] = top + logsumexp(np.concatenate([[nontail - top], lw])) - np.log(n)
    return {"khat": khat, "log_mean_weight": lmw}


def weights(lw, k=0):
    """Normalised weights (n,) of alternative k, ready for the weights= arguments of the bands and summaries: exp(lw[k]) over
    its sum; a sample that did not finish (NaN) weighs 0."""
    row = np.atleast_2d(np.asarray(lw, dtype=np.float64))[k]
    used = ~np.isnan(row)
    w = np.zeros(row.size)
    if np.any(used):
        top = np.max(row[used])
        if top == -np.inf:
            raise ValueError(f"every sample has weight 0 under alternative {k}")
        w[used] = np.exp(row[used] - top)
        w /= np.sum(w)
    return w


def sensitivity(samples, lw):
    """{"mean", "std", "mean_err": (ndim,), "weighted_mean", "weighted_std", "weighted_mean_err": (n_alt, ndim), "n_eff": (n_alt,)}
    of the parameters: over the samples that finished as they are, and under the weights of every alternative.  The errors are
    those of independent samples: std / sqrt(n), and for the self-normalised weighted mean the delta method's sqrt(sum w_i^2 (x_i
    - mean)^2) with the weights summing to 1 (Owen 2013, Monte Carlo theory, methods and examples, 9.2), which -- unlike
    weighted_std / sqrt(n_eff) -- sees it when the large weights sit on the extreme samples.  Thin a chain by its
    autocorrelation time first."""
    x = np.asarray(samples, dtype=np.float64)
    rows = np.atleast_2d(np.asarray(lw, dtype=np.float64))
    if x.ndim != 2 or rows.shape[1] != x.shape[0]:
        raise ValueError(f"samples (n, ndim) and lw (n_alt, n) expected, got {x.shape} and {rows.shape}")
    used = ~np.isnan(rows[0])
    out = {"mean": np.mean(x[used], axis=0), "std": np.std(x[used], axis=0)}
    out["mean_err"] = out["std"] / np.sqrt(max(int(used.sum()), 1))
    shape = (rows.shape[0], x.shape[1])
    wm, ws, we, ne = np.empty(shape), np.empty(shape), np.empty(shape), np.empty(rows.shape[0])
    for k in range(rows.shape[0]):
        w = weights(rows, k)
        wm[k] = w @ x
        ws[k] = np.sqrt(w @ (x - wm[k]) ** 2)
        we[k] = np.sqrt((w * w) @ (x - wm[k]) ** 2)
        ne[k] = 1.0 / np.sum(w * w)
    out.update(weighted_mean=wm, weighted_std=ws, weighted_mean_err=we, n_eff=ne)
    return out
