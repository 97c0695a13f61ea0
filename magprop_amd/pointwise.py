"""Pointwise predictive scores of a fit: WAIC, importance-sampling and Pareto-smoothed leave-one-out (PSIS-LOO) with the
Pareto-k diagnostic, from the per-observation table mp_model_pointwise returns.

Host only (numpy and scipy.special).  The table comes from the device (``Handle.model_pointwise``: one row per observation,
the columns of include/magprop_amd.h MP_POINTWISE_*, and the row of the largest r per observation); the matrix of pointwise
log-likelihoods of S samples x n_obs observations never reaches the host.  With ll = -r the log-likelihood term of a cell and
r its log importance ratio for leaving the observation out, the cells at or below the cut contribute weight x likelihood = 1
each and their weights through one log-sum-exp, and the cells above the cut are in the tail row: enough for plain importance
sampling, for PSIS (which changes the tail's weights only) and for WAIC.

The log-likelihood is the project's unnormalised ``lnlike`` term -0.5 ((y - model) / yerr)^2.  That is what differences between
models on one dataset need: the constant ``normalisation(yerr)`` per point is the same for every model.  Add it to ``lppd``,
``elpd_loo`` and ``elpd_waic`` for normalised densities.

Rows of a nested-sampling run are weighted and are not taken here; resample them to equal weights first
(``NestedSampler.resample_equal``, ``nested.resample_equal``) and pass the rows to ``synth.model_pointwise`` / ``mcmc_eqns.model_pointwise``.

References: Vehtari, Gelman & Gabry (2017), Statistics and Computing 27, 1413; Vehtari, Simpson, Gelman, Yao & Gabry (2024),
JMLR 25(72); Zhang & Stephens (2009), Technometrics 51, 316; Watanabe (2010), JMLR 11, 3571.
"""
import numpy as np
from scipy.special import logsumexp

# column names in the order of include/magprop_amd.h MP_POINTWISE_* (tests/test_pointwise_cpu.py holds the two together)
NAMES = ("n_used", "z_mean", "r_mean", "ll_var", "r_min", "r_max", "lppd_m", "lppd_s", "cut", "nontail_count", "nontail_m",
         "nontail_s")
N_USED, Z_MEAN, R_MEAN, LL_VAR, R_MIN, R_MAX, LPPD_M, LPPD_S, CUT, NONTAIL_COUNT, NONTAIL_M, NONTAIL_S = range(12)
MAX_SAMPLES, MAX_CELLS = 262144, 1 << 28   # MP_POINTWISE_MAX_SAMPLES, MP_POINTWISE_MAX_CELLS
KHAT_BAD = 0.7                             # above it the PSIS estimate of a point is not reliable (Vehtari et al. 2024)
MIN_TAIL = 5                               # a generalised-Pareto fit needs at least 5 values above the cut


def tail_len(n_used):
    """T(n) = M + 1 with M = ceil(min(n / 5, 3 sqrt(n))) the length of the Pareto tail, in integers as mp_pointwise.h computes
    it: M = min((n + 4) // 5, the least m with m * m >= 9 n).  0 for n < 1."""
    n = int(n_used)
    if n < 1:
        return 0
    m = int(np.sqrt(9.0 * n))
    while m * m < 9 * n:
        m += 1
    while m > 1 and (m - 1) * (m - 1) >= 9 * n:
        m -= 1
    return min((n + 4) // 5, m) + 1


def as_dict(obs):
    """{name: column} of a table (n_obs, 12) (views of it)."""
    v = np.asarray(obs)
    if v.shape[-1] != len(NAMES):
        raise ValueError(f"a pointwise table has {len(NAMES)} columns, got shape {v.shape}")
    return {name: v[..., k] for k, name in enumerate(NAMES)}


def normalisation(yerr):
    """-0.5 ln(2 pi yerr^2) per point: what turns the unnormalised lnlike term into the log density of a normal error."""
    s = np.asarray(yerr, dtype=np.float64)
    return -0.5 * np.log(2.0 * np.pi * s * s)


def gpdfit(x):
    """(k, sigma) of a generalised Pareto distribution fitted to the exceedances x (1-D, ascending, positive): the empirical
    Bayes estimate of Zhang & Stephens (2009), with the weakly informative prior on k of Vehtari, Gelman & Gabry (2017,
    appendix; PSIS 2024 section 6) that pulls it towards 0.5 with the weight of 10 observations."""
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    prior_bs, prior_k = 3.0, 10.0
    m = 30 + int(np.sqrt(n))
    b = 1.0 - np.sqrt(m / (np.arange(1, m + 1, dtype=np.float64) - 0.5))
    b /= prior_bs * x[int(n / 4.0 + 0.5) - 1]
    b += 1.0 / x[-1]
    k = np.mean(np.log1p(-b[:, None] * x[None, :]), axis=1)
    length = n * (np.log(-(b / k)) - k - 1.0)                 # profile log-likelihood of every candidate b
    with np.errstate(over="ignore"):
        w = 1.0 / np.sum(np.exp(length[None, :] - length[:, None]), axis=1)
    keep = w >= 10.0 * np.finfo(np.float64).eps
    w, b = w[keep], b[keep]
    w = w / np.sum(w)
    b_post = np.sum(b * w)
    k_post = np.mean(np.log1p(-b_post * x))
    sigma = -k_post / b_post
    k_post = (n * k_post + prior_k * 0.5) / (n + prior_k)
    return float(k_post), float(sigma)


def gpdinv(p, k, sigma):
    """Quantile function of the generalised Pareto distribution (location 0)."""
    p = np.asarray(p, dtype=np.float64)
    if abs(k) < 1.0e-30:
        return -sigma * np.log1p(-p)
    return sigma * np.expm1(-k * np.log1p(-p)) / k


def _check(obs, tail=None):
    o = np.asarray(obs, dtype=np.float64)
    if o.ndim != 2 or o.shape[1] != len(NAMES):
        raise ValueError(f"obs must be 2-D (n_obs, {len(NAMES)}), got shape {o.shape}")
    if tail is None:
        return o, None
    t = np.asarray(tail, dtype=np.float64)
    if t.ndim != 2 or t.shape[0] != o.shape[0]:
        raise ValueError(f"tail must be 2-D ({o.shape[0]}, T), got shape {t.shape}")
    return o, t


def lppd(obs):
    """Per point, the log of the posterior mean of the likelihood: LPPD_M + log LPPD_S - log N_USED (NaN without a sample)."""
    o, _ = _check(obs)
    with np.errstate(divide="ignore", invalid="ignore"):
        return o[:, LPPD_M] + np.log(o[:, LPPD_S]) - np.log(o[:, N_USED])


def waic(obs):
    """{"lppd", "p_waic", "elpd_waic"} per point (Watanabe 2010; Vehtari, Gelman & Gabry 2017 eq. 11-13): p_waic is the posterior
    variance of the pointwise log-likelihood (LL_VAR), elpd_waic = lppd - p_waic."""
    o, _ = _check(obs)
    lp = lppd(o)
    return {"lppd": lp, "p_waic": o[:, LL_VAR].copy(), "elpd_waic": lp - o[:, LL_VAR]}


def psis_point(n_used, r_max, cut, nontail_count, nontail_lse, above):
    """(elpd_loo, khat) of one observation from its split: `above` the r above the cut (ascending), nontail_lse the log of the sum
    of exp(r) over the nontail_count cells at or below it.  With fewer than MIN_TAIL values above the cut no tail is fitted:
    khat = inf and the estimate is plain importance sampling.  A point some sample gives zero likelihood (r = inf) has
    elpd_loo = -inf."""
    if not n_used >= 1:
        return np.nan, np.nan
    if not np.isfinite(r_max):
        return -np.inf, np.inf
    above = np.asarray(above, dtype=np.float64)
    lw = above - r_max                                         # log weights of the tail, the largest at 0
    khat = np.inf
    if above.size >= MIN_TAIL:
        c = np.exp(cut - r_max)
        x = np.exp(lw) - c
        if x[0] > 0.0 and np.isfinite(x[-1]):
            k, sigma = gpdfit(x)
            if np.isfinite(k):
                khat = k
                p = (np.arange(above.size, dtype=np.float64) + 0.5) / above.size
                with np.errstate(divide="ignore"):
                    lw = np.minimum(np.log(gpdinv(p, k, sigma) + c), 0.0)    # truncated at the largest raw weight
    with np.errstate(divide="ignore"):
        den = logsumexp(np.concatenate([[nontail_lse - r_max], lw]))
        num = logsumexp(np.concatenate([[np.log(nontail_count) - r_max], lw - above]))
    return num - den, khat


def psis_loo(obs, tail):
    """{"elpd_loo", "khat", "p_loo", "lppd"} per point from the table and the tail rows of mp_model_pointwise: Pareto-smoothed
    importance-sampling leave-one-out (Vehtari, Gelman & Gabry 2017; Vehtari et al. 2024).  The M = T - 1 largest importance
    ratios exp(r) above the cut are replaced by the expected order statistics of the generalised Pareto distribution fitted to
    them (gpdfit), truncated at the largest raw ratio; khat is the fitted shape (above KHAT_BAD = 0.7: unreliable).
    p_loo = lppd - elpd_loo is the effective number of parameters the point takes."""
    o, t = _check(obs, tail)
    n_obs = o.shape[0]
    elpd, khat = np.full(n_obs, np.nan), np.full(n_obs, np.nan)
    with np.errstate(divide="ignore", invalid="ignore"):
        nontail = o[:, NONTAIL_M] + np.log(o[:, NONTAIL_S])
    for j in range(n_obs):
        n = o[j, N_USED]
        if not n >= 1:
            continue
        n_above = int(n - o[j, NONTAIL_COUNT])
        held = int(np.sum(~np.isnan(t[j])))
        if n_above > held:
            raise ValueError(f"observation {j}: {n_above} cells lie above the cut but its tail row holds {held}")
        above = t[j, held - n_above:held]
        elpd[j], khat[j] = psis_point(n, o[j, R_MAX], o[j, CUT], o[j, NONTAIL_COUNT], nontail[j], above)
    lp = lppd(o)
    with np.errstate(invalid="ignore"):
        p_loo = lp - elpd
    return {"elpd_loo": elpd, "khat": khat, "p_loo": p_loo, "lppd": lp}


def _total(v):
    v = np.asarray(v, dtype=np.float64)
    n = v.size
    with np.errstate(invalid="ignore"):
        se = float(np.sqrt(n * np.var(v, ddof=1))) if n > 1 else np.nan
    return float(np.sum(v)), se


def summarize(scores, worst=5):
    """Totals of per-point scores (the dictionaries psis_loo and waic return, or their union): for every of "elpd_loo", "p_loo",
    "elpd_waic", "p_waic", "lppd" present, name -> total and name + "_se" -> sqrt(n_obs x variance over the points); with
    "khat": "n_bad" the number of points with khat > 0.7 and "worst" the indices of the `worst` largest khat, largest first."""
    out = {}
    for name in ("elpd_loo", "p_loo", "elpd_waic", "p_waic", "lppd"):
        if name in scores:
            out[name], out[name + "_se"] = _total(scores[name])
            out["n_obs"] = int(np.asarray(scores[name]).size)
    if "khat" in scores:
        k = np.asarray(scores["khat"], dtype=np.float64)
        out["n_bad"] = int(np.sum(k > KHAT_BAD))
        order = np.argsort(-np.where(np.isnan(k), -np.inf, k), kind="stable")
        out["worst"] = order[:max(0, int(worst))]
    return out


def compare(a, b):
    """(difference, standard error) of two models' per-point elpd on the SAME observations (arrays, or the dictionaries of
    psis_loo / waic): sum(a - b) and the paired sqrt(n_obs x variance of a - b).  Positive: a predicts better."""
    def elpd(v):
        if isinstance(v, dict):
            return v["elpd_loo"] if "elpd_loo" in v else v["elpd_waic"]
        return v
    x, y = np.asarray(elpd(a), dtype=np.float64), np.asarray(elpd(b), dtype=np.float64)
    if x.shape != y.shape or x.ndim != 1:
        raise ValueError(f"two per-point arrays of one length expected, got shapes {x.shape} and {y.shape}")
    return _total(x - y)
