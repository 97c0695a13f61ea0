"""Parallel tempering: the host-side pieces that need no GPU.

A tempered `EnsembleSampler` (betas=...) samples prior x L^beta on a ladder 1 = beta_0 > beta_1 > ... > beta_{T-1} > 0
(include/magprop_amd.h mp_sampler_set_temperatures).  The evidence follows by thermodynamic integration,

    ln Z(1) - ln Z(0+) = integral_0^1 <ln L>_beta d beta,

with the per-temperature means of the stored (untempered) lnL, integrated with the trapezoid rule in beta over the ladder
and a beta = 0 point that carries the hottest mean.  Z(0+) is the prior mass of the region where the model succeeds
(f_valid): tempered walkers never enter the region where lnprob = -inf, so EnsembleSampler.log_evidence adds ln f_valid
from uniform draws in the prior box (validity_term).
"""
import numpy as np


def check_ladder(betas):
    """The ladder as a float64 array; ValueError unless betas[0] == 1, strictly decreasing, every entry finite and > 0, and
    at least 2 entries (the rule of mp_sampler_set_temperatures).  beta = 0 is refused: failed models have lnprob = -inf, and
    0 x -inf is NaN."""
    b = np.asarray(betas, dtype=np.float64)
    if b.ndim != 1 or b.size < 2:
        raise ValueError(f"a temperature ladder needs at least 2 inverse temperatures, got shape {b.shape}")
    if not np.all(np.isfinite(b)) or not np.all(b > 0.0):
        raise ValueError("every inverse temperature must be finite and > 0")
    if b[0] != 1.0:
        raise ValueError(f"betas[0] must be 1, got {b[0]!r}")
    if not np.all(np.diff(b) < 0.0):
        raise ValueError("the inverse temperatures must be strictly decreasing")
    return b


def geometric_ladder(n_temps, beta_min):
    """n_temps inverse temperatures spaced evenly in ln beta from 1 down to beta_min (the common default ladder)."""
    n_temps = int(n_temps)
    if n_temps < 2 or not 0.0 < beta_min < 1.0:
        raise ValueError("geometric_ladder needs n_temps >= 2 and 0 < beta_min < 1")
    b = np.geomspace(1.0, float(beta_min), n_temps)
    b[0] = 1.0
    return check_ladder(b)


def adaptation_rate(t, lag, time):
    """kappa_t = lag / (time * (t + lag)) of ladder update t (0 for the first), in double with exactly these three operations,
    as mp_sampler_run forms it (include/magprop_amd.h mp_sampler_set_ladder_adaptation; ptemcee: lag = 10000, time = 100)."""
    t, lag, time = float(int(t)), float(lag), float(time)
    return lag / (time * (t + lag))


def ladder_gaps(betas):
    """g_i = ln beta_i - ln beta_{i+1}, the gaps of ln beta that the ladder adaptation moves: (..., T - 1) of a ladder or of an
    array of ladders (..., T).  A geometric ladder has equal gaps."""
    lb = np.log(np.asarray(betas, dtype=np.float64))
    return lb[..., :-1] - lb[..., 1:]


def swap_spread(acc):
    """max - min over the pairs of the swap acceptance fractions acc (..., T - 1): 0 on the ladder the adaptation aims at."""
    a = np.asarray(acc, dtype=np.float64)
    return a.max(axis=-1) - a.min(axis=-1)


def adaptation_settings(adapt_ladder):
    """(steps, lag, time, history) of EnsembleSampler's adapt_ladder=: an int (steps; ptemcee's lag and time, no history) or a
    dict with "steps" and optionally "lag", "time", "history"."""
    if isinstance(adapt_ladder, dict):
        extra = set(adapt_ladder) - {"steps", "lag", "time", "history"}
        if extra or "steps" not in adapt_ladder:
            raise ValueError(f"adapt_ladder takes 'steps' and optionally 'lag', 'time', 'history', got {sorted(adapt_ladder)}")
        d = adapt_ladder
    else:
        d = {"steps": adapt_ladder}
    steps = int(d["steps"])
    if steps != d["steps"] or isinstance(d["steps"], bool):
        raise ValueError(f"adapt_ladder: steps must be a whole number, got {d['steps']!r}")
    return steps, float(d.get("lag", 10000.0)), float(d.get("time", 100.0)), bool(d.get("history", False))


def thermodynamic_integral(betas, mean_lnl):
    """Trapezoid rule in beta over the ladder and a beta = 0 point carrying the hottest mean:
    sum_t (beta_t - beta_{t+1}) (m_t + m_{t+1}) / 2, t = 0 .. T-1, with beta_T = 0 and m_T = m_{T-1}."""
    b = check_ladder(betas)
    m = np.asarray(mean_lnl, dtype=np.float64)
    if m.shape != b.shape:
        raise ValueError(f"one mean per temperature expected: {m.shape} against {b.shape}")
    if not np.all(np.isfinite(m)):
        raise ValueError("a per-temperature mean of lnL is not finite (walkers without a valid model: discard more steps)")
    bb = np.append(b, 0.0)
    mm = np.append(m, m[-1])
    return float(np.sum((bb[:-1] - bb[1:]) * (mm[:-1] + mm[1:])) * 0.5)


def every_other(n_temps):
    """Indices of the coarser ladder of the error estimate: every other temperature, both ends kept."""
    idx = list(range(0, int(n_temps), 2))
    if idx[-1] != n_temps - 1:
        idx.append(n_temps - 1)
    return np.array(idx)


def ti_log_evidence(betas, mean_lnl):
    """(TI, dTI): the thermodynamic integral of the ladder and |TI - TI over every other temperature (both ends kept)|,
    the usual estimate of the discretisation error (ptemcee's)."""
    b = check_ladder(betas)
    m = np.asarray(mean_lnl, dtype=np.float64)
    fine = thermodynamic_integral(b, m)
    idx = every_other(b.size)
    coarse = thermodynamic_integral(b[idx], m[idx])
    return fine, abs(fine - coarse)


def validity_term(n_finite, n_draws):
    """(ln f_valid, its binomial error): f_valid = n_finite / n_draws, the fraction of uniform prior draws with a finite
    lnprob; d ln f = sqrt((1 - f) / (f n))."""
    n_finite, n_draws = int(n_finite), int(n_draws)
    if n_draws <= 0 or n_finite <= 0:
        raise ValueError("no prior draw had a finite lnprob: the evidence of this model is zero on the draws taken")
    f = n_finite / n_draws
    return float(np.log(f)), float(np.sqrt((1.0 - f) / (f * n_draws)))
