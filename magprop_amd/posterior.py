"""Posterior summaries from binned samples: what EnsembleSampler.get_posterior / get_quantiles make of the accumulators of the
device posterior monitor (include/magprop_amd.h mp_sampler_set_posterior states their definition).  Host only, numpy only: the
same functions serve histograms made of a stored chain."""
import warnings

import numpy as np


def edges(lower, upper, bins):
    """Bin edges lower + (upper - lower) k / bins, k = 0 .. bins: (bins + 1,) for scalars, (ndim, bins + 1) for arrays."""
    lo, hi = np.asarray(lower, dtype=np.float64), np.asarray(upper, dtype=np.float64)
    k = np.arange(int(bins) + 1, dtype=np.float64) / int(bins)
    return lo[..., None] + (hi - lo)[..., None] * k


def hist_quantiles(hist1, below, above, lower, upper, q):
    """Quantiles q of the binned samples of every dimension: (len(q), ndim), or (len(q),) for a single histogram.
    hist1 (ndim, bins) with the counts below[ndim] and above[ndim] the range [lower, upper).  The rank is r = q N over
    N = below + sum(hist1) + above, and the value is linear inside the bin that holds the rank.  Where the rank falls into
    `below` or `above` the range was too narrow: NaN there, and a RuntimeWarning that names the dimension."""
    h = np.asarray(hist1, dtype=np.float64)
    single = h.ndim == 1
    h = np.atleast_2d(h)
    ndim, bins = h.shape
    lo, hi = (np.broadcast_to(np.asarray(v, dtype=np.float64), (ndim,)) for v in (lower, upper))
    bl, ab = (np.broadcast_to(np.asarray(v, dtype=np.float64), (ndim,)) for v in (below, above))
    qa = np.atleast_1d(np.asarray(q, dtype=np.float64))
    if np.any(~((qa >= 0.0) & (qa <= 1.0))):
        raise ValueError("every quantile in q must be in [0, 1]")
    out = np.full((qa.size, ndim), np.nan)
    for d in range(ndim):
        cum = bl[d] + np.concatenate([[0.0], np.cumsum(h[d])])      # samples below edge k
        n = cum[-1] + ab[d]
        if n == 0:
            continue
        width = (hi[d] - lo[d]) / bins
        for i, qq in enumerate(qa):
            r = qq * n
            if r < bl[d] or r > cum[-1]:
                warnings.warn(f"quantile {qq:g} of dimension {d} lies {'below' if r < bl[d] else 'above'} the histogram's range "
                              f"[{lo[d]:g}, {hi[d]:g}): widen the range", RuntimeWarning, stacklevel=2)
                continue
            k = min(int(np.searchsorted(cum[1:], r, side="left")), bins - 1)
            frac = (r - cum[k]) / h[d, k] if h[d, k] > 0 else 0.0
            out[i, d] = lo[d] + (k + frac) * width
    return out[:, 0] if single else out


def mean_cov(sum1, sum2, pivot, n, ddof=1):
    """(mean[ndim], cov[ndim, ndim]) from the sums of y = x - pivot and of y_a y_b over n samples."""
    s1, s2, p = (np.asarray(v, dtype=np.float64) for v in (sum1, sum2, pivot))
    n = int(n)
    if n < 1:
        return np.full(s1.shape, np.nan), np.full(s2.shape, np.nan)
    mean = p + s1 / n
    with np.errstate(divide="ignore", invalid="ignore"):
        cov = (s2 - np.outer(s1, s1) / n) / (n - ddof)
    return mean, cov


def hist2_levels(h, mass=(0.393, 0.865)):
    """The count thresholds of a 2-D histogram whose bins at or above them enclose the masses `mass` (corner's contour levels;
    0.393 and 0.865 are the 1- and 2-sigma masses of a 2-D Gaussian): the bins sorted downwards, the count of the bin with which
    the running total first reaches mass x total.  NaN for an empty histogram."""
    flat = np.sort(np.asarray(h, dtype=np.float64).ravel())[::-1]
    run = np.cumsum(flat)
    if run.size == 0 or run[-1] == 0:
        return np.full(len(mass), np.nan)
    return np.array([flat[min(int(np.searchsorted(run, m * run[-1], side="left")), flat.size - 1)] for m in mass])


def ensemble_range(pos, lower, upper):
    """(lower, upper) of a histogram range around the walkers pos (n, ndim): per dimension [min - span, max + span] with
    span = max - min, clipped to the box [lower, upper].  Raises where a span is 0."""
    p = np.asarray(pos, dtype=np.float64)
    p = p.reshape(-1, p.shape[-1])
    mn, mx = p.min(axis=0), p.max(axis=0)
    span = mx - mn
    if np.any(~(span > 0.0)):
        raise ValueError(f"range='ensemble' needs walkers that differ in every dimension, spans: {span}")
    lo, hi = np.maximum(mn - span, np.asarray(lower, dtype=np.float64)), np.minimum(mx + span, np.asarray(upper, dtype=np.float64))
    if np.any(~(lo < hi)):
        raise ValueError(f"range='ensemble': the walkers lie outside the box [{lower}, {upper}]")
    return lo, hi
