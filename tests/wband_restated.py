"""The weighted band (mp_model_band_weighted, include/magprop_amd.h) restated in numpy: the integer units of the weights and the
per-column weighted quantile, without interpolation.  Every sum is an integer sum, so the order of the rows does not matter."""
import numpy as np

UNIT_SCALE = 2147483648.0     # 2^31: the units of the heaviest row


def weight_units(w):
    """u_i = floor((w_i / max(w)) * 2^31) as uint32; None where mp_band_weight_units returns MP_EINVAL (a weight that is not
    finite or is negative, or no weight > 0)."""
    w = np.asarray(w, dtype=np.float64)
    if w.size == 0 or not np.all(np.isfinite(w)) or np.any(w < 0.0) or not np.any(w > 0.0):
        return None
    return np.floor((w / np.max(w)) * UNIT_SCALE).astype(np.uint32)


def band_key(x):
    """mp_band.h band_key: unsigned keys that order as the (non-NaN) values do, -0.0 just below +0.0."""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63), ~b, b | np.uint64(1 << 63))


def weight_target(q, W):
    """T = ceil(q * (double)W) clamped to [1, W] (mp_band.h band_weight_target); W >= 1 below 2^53."""
    t = int(np.ceil(np.float64(q) * np.float64(W)))
    return min(max(t, 1), int(W))


def weighted_quantile(x, u, q):
    """Per quantile of q: the least non-NaN value of x whose cumulative units, over the values <= it in key order, reach the
    target; NaN where the non-NaN values carry no unit."""
    x, u = np.asarray(x, dtype=np.float64), np.asarray(u, dtype=np.uint32)
    q = np.atleast_1d(np.asarray(q, dtype=np.float64))
    used = ~np.isnan(x)
    xs, us = x[used], u[used].astype(np.int64)
    W = int(us.sum())
    if W == 0:
        return np.full(q.size, np.nan)
    order = np.argsort(band_key(xs), kind="stable")
    xs, cum = xs[order], np.cumsum(us[order])
    return np.array([xs[np.searchsorted(cum, weight_target(qq, W), side="left")] for qq in q])


def weighted_band(cols, u, q):
    """cols[n_grid][n] (point-major, as band_wselect_kernel reads them), u[n] -> out[nq][n_grid]: weighted_quantile of every
    column, all columns at once (tests/test_wband_cpu.py holds the two together)."""
    cols = np.atleast_2d(np.asarray(cols, dtype=np.float64))
    q = np.atleast_1d(np.asarray(q, dtype=np.float64))
    nan = np.isnan(cols)
    keys = np.where(nan, np.uint64(0xFFFFFFFFFFFFFFFF), band_key(cols))          # (no non-NaN value has the all-ones key)
    us = np.where(nan, 0, np.asarray(u, dtype=np.uint32).astype(np.int64)[None, :])
    order = np.argsort(keys, axis=1, kind="stable")
    xs, cum = np.take_along_axis(cols, order, axis=1), np.cumsum(np.take_along_axis(us, order, axis=1), axis=1)
    W = cum[:, -1]
    out = np.full((q.size, cols.shape[0]), np.nan)
    has = W > 0
    for j, qq in enumerate(q):
        T = np.clip(np.ceil(np.float64(qq) * W.astype(np.float64)), 1.0, np.maximum(W, 1).astype(np.float64)).astype(np.int64)
        idx = np.minimum(np.sum(cum < T[:, None], axis=1), cols.shape[1] - 1)
        out[j, has] = xs[np.arange(cols.shape[0]), idx][has]
    return out
