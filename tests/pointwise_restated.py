"""The three kernels of the pointwise scores (magprop_amd/csrc/mp_pointwise.hip) restated in numpy, in the order
magprop_amd/csrc/mp_pointwise.h states: the cell, the tail length, the cut and the tail row, and the per-observation columns.

Everything but the S halves of the log-sum-exp pairs is bit for bit what the kernels compute: numpy rounds every operation on
its own, and the sums run in the kernels' order (thread k of 256 takes samples k, k + 256, ..., the xor butterfly over a
wavefront's 64 partial results, the four wavefronts in order).  The log-sum-exp pairs follow lse_add, wave_lse and lse_merge
of mp_math.hpp with numpy's exp, which is not the device's: they agree with the kernels to rounding only.  `definition` is the
same table in long double without any prescribed order, for bounds."""
import numpy as np

N = 12
N_USED, Z_MEAN, R_MEAN, LL_VAR, R_MIN, R_MAX, LPPD_M, LPPD_S, CUT, NONTAIL_COUNT, NONTAIL_M, NONTAIL_S = range(N)
THREADS, WAVE = 256, 64
MAX_SAMPLES, MAX_CELLS, MAX_TAIL = 262144, 1 << 28, 1537
EXACT = (N_USED, Z_MEAN, R_MEAN, LL_VAR, R_MIN, R_MAX, LPPD_M, CUT, NONTAIL_COUNT, NONTAIL_M)   # columns without an exp in them
ORDER_FREE = (N_USED, R_MIN, R_MAX, LPPD_M, CUT, NONTAIL_COUNT, NONTAIL_M)                      # ... and without a sum


def tail_len(n):
    """T(n) = M + 1, M = min((n + 4) // 5, the least m with m * m >= 9 n), in Python integers; 0 for n < 1."""
    n = int(n)
    if n < 1:
        return 0
    m = 1
    while m * m < 9 * n:
        m += 1
    return min((n + 4) // 5, m) + 1


def digest(t, x):
    """(g, dx, idt) of observation times x (ascending) on the grid t, as mp_set_dataset brackets them: t[g] <= x < t[g + 1],
    the last grid point in the last interval."""
    t, x = np.asarray(t, dtype=np.float64), np.asarray(x, dtype=np.float64)
    if not np.all((x >= t[0]) & (x <= t[-1])):              # (NaN too) interp1d(bounds_error=True): mp_set_dataset refuses these
        raise ValueError("A value in x_new is outside the interpolation range.")
    g = np.clip(np.searchsorted(t, x, side="right") - 1, 0, t.size - 2).astype(np.int32)
    return g, x - t[g], 1.0 / (t[g + 1] - t[g])


def tile_ptr(g, n_tiles, bucket=64):
    """tile_ptr[n_tiles + 1] of mp_set_dataset: the observations of the buckets of `bucket` grid intervals before bucket k"""
    counts = np.zeros(int(n_tiles) + 1, dtype=np.int32)
    for gj in np.asarray(g):
        counts[int(gj) // bucket + 1] += 1
    return np.cumsum(counts, dtype=np.int32)


def cells(ltot, status, g, dx, idt, y, yerr):
    """Z[n_obs][n]: z = (y - (((Lb - La) * idt) * dx + La)) / yerr per finished row, NaN for the others."""
    ltot = np.asarray(ltot, dtype=np.float64)
    n = ltot.shape[0]
    z = np.full((len(g), n), np.nan)
    ok = np.asarray(status) == 0
    with np.errstate(all="ignore"):
        la, lb = ltot[ok][:, g], ltot[ok][:, np.asarray(g) + 1]              # [ok rows][n_obs]
        mod = ((lb - la) * idt) * dx + la
        z[:, ok] = ((y - mod) / yerr).T
    return z


def _r(z):
    with np.errstate(over="ignore", invalid="ignore"):
        return 0.5 * (z * z)


def select(z, tail_stride=None):
    """(cut[n_obs], tail[n_obs][tail_stride]) of a cell matrix: per observation the min(T, n_used)-th largest r and the
    min(T, n_used) largest r ascending, NaN behind them (no used cell: all NaN)."""
    z = np.atleast_2d(np.asarray(z, dtype=np.float64))
    stride = tail_len(z.shape[1]) if tail_stride is None else int(tail_stride)
    cut = np.full(z.shape[0], np.nan)
    tail = np.full((z.shape[0], stride), np.nan)
    for j, col in enumerate(z):
        r = np.sort(_r(col[~np.isnan(col)]))
        m = r.size
        if m == 0:
            continue
        tm = min(tail_len(m), m)
        cut[j] = r[m - tm]
        k = min(tm, stride)
        tail[j, :k] = r[m - tm:m - tm + k]
    return cut, tail


def _lanes(n):
    """sample index of (step, thread): [steps][256]"""
    steps = (n + THREADS - 1) // THREADS
    return np.arange(steps * THREADS).reshape(steps, THREADS)


def _butterfly(v, op):
    """the xor butterfly over the last axis' wavefronts: v[..., 256] -> every lane of a wavefront holds its combination"""
    lanes = np.arange(THREADS)
    for d in (32, 16, 8, 4, 2, 1):
        v = op(v, v[..., lanes ^ d])
    return v


def block_sum(vals, valid):
    """vals, valid [n_obs][n] -> [n_obs]: the kernels' sum of the valid entries"""
    n_obs, n = vals.shape
    idx = _lanes(n)
    pad_v = np.zeros((n_obs, idx.size))
    pad_ok = np.zeros((n_obs, idx.size), dtype=bool)
    pad_v[:, :n], pad_ok[:, :n] = np.where(valid, vals, 0.0), valid
    acc = np.zeros((n_obs, THREADS))
    with np.errstate(all="ignore"):
        for step in idx:
            acc = np.where(pad_ok[:, step], acc + pad_v[:, step], acc)
        acc = _butterfly(acc, lambda a, b: a + b)
        out = acc[:, 0]
        for w in range(1, THREADS // WAVE):
            out = out + acc[:, w * WAVE]
    return out


def lse_add(m, s, v, on):
    """lse_add of mp_math.hpp on arrays, applied where `on`"""
    with np.errstate(all="ignore"):
        up = on & (v > m)
        plain = on & ~(v > m) & (v > -np.inf)
        s_up = s * np.exp(m - v) + 1.0
        s_pl = s + np.exp(v - m)
    return np.where(up, v, m), np.where(up, s_up, np.where(plain, s_pl, s))


def lse_merge(m, s, mo, so):
    with np.errstate(all="ignore"):
        mx = np.fmax(m, mo)
        a = np.where(s != 0.0, s * np.exp(m - mx), 0.0)
        b = np.where(so != 0.0, so * np.exp(mo - mx), 0.0)
        sn = a + b
    return np.where(sn != 0.0, mx, -np.inf), sn


def block_lse(vals, valid):
    """vals, valid [n_obs][n] -> (m, s) [n_obs] each: the kernels' running log-sum-exp of the valid entries"""
    n_obs, n = vals.shape
    idx = _lanes(n)
    pad_v = np.zeros((n_obs, idx.size))
    pad_ok = np.zeros((n_obs, idx.size), dtype=bool)
    pad_v[:, :n], pad_ok[:, :n] = np.where(valid, vals, 0.0), valid
    m, s = np.full((n_obs, THREADS), -np.inf), np.zeros((n_obs, THREADS))
    for step in idx:
        m, s = lse_add(m, s, pad_v[:, step], pad_ok[:, step])
    lanes = np.arange(THREADS)
    for d in (32, 16, 8, 4, 2, 1):
        m, s = lse_merge(m, s, m[:, lanes ^ d], s[:, lanes ^ d])
    om, os_ = m[:, 0], s[:, 0]
    for w in range(1, THREADS // WAVE):
        om, os_ = lse_merge(om, os_, m[:, w * WAVE], s[:, w * WAVE])
    return om, os_


def reduce(z, cut):
    """obs[n_obs][N] of a cell matrix and the select kernel's cut (column CUT is the cut handed in)"""
    z = np.atleast_2d(np.asarray(z, dtype=np.float64))
    cut = np.asarray(cut, dtype=np.float64)
    used = ~np.isnan(z)
    r = _r(z)
    out = np.full((z.shape[0], N), np.nan)
    m = used.sum(axis=1)
    with np.errstate(all="ignore"):
        nontail = used & (r <= cut[:, None])
        out[:, N_USED] = m
        out[:, Z_MEAN] = block_sum(z, used) / m.astype(np.float64)
        rmean = block_sum(r, used) / m.astype(np.float64)
        out[:, R_MEAN] = rmean
        dev = -r - (-rmean)[:, None]
        ss = block_sum(dev * dev, used)
        out[:, LL_VAR] = np.where(m >= 2, ss / (m - 1).astype(np.float64), np.nan)
        out[:, R_MIN] = np.where(m > 0, np.min(np.where(used, r, np.inf), axis=1), np.nan)
        out[:, R_MAX] = np.where(m > 0, np.max(np.where(used, r, -np.inf), axis=1), np.nan)
        out[:, LPPD_M], out[:, LPPD_S] = block_lse(-r, used)
        out[:, CUT] = cut
        out[:, NONTAIL_COUNT] = nontail.sum(axis=1)
        out[:, NONTAIL_M], out[:, NONTAIL_S] = block_lse(r, nontail)
    return out


def pointwise(z, tail_stride=None):
    """(obs, tail) of a cell matrix: select, then reduce"""
    cut, tail = select(z, tail_stride)
    return reduce(z, cut), tail


def definition(z):
    """The table in long double with no prescribed order: {"n", "z_mean", "r_mean", "ll_var", "r_min", "r_max", "lppd",
    "cut", "nontail_count", "nontail"} per observation, lppd and nontail the logs of the sums of exp(ll) and of exp(r) over
    the cells at or below the cut (-inf: an empty sum), and "tail" the rows of select."""
    L = np.longdouble
    z = np.atleast_2d(np.asarray(z, dtype=np.float64))
    cut, tail = select(z)
    keys = ("n", "z_mean", "r_mean", "ll_var", "r_min", "r_max", "lppd", "cut", "nontail_count", "nontail")
    out = {k: np.full(z.shape[0], np.nan, dtype=L) for k in keys}
    out["tail"] = tail

    def lse(v):
        if v.size == 0 or np.max(v) == -np.inf:
            return L(-np.inf)
        mx = np.max(v)
        if mx == np.inf:
            return L(np.inf)
        return L(mx) + np.log(np.sum(np.exp(v.astype(L) - L(mx))))

    with np.errstate(all="ignore"):
        for j, col in enumerate(z):
            c = col[~np.isnan(col)]
            r = _r(c)                                       # (the cell's own roundings are part of the definition)
            m = c.size
            out["n"][j], out["cut"][j] = m, cut[j]
            out["nontail_count"][j] = np.sum(r <= cut[j])
            out["lppd"][j] = lse(-r)
            out["nontail"][j] = lse(r[r <= cut[j]])
            if m == 0:
                continue
            out["z_mean"][j] = np.sum(c.astype(L)) / L(m)
            out["r_mean"][j] = np.sum(r.astype(L)) / L(m)
            out["r_min"][j], out["r_max"][j] = r.min(), r.max()
            if m >= 2:
                d = -r.astype(L) + out["r_mean"][j]
                out["ll_var"][j] = np.sum(d * d) / L(m - 1)
    return out
