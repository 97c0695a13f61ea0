"""The three kernels of the importance reweighting (magprop_amd/csrc/mp_reweight.hip) restated in numpy, in the order
magprop_amd/csrc/mp_reweight.h and include/magprop_amd.h state: the term, the row sum, the cut and the tail row, and the
per-alternative columns.

numpy rounds every operation on its own, and the sums run in the kernels' order (a row: lane l of 64 takes observations l, l +
64, ... from 0.0, then the xor butterfly; a column: thread k of 256 takes samples k, k + 256, ..., the butterfly over a
wavefront's 64 partial results, the four wavefronts in order).  log, log1p and exp are injectable (`Libm`): with the device
runtime's (libmp_probe_reweight.so mpr_libm) every number is the device's bit for bit; with numpy's the CPU tests hold the
restatement to the definition in long double (`definition_rows`)."""
from typing import Callable, NamedTuple

import numpy as np

import pointwise_restated as pr

N = 12
N_USED, LW_MEAN, LW_MIN, LW_MAX, LSE1_M, LSE1_S, LSE2_M, LSE2_S, CUT, NONTAIL_COUNT, NONTAIL_M, NONTAIL_S = range(N)
GAUSS, STUDENT, MAX_ALT, WAVE, THREADS = 0, 1, 64, 64, 256


class Libm(NamedTuple):
    log: Callable = np.log
    log1p: Callable = np.log1p
    exp: Callable = np.exp


NUMPY = Libm()


def model(ltot, g, dx, idt, y):
    """(mod, res) [rows][n_obs] of Ltot rows: mod = ((Lb - La) * idt) * dx + La, res = y - mod"""
    ltot, g = np.atleast_2d(np.asarray(ltot, dtype=np.float64)), np.asarray(g)
    with np.errstate(all="ignore"):
        la, lb = ltot[:, g], ltot[:, g + 1]
        mod = ((lb - la) * idt) * dx + la
        return mod, y - mod


def terms(mod, res, ye, kind, alt, libm=NUMPY):
    """t[n_alt][rows][n_obs] of the alternatives kind[n_alt], alt[n_alt][3] (scale, jitter, nu)"""
    kind, alt = np.asarray(kind), np.asarray(alt, dtype=np.float64).reshape(-1, 3)
    scale, jitter, nu = (alt[:, i][:, None, None] for i in range(3))
    with np.errstate(all="ignore"):
        se = scale * ye
        jm = jitter * mod
        var = se * se + jm * jm
        q = (res * res) / var
        g = 0.5 * np.asarray(libm.log(var), dtype=np.float64).reshape(var.shape)
        t = -(0.5 * q + g)
        st = kind == STUDENT
        if np.any(st):
            u = q[st] / nu[st]
            p = (0.5 * (nu[st] + 1.0)) * np.asarray(libm.log1p(u), dtype=np.float64).reshape(u.shape)
            t[st] = -(p + g[st])
    return t


def base_term(mod, res, ye, libm=NUMPY):
    """t_0[rows][n_obs]: the Gaussian term of scale 1 and jitter 0"""
    return terms(mod, res, ye, [GAUSS], [[1.0, 0.0, 0.0]], libm)[0]


def differences(t, t0, obs_w=None):
    """d[n_alt][rows][n_obs] = w t - t_0 (w == 0: -t_0)"""
    with np.errstate(all="ignore"):
        if obs_w is None:
            return t - t0
        w = np.asarray(obs_w, dtype=np.float64)[:, None, :]
        return np.where(w == 0.0, -t0, w * t - t0)


def wave_sum(acc):
    """the xor butterfly over the last axis of 64 lanes; every lane ends with the same value: [..., 64] -> [...]"""
    lanes = np.arange(WAVE)
    with np.errstate(all="ignore"):
        for d in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[..., lanes ^ d]
    return acc[..., 0]


def row_sum(d):
    """[..., n_obs] -> [...]: lane l adds entries l, l + 64, ... in increasing order from 0.0, then wave_sum"""
    n_obs = d.shape[-1]
    acc = np.zeros(d.shape[:-1] + (WAVE,))
    with np.errstate(all="ignore"):
        for j0 in range(0, n_obs, WAVE):
            part = d[..., j0:j0 + WAVE]
            acc[..., :part.shape[-1]] = acc[..., :part.shape[-1]] + part
    return wave_sum(acc)


def rows(ltot, status, g, dx, idt, y, yerr, kind, alt, obs_w=None, libm=NUMPY):
    """lw[n_alt][rows]: NaN for a row whose status is not 0 (its curve is not read)"""
    status = np.asarray(status)
    ok = status == 0
    out = np.full((len(kind), status.size), np.nan)
    if np.any(ok):
        mod, res = model(np.asarray(ltot, dtype=np.float64)[ok], g, dx, idt, y)
        t0 = base_term(mod, res, yerr, libm)
        out[:, ok] = row_sum(differences(terms(mod, res, yerr, kind, alt, libm), t0, obs_w))
    return out


def key(v):
    """band_key of mp_band.h: unsigned keys that order doubles by value, -0.0 below +0.0"""
    b = np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63), ~b, b | np.uint64(1 << 63))


def select(lw, tail_stride=None):
    """(cut[n_alt], tail[n_alt][tail_stride]) of lw[n_alt][n]: per alternative the min(T, n_used)-th largest lw and the min(T,
    n_used) largest ascending, NaN behind them (no used sample: all NaN)."""
    lw = np.atleast_2d(np.asarray(lw, dtype=np.float64))
    stride = pr.tail_len(lw.shape[1]) if tail_stride is None else int(tail_stride)
    cut, tail = np.full(lw.shape[0], np.nan), np.full((lw.shape[0], stride), np.nan)
    for k, col in enumerate(lw):
        v = col[~np.isnan(col)]
        v = v[np.argsort(key(v), kind="stable")]
        m = v.size
        if m == 0:
            continue
        tm = min(pr.tail_len(m), m)
        cut[k] = v[m - tm]
        tail[k, :min(tm, stride)] = v[m - tm:m - tm + min(tm, stride)]
    return cut, tail


def _lse_add(m, s, v, on, exp):
    with np.errstate(all="ignore"):
        up = on & (v > m)
        plain = on & ~(v > m) & (v > -np.inf)
        s_up = s * np.asarray(exp(m - v)).reshape(s.shape) + 1.0
        s_pl = s + np.asarray(exp(v - m)).reshape(s.shape)
    return np.where(up, v, m), np.where(up, s_up, np.where(plain, s_pl, s))


def _lse_merge(m, s, mo, so, exp):
    with np.errstate(all="ignore"):
        mx = np.fmax(m, mo)
        a = np.where(s != 0.0, s * np.asarray(exp(m - mx)).reshape(s.shape), 0.0)
        b = np.where(so != 0.0, so * np.asarray(exp(mo - mx)).reshape(s.shape), 0.0)
        sn = a + b
    return np.where(sn != 0.0, mx, -np.inf), sn


def block_lse(vals, valid, exp=np.exp):
    """vals, valid [rows][n] -> (m, s) [rows] each: the kernels' running log-sum-exp of the valid entries (lse_add, wave_lse
    and lse_merge of mp_math.hpp in the order of mp_wg.h)"""
    n_rows, n = vals.shape
    steps = (n + THREADS - 1) // THREADS
    pad_v, pad_ok = np.zeros((n_rows, steps * THREADS)), np.zeros((n_rows, steps * THREADS), dtype=bool)
    pad_v[:, :n], pad_ok[:, :n] = np.where(valid, vals, 0.0), valid
    m, s = np.full((n_rows, THREADS), -np.inf), np.zeros((n_rows, THREADS))
    for step in range(steps):
        sl = slice(step * THREADS, (step + 1) * THREADS)
        m, s = _lse_add(m, s, pad_v[:, sl], pad_ok[:, sl], exp)
    lanes = np.arange(THREADS)
    for d in (32, 16, 8, 4, 2, 1):
        m, s = _lse_merge(m, s, m[:, lanes ^ d], s[:, lanes ^ d], exp)
    om, os_ = m[:, 0], s[:, 0]
    for w in range(1, THREADS // WAVE):
        om, os_ = _lse_merge(om, os_, m[:, w * WAVE], s[:, w * WAVE], exp)
    return om, os_


def reduce(lw, cut, libm=NUMPY):
    """table[n_alt][N] of lw[n_alt][n] and the select kernel's cut (column CUT is the cut handed in)"""
    lw = np.atleast_2d(np.asarray(lw, dtype=np.float64))
    cut = np.asarray(cut, dtype=np.float64)
    used = ~np.isnan(lw)
    k = key(lw)
    out = np.full((lw.shape[0], N), np.nan)
    m = used.sum(axis=1)
    with np.errstate(all="ignore"):
        nontail = used & (k <= key(cut)[:, None])
        out[:, N_USED] = m
        out[:, LW_MEAN] = pr.block_sum(lw, used) / m.astype(np.float64)
        for j in range(lw.shape[0]):
            if m[j]:
                v = lw[j][used[j]]
                order = np.argsort(k[j][used[j]], kind="stable")
                out[j, LW_MIN], out[j, LW_MAX] = v[order[0]], v[order[-1]]
        out[:, LSE1_M], out[:, LSE1_S] = block_lse(lw, used, libm.exp)
        out[:, LSE2_M], out[:, LSE2_S] = block_lse(2.0 * lw, used, libm.exp)
        out[:, CUT] = cut
        out[:, NONTAIL_COUNT] = nontail.sum(axis=1)
        out[:, NONTAIL_M], out[:, NONTAIL_S] = block_lse(lw, nontail, libm.exp)
    return out


def cols(lw, tail_stride=None, libm=NUMPY):
    """(table, tail) of lw[n_alt][n]: select, then reduce"""
    cut, tail = select(lw, tail_stride)
    return reduce(lw, cut, libm), tail


# ---------------------------------------------------------------- the definition, for bounds
def definition_rows(mod, res, ye, kind, alt, obs_w=None):
    """(lw, allowance) [n_alt][rows] in long double from the float64 mod and res (their roundings are part of the definition):
    lw the sum of w t_k - t_0 with no prescribed order, and the allowance of the float64 restatement against it: per term 32 x
    2^-53 (|w t_k| + |t_0| + 1) -- at most 16 roundings, plus the absolute error log(var) inherits from var -- and (ceil(n_obs /
    64) + 6) 2^-53 sum |d| for the sum."""
    L = np.longdouble
    u = L(2.0) ** -53
    kind, alt = np.asarray(kind), np.asarray(alt, dtype=np.float64).reshape(-1, 3)
    mod, res, ye = (np.asarray(a, dtype=np.float64).astype(L) for a in (mod, res, ye))
    n_obs = mod.shape[-1]

    def term(kd, scale, jitter, nu):
        var = (L(scale) * ye) ** 2 + (L(jitter) * mod) ** 2
        q = res * res / var
        g = L(0.5) * np.log(var)
        if kd == STUDENT:
            return -(L(0.5) * (L(nu) + 1) * np.log1p(q / L(nu)) + g)
        return -(L(0.5) * q + g)

    t0 = term(GAUSS, 1.0, 0.0, 0.0)
    lw = np.empty((len(kind),) + mod.shape[:-1], dtype=L)
    allow = np.empty_like(lw)
    for k in range(len(kind)):
        w = np.ones(n_obs, dtype=L) if obs_w is None else np.asarray(obs_w, dtype=np.float64)[k].astype(L)
        wt = np.where(w == 0, L(0), w * term(kind[k], *alt[k]))
        d = wt - t0
        lw[k] = np.sum(d, axis=-1)
        per_term = 32 * u * (np.abs(wt) + np.abs(t0) + 1)
        allow[k] = np.sum(per_term, axis=-1) + (-(-n_obs // WAVE) + 6) * u * np.sum(np.abs(d), axis=-1)
    return lw, allow
