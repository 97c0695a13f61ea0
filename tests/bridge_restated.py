"""numpy restatement of the bridge-sampling evidence estimate (include/magprop_amd.h mp_bridge_logz; magprop_amd/csrc/mp_bridge.hip,
mp_bridge.h): the moments of the fit rows in blocks, the host's Cholesky rule, the Philox / Box-Muller draws, the proposal
density at the estimator rows, and the fixed point in logs.  Test infrastructure: the GPU tests compare the device's numbers with
it bit for bit, the CPU tests check with it that the scheme gives the evidence of cases with a closed form.

Every product, sum and difference is a separately rounded float64 operation in the kernels' order.  The elementary functions the
kernels take from the device runtime come in as `libm` (exp, log, cos, sin, sqrt over arrays): numpy's on the CPU, the device's
(the mpt_libm and mpl_libm probes) where a device value is compared bit for bit.  What the header calls "the host's log" is
math.log here, the C library's, as in the product.  A running log-sum-exp asks for its exponentials in one batch per stage: the
arguments of a thread's sequence follow from its running maximum alone."""
import math
from typing import Callable, NamedTuple

import numpy as np

from oracle.stretch_oracle import philox4x32_10

M32 = 0xFFFFFFFF
CTR = 0x42524700
BLOCK, MAX_REP, MAX_ROWS, NOUT = 4096, 64, 1 << 22, 12     # MP_BRIDGE_*
OK, ITER_LIMIT, NO_OVERLAP = 0, 1, 2
LNZ, LAMBDA, LN_VOLUME, DLNZ, NITER, STATUS, NFINITE, LAMBDA0, MEAN1, VAR1, MEAN2, VAR2 = range(NOUT)
WG, WAVE = 256, 64
LN_2PI = 1.8378770664093453
TWO_PI = 6.283185307179586


class Libm(NamedTuple):
    exp: Callable
    log: Callable
    cos: Callable
    sin: Callable
    sqrt: Callable


def _quiet(f):
    def g(x):
        with np.errstate(all="ignore"):
            return f(np.asarray(x, dtype=np.float64))
    return g


NUMPY = Libm(*(_quiet(f) for f in (np.exp, np.log, np.cos, np.sin, np.sqrt)))


def tri(a, b):
    """index of entry (a, b <= a) of a packed lower triangle"""
    return a * (a + 1) // 2 + b


def n_moments(ndim):
    return ndim + ndim * (ndim + 1) // 2


# ---------------------------------------------------------------- the order of mp_wg.h
def _threads(v, fill):
    """v[n] -> [rows][256]: element k + 256 r at [r][k], padded with fill"""
    v = np.asarray(v, dtype=np.float64)
    rows = max(1, -(-v.size // WG))
    pad = np.full(rows * WG, fill)
    pad[:v.size] = v
    return pad.reshape(rows, WG)


def wg_sum(v):
    """the sum of v: thread k adds its elements k, k + 256, ... in order from 0.0, then the xor butterfly inside each wavefront
    and the four wavefronts in order"""
    acc = np.zeros(WG)
    rows = _threads(v, 0.0)
    n = np.asarray(v).size
    for r, row in enumerate(rows):
        live = np.arange(WG) + r * WG < n
        acc = np.where(live, acc + row, acc)
    lanes = np.arange(WG)
    for d in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[lanes ^ d]
    out = acc[0]
    for w in range(1, WG // WAVE):
        out = out + acc[w * WAVE]
    return float(out)


def lse_merge(m, s, mo, so, exp):
    """lse_merge of mp_math.hpp on arrays"""
    with np.errstate(all="ignore"):
        mx = np.fmax(m, mo)
        e = exp(np.concatenate([m - mx, mo - mx]))
        a = np.where(s != 0.0, s * e[:m.size], 0.0)
        b = np.where(so != 0.0, so * e[m.size:], 0.0)
        sn = a + b
    return np.where(sn != 0.0, mx, -np.inf), sn


def wg_lse(v, libm):
    """LSE of v in the kernel's order: (M, s) with the sum e^M s; per thread lse_add over its elements in order, then wg_lse"""
    rows = _threads(v, -np.inf)
    with np.errstate(all="ignore"):
        # the running maximum before every element, and with it the argument of every exponential
        before = np.vstack([np.full((1, WG), -np.inf), np.maximum.accumulate(rows, axis=0)[:-1]])
        up = rows > before
        arg = np.where(up, before - rows, rows - before)
        e = exp_shaped(libm.exp, arg)
        m, s = np.full(WG, -np.inf), np.zeros(WG)
        for r in range(rows.shape[0]):
            plain = ~up[r] & (rows[r] > -np.inf)
            s = np.where(up[r], s * e[r] + 1.0, np.where(plain, s + e[r], s))
            m = np.where(up[r], rows[r], m)
    lanes = np.arange(WG)
    for d in (32, 16, 8, 4, 2, 1):
        m, s = lse_merge(m, s, m[lanes ^ d], s[lanes ^ d], libm.exp)
    om, os_ = m[:1], s[:1]
    for w in range(1, WG // WAVE):
        om, os_ = lse_merge(om, os_, m[w * WAVE:w * WAVE + 1], s[w * WAVE:w * WAVE + 1], libm.exp)
    return float(om[0]), float(os_[0])


def exp_shaped(f, x):
    return f(x.ravel()).reshape(x.shape)


def lse_value(pair, libm):
    m, s = pair
    with np.errstate(all="ignore"):
        return float(np.float64(m) + libm.log(np.array([s]))[0])


def lse2(u, v, libm):
    """max + log(1 + exp(min - max)) on arrays"""
    u, v = np.broadcast_arrays(np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64))
    with np.errstate(all="ignore"):
        mx, mn = np.fmax(u, v), np.fmin(u, v)
        return mx + libm.log(1.0 + libm.exp(mn - mx))


# ---------------------------------------------------------------- moments, factor
def moments(x, chunk_blocks=None):
    """The sums of (x - x[0]) and of their pairwise products over the rows of x[n][ndim]: [ndim + ndim (ndim + 1) / 2].
    chunk_blocks: the rows go through in chunks of that many blocks, as the product moves them; any value gives the same
    bits, for the blocks are cut from the rows alone."""
    x = np.asarray(x, dtype=np.float64)
    n, nd = x.shape
    d = x - x[0]
    n_blocks = -(-n // BLOCK)
    part = np.zeros((n_blocks, n_moments(nd)))
    step = n_blocks if chunk_blocks is None else int(chunk_blocks)
    for first in range(0, n_blocks, step):                      # a chunk: a launch of its own over whole blocks
        for blk in range(first, min(first + step, n_blocks)):
            rows = d[blk * BLOCK:(blk + 1) * BLOCK]
            for a in range(nd):
                part[blk, a] = wg_sum(rows[:, a])
                for b in range(a + 1):
                    part[blk, nd + tri(a, b)] = wg_sum(rows[:, a] * rows[:, b])
    out = part[0].copy()
    for blk in range(1, n_blocks):
        out = out + part[blk]
    return out


def factor(mom, pivot, n, ndim):
    """(m[ndim], L packed, c) of the host's rule; ValueError naming the dimension where a pivot is not finite and > 0."""
    s, P = [float(v) for v in mom[:ndim]], [float(v) for v in mom[ndim:]]
    dn, dn1 = float(n), float(n - 1)
    m, L = [0.0] * ndim, [0.0] * (ndim * (ndim + 1) // 2)
    sum_ln = 0.0
    for a in range(ndim):
        m[a] = float(pivot[a]) + s[a] / dn
        for b in range(a + 1):
            t = (P[tri(a, b)] - (s[a] * s[b]) / dn) / dn1
            for k in range(b):
                t = t - L[tri(a, k)] * L[tri(b, k)]
            if b < a:
                L[tri(a, b)] = t / L[tri(b, b)]
            else:
                r = math.sqrt(t) if t >= 0.0 else math.nan
                if not (math.isfinite(r) and r > 0.0):
                    raise ValueError(f"the covariance of x_fit is not positive definite at dimension {a}")
                L[tri(a, a)] = r
                sum_ln = sum_ln + math.log(r)
    return np.array(m), np.array(L), sum_ln + (0.5 * ndim) * LN_2PI


def unpack(L, ndim):
    out = np.zeros((ndim, ndim))
    for a in range(ndim):
        for b in range(a + 1):
            out[a, b] = L[tri(a, b)]
    return out


# ---------------------------------------------------------------- draws, densities
def u01(hi, lo):
    return (((hi << np.uint64(32)) | lo) >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def lnq_of(z, c):
    q = np.zeros(z.shape[0])
    for a in range(z.shape[1]):
        q = q + z[:, a] * z[:, a]
    return -0.5 * q - c


def draws(m, L, c, seed, n_draws, n_rep, libm=NUMPY):
    """(x[n_rep][n_draws][ndim], lnq[n_rep][n_draws], z): draw j of repetition r from Philox (seed; j, r, p, 0x42524700)."""
    nd, seed = len(m), int(seed)
    j = np.tile(np.arange(n_draws, dtype=np.uint64), n_rep)
    r = np.repeat(np.arange(n_rep, dtype=np.uint64), n_draws)
    z = np.zeros((j.size, nd + 1))
    for p in range((nd + 1) // 2):
        w = philox4x32_10(seed & M32, seed >> 32, j, r, np.full(j.size, p, dtype=np.uint64), np.full(j.size, CTR, dtype=np.uint64))
        rad = libm.sqrt(-2.0 * libm.log(1.0 - u01(w[0], w[1])))
        ang = TWO_PI * u01(w[2], w[3])
        z[:, 2 * p], z[:, 2 * p + 1] = rad * libm.cos(ang), rad * libm.sin(ang)
    z = z[:, :nd]
    x = np.empty((j.size, nd))
    for a in range(nd):
        s = np.zeros(j.size)
        for b in range(a + 1):
            s = s + L[tri(a, b)] * z[:, b]
        x[:, a] = m[a] + s
    return x.reshape(n_rep, n_draws, nd), lnq_of(z, c).reshape(n_rep, n_draws), z


def est_lnq(m, L, c, x):
    """lnq of the rows x by forward substitution"""
    x = np.asarray(x, dtype=np.float64)
    z = np.zeros(x.shape)
    for a in range(x.shape[1]):
        t = x[:, a] - m[a]
        for b in range(a):
            t = t - L[tri(a, b)] * z[:, b]
        z[:, a] = t / L[tri(a, a)]
    return lnq_of(z, c)


def target_lnp(x, target):
    """point_eval's test targets on rows: 1 the unit Gaussian, 2 the same on terraces along x_0"""
    x = np.asarray(x, dtype=np.float64)
    v = np.zeros(x.shape[0])
    for d in range(x.shape[1]):
        v = v - (0.5 * x[:, d]) * x[:, d]
    if target == 2:
        v = v - 1.0e-3 * np.floor(37.0 * x[:, 0])
    return v


def form_b(x, lnp, lnq, lower=None, upper=None):
    inside = np.ones(x.shape[0], dtype=bool)
    if lower is not None:
        with np.errstate(invalid="ignore"):
            inside = np.all((x >= np.asarray(lower)) & (x <= np.asarray(upper)), axis=1)
    with np.errstate(invalid="ignore"):
        return np.where(inside & np.isfinite(lnp), lnp - lnq, -np.inf)


# ---------------------------------------------------------------- the fixed point
def constants(n1, n2, neff, lower=None, upper=None):
    """(ln s1, ln s2, ln N1, ln N2, tau, ln_volume) as the host forms them"""
    den = float(neff) + float(n2)
    lv = 0.0
    if lower is not None:
        for lo, hi in zip(lower, upper):
            lv = lv + math.log(float(hi) - float(lo))
    return math.log(float(neff) / den), math.log(float(n2) / den), math.log(float(n1)), math.log(float(n2)), float(n1) / float(neff), lv


def update(lam, a, b, ln_s1, ln_s2, ln_n1, ln_n2, libm=NUMPY):
    """one update of the fixed point at lam"""
    c2 = ln_s2 + lam
    with np.errstate(all="ignore"):
        num = lse_value(wg_lse(b - lse2(ln_s1 + b, c2, libm), libm), libm)
        den = lse_value(wg_lse(-lse2(ln_s1 + a, c2, libm), libm), libm)
        return float((np.float64(num) - ln_n2) - (np.float64(den) - ln_n1))


def f_terms(lam, a, b, ln_s1, ln_s2, libm=NUMPY):
    with np.errstate(all="ignore"):
        f1 = libm.exp(-lse2((ln_s1 + a) - lam, ln_s2, libm))
        f2 = libm.exp((b - lam) - lse2((ln_s1 + b) - lam, ln_s2, libm))
    return f1, f2


def fixed_point(a, b, ln_s1, ln_s2, ln_n1, ln_n2, tau, ln_volume, max_iter, tol, libm=NUMPY):
    """out[NOUT] of one repetition over a[n1] and b[n2]"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    n1, n2 = a.size, b.size
    out = np.full(NOUT, np.nan)
    out[LN_VOLUME] = ln_volume
    n_finite = int(np.count_nonzero(b > -np.inf))
    with np.errstate(all="ignore"):
        lam0 = float(np.float64(lse_value(wg_lse(b, libm), libm)) - ln_n2)
    if n_finite == 0:
        out[NITER], out[STATUS], out[NFINITE], out[LAMBDA0] = 0.0, NO_OVERLAP, 0.0, -np.inf
        return out
    lam, niter, status = lam0, 0, ITER_LIMIT
    while niter < max_iter:
        nxt = update(lam, a, b, ln_s1, ln_s2, ln_n1, ln_n2, libm)
        with np.errstate(all="ignore"):
            step = abs(np.float64(nxt) - lam)
        lam = nxt
        niter += 1
        if step <= tol:
            status = OK
            break
    f1, f2 = f_terms(lam, a, b, ln_s1, ln_s2, libm)
    with np.errstate(all="ignore"):
        mean1 = np.float64(wg_sum(f1)) / float(n1)
        var1 = np.float64(wg_sum((f1 - mean1) * (f1 - mean1))) / float(n1)
        mean2 = np.float64(wg_sum(f2)) / float(n2)
        var2 = np.float64(wg_sum((f2 - mean2) * (f2 - mean2))) / float(n2)
        t2 = var2 / (float(n2) * (mean2 * mean2))
        t1 = tau * (var1 / (float(n1) * (mean1 * mean1)))
        dlnz = libm.sqrt(np.array([t2 + t1]))[0]
        out[:] = [np.float64(lam) - ln_volume, lam, ln_volume, dlnz, niter, status, n_finite, lam0, mean1, var1, mean2, var2]
    return out


def logz(x_fit, x_est, lnp_est, lower=None, upper=None, n_draws=None, n_rep=1, seed=0, neff=None, max_iter=1000, tol=1.0e-10,
         target=1, lnprob=None, libm=NUMPY, chunk_blocks=None):
    """What Handle.bridge_logz(..., details=True) returns, restated.  target 1, 2: point_eval's test targets; lnprob: a function
    of rows that stands for the evaluation instead (target 0's mp_lnprob_batch, or a closed-form density on the CPU)."""
    x_fit, x_est = np.asarray(x_fit, dtype=np.float64), np.asarray(x_est, dtype=np.float64)
    lnp_est = np.asarray(lnp_est, dtype=np.float64)
    n_fit, nd = x_fit.shape
    n_est = x_est.shape[0]
    n_draws = n_est if n_draws is None else int(n_draws)
    neff = float(n_est) if neff is None else float(neff)
    mom = moments(x_fit, chunk_blocks)
    m, L, c = factor(mom, x_fit[0], n_fit, nd)
    x, lnq, _ = draws(m, L, c, seed, n_draws, n_rep, libm)
    flat = x.reshape(-1, nd)
    lnp = np.asarray(lnprob(flat), dtype=np.float64) if lnprob is not None else target_lnp(flat, target)
    b = form_b(flat, lnp, lnq.ravel(), lower, upper).reshape(n_rep, n_draws)
    q_est = est_lnq(m, L, c, x_est)
    a = lnp_est - q_est
    k = constants(n_est, n_draws, neff, lower, upper)
    out = np.array([fixed_point(a, b[r], *k, max_iter, tol, libm) for r in range(n_rep)])
    return {"out": out, "moments": mom, "draws": x, "draw_lnp": lnp.reshape(n_rep, n_draws), "draw_lnq": lnq, "est_lnq": q_est,
            "a": a, "b": b, "m": m, "L": L, "c": c}
