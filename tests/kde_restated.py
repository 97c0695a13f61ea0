"""numpy restatement of the sampler's KDE move (include/magprop_amd.h MP_MOVE_KDE) over the step's two-way split, alone or in
a mixture with the moves of tests/moves_restated.py, with the swap sweep of a tempered sampler.  Test infrastructure: the GPU
tests compare the device chains with it on the unit-Gaussian target, the CPU tests check it against scipy.stats.gaussian_kde
and that it samples a correlated Gaussian.  The proposal arithmetic is unfused float64 in the kernel's order; the kernel's
sums over the other half run in an order of their own, and log / exp / sqrt / cos / sin are not numpy's, so the device
agrees with this to rounding, not bit for bit."""
import math

import numpy as np

from moves_restated import draw_move, pick, propose, resolve
from oracle.stretch_oracle import gaussian_lnprob, philox4x32_10, split, u01

M32 = 0xFFFFFFFF
KDE = 3                  # MP_MOVE_KDE
KDE_CTR = 0x4B00         # Philox c3: 0x4B00 partner and ln u, 0x4B01 + p normals 2p, 2p + 1
TWO_PI = 6.283185307179586


def bandwidth(p0, n_comp, ndim):
    """The factor f of params[0] (0 Scott, -1 Silverman, > 0 as is), as scipy.stats.gaussian_kde computes it."""
    if p0 > 0.0:
        return float(p0)
    n = float(n_comp) if p0 == 0.0 else n_comp * (ndim + 2.0) / 4.0
    return float(np.power(n, -1.0 / (ndim + 4)))


def fit(x, f):
    """(Sigma = f^2 S, its Cholesky factor L or None where S is not positive definite) of the points x[n_comp, ndim]: the
    mean and the centred products summed in slot order, S = sums / (n_comp - 1), L by rows."""
    n, d = x.shape
    mu = np.add.accumulate(x, axis=0)[-1] / n
    e = x - mu
    prods = np.add.accumulate(e[:, :, None] * e[:, None, :], axis=0)[-1]
    sigma = (f * f) * (prods / (n - 1.0))
    L = np.zeros((d, d))
    ok = True
    for a in range(d):
        for b in range(a + 1):
            s = sigma[a, b]
            for c in range(b):
                s = s - L[a, c] * L[b, c]
            if a == b:
                ok = ok and 0.0 < s < math.inf
                with np.errstate(invalid="ignore"):
                    L[a, a] = np.sqrt(s)
            else:
                with np.errstate(invalid="ignore", divide="ignore"):
                    L[a, b] = s / L[b, b]
    return sigma, (L if ok else None)


def log_kernel_sum(x, pts, L):
    """lse_j(-|L^-1 (x - pts_j)|^2 / 2), the maximum subtracted first (forward substitution, times 1 / L_aa)."""
    d = L.shape[0]
    inv = 1.0 / np.diag(L)
    u = x[None, :] - pts
    y = np.empty_like(u)
    for a in range(d):
        s = u[:, a]
        for b in range(a):
            s = s - L[a, b] * y[:, b]
        y[:, a] = s * inv[a]
    v = np.zeros(len(pts))
    for a in range(d):
        v = v + y[:, a] * y[:, a]
    v = -0.5 * v
    m = v.max()
    return m + np.log(np.sum(np.exp(v - m)))


def normals(seed, step, half, k, d):
    n = np.empty(d + 1)
    for p in range((d + 1) // 2):
        s = philox4x32_10(seed & M32, seed >> 32, step, half, k, KDE_CTR + 1 + p)
        rad = math.sqrt(-2.0 * math.log(1.0 - u01(s[0], s[1])))
        ang = TWO_PI * u01(s[2], s[3])
        n[2 * p], n[2 * p + 1] = rad * math.cos(ang), rad * math.sin(ang)
    return n[:d]


def propose_kde(pos, k, comp, seed, step, half, L, zero_hastings=False):
    """(proposal, Hastings term, ln u) of walker k; comp = global indices of the other half in split order, L = the factor
    of fit() over them (None: NaN proposal)."""
    d = pos.shape[1]
    r = philox4x32_10(seed & M32, seed >> 32, step, half, k, KDE_CTR)
    with np.errstate(divide="ignore"):
        logu = np.log(u01(r[2], r[3]))
    if L is None:
        return np.full(d, np.nan), np.nan, logu
    xc = pos[comp[pick(u01(r[0], r[1]), len(comp))]]
    n = normals(seed, step, half, k, d)
    q = np.empty(d)
    for a in range(d):
        s = 0.0
        for b in range(a + 1):
            s = s + L[a, b] * n[b]
        q[a] = xc[a] + s
    if zero_hastings:
        return q, 0.0, logu
    pts = pos[comp]
    return q, log_kernel_sum(pos[k], pts, L) - log_kernel_sum(q, pts, L), logu


def swap_sweep(pos, lnp, perms, seed, step, betas, n_temps, n):
    """The swap sweep of a tempered step (mp_kernels.hip stretch_swap_kernel), in place."""
    for e0 in range(0, len(perms), n_temps):
        for t in range(n_temps - 1, 0, -1):
            ec, eh = e0 + t - 1, e0 + t
            dbeta = betas[ec] - betas[eh]
            for i in range(n):
                kc, kh = ec * n + perms[ec][i], eh * n + perms[eh][i]
                r = philox4x32_10(seed & M32, seed >> 32, step, 2, kc, 0)
                u = u01(r[0], r[1])
                if (math.log(u) if u > 0.0 else -math.inf) < dbeta * (lnp[kh] - lnp[kc]):
                    pos[[kc, kh]] = pos[[kh, kc]]
                    lnp[kc], lnp[kh] = lnp[kh], lnp[kc]


def run(pos, n_steps, seed, table, lnprob_fn=gaussian_lnprob, n_ensembles=1, step0=0, betas=None, n_temps=0,
        zero_hastings=False):
    """table = [(kind, weight, p0, p1)] over MP_MOVE_* (KDE: p0 as mp_sampler_set_moves takes it).  betas[e] per ensemble
    and n_temps > 1: the decisions against beta and the swap sweep after every step.  pos is advanced in place.
    Returns chain (n_steps, n_total, ndim), chain_lnp, n_accepted, moves drawn per step, accepted[n_steps, n_total]."""
    n_total, ndim = pos.shape
    n = n_total // n_ensembles
    half_n = n // 2
    n_comp = n - half_n
    moves, cum = resolve(table, ndim)   # (KDE entries pass through as they are)
    lnp = np.array([lnprob_fn(p) for p in pos])
    acc = np.zeros(n_total, dtype=np.int64)
    chain = np.empty((n_steps, n_total, ndim))
    chain_lnp = np.empty((n_steps, n_total))
    accepted = np.zeros((n_steps, n_total), dtype=bool)
    drawn = np.empty(n_steps, dtype=np.int64)
    for s in range(n_steps):
        step = step0 + s
        m = draw_move(seed, step, cum)
        drawn[s] = m
        kde = table[m][0] == KDE
        perms = [split(seed, step, e, n) for e in range(n_ensembles)]
        for half in range(2):
            for e in range(n_ensembles):
                base, perm = e * n, perms[e]
                b = 1.0 if betas is None else float(betas[e])
                comp = [base + perm[(1 - half) * half_n + c] for c in range(n_comp)]
                L = fit(pos[comp], bandwidth(table[m][2], n_comp, ndim))[1] if kde else None
                for slot in range(half_n):
                    k = base + perm[half * half_n + slot]
                    if kde:
                        q, h, logu = propose_kde(pos, k, comp, seed, step, half, L, zero_hastings)
                    else:
                        q, h, logu = propose(moves[m], pos, k, comp, seed, step, half, zero_hastings)
                    new = lnprob_fn(q)
                    with np.errstate(invalid="ignore"):
                        accept = (h + b * new) - b * lnp[k] > logu
                    if accept:
                        pos[k] = q
                        lnp[k] = new
                        acc[k] += 1
                        accepted[s, k] = True
        if betas is not None and n_temps > 1:
            swap_sweep(pos, lnp, perms, seed, step, betas, n_temps, n)
        chain[s] = pos
        chain_lnp[s] = lnp
    return chain, chain_lnp, acc, drawn, accepted


def correlated_gaussian_nd(cov):
    """lnprob of the zero-mean Gaussian of covariance cov (up to a constant)."""
    prec = np.linalg.inv(np.asarray(cov, dtype=np.float64))

    def fn(p):
        p = np.asarray(p, dtype=np.float64)
        return -0.5 * float(p @ prec @ p)
    return fn
