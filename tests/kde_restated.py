"""numpy restatement of the sampler's KDE move (include/magprop_amd.h MP_MOVE_KDE): bandwidth, fit of the other half, density
sums and the proposal.  Test infrastructure: the step loop of tests/sampler_restated.py proposes with it, alone or in a
mixture with the moves of tests/moves_restated.py; the GPU tests compare the device chains with that loop on the
unit-Gaussian target, the CPU tests check it against scipy.stats.gaussian_kde and that it samples a correlated Gaussian.
The proposal arithmetic is unfused float64 in the kernel's order; the kernel's sums over the other half run in an order of
their own, and log / exp / sqrt / cos / sin are not numpy's, so the device agrees with this to rounding, not bit for bit --
unless the sums are taken in the kernel's order (kernel_sum, fit(waves=)) and the normals through the device's functions
(normals_batch), which tests/test_gpu_sampler_posterior.py does: the proposal is then the kernel's bit for bit (the Hastings
term, which only decides, stays restated to rounding)."""
import math

import numpy as np

from moves_restated import pick
from oracle.stretch_oracle import philox4x32_10, u01

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


def kernel_sum(terms, waves):
    """The sum of terms[n, ...] over n in the order of kde_proposal on a workgroup of `waves` wavefronts: thread t adds the
    terms t, t + 64 waves, ... in order, a butterfly over the 64 lanes of a wavefront (wave_sum: xor 32, 16, .. 1), then the
    wavefronts' sums in order."""
    nt, shape = 64 * waves, terms.shape[1:]
    acc = np.zeros((nt,) + shape)
    for r in range(0, len(terms), nt):
        chunk = terms[r:r + nt]
        acc[:len(chunk)] = acc[:len(chunk)] + chunk
    acc = acc.reshape((waves, 64) + shape)
    lanes = np.arange(64)
    for dist in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lanes ^ dist]
    s = np.zeros(shape)
    for w in range(waves):
        s = s + acc[w, 0]
    return s


def fit(x, f, waves=0, sqrt=np.sqrt):
    """(Sigma = f^2 S, its Cholesky factor L or None where S is not positive definite) of the points x[n_comp, ndim]: the
    mean and the centred products summed in slot order, S = sums / (n_comp - 1), L by rows.  waves > 0: the sums in the
    kernel's own order on a workgroup of that many wavefronts (kernel_sum) and the pivots through `sqrt` (the device's), which
    makes L the kernel's bit for bit."""
    n, d = x.shape
    if waves:
        mu = kernel_sum(x, waves) / n
        e = x - mu
        prods = kernel_sum(e[:, :, None] * e[:, None, :], waves)
    else:
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
                    L[a, a] = sqrt(s)
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


def normals_batch(seed, step, half, ks, d, libm):
    """normals() of the walkers ks, [len(ks), d], with log, sqrt, cos and sin taken from libm (the device's: bit for bit the
    kernel's normals), one call of each for the whole batch."""
    pairs = (d + 1) // 2
    ua, ub = np.empty((len(ks), pairs)), np.empty((len(ks), pairs))
    for i, k in enumerate(ks):
        for p in range(pairs):
            s = philox4x32_10(seed & M32, seed >> 32, step, half, int(k), KDE_CTR + 1 + p)
            ua[i, p], ub[i, p] = u01(s[0], s[1]), u01(s[2], s[3])
    rad = libm.sqrt(-2.0 * libm.log(1.0 - ua))
    ang = TWO_PI * ub
    n = np.empty((len(ks), 2 * pairs))
    n[:, 0::2], n[:, 1::2] = rad * libm.cos(ang), rad * libm.sin(ang)
    return n[:, :d]


def propose_kde(pos, k, comp, seed, step, half, L, zero_hastings=False, nrm=None):
    """(proposal, Hastings term, ln u) of walker k; comp = global indices of the other half in split order, L = the factor
    of fit() over them (None: NaN proposal); nrm: the walker's normals where they come from normals_batch."""
    d = pos.shape[1]
    r = philox4x32_10(seed & M32, seed >> 32, step, half, k, KDE_CTR)
    with np.errstate(divide="ignore"):
        logu = np.log(u01(r[2], r[3]))
    if L is None:
        return np.full(d, np.nan), np.nan, logu
    xc = pos[comp[pick(u01(r[0], r[1]), len(comp))]]
    n = normals(seed, step, half, k, d) if nrm is None else nrm
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


def correlated_gaussian_nd(cov):
    """lnprob of the zero-mean Gaussian of covariance cov (up to a constant)."""
    prec = np.linalg.inv(np.asarray(cov, dtype=np.float64))

    def fn(p):
        p = np.asarray(p, dtype=np.float64)
        return -0.5 * float(p @ prec @ p)
    return fn
