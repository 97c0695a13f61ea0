"""numpy restatement of the sampler's proposal moves (include/magprop_amd.h mp_sampler_set_moves): the proposals of stretch,
differential evolution and snooker, the index draws and the mixture rule.  Test infrastructure: the step loop of
tests/sampler_restated.py proposes with it; the GPU tests compare the device chains with that loop bit for bit on the
unit-Gaussian target, the CPU tests check with it that the moves sample a correlated Gaussian.  Every product and sum is a
separately rounded float64 operation in the kernel's order."""
import math

import numpy as np

from oracle.stretch_oracle import _draw, philox4x32_10, u01

M32 = 0xFFFFFFFF
STRETCH, DE, SNOOKER = 0, 1, 2      # MP_MOVE_*


def pick(u, m):
    return min(int(u * m), m - 1)


def pick_skip(u, m, c):
    t = pick(u, m - 1)
    return t + 1 if t >= c else t


def pick_skip2(u, m, c0, c1):
    t = pick(u, m - 2)
    t = t + 1 if t >= min(c0, c1) else t
    return t + 1 if t >= max(c0, c1) else t


def resolve(table, ndim):
    """[(kind, weight, p0, p1)] as given to mp_sampler_set_moves -> [(kind, p0, p1)] as the library keeps them (DE: g0
    resolved, s = sigma sqrt(3)) and the cumulative weights."""
    moves, cum, c = [], [], 0.0
    for kind, w, p0, p1 in table:
        if kind == DE:
            moves.append((DE, p0 if p0 > 0.0 else 2.38 / math.sqrt(2.0 * ndim), p1 * math.sqrt(3.0)))
        else:
            moves.append((kind, p0, p1))
        c = c + w
        cum.append(c)
    return moves, cum


def draw_move(seed, step, cum):
    """Index of the move of step `step`: r = Philox(seed; step, 3, 0, 0x30FE), the first m with u01(r0, r1) C_last < C_m."""
    if len(cum) <= 1:
        return 0
    r = philox4x32_10(seed & M32, seed >> 32, step & M32, 3, 0, 0x30FE)
    x = u01(r[0], r[1]) * cum[-1]
    for m in range(len(cum) - 1):
        if x < cum[m]:
            return m
    return len(cum) - 1


def propose(move, pos, k, comp, seed, step, half, zero_hastings=False):
    """(proposal, Hastings term, ln u) of walker k; comp = global indices of the other half's slots in split order."""
    kind, p0, p1 = move
    ndim = pos.shape[1]
    n_comp = len(comp)
    if kind == STRETCH:
        jc, zz, logu = _draw(seed, step, half, k, n_comp, p0)
        j = comp[jc]
        q = pos[j] - (pos[j] - pos[k]) * zz
        h = (ndim - 1.0) * np.log(zz)
        return q, (0.0 if zero_hastings else h), logu
    r = philox4x32_10(seed & M32, seed >> 32, step, half, k, 2)
    r2 = philox4x32_10(seed & M32, seed >> 32, step, half, k, 3)
    with np.errstate(divide="ignore"):
        logu = np.log(u01(r2[2], r2[3]))
    if kind == DE:
        c1 = pick(u01(r[0], r[1]), n_comp)
        c2 = pick_skip(u01(r[2], r[3]), n_comp, c1)
        gamma = p0 * (1.0 + p1 * (2.0 * u01(r2[0], r2[1]) - 1.0))
        return pos[k] + gamma * (pos[comp[c1]] - pos[comp[c2]]), 0.0, logu
    cz = pick(u01(r[0], r[1]), n_comp)
    c1 = pick_skip(u01(r[2], r[3]), n_comp, cz)
    c2 = pick_skip2(u01(r2[0], r2[1]), n_comp, cz, c1)
    z, z1, z2 = pos[comp[cz]], pos[comp[c1]], pos[comp[c2]]
    d = pos[k] - z
    dz = z1 - z2
    dd = p = np.float64(0.0)
    for i in range(ndim):
        dd = dd + d[i] * d[i]
        p = p + d[i] * dz[i]
    with np.errstate(divide="ignore", invalid="ignore"):
        f = p0 * (p / dd)
        q = pos[k] + f * d
        e = q - z
        qq = np.float64(0.0)
        for i in range(ndim):
            qq = qq + e[i] * e[i]
        h = (0.5 * (ndim - 1.0)) * (np.log(qq) - np.log(dd))
    return q, (0.0 if zero_hastings else h), logu


def correlated_gaussian(rho):
    """lnprob of the 2-D Gaussian with unit variances and correlation rho."""
    c = 1.0 / (1.0 - rho * rho)

    def fn(p):
        x, y = float(p[0]), float(p[1])
        return -0.5 * c * (x * x - 2.0 * rho * x * y + y * y)
    return fn
