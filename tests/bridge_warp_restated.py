"""numpy restatement of the bridge-sampling evidence with a Student-t proposal and with Warp-III (include/magprop_amd.h
mp_bridge_logz_warp; magprop_amd/csrc/mp_bridge.hip, mp_bridge.h): the host's constants of the t proposal, the chi-square normals
of a t draw, the mirror rows, the test targets 3 and 4, and the pairs' log-ratios a and b.  The moments, the Cholesky rule,
Philox, the workgroup's log-sum-exp and the fixed point are tests/bridge_restated.py's, unchanged.  Test infrastructure, as that
file is: the GPU tests compare the device's numbers with it bit for bit, the CPU tests check it against closed forms.

Every product, sum and difference is a separately rounded float64 operation in the kernels' order; `libm` is taken as
bridge_restated takes it (numpy's on the CPU, the device's through the probes on the GPU); what the header calls the host's sqrt
and log are math's, the C library's, as in the product, and the host's lgamma is the C library's through ctypes (math.lgamma is
an implementation of CPython's own and differs from it in the last bits)."""
import ctypes
import ctypes.util
import math

import numpy as np

import bridge_restated as br
from oracle.stretch_oracle import philox4x32_10

CTR_CHI = 0x42524701
NORMAL, STUDENT, MAX_NU, WARP_NOUT = 0, 1, 32, 14          # MP_BRIDGE_NORMAL, _STUDENT, _MAX_NU, _WARP_NOUT
EST_MIRRORS, DRAW_MIRRORS = 12, 13
LN_2 = 0.6931471805599453
PI = 3.141592653589793


# ---------------------------------------------------------------- the host's rule of the t proposal
_LIBM = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_LIBM.lgamma.restype, _LIBM.lgamma.argtypes = ctypes.c_double, [ctypes.c_double]


def host_lgamma(x):
    return float(_LIBM.lgamma(float(x)))


def student(L, ndim, nu):
    """(L_t packed, c_t, h) of the factor L and nu degrees of freedom"""
    dn, dd = float(nu), float(ndim)
    k = math.sqrt((dn - 2.0) / dn)
    Lt = [k * float(v) for v in L]
    sum_ln = 0.0
    for a in range(ndim):
        sum_ln = sum_ln + math.log(Lt[br.tri(a, a)])
    c_t = ((sum_ln + (0.5 * dd) * math.log(dn * PI)) + host_lgamma(dn / 2.0)) - host_lgamma((dn + dd) / 2.0)
    return np.array(Lt), c_t, 0.5 * (dn + dd)


# ---------------------------------------------------------------- draws, densities, mirrors
def normal_pairs(seed, j, r, p, ctr, libm):
    """the two normals of the Philox draw (seed; j, r, p, ctr) by the kernels' Box-Muller formula"""
    seed = int(seed)
    w = philox4x32_10(seed & br.M32, seed >> 32, j, r, np.full(j.size, p, dtype=np.uint64), np.full(j.size, ctr, dtype=np.uint64))
    rad = libm.sqrt(-2.0 * libm.log(1.0 - br.u01(w[0], w[1])))
    ang = br.TWO_PI * br.u01(w[2], w[3])
    return rad * libm.cos(ang), rad * libm.sin(ang)


def chi_normals(seed, n_draws, n_rep, nu, libm=br.NUMPY):
    """g[n_rep n_draws][nu]: the normals behind the chi-square of every draw, pair p from (seed; j, r, p, 0x42524701); an odd nu
    leaves the second normal of its last pair unused"""
    j = np.tile(np.arange(n_draws, dtype=np.uint64), n_rep)
    r = np.repeat(np.arange(n_rep, dtype=np.uint64), n_draws)
    g = np.zeros((j.size, 2 * ((nu + 1) // 2)))
    for p in range((nu + 1) // 2):
        g[:, 2 * p], g[:, 2 * p + 1] = normal_pairs(seed, j, r, p, CTR_CHI, libm)
    return g[:, :nu]


def lnq_t(xi, h, nu, c_t, libm):
    q = np.zeros(xi.shape[0])
    for a in range(xi.shape[1]):
        q = q + xi[:, a] * xi[:, a]
    with np.errstate(all="ignore"):
        return (-h) * libm.log(1.0 + q / float(nu)) - c_t


def draws(m, L, c, seed, n_draws, n_rep, libm=br.NUMPY, nu=None, h=None, warp=False):
    """(x, mirrors or None, lnq, z, scale) of the draws, flat over the repetitions: nu=None the Gaussian N(m, L L^T) with constant
    c; else the t proposal, L and c being L_t and c_t"""
    nd = len(m)
    _, lnq, z = br.draws(m, L, c, seed, n_draws, n_rep, libm)
    n = z.shape[0]
    scale = np.ones(n)
    if nu is not None:
        g = chi_normals(seed, n_draws, n_rep, nu, libm)
        w = np.zeros(n)
        for k in range(nu):
            w = w + g[:, k] * g[:, k]
        with np.errstate(all="ignore"):
            scale = libm.sqrt(float(nu) / w)
    x, xm = np.empty((n, nd)), np.empty((n, nd))
    for a in range(nd):
        s = np.zeros(n)
        for b in range(a + 1):
            s = s + L[br.tri(a, b)] * z[:, b]
        d = scale * s if nu is not None else s
        x[:, a], xm[:, a] = m[a] + d, m[a] - d
    if nu is not None:
        lnq = lnq_t(scale[:, None] * z, h, nu, c, libm)
    else:
        lnq = lnq.ravel()
    return x, (xm if warp else None), lnq, z, scale


def residuals(m, L, x):
    """z of the rows x by forward substitution, and the rows' mirrors m - (x - m)"""
    x = np.asarray(x, dtype=np.float64)
    z, xm = np.zeros(x.shape), np.empty(x.shape)
    for a in range(x.shape[1]):
        d = x[:, a] - m[a]
        xm[:, a] = m[a] - d
        t = d
        for b in range(a):
            t = t - L[br.tri(a, b)] * z[:, b]
        z[:, a] = t / L[br.tri(a, a)]
    return z, xm


def target_lnp(x, target, libm=br.NUMPY):
    """the test targets on rows: 1 and 2 bridge_restated's; 3 the split normal, 4 the product of t_3 densities"""
    if target in (1, 2):
        return br.target_lnp(x, target)
    x = np.asarray(x, dtype=np.float64)
    v = np.zeros(x.shape[0])
    for d in range(x.shape[1]):
        if target == 3:
            u = np.where(x[:, d] < 0.0, x[:, d], 0.25 * x[:, d])
            v = v - (0.5 * u) * u
        else:
            with np.errstate(all="ignore"):
                v = v - 2.0 * libm.log(1.0 + (x[:, d] * x[:, d]) / 3.0)
    return v


def counts(x, lnp, lower=None, upper=None):
    """where a point counts: inside the box in every coordinate and with a finite lnprob"""
    inside = np.ones(x.shape[0], dtype=bool)
    if lower is not None:
        with np.errstate(invalid="ignore"):
            inside = np.all((x >= np.asarray(lower)) & (x <= np.asarray(upper)), axis=1)
    return inside & np.isfinite(lnp)


def pair(v, ok, vm, okm, lnq, libm=br.NUMPY):
    """the log-ratio of rows with lnprob v (counting where ok) and mirrors vm (okm; None: no warp)"""
    v, lnq = np.asarray(v, dtype=np.float64), np.asarray(lnq, dtype=np.float64)
    with np.errstate(all="ignore"):
        if vm is None:
            return np.where(ok, v - lnq, -np.inf)
        both = np.where(ok, v, np.where(okm, vm, -np.inf))
        two = ok & okm
        if np.any(two):                                   # lse2 of two finite values only
            both[two] = br.lse2(v[two], np.asarray(vm)[two], libm)
        return np.where(ok | okm, (both - LN_2) - lnq, -np.inf)


# ---------------------------------------------------------------- the whole call
def logz(x_fit, x_est, lnp_est, lower=None, upper=None, n_draws=None, n_rep=1, seed=0, neff=None, max_iter=1000, tol=1.0e-10,
         target=1, proposal=NORMAL, nu=5, warp=False, lnprob=None, libm=br.NUMPY, chunk_blocks=None):
    """What Handle.bridge_logz(..., proposal=, nu=, warp=, details=True) returns, restated.  target 1 .. 4: the test targets;
    lnprob: a function of rows that stands for the evaluation instead (target 0's batches, or a closed-form density)."""
    x_fit, x_est = np.asarray(x_fit, dtype=np.float64), np.asarray(x_est, dtype=np.float64)
    lnp_est = np.asarray(lnp_est, dtype=np.float64)
    n_fit, nd = x_fit.shape
    n_est = x_est.shape[0]
    n_draws = n_est if n_draws is None else int(n_draws)
    neff = float(n_est) if neff is None else float(neff)
    ev = (lambda rows: np.asarray(lnprob(rows), dtype=np.float64)) if lnprob is not None else (lambda rows: target_lnp(rows, target, libm))
    mom = br.moments(x_fit, chunk_blocks)
    m, L, c = br.factor(mom, x_fit[0], n_fit, nd)
    t_nu, h = None, None
    if proposal == STUDENT:
        t_nu = int(nu)
        L, c, h = student(L, nd, t_nu)
    x, xm, lnq, _, _ = draws(m, L, c, seed, n_draws, n_rep, libm, t_nu, h, warp)
    lnp = ev(x)
    lnp_m = ev(xm) if warp else None
    ok_m = counts(xm, lnp_m, lower, upper) if warp else None
    b = pair(lnp, counts(x, lnp, lower, upper), lnp_m, ok_m, lnq, libm).reshape(n_rep, n_draws)
    z, est_m = residuals(m, L, x_est)
    q_est = lnq_t(z, h, t_nu, c, libm) if t_nu is not None else br.lnq_of(z, c)
    est_lnp_m = ev(est_m) if warp else None
    est_ok_m = counts(est_m, est_lnp_m, lower, upper) if warp else None
    a = pair(lnp_est, np.ones(n_est, dtype=bool), est_lnp_m, est_ok_m, q_est, libm)
    k = br.constants(n_est, n_draws, neff, lower, upper)
    out = np.zeros((n_rep, WARP_NOUT))
    for r in range(n_rep):
        out[r, :br.NOUT] = br.fixed_point(a, b[r], *k, max_iter, tol, libm)
        if warp:
            out[r, EST_MIRRORS] = np.count_nonzero(est_ok_m)
            out[r, DRAW_MIRRORS] = np.count_nonzero(ok_m.reshape(n_rep, n_draws)[r])
    res = {"out": out, "moments": mom, "draws": x.reshape(n_rep, n_draws, nd), "draw_lnp": lnp.reshape(n_rep, n_draws),
           "draw_lnq": lnq.reshape(n_rep, n_draws), "est_lnq": q_est, "a": a, "b": b, "m": m, "L": L, "c": c, "h": h}
    if warp:
        res.update(draw_mirrors=xm.reshape(n_rep, n_draws, nd), draw_mirror_lnp=lnp_m.reshape(n_rep, n_draws), est_mirrors=est_m,
                   est_mirror_lnp=est_lnp_m)
    return res
