"""Cases of the bridge-sampling evidence (include/magprop_amd.h mp_bridge_logz), shared by tests/test_bridge_cpu.py (the
restatement alone) and tests/test_gpu_bridge_kernels.py (the device against the restatement, bit for bit).

CLOSED: densities with a known ln Z and iid samples, so that neff = N1.  FIXED: crafted arrays (a, b) for the fixed point alone.
CALLS: crafted whole calls on the test target 1 (the unit Gaussian -0.5 sum x^2) and 2.  Everything is generated from fixed
numpy seeds; nothing here touches a device."""
import math

import numpy as np

import bridge_restated as br

SIZES = (1, 63, 64, 65, 255, 256, 257, br.BLOCK - 1, br.BLOCK, br.BLOCK + 1, 2 * br.BLOCK + 1)   # wavefront, workgroup, block


# ---------------------------------------------------------------- closed forms
def _gauss(d):
    return {"ndim": d, "truth": 0.5 * d * math.log(2.0 * math.pi), "lower": None, "upper": None,
            "lnprob": lambda x: -0.5 * np.sum(x * x, axis=1), "sample": lambda rng, n: rng.standard_normal((n, d))}


def _truncated(d, lo, hi):
    one = math.sqrt(0.5 * math.pi) * (math.erf(hi / math.sqrt(2.0)) - math.erf(lo / math.sqrt(2.0)))

    def sample(rng, n):
        out = np.empty((0, d))
        while out.shape[0] < n:
            x = rng.standard_normal((2 * n, d))
            out = np.concatenate([out, x[np.all((x >= lo) & (x <= hi), axis=1)]])
        return out[:n]

    # (the box is the support: ln_volume is taken off by the estimate, so the truth is that of lnz + ln_volume = lambda)
    return {"ndim": d, "truth": d * math.log(one), "lower": np.full(d, lo), "upper": np.full(d, hi),
            "lnprob": lambda x: -0.5 * np.sum(x * x, axis=1), "sample": sample}


def _laplace(d):
    return {"ndim": d, "truth": d * math.log(2.0), "lower": None, "upper": None,
            "lnprob": lambda x: -np.sum(np.abs(x), axis=1), "sample": lambda rng, n: rng.laplace(size=(n, d))}


CLOSED = {"gauss3": _gauss(3), "gauss6": _gauss(6), "truncated3": _truncated(3, -1.0, 1.5), "laplace3": _laplace(3)}
CLOSED_N, CLOSED_SEEDS = 4096, (1, 2, 3, 4, 5)


def closed_run(name, seed, libm=br.NUMPY, **kw):
    """The restated estimate of closed case `name`: N1 = N2 = n_fit = CLOSED_N iid samples from numpy's generator `seed`, the
    draws from the same seed.  Returns br.logz's dict; its "out"[0][LAMBDA] estimates the case's truth."""
    c = CLOSED[name]
    rng = np.random.default_rng(seed)
    fit, est = c["sample"](rng, CLOSED_N), c["sample"](rng, CLOSED_N)
    args = dict(lower=c["lower"], upper=c["upper"], n_draws=CLOSED_N, seed=seed, lnprob=c["lnprob"], libm=libm)
    args.update(kw)
    return br.logz(fit, est, c["lnprob"](est), **args)


# ---------------------------------------------------------------- the fixed point alone
def _ab(seed, n1, n2, shift=0.0):
    """log-ratios of an overlapping pair: the posterior the unit Gaussian in 2-D, the proposal a Gaussian 1.2 times as wide"""
    rng = np.random.default_rng(seed)
    s = 1.2
    ln_q = lambda x: -0.5 * np.sum(x * x, axis=1) / (s * s) - 2.0 * math.log(s) - math.log(2.0 * math.pi)
    ln_p = lambda x: -0.5 * np.sum(x * x, axis=1) + shift
    xp, xq = rng.standard_normal((n1, 2)), s * rng.standard_normal((n2, 2))
    return ln_p(xp) - ln_q(xp), ln_p(xq) - ln_q(xq)


def _fixed(a, b, neff=None, max_iter=200, tol=1.0e-10, expect=br.OK, box=None):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.atleast_2d(np.ascontiguousarray(b, dtype=np.float64))
    return {"a": a, "b": b, "neff": float(a.size if neff is None else neff), "max_iter": max_iter, "tol": tol, "expect": expect,
            "lower": None if box is None else box[0], "upper": None if box is None else box[1]}


def _one_finite():
    a, b = _ab(11, 300, 300)
    b[:] = -np.inf
    b[137] = 0.25
    return _fixed(a, b)


def _two_reps():
    a, b0 = _ab(12, 500, 700)
    _, b1 = _ab(13, 500, 700)
    b1[::3] = -np.inf
    return _fixed(a, np.stack([b0, b1]), neff=125.0, box=(np.array([-1.0, 0.0]), np.array([2.0, 4.0])))


FIXED = {
    "no_overlap": _fixed(_ab(10, 300, 300)[0], np.full(300, -np.inf), expect=br.NO_OVERLAP),
    "one_finite": _one_finite(),
    "iter_limit": _fixed(*_ab(14, 300, 300), max_iter=1, tol=0.0, expect=br.ITER_LIMIT),
    "offset_minus_1e9": _fixed(*_ab(15, 300, 300, shift=-1.0e9), tol=1.0e-6),      # (tol above the ulp of lambda)
    "offset_plus_1e6": _fixed(*_ab(15, 300, 300, shift=1.0e6), tol=1.0e-9),
    "a_all_equal": _fixed(np.full(300, 0.75), _ab(16, 300, 300)[1]),
    "neff_1": _fixed(*_ab(17, 300, 300), neff=1.0),
    "neff_n1": _fixed(*_ab(17, 300, 300), neff=300.0),
    "two_repetitions_and_a_box": _two_reps(),
}
FIXED.update({f"n1_{n}_n2_{m}": _fixed(*_ab(100 + k, n, m), tol=1.0e-8)
              for k, (n, m) in enumerate(list(zip(SIZES, SIZES[::-1])) + [(n, n) for n in SIZES])})


def fixed_expected(case, libm=br.NUMPY):
    """out[n_rep][NOUT] of a FIXED case by the restatement, and the constants the probe takes"""
    a, b = case["a"], case["b"]
    k = br.constants(a.size, b.shape[1], case["neff"], case["lower"], case["upper"])
    return np.array([br.fixed_point(a, row, *k, case["max_iter"], case["tol"], libm) for row in b]), k


# ---------------------------------------------------------------- whole calls on the test targets
def _call(seed, ndim, n_fit, n_est, n_draws, target=1, n_rep=1, box=None, neff=None, scale=None, max_iter=200, tol=1.0e-9, const=None):
    rng = np.random.default_rng(seed)
    sc = np.ones(ndim) if scale is None else np.asarray(scale, dtype=np.float64)
    fit, est = sc * rng.standard_normal((n_fit, ndim)), sc * rng.standard_normal((n_est, ndim))
    if box is not None:                         # (the estimator rows lie in the support)
        est = np.clip(est, box[0] + 1e-3, box[1] - 1e-3)
    if const is not None:
        fit[:, const] = 0.5
    return {"x_fit": fit, "x_est": est, "lnp_est": br.target_lnp(est, target), "target": target, "n_draws": n_draws, "n_rep": n_rep,
            "lower": None if box is None else np.full(ndim, box[0]), "upper": None if box is None else np.full(ndim, box[1]),
            "neff": neff, "seed": 1000 + seed, "max_iter": max_iter, "tol": tol}


CALLS = {f"sizes_{n}": _call(200 + k, 2, max(n, 4), n, n) for k, n in enumerate(SIZES)}
CALLS.update({
    "ndim_1": _call(300, 1, 300, 300, 300),
    "ndim_6": _call(301, 6, 600, 300, 300),
    "ndim_9": _call(302, 9, 900, 300, 300, n_rep=2),
    "terraces": _call(303, 3, 400, 300, 300, target=2),
    "box_cuts_the_draws": _call(304, 2, 400, 300, 300, box=(-0.8, 1.1), neff=75.0, n_rep=3),
    "narrow_and_shifted": _call(305, 3, 500, 257, 511, scale=(1.0e-3, 1.0, 40.0)),
})
ERANGE_CALL = _call(306, 3, 300, 300, 300, const=1)


def call_expected(case, libm=br.NUMPY):
    keys = ("lower", "upper", "n_draws", "n_rep", "seed", "neff", "max_iter", "tol", "target")
    return br.logz(case["x_fit"], case["x_est"], case["lnp_est"], libm=libm, **{k: case[k] for k in keys})
