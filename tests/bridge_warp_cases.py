"""Cases of the bridge-sampling evidence with a Student-t proposal and with Warp-III (include/magprop_amd.h mp_bridge_logz_warp),
shared by tests/test_bridge_warp_cpu.py (the restatement alone) and tests/test_gpu_bridge_warp_kernels.py (the device against
the restatement, bit for bit).

CLOSED: densities with a known ln Z and iid samples, so that neff = N1; every one runs under the four VARIANTS.  CALLS: crafted
whole calls on the test targets 1 .. 4.  Everything is generated from fixed numpy seeds; nothing here touches a device."""
import math

import numpy as np

import bridge_restated as br
import bridge_warp_restated as bw
from bridge_cases import CLOSED_N, CLOSED_SEEDS

# (proposal, warp) of the four variants, the t proposal with nu = 5
VARIANTS = {"plain": (bw.NORMAL, False), "warped": (bw.NORMAL, True), "t": (bw.STUDENT, False), "warped_t": (bw.STUDENT, True)}
CLOSED_NU = 5


# ---------------------------------------------------------------- closed forms
def _split_normal(d):
    """sigma = 1 left of 0 and 4 right of it in every coordinate (test target 3): a fifth of the mass lies left"""
    def sample(rng, n):
        right = rng.random((n, d)) < 0.8
        return np.abs(rng.standard_normal((n, d))) * np.where(right, 4.0, -1.0)

    return {"ndim": d, "truth": d * (math.log(2.5) + 0.5 * math.log(2.0 * math.pi)), "lower": None, "upper": None,
            "lnprob": lambda x: bw.target_lnp(x, 3), "sample": sample}


def _t3(d):
    """the product of t_3 densities (test target 4)"""
    return {"ndim": d, "truth": d * math.log(math.sqrt(3.0) * math.pi / 2.0), "lower": None, "upper": None,
            "lnprob": lambda x: bw.target_lnp(x, 4), "sample": lambda rng, n: rng.standard_t(3.0, size=(n, d))}


def _half_normal(d, hi):
    """the unit Gaussian on the box [0, hi]^d, its mode in a corner: the mirror of a row about the mean (0.8 a coordinate) leaves
    the support wherever a coordinate exceeds 1.6, three rows in ten for d = 3"""
    one = math.sqrt(0.5 * math.pi) * math.erf(hi / math.sqrt(2.0))

    def sample(rng, n):
        out = np.empty((0, d))
        while out.shape[0] < n:
            x = np.abs(rng.standard_normal((2 * n, d)))
            out = np.concatenate([out, x[np.all(x <= hi, axis=1)]])
        return out[:n]

    return {"ndim": d, "truth": d * math.log(one), "lower": np.zeros(d), "upper": np.full(d, hi),
            "lnprob": lambda x: -0.5 * np.sum(x * x, axis=1), "sample": sample}


CLOSED = {"split3": _split_normal(3), "split6": _split_normal(6), "t3_3": _t3(3), "t3_6": _t3(6), "half_normal3": _half_normal(3, 5.0)}


def closed_run(name, variant, seed, libm=br.NUMPY, **kw):
    """The restated estimate of closed case `name` under VARIANTS[variant]: N1 = N2 = n_fit = CLOSED_N iid samples from numpy's
    generator `seed` (the same rows for every variant), the draws from the same seed.  Returns bw.logz's dict; its
    "out"[0][LAMBDA] estimates the case's truth."""
    c = CLOSED[name]
    rng = np.random.default_rng(seed)
    fit, est = c["sample"](rng, CLOSED_N), c["sample"](rng, CLOSED_N)
    proposal, warp = VARIANTS[variant]
    args = dict(lower=c["lower"], upper=c["upper"], n_draws=CLOSED_N, seed=seed, lnprob=c["lnprob"], libm=libm, proposal=proposal,
                nu=CLOSED_NU, warp=warp)
    args.update(kw)
    return bw.logz(fit, est, c["lnprob"](est), **args)


# ---------------------------------------------------------------- whole calls on the test targets
def _call(seed, ndim, n_fit, n_est, n_draws, target, proposal=bw.NORMAL, nu=5, warp=True, n_rep=1, box=None, neff=None, max_iter=200,
          tol=1.0e-9, shift=0.0, clip=True):
    rng = np.random.default_rng(seed)
    fit, est = shift + rng.standard_normal((n_fit, ndim)), shift + rng.standard_normal((n_est, ndim))
    if box is not None and clip:                         # (the estimator rows lie in the support)
        est = np.clip(est, box[0] + 1e-3, box[1] - 1e-3)
    return {"x_fit": fit, "x_est": est, "lnp_est": bw.target_lnp(est, target), "target": target, "n_draws": n_draws, "n_rep": n_rep,
            "lower": None if box is None else np.full(ndim, box[0]), "upper": None if box is None else np.full(ndim, box[1]),
            "neff": neff, "seed": 5000 + seed, "max_iter": max_iter, "tol": tol, "proposal": proposal, "nu": nu, "warp": warp}


SIZES = (1, 63, 64, 65, 255, 256, 257)                                       # wavefront and workgroup edges
_KINDS = [(3, bw.STUDENT, 5), (4, bw.STUDENT, 3), (1, bw.NORMAL, 5), (2, bw.STUDENT, 4)]      # (target, proposal, nu) in turn
CALLS = {f"sizes_{n}_{m}": _call(400 + k, 2, max(n, 4), n, m, _KINDS[k % 4][0], _KINDS[k % 4][1], _KINDS[k % 4][2])
         for k, (n, m) in enumerate(zip(SIZES, SIZES[::-1]))}
CALLS.update({
    "block_plus_1": _call(420, 2, 600, br.BLOCK + 1, br.BLOCK + 1, 3, bw.STUDENT, 5),
    "ndim_1_nu_3": _call(421, 1, 300, 257, 255, 4, bw.STUDENT, 3),
    "ndim_6_nu_4": _call(422, 6, 600, 300, 300, 3, bw.STUDENT, 4),
    "ndim_9_nu_32_three_reps": _call(423, 9, 900, 300, 300, 4, bw.STUDENT, 32, n_rep=3),
    "t_5_unwarped_three_reps": _call(424, 3, 400, 300, 300, 4, bw.STUDENT, 5, warp=False, n_rep=3, neff=75.0),
    "warped_normal_split": _call(425, 3, 400, 300, 300, 3),
    "warped_normal_terraces": _call(426, 3, 400, 300, 300, 2, shift=0.3),
    "normal_unwarped_split": _call(427, 2, 400, 300, 300, 3, warp=False),
    # the box [-0.05, 8] on rows about 0: about half the draws lie inside, and then their mirrors outside
    "box_cuts_half_the_mirrors": _call(428, 1, 400, 300, 300, 1, bw.STUDENT, 5, box=(-0.05, 8.0), neff=75.0, n_rep=3),
    # in two dimensions a draw and its mirror both miss the box about half the time: b = -inf
    "draw_and_mirror_both_outside": _call(429, 2, 400, 300, 300, 3, box=(-0.05, 8.0)),
    # a box no draw and no mirror reaches: NO_OVERLAP (the estimator rows are taken as given)
    "no_draw_inside": _call(430, 2, 400, 300, 300, 1, bw.STUDENT, 4, box=(50.0, 60.0), clip=False),
})


def call_expected(case, libm=br.NUMPY):
    keys = ("lower", "upper", "n_draws", "n_rep", "seed", "neff", "max_iter", "tol", "target", "proposal", "nu", "warp")
    return bw.logz(case["x_fit"], case["x_est"], case["lnp_est"], libm=libm, **{k: case[k] for k in keys})
