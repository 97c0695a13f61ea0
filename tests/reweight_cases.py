"""The named cases of the importance-reweighting kernels: tests/test_reweight_cases_cpu.py holds the numpy restatement
(tests/reweight_restated.py) to the definition on them, tests/test_gpu_reweight_kernels.py runs the same lists through the
kernels (libmp_probe_reweight.so), so that no case exists on one side only.

A row case is what reweight_rows_kernel reads: Ltot rows on a small grid, statuses, a digested dataset, alternatives and
observation weights.  A column case is a matrix lw[n_alt][n] whose rows are the shapes a column can take."""
from typing import NamedTuple, Optional

import numpy as np

import pointwise_restated as pr
import reweight_restated as rr

GROUP = 8                                  # kReweightGroup of mp_reweight.h (the probe's mpr_group; held by the GPU test)
N_OBS = (1, 63, 64, 65, 129, 340)
ROWS = (1, 3, 4, 5, 9)
N_ALT = (1, GROUP - 1, GROUP, GROUP + 1, 2 * GROUP, 2 * GROUP + 1, 64)
COLUMN_N = (1, 4, 5, 6, 224, 225, 226, 255, 256, 257, 1025)   # (the tail rule's two branches cross at 225)


class RowCase(NamedTuple):
    t: np.ndarray                          # the grid
    ltot: np.ndarray                       # [rows][n_grid]
    status: np.ndarray                     # [rows] int32
    g: np.ndarray                          # the digested dataset, observations ascending in time
    dx: np.ndarray
    idt: np.ndarray
    y: np.ndarray
    yerr: np.ndarray
    kind: np.ndarray                       # [n_alt] int32
    alt: np.ndarray                        # [n_alt][3]
    obs_w: Optional[np.ndarray]            # [n_alt][n_obs] or None
    definition: bool = True                # held to the long-double definition too (not where var underflows)


def alternatives(n_alt, rng):
    """the identity first, then Gaussians and Student-t's in turn with scales, jitters and nu of every size"""
    kind = np.array([rr.GAUSS if k % 2 == 0 else rr.STUDENT for k in range(n_alt)], dtype=np.int32)
    alt = np.empty((n_alt, 3))
    alt[:, 0] = np.exp(rng.uniform(-1.0, 1.0, n_alt))
    alt[:, 1] = np.where(rng.random(n_alt) < 0.5, 0.0, rng.uniform(0.0, 0.5, n_alt))
    alt[:, 2] = np.exp(rng.uniform(np.log(0.5), np.log(200.0), n_alt))
    alt[0] = (1.0, 0.0, 0.0)
    return kind, alt


def _curves(n_rows, t, rng):
    """smooth positive rows around a falling power law, each its own"""
    amp, slope = np.exp(rng.uniform(-1.0, 1.0, (n_rows, 1))), rng.uniform(0.5, 1.5, (n_rows, 1))
    return amp * t[None, :] ** -slope * (1.0 + 0.1 * rng.standard_normal((n_rows, t.size)))


def _dataset(t, x, rng, frac=0.25):
    """(g, dx, idt, y, yerr) of observations at the times x (sorted here) scattered about a power law"""
    x = np.sort(np.asarray(x, dtype=np.float64))
    g, dx, idt = pr.digest(t, x)
    truth = x ** -1.0
    yerr = frac * truth * np.exp(0.3 * rng.standard_normal(x.size))
    return g, dx, idt, truth + yerr * rng.standard_normal(x.size), yerr


def general(n_obs, n_rows, n_alt, seed, weights=None):
    """weights: None, "fractional" (every alternative its own in (0, 2)), "zeros" (a third of them 0), "loo" (alternative k
    leaves observation k % n_obs out)"""
    rng = np.random.default_rng(seed)
    t = np.logspace(0.0, 3.0, 41)
    x = np.clip(np.exp(rng.uniform(np.log(t[0]), np.log(t[-1]), n_obs)), t[0], t[-1])
    kind, alt = alternatives(n_alt, rng)
    obs_w = None
    if weights == "fractional":
        obs_w = rng.uniform(0.05, 2.0, (n_alt, n_obs))
    elif weights == "zeros":
        obs_w = np.where(rng.random((n_alt, n_obs)) < 1.0 / 3.0, 0.0, rng.uniform(0.05, 2.0, (n_alt, n_obs)))
    elif weights == "loo":
        obs_w = np.ones((n_alt, n_obs))
        obs_w[np.arange(n_alt), np.arange(n_alt) % n_obs] = 0.0
    return RowCase(t, _curves(n_rows, t, rng), np.zeros(n_rows, dtype=np.int32), *_dataset(t, x, rng), kind, alt, obs_w)


def _knots():
    """observations on knots, the first and the last among them, and inside the first and the last interval"""
    rng = np.random.default_rng(40)
    t = np.logspace(0.0, 3.0, 41)
    x = np.array([t[0], 0.5 * (t[0] + t[1]), t[1], t[7], t[20], np.nextafter(t[21], 0.0), t[-2], 0.5 * (t[-2] + t[-1]), t[-1]])
    kind, alt = alternatives(GROUP + 1, rng)
    return RowCase(t, _curves(5, t, rng), np.zeros(5, dtype=np.int32), *_dataset(t, x, rng), kind, alt, None)


def _failed_rows():
    """rows that did not finish hold NaN curves and are not read: between, before and behind rows that did"""
    c = general(65, 9, GROUP + 1, 41, "fractional")
    status = np.array([1, 0, 0, 3, 2, 0, 4, 0, 1], dtype=np.int32)
    ltot = c.ltot.copy()
    ltot[status != 0] = np.nan
    return c._replace(ltot=ltot, status=status)


def _mod_zero():
    """a curve that is 0 where it is observed: jm = 0 exactly with a jitter > 0, var = a; and a curve of -0.0"""
    c = general(65, 3, GROUP, 42)
    ltot = c.ltot.copy()
    ltot[0], ltot[1] = 0.0, -0.0
    alt = c.alt.copy()
    alt[1:, 1] = np.linspace(0.05, 0.5, GROUP - 1)
    return c._replace(ltot=ltot, alt=alt)


def _nu_extremes():
    """nu = 0.5 (heavier than Cauchy) and 1e12 (the Gaussian to rounding), with and without jitter"""
    c = general(129, 4, 4, 43)
    kind = np.full(4, rr.STUDENT, dtype=np.int32)
    alt = np.array([[1.0, 0.0, 0.5], [1.0, 0.0, 1.0e12], [1.3, 0.1, 0.5], [0.7, 0.2, 1.0e12]])
    return c._replace(kind=kind, alt=alt)


def _small_q():
    """residuals of a few hundredths of the error (q < 1e-2): where a Student-t of nu = 1e12 is the Gaussian to rounding"""
    c = general(129, 3, 4, 45)
    ltot = c.ltot[:1] * (1.0 + 1.0e-4 * np.arange(3))[:, None]
    mod = rr.model(ltot[:1], c.g, c.dx, c.idt, c.y)[0][0]
    yerr = 0.25 * np.abs(mod)
    y = mod + 0.03 * yerr * np.clip(np.random.default_rng(46).standard_normal(mod.size), -2.0, 2.0)
    kind = np.array([rr.GAUSS, rr.STUDENT, rr.GAUSS, rr.STUDENT], dtype=np.int32)
    alt = np.array([[1.0, 0.0, 0.0], [1.0, 0.0, 1.0e12], [1.3, 0.1, 0.0], [1.3, 0.1, 1.0e12]])
    return c._replace(ltot=ltot, y=y, yerr=yerr, kind=kind, alt=alt)


def _underflow():
    """errors so small that var = (scale ye)^2 is subnormal or 0: q overflows, log(var) is -inf or that of a subnormal"""
    c = general(65, 3, GROUP, 44)
    yerr = c.yerr.copy()
    yerr[::4], yerr[1::4] = 1.0e-160, 1.0e-170
    return c._replace(yerr=yerr, definition=False)


ROW_CASES = {
    "obs1_rows1_alt1": lambda: general(1, 1, 1, 1),
    "obs63_rows3_alt7": lambda: general(63, 3, GROUP - 1, 2),
    "obs64_rows4_alt8": lambda: general(64, 4, GROUP, 3),
    "obs65_rows5_alt9": lambda: general(65, 5, GROUP + 1, 4),
    "obs129_rows9_alt16": lambda: general(129, 9, 2 * GROUP, 5),
    "obs340_rows3_alt17": lambda: general(340, 3, 2 * GROUP + 1, 6),
    "obs65_rows4_alt64": lambda: general(65, 4, 64, 7),
    "fractional_weights": lambda: general(129, 4, GROUP + 1, 8, "fractional"),
    "zero_weights": lambda: general(65, 5, 2 * GROUP, 9, "zeros"),
    "leave_one_out": lambda: general(63, 3, 64, 10, "loo"),
    "knots": _knots,
    "failed_rows": _failed_rows,
    "mod_zero": _mod_zero,
    "nu_extremes": _nu_extremes,
    "small_q": _small_q,
    "underflow": _underflow,
}


def row_names():
    return list(ROW_CASES)


def row_case(name):
    return ROW_CASES[name]()


def column_case(n):
    """lw[8][n]: a random column; one with failed samples; a constant; ties straddling the cut; -inf entries; mixed signs with
    -0.0 and +0.0; all NaN; one used sample"""
    rng = np.random.default_rng(100 + n)
    lw = np.empty((8, n))
    lw[0] = 30.0 * rng.standard_normal(n)
    lw[1] = 5.0 * rng.standard_normal(n)
    lw[1, rng.random(n) < 0.3] = np.nan
    lw[2] = -3.25
    tm = min(pr.tail_len(n), n)
    lw[3] = np.round(rng.standard_normal(n))                 # few distinct values: the cut falls among equals
    lw[3, rng.permutation(n)[:tm // 2]] = 7.0                # ... below copies of the largest that fill half the tail
    lw[4] = 2.0 * rng.standard_normal(n)
    lw[4, rng.random(n) < 0.4] = -np.inf
    lw[4, -1] = -np.inf
    lw[5] = rng.choice(np.array([-1.5, -0.0, 0.0, 2.0 ** -1074, -2.0 ** -1074, 1.5]), n)
    lw[6] = np.nan
    lw[7] = np.nan
    lw[7, n // 2] = -12.5
    return lw
