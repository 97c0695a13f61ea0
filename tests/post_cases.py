"""Named cases for the kernels of the posterior monitor (magprop_amd/csrc/mp_post.hip).  numpy only, seeded and deterministic.
A case is one sample sequence (chain and lnprob of every ensemble) with its shape, the monitor's settings and a list of runs:
ways to cut the sequence into chunks, all of which must give the same accumulators.  tests/test_post_cases_cpu.py runs every
case through the restatement (tests/post_restated.py) and checks that it has the property its name claims;
tests/test_gpu_post_kernels.py runs the same list through the kernels (libmp_probe_post.so), so that no case exists on one
side only."""
import zlib
from collections import namedtuple
from functools import lru_cache

import numpy as np

import post_restated as pr

THREADS = 256                                       # kPostThreads (mp_post.h)
MAX_BINS, MAX_BINS2, MAX_NDIM = 4096, 128, 9        # MP_POST_MAX_BINS, MP_POST_MAX_BINS2, MP_MAX_NDIM
SPLIT = [63, 1, 64, 65]                             # the chunk list of the issue: 193 steps
BELOW5 = np.nextafter(5.0, -np.inf)                 # the largest double below 5: (v + 5) * (256 / 10) rounds to 256.0

# chain[n][n_ensembles * n_walkers][ndim], lnp[n][n_ensembles * n_walkers]; runs: {name: chunk lengths summing to n}
Case = namedtuple("Case", "name chain lnp n_walkers n_ensembles ndim bins1 bins2 lower upper runs")


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def runs_of(n, *extra):
    """The whole sequence as one chunk and one step at a time, plus the chunk lists given (each summing to n)."""
    out = {"whole": [n], "ones": [1] * n}
    for k, rows in enumerate(extra):
        assert sum(rows) == n
        out[f"list{k}"] = list(rows)
    return out


def gauss(name, n, n_walkers, n_ensembles, ndim, bins1, bins2, lower=-1.5, upper=2.0, runs=None, edit=None):
    """Standard-normal positions (every ensemble shifted and scaled a little differently, so a swapped ensemble shows) with
    lnprob = -|x|^2 / 2; the range [-1.5, 2) leaves samples below and above.  edit(chain, lnp, rng) changes them in place."""
    rng = _rng(name)
    nt = n_walkers * n_ensembles
    chain = rng.standard_normal((n, nt, ndim))
    for e in range(n_ensembles):
        chain[:, e * n_walkers:(e + 1) * n_walkers] *= 1.0 + 0.125 * e
        chain[:, e * n_walkers:(e + 1) * n_walkers] += 0.0625 * e
    lnp = -0.5 * np.sum(chain * chain, axis=2)
    if edit is not None:
        edit(chain, lnp, rng)
    lo, hi = np.full(ndim, float(lower)), np.full(ndim, float(upper))
    return Case(name, chain, lnp, n_walkers, n_ensembles, ndim, bins1, bins2, lo, hi, runs or runs_of(n))


# ================================================================ the cases
def _one_bin():
    """70 000 samples of one ensemble, every coordinate in one bin: every lane of every wavefront on one counter, and a count
    no 16-bit counter holds."""
    n, nw, ndim = 1000, 70, 2
    rng = _rng("one-bin")
    chain = np.full((n, nw, ndim), 0.3) + 1.0e-4 * rng.random((n, nw, ndim))      # bin 135 of 256 over [-5, 5): [0.2734, 0.3125)
    lnp = -0.5 * np.sum(chain * chain, axis=2)
    return Case("one-bin-70000", chain, lnp, nw, 1, ndim, 256, 64, np.full(2, -5.0), np.full(2, 5.0), {"whole": [n], "by250": [250] * 4})


def _edges():
    """Values exactly lower, exactly upper and the largest double below upper with (-5, 5, 256) in dimension 0; -0.0, 0.0 and
    the smallest subnormal with lower = 0 in dimension 1."""
    d0 = [-5.0, 5.0, BELOW5, np.nextafter(-5.0, -np.inf), np.nextafter(-5.0, np.inf), 0.0, -0.0, 4.99]
    d1 = [-0.0, 0.0, 5e-324, -5e-324, 1.0, np.nextafter(1.0, 0.0), 0.5, 0.25]
    chain = np.empty((4, 2, 2))
    chain[..., 0] = np.array(d0).reshape(4, 2)
    chain[..., 1] = np.array(d1).reshape(4, 2)
    lnp = np.arange(8.0).reshape(4, 2)
    return Case("edges", chain, lnp, 2, 1, 2, 256, 128, np.array([-5.0, 0.0]), np.array([5.0, 1.0]), runs_of(4, [1, 3], [2, 0, 2]))


def _nonfinite_one(chain, lnp, rng):
    chain[3, 1, 2], chain[5, 0, 2], chain[7, 4, 2] = np.nan, np.inf, -np.inf


def _nonfinite_all(chain, lnp, rng):
    chain[3, 1, :], chain[5, 0, :], chain[7, 4, :] = np.nan, np.inf, -np.inf
    chain[9, 2, :] = [np.nan, np.inf, -np.inf]


def _lnp_all_minus_inf(chain, lnp, rng):
    lnp[:] = -np.inf


def _lnp_nan_among_finite(chain, lnp, rng):
    lnp[rng.random(lnp.shape) < 0.3] = np.nan
    lnp[0, 0] = np.nan
    lnp[2, 1] = np.inf                     # +inf is a number like any other: it wins
    lnp[4, 3] = np.inf


def _lnp_tie(chain, lnp, rng):
    """The maximum at two walkers of one step and again two steps later (per ensemble): the first occurrence holds."""
    nw = 34
    for e in range(lnp.shape[1] // nw):
        for t, w in ((70, 20), (70, 5), (72, 1), (150, 0)):
            lnp[t, e * nw + w] = 1.0


def _lnp_max_last(chain, lnp, rng):
    lnp[-1, -1] = 3.0
    lnp[-1, lnp.shape[1] // 3 - 1] = 2.0   # (3 ensembles: the last walker of the first one)


@lru_cache(maxsize=None)
def cases():
    n = sum(SPLIT)
    split = runs_of(n, SPLIT)
    return (
        _one_bin(),
        _edges(),
        gauss("nonfinite-one-coordinate", 12, 6, 1, 3, 16, 8, edit=_nonfinite_one),
        gauss("nonfinite-all-coordinates", 12, 6, 1, 3, 16, 8, edit=_nonfinite_all),
        gauss("bins-1-and-0", 40, 6, 1, 3, 1, 0),
        gauss("bins-7-and-1", 40, 6, 1, 3, 7, 1),
        gauss("bins-4096-and-128-ndim-6", n, 34, 1, 6, 4096, 128, runs=split),
        gauss("ndim-1", 40, 34, 1, 1, 256, 64),
        gauss("ndim-9-bins2-128", 40, 34, 1, 9, 4096, 128, runs=runs_of(40, [17, 23])),
        gauss("walkers-2", n, 2, 1, 3, 256, 64, runs=split),
        gauss("walkers-34-ensembles-3", n, 34, 3, 3, 256, 64, runs=split),
        gauss("walkers-64", n, 64, 1, 3, 256, 64, runs=split),
        gauss("walkers-66-ensembles-3", n, 66, 3, 6, 256, 64, runs=split),
        gauss("one-row", 1, 34, 3, 3, 256, 64, runs={"whole": [1]}),
        gauss("lnprob-all-minus-inf", 20, 6, 3, 3, 16, 8, edit=_lnp_all_minus_inf),
        gauss("lnprob-nan-among-finite", 20, 6, 3, 3, 16, 8, edit=_lnp_nan_among_finite),
        gauss("lnprob-tie", n, 34, 3, 3, 16, 8, runs=split, edit=_lnp_tie),
        gauss("lnprob-max-in-last-row", n, 34, 3, 3, 16, 8, runs=split, edit=_lnp_max_last),
    )


def by_name(name):
    return next(c for c in cases() if c.name == name)


def ensemble(c, e):
    """(chain[n][n_walkers][ndim], lnp[n][n_walkers]) of ensemble e."""
    s = slice(e * c.n_walkers, (e + 1) * c.n_walkers)
    return c.chain[:, s], c.lnp[:, s]


@lru_cache(maxsize=None)
def expected(name):
    """The restatement's accumulators of every ensemble of the case, computed once."""
    c = by_name(name)
    return tuple(pr.accumulate(*ensemble(c, e), c.bins1, c.bins2, c.lower, c.upper) for e in range(c.n_ensembles))


def device_layout(c):
    """The restatement's accumulators of the case as the device holds them (magprop_amd/csrc/mp_post.h): hist1[ne][ndim][bins1 +
    3], hist2[ne][npairs][bins2^2], outside2[ne][npairs], mom[n_entries][n_total], nfin[n_total], best_x[ne][ndim], best_lnp[ne],
    best_idx[ne]; hist2 and outside2 None where there is no 2-D histogram."""
    ex = expected(c.name)
    out = {"hist1": np.stack([np.concatenate([x["hist1"], x["below"][:, None], x["above"][:, None], x["nonfinite"][:, None]], axis=1) for x in ex]),
           "mom": np.concatenate([x["mom"] for x in ex], axis=1), "nfin": np.concatenate([x["nfin"] for x in ex]),
           "best_x": np.stack([x["best_x"] for x in ex]), "best_lnp": np.array([x["best_lnp"] for x in ex]),
           "best_idx": np.array([x["best_idx"] for x in ex], dtype=np.int64), "hist2": None, "outside2": None}
    if c.bins2 and c.ndim > 1:
        out["hist2"] = np.stack([x["hist2"].reshape(len(x["hist2"]), -1) for x in ex])
        out["outside2"] = np.stack([x["outside2"] for x in ex])
    return out
