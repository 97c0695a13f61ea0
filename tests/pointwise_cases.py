"""Named cases of the pointwise-score kernels, shared by tests/test_pointwise_cases_cpu.py (restatement against the long-double
definition) and tests/test_gpu_pointwise_kernels.py (kernels against the restatement).

A case is curves on a grid of about 130 points, statuses and a digested dataset: what the cells kernel reads.  Its cell matrix
(the restatement's) is what the select and reduce kernels read.  Sizes: n_obs of 1, 63, 64, 65 and 130 (a tile is 64 x 64),
sample counts around the workgroup (255 .. 257), the wavefront and the tile (63 .. 65), the tail rule's small values (1, 2, 5,
6, 24 .. 26) and the point where its two branches meet (n / 5 = 3 sqrt(n) = 45 at n = 225: 224 .. 226), 1 000 and 4 096 (16
cells per thread, a tail of 193).  Planted cases put every observation on a knot with y = 0 and yerr = 1, where z = -Ltot at
the knot exactly, so that ties, zeros, overflow and outliers are in the cells bit for bit."""
import collections

import numpy as np

import pointwise_restated as pr

Case = collections.namedtuple("Case", "name t ltot status g dx idt y yerr chunks")

GRID = 131
SAMPLES = (1, 2, 5, 6, 24, 25, 26, 63, 64, 65, 224, 225, 226, 255, 256, 257, 1000, 4096)
N_OBS = (1, 63, 64, 65, 130)


def _grid():
    return np.logspace(0.0, 3.0, GRID)


def _times(t, n_obs, rng):
    """observation times: the first and last grid point, the first and last interval, knots and points between knots"""
    x = [t[0], 0.5 * (t[0] + t[1]), t[-1], 0.25 * t[-2] + 0.75 * t[-1], t[40], t[41], np.sqrt(t[41] * t[42])]
    if n_obs <= len(x):
        return np.sort(np.array(x[:n_obs])) if n_obs > 1 else np.array([np.sqrt(t[41] * t[42])])
    knots = rng.choice(np.arange(2, GRID - 2), size=(n_obs - len(x)) // 2, replace=False)
    free = np.exp(rng.uniform(np.log(t[0]), np.log(t[-1]), n_obs - len(x) - knots.size))
    return np.sort(np.concatenate([x, t[knots], free]))


def _generic(name, n, n_obs, seed, failed=(), chunks=None):
    rng = np.random.default_rng(seed)
    t = _grid()
    amp = np.exp(0.3 * rng.standard_normal((n, 1)))
    ltot = amp * t[None, :] ** -0.8 * (1.0 + 0.05 * rng.standard_normal((n, GRID)))
    x = _times(t, n_obs, rng)
    g, dx, idt = pr.digest(t, x)
    yerr = 0.1 * x ** -0.8 * np.exp(0.2 * rng.standard_normal(n_obs))
    y = x ** -0.8 + yerr * rng.standard_normal(n_obs)
    status = np.zeros(n, dtype=np.int32)
    for r in failed:
        status[r] = 1 + (r % 3)
        ltot[r] = np.nan
    return Case(name, t, ltot, status, g, dx, idt, y, yerr, chunks or ((0, n),))


def _planted(name, zplant, seed, failed=()):
    """every observation on a knot of its own, y = 0, yerr = 1: z[j][s] = zplant[j][s] exactly"""
    zplant = np.asarray(zplant, dtype=np.float64)
    n_obs, n = zplant.shape
    rng = np.random.default_rng(seed)
    t = _grid()
    ltot = np.exp(rng.standard_normal((n, GRID)))
    g = (3 + 2 * np.arange(n_obs)).astype(np.int32)
    ltot[:, g] = -zplant.T
    status = np.zeros(n, dtype=np.int32)
    for r in failed:
        status[r] = 2
        ltot[r] = np.nan
    _, dx, idt = pr.digest(t, t[g])
    assert np.all(dx == 0.0)
    return Case(name, t, ltot, status, g, dx, idt, np.zeros(n_obs), np.ones(n_obs), ((0, n),))


def _build():
    cases = []
    # every sample count, the observation counts taken in turn
    for k, n in enumerate(SAMPLES):
        cases.append(lambda n=n, k=k: _generic(f"s{n}_o{N_OBS[k % 5]}", n, N_OBS[k % 5], 100 + k))
    # every observation count at a size of more than one tile of samples, in two and three chunks
    for k, n_obs in enumerate(N_OBS):
        cases.append(lambda n_obs=n_obs, k=k: _generic(f"o{n_obs}_s130_chunks", 130, n_obs, 200 + k,
                                                       chunks=((0, 64), (64, 66)) if k % 2 else ((0, 1), (1, 100), (101, 29))))
    cases.append(lambda: _generic("failed_between", 257, 65, 300, failed=(0, 5, 63, 64, 65, 128, 255, 256)))
    cases.append(lambda: _generic("failed_leave_one", 65, 3, 301, failed=tuple(range(64))))
    cases.append(lambda: _generic("all_failed", 65, 3, 302, failed=tuple(range(65))))

    def planted():
        rng = np.random.default_rng(400)
        n = 226
        z = np.empty((8, n))
        z[0] = 1.5                                             # a constant column: every cell ties, nothing lies above the cut
        z[1] = rng.choice([1.0, -1.0, 2.0, -2.0, 3.0], n)      # ties straddling the cut (46 values at the cut's level or above)
        z[2] = rng.standard_normal(n)
        z[2, ::7] = 0.0                                        # z = 0
        z[3] = rng.standard_normal(n)
        z[3, [0, 100, 225]] = [1.0e200, -1.0e200, 1.3e154]     # r overflows to inf in two cells and just does not in the third
        z[4] = 0.1 * rng.standard_normal(n)
        z[4, 77] = 40.0                                        # one dominant importance ratio
        z[5] = 10.0 + rng.standard_normal(n)
        z[5, 200] = 1.0e-3                                     # one dominant likelihood
        z[6] = np.repeat(rng.standard_normal(n // 2), 2)       # every value twice
        z[7] = np.where(np.arange(n) < 180, 0.5, 2.5)          # the cut falls inside the lower of two levels
        return _planted("planted_226", z, 401)

    cases.append(planted)

    def planted_failed():
        rng = np.random.default_rng(410)
        z = rng.standard_normal((3, 300))
        z[1] = np.round(z[1] * 2.0) / 2.0
        return _planted("planted_failed_300", z, 411, failed=(1, 2, 3, 64, 299))

    cases.append(planted_failed)
    return cases


_BUILDERS = _build()
_NAMES = None
_CACHE = {}


def names():
    global _NAMES
    if _NAMES is None:
        _NAMES = [b().name for b in _BUILDERS]
    return list(_NAMES)


def case(name):
    """the case and its restated cell matrix (computed once, never modified: read-only arrays)"""
    if name not in _CACHE:
        c = _BUILDERS[names().index(name)]()
        z = pr.cells(c.ltot, c.status, c.g, c.dx, c.idt, c.y, c.yerr)
        for a in (c.t, c.ltot, c.status, c.g, c.dx, c.idt, c.y, c.yerr, z):
            a.setflags(write=False)
        _CACHE[name] = (c, z)
    return _CACHE[name]
