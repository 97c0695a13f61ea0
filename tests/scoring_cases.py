"""Named light curves that place observations where the index arithmetic of observation scoring can slip, shared by
tests/test_scoring_cases_cpu.py (the digest and the routes restated, sensitivity of every case) and tests/test_gpu_scoring.py
(every kernel build against exact interpolation of the device's own curve), and a pure-Python restatement of which observation
each route of walker_eval (magprop_amd/csrc/mp_eval.hpp) scores in a tile that keeps the grid intervals [g_lo, g_hi).

The grid is the synthetic one: 10 001 knots, 64-interval buckets (tile_ptr), the first 32 intervals sub-stepped.  A case is
(x, y, yerr) in the caller's order with y0 = interp(x) of a canonical model curve (the C oracle's, in units of 1e50 erg/s),
yerr = 0.2 y0 and y = y0 + yerr * nu, nu standard normal with |nu| held at or above 0.25: every observation contributes about 1
to chi^2 at the truth and never nearly nothing, so that one dropped or doubled observation moves lnprob by about 0.5.

`what` says what a case is for, `reach` names the facts the CPU test asserts of its digest (so that a case cannot drift away
from its purpose), `deciding` the observations (sorted order) whose index the sensitivity mutants move, `swap` the observation
whose dx they exchange with its successor's, `kind` the canonical curve behind y.  Where a case could not clear the sensitivity
condition of the CPU test, its deciding observations or its curve were moved away from a flat stretch, never the condition."""
import collections
import os

import numpy as np

import pointwise_restated as pr

Case = collections.namedtuple("Case", "name x y yerr what reach deciding kind swap")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N_GRID, BUCKET, PRE_FINE = 10001, 64, 32
N_INT = N_GRID - 1
N_TILES = (N_INT + BUCKET - 1) // BUCKET                     # mp_capi.cpp: buckets of 64 intervals
C_ERR = 0.2
MID = 5003                                                   # a mid-grid interval (no multiple of 8: inside a stride-8 step)
ONE_G = (0, 31, 32, 63, 64, MID, N_GRID - 2)
ONE_N = (1, 64, 65, 300)
SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 257, 321, 1944)
ONE_HOT = (0, 63, 64, 65, 127, 128, 129)
TYPES = ("Humped", "Classic", "Sloped", "Stuttering")
CANON = {"Humped": [1.0, 5.0, 1.0e-3, 100.0, 0.1, 1.0], "Classic": [1.0, 5.0, 1.0e-3, 1000.0, 0.1, 1.0],
         "Sloped": [1.0, 1.0, 1.0e-3, 100.0, 10.0, 10.0], "Stuttering": [1.0, 5.0, 1.0e-5, 100.0, 0.1, 100.0]}
TRUTHS = {"Humped": [1.0, 5.0, -3.0, 2.0, -1.0, 0.0], "Classic": [1.0, 5.0, -3.0, 3.0, -1.0, 0.0],
          "Sloped": [1.0, 1.0, -3.0, 2.0, 1.0, 1.0], "Stuttering": [1.0, 5.0, -5.0, 2.0, -1.0, 2.0]}
LOG_MASK = 0b111100

_T = None
_CURVES = {}


def grid():
    global _T
    if _T is None:
        _T = np.logspace(0.0, 6.0, num=N_GRID, base=10.0)
        _T.setflags(write=False)
    return _T


def unlog(p):
    q = np.array(p, dtype=np.float64)
    q[..., 2:] = 10.0 ** q[..., 2:]
    return q


def oracle_curve(phys):
    """(status, Ltot[n_grid] in units of 1e50) of the C oracle for physical parameters"""
    from oracle import c_oracle as co
    st, out = co.model_lc(co.cfg_synth(), np.asarray(phys, dtype=np.float64), grid())
    return st, out[1]


def base_curve(kind):
    if kind not in _CURVES:
        st, lc = oracle_curve(CANON[kind])
        assert st == 0 and np.all(lc > 0.0)
        lc.setflags(write=False)
        _CURVES[kind] = lc
    return _CURVES[kind]


def walkers():
    """(P[24][6] in sampler coordinates, prior_lower, prior_upper): three walkers around each of the four truths (sigma 0.02: their
    tiles run at stride 8), then a dozen prior-wide points of the flag scan that finish (cut tiles and kinks)."""
    rng = np.random.default_rng(4101)
    cloud = np.concatenate([np.array(TRUTHS[k]) + 0.02 * rng.standard_normal((3, 6)) for k in TYPES])
    gs = np.load(os.path.join(GOLDEN, "golden_synth.npz"))
    gf = np.load(os.path.join(GOLDEN, "golden_flagscan.npz"))
    lower, upper = np.array(gs["prior_lower"], dtype=np.float64), np.array(gs["prior_upper"], dtype=np.float64)
    pars, ok = gf["pars"], np.nonzero(gf["status"] == 0)[0]
    inside = [i for i in ok if np.all(pars[i] > lower) and np.all(pars[i] < upper)]
    wide = pars[np.array(inside)[:: max(len(inside) // 12, 1)][:12]]
    assert wide.shape == (12, 6)
    return np.concatenate([cloud, wide]), lower, upper


def own_walkers(c):
    """rows of walkers() around the truth whose curve the case's y was drawn from: where chi^2 is about n, the walkers the
    sensitivity condition is stated for; every launch of the GPU test scores every case with at least one of them"""
    k = TYPES.index(c.kind)
    return np.arange(3 * k, 3 * k + 3)


def partition_aligned(spl):
    """uncut tiles at stride 1 whose ends all fall on multiples of 64 (the start's second tile ends the start; one cut tile realigns)"""
    tiles, pos = [], 0
    while pos < PRE_FINE:
        tiles.append((pos, min(pos + 8 * spl, PRE_FINE)))
        pos = tiles[-1][1]
    tiles.append((pos, 64))
    pos = 64
    while pos < N_INT:
        tiles.append((pos, min(pos + 64 * spl, N_INT)))
        pos = tiles[-1][1]
    return tiles


# ---------------------------------------------------------------- generators
def _inside(g, u):
    """times at the fractions u (0 < u < 1) of interval g"""
    t = grid()
    x = t[g] + np.asarray(u) * (t[g + 1] - t[g])
    assert np.all(x > t[g]) and np.all(x < t[g + 1])
    return x


def _spread(rng, n, lo=0, hi=N_INT):
    """n times log-uniform over the intervals [lo, hi), ascending, none on a knot"""
    t = grid()
    x = np.sort(10.0 ** rng.uniform(np.log10(t[lo]), np.log10(t[hi]), n))
    x = np.clip(x, np.nextafter(t[lo], np.inf), np.nextafter(t[hi], -np.inf))
    return x


def _observe(x, seed, kind):
    """(y, yerr) around the canonical curve `kind`"""
    rng = np.random.default_rng(10_000 + seed)
    y0 = np.interp(x, grid(), base_curve(kind))
    nu = rng.standard_normal(x.size)
    nu = np.where(nu < 0.0, -1.0, 1.0) * np.maximum(np.abs(nu), 0.25)
    yerr = C_ERR * y0
    return y0 + yerr * nu, yerr


def _case(name, x, seed, what, reach=None, deciding=None, kind=None, swap="auto"):
    """deciding: the observations (sorted order) whose interval the sensitivity mutants move by one, by default the middle and
    the last one and, where they exist, 63 and 64; swap: the mutant that exchanges dx of two neighbours takes swap and swap + 1.
    kind: the canonical curve behind y (by the seed: Humped or Classic, whose steps are the most even over the grid)"""
    x = np.asarray(x, dtype=np.float64)
    kind = TYPES[seed % 2] if kind is None else kind
    y, yerr = _observe(x, seed, kind)
    n = x.size
    if deciding is None:
        deciding = tuple(sorted({n // 2, n - 1} | ({63, 64} if n > 64 else set()) | ({63} if n == 64 else set())))
    if swap == "widest":                                      # the neighbours of the later half whose fractions of their intervals differ most
        _, dx, idt = pr.digest(grid(), np.sort(x))
        swap = n // 2 + int(np.argmax(np.abs(np.diff((dx * idt)[n // 2:]))))
    if swap == "auto":
        swap = 63 if n > 64 else (min(n // 2, n - 2) if n >= 2 else None)
    r = {"n": n}
    r.update(reach or {})
    return Case(name, x, y, yerr, what, r, tuple(deciding), kind, swap)


def _with(c, **kw):
    d = c._asdict()
    for k, v in kw.items():
        d[k] = v
    return Case(**d)


def _one_interval(g, n, seed):
    """n observations inside interval g in two clusters, the lower fifth and the upper fifth of the interval, with the gap
    between sorted observations 63 and 64 (up to 64 observations: in the middle): exchanging dx across the gap moves the model
    by half a grid step.  The early intervals are drawn from the Stuttering curve, whose steps there are 7e-3 to 3e-2 (the other
    three: 4e-6 to 4e-5, which 300 observations dilute below the factor 1 000)."""
    rng = np.random.default_rng(seed)
    low = 64 if n > 64 else (n + 1) // 2
    u = np.concatenate([np.sort(rng.uniform(0.05, 0.25, low)), np.sort(rng.uniform(0.75, 0.95, n - low))])
    x = _inside(g, u)
    if g == N_GRID - 2:
        x[-1] = grid()[-1]                                    # x = t[-1]: g clamped into the last interval, dx the whole interval
    chunks = (max(n - 64, 0) + 63) // 64
    return _case(f"one_g{g}_n{n}", x, seed, f"all {n} observations in interval {g}", {"g_all": g, "chunks": chunks, "last_knot": g == N_GRID - 2},
                 deciding=tuple(sorted({0, low - 1, n - 1} | ({low} if n > low else set()))), kind="Stuttering" if g <= 64 else "Classic",
                 swap=low - 1 if n > low else None)


def _build():
    t = grid()
    B = []
    for k, n in enumerate(SIZES):
        # (321: observation 64 falls at g = 2 000, next to the flattest stretch of the Humped and Classic curves, 1 794 .. 1 939;
        # 1 944: neighbours 63 and 64 lie too early for their dx to count among 1 944 terms, the pair in the middle is exchanged)
        B.append(lambda n=n, k=k: _case(f"size_{n}", _spread(np.random.default_rng(500 + k), n), 500 + k, f"{n} observations log-uniform",
                                        kind="Sloped" if n == 321 else None, swap="widest" if n == 1944 else "auto"))
    for a, g in enumerate(ONE_G):
        for b, n in enumerate(ONE_N):
            B.append(lambda g=g, n=n, s=600 + 4 * a + b: _one_interval(g, n, s))
    B.append(lambda: _one_interval(MID, 340, 640))            # 276 observations behind the first 64: W + 1 = 5 chunks in one tile

    def boundaries():
        g = np.array([[64 * k - 1, 64 * k] for k in range(1, N_INT // 64 + 1)]).ravel()
        assert g.size == 312 and g[-1] <= N_GRID - 2
        rng = np.random.default_rng(650)
        x = t[g] + rng.uniform(0.2, 0.8, g.size) * (t[g + 1] - t[g])
        return _case("bucket_boundaries", x, 650, "one observation in each of g = 64k - 1 and 64k", {"g_list": g}, deciding=(63, 64, 65, 310, 311))

    B.append(boundaries)

    def split_same():
        rng = np.random.default_rng(660)
        x = np.concatenate([_spread(rng, 63, 0, MID), _inside(MID, [0.3, 0.7]), _spread(rng, 35, MID + 1, N_INT)])
        return _case("split_same_interval", x, 660, "sorted observations 63 and 64 share an interval", {"same_63_64": True}, deciding=(62, 63, 64, 65))

    def bucket0():
        rng = np.random.default_rng(661)
        x = np.concatenate([_spread(rng, 70, 0, 64), _spread(rng, 60, 64, N_INT)])
        return _case("bucket0_70", x, 661, "bucket 0 holds 70 observations: tptr[0] = 0 < 64 < tptr[1]", {"bucket": (0, 0, 70), "binding": True}, deciding=(0, 63, 64, 69, 70),
                     kind="Stuttering")                       # (the curve with steps to speak of in the first 64 intervals)

    def mid_bucket():
        rng = np.random.default_rng(662)
        x = np.concatenate([_spread(rng, 40, 0, 3200), _spread(rng, 50, 3200, 3264), _spread(rng, 30, 3264, N_INT)])
        return _case("first64_mid_bucket", x, 662, "the first 64 end inside bucket 50: tptr[50] = 40 < 64 < tptr[51] = 90", {"bucket": (50, 40, 90), "binding": True},
                     deciding=(39, 40, 63, 64, 89, 90))

    B += [split_same, bucket0, mid_bucket]

    def knots(name, what, flag, jitter=0, ends=False, mult=False):
        rng = np.random.default_rng(670)
        if mult:
            g = 64 * np.sort(rng.choice(np.arange(1, N_INT // 64 + 1), 50, replace=False))
            g[0], g[1], g[-1] = 64, 128, 64 * (N_INT // 64)
            g = np.unique(g)
        else:
            g = np.sort(rng.choice(np.arange(40, N_GRID - 40), 50, replace=False))
            g[7] = 64 * 31                                    # (one interior knot on a bucket boundary too)
            g = np.unique(g)
        if ends:
            g = np.concatenate([[0], g[1:-1], [N_GRID - 1]])
        x = t[g].copy()
        d = 20
        if jitter:
            x[d] = np.nextafter(x[d], jitter * np.inf)
        return _case(name, x, 670 + abs(jitter) + (jitter < 0), what, {"on_knots": flag, "jitter": (d, jitter) if jitter else None, "ends": ends},
                     deciding=(1, d, x.size - 2))

    B.append(lambda: knots("knots_interior", "every observation on an interior knot: the on-knots flag", True))
    B.append(lambda: knots("knots_above", "one observation at the double just above its knot", False, jitter=1))
    B.append(lambda: knots("knots_below", "one observation at the double just below its knot: the interval before, dx almost all of it", False, jitter=-1))
    B.append(lambda: knots("knots_ends", "on knots with t[0] and t[-1]: the clamp makes dx != 0 at the last knot", False, ends=True))
    B.append(lambda: knots("knots_64k", "on knots at multiples of 64: the bucket boundaries", True, mult=True))

    def order(name, perm):
        c = _case("order", _spread(np.random.default_rng(680), 129), 680, "")
        p = perm(np.random.default_rng(681), 129)
        return Case(name, c.x[p], c.y[p], c.yerr[p], "one 129-point set " + name[6:], {"n": 129, "order_of": "order_asc"}, c.deciding, c.kind, c.swap)

    B.append(lambda: order("order_asc", lambda r, n: np.arange(n)))
    B.append(lambda: order("order_rev", lambda r, n: np.arange(n)[::-1]))
    B.append(lambda: order("order_shuf", lambda r, n: r.permutation(n)))

    def ties():
        x = _spread(np.random.default_rng(690), 80)
        x[63] = x[64] = x[62]                                 # sorted 62, 63, 64: one time three times, across the 64 / 65 split
        return _case("ties_3", x, 690, "one time three times under different y, across observation 63 / 64", {"ties": (62, 63, 64)}, deciding=(61, 62, 63, 64, 65))

    B.append(ties)
    for k in ONE_HOT:
        def one_hot(k=k):
            c = _case(f"one_hot_{k}", _spread(np.random.default_rng(700), 130), 700, f"yerr = 1e200 but at observation {k}: lnprob = -z_k^2 / 2", {"hot": k}, deciding=(k,), swap=min(k, 128))
            yerr = np.full(130, 1.0e200)
            yerr[k] = c.yerr[k]
            return _with(c, yerr=yerr)
        B.append(one_hot)
    for n, at in ((50, 10), (65, 64)):
        for kind in ("yerr0", "yerrinf", "ynan", "yerrneg"):
            def degenerate(n=n, at=at, kind=kind):
                c = _case(f"deg_{kind}_{n}", _spread(np.random.default_rng(710 + n), n), 710 + n, f"{kind} at observation {at} of {n}", {"degenerate": (kind, at)})
                y, yerr = c.y.copy(), c.yerr.copy()
                if kind == "yerr0":
                    yerr[at] = 0.0
                elif kind == "yerrinf":
                    yerr[at] = np.inf
                elif kind == "ynan":
                    y[at] = np.nan
                else:
                    yerr[at] = -yerr[at]
                return _with(c, y=y, yerr=yerr)
            B.append(degenerate)
    return B


_BUILDERS = _build()
_CACHE = None


def cases():
    """every case, in the order the long handle registers them (computed once, read-only arrays)"""
    global _CACHE
    if _CACHE is None:
        _CACHE = [b() for b in _BUILDERS]
        for c in _CACHE:
            for a in (c.x, c.y, c.yerr):
                a.setflags(write=False)
        assert len({c.name for c in _CACHE}) == len(_CACHE)
    return list(_CACHE)


def case(name):
    return next(c for c in cases() if c.name == name)


def short_cases():
    """the cases of at most 64 observations: a handle that holds only these runs the builds without the long path"""
    return [c for c in cases() if c.x.size <= 64]


def digested(c):
    """(g, dx, idt, y, yerr, tptr) of a case as mp_set_dataset keeps it: stable sort by time, restated digest, buckets"""
    order = np.argsort(c.x, kind="stable")
    g, dx, idt = pr.digest(grid(), c.x[order])
    return g, dx, idt, c.y[order], c.yerr[order], pr.tile_ptr(g, N_TILES)


# ---------------------------------------------------------------- the routes, restated
def partition(rng, spl, cut=0.5, strides=(1, 2, 4, 8)):
    """A walker's kept ranges [(g_lo, g_hi), ...] over the grid's intervals as the tile loop can produce them: the sub-stepped
    start in tiles of 64 spl / 8 intervals, then tiles of 64 spl steps over 1, 2, 4 or 8 intervals each, any of them cut after a
    whole number of steps (the start: of intervals) with probability `cut`."""
    tiles, pos = [], 0
    while pos < PRE_FINE:
        n = min(8 * spl, PRE_FINE - pos)
        if rng.random() < cut:
            n = int(rng.integers(1, n + 1))
        tiles.append((pos, pos + n))
        pos += n
    while pos < N_INT:
        s = int(rng.choice(strides))
        if (N_INT - pos) // s == 0:
            s = 1
        n = min(64 * spl, (N_INT - pos) // s)
        if rng.random() < cut:
            n = int(rng.integers(1, n + 1))
        tiles.append((pos, pos + n * s))
        pos += n * s
    return tiles


def window(tptr, lo, hi, use_max=True):
    """(j0, j1, binding) of the tile [lo, hi): the observations 64.. of the buckets it touches"""
    b_lo, b_hi = lo // BUCKET, min((hi + BUCKET - 1) // BUCKET, N_TILES)
    j0, j1 = int(tptr[b_lo]), int(tptr[b_hi])
    binding = j0 < 64 < j1
    return (max(j0, 64) if use_max else j0), j1, binding


def route_first64(g, tiles):
    """times each of the first 64 observations is captured: the lane's grid interval starts inside the kept range"""
    count = np.zeros(g.size, dtype=np.int64)
    head = g[:64]
    for lo, hi in tiles:
        count[:head.size] += (head >= lo) & (head < hi)
    return count


def route_long(g, tptr, tiles, W, use_max=True, closed=False):
    """(count, largest chunk count of a tile, whether max(tptr[b_lo], 64) was binding) of the observations 64..: per tile the
    chunks jb = j0 + 64 wave, step 64 W, of wavefront `wave`, lane by lane, filtered by mine.  use_max / closed: the two mutants
    (j0 without the max; g <= g_hi)."""
    count = np.zeros(g.size, dtype=np.int64)
    lanes = np.arange(64)
    most, bound = 0, False
    if g.size <= 64:
        return count, most, bound
    for lo, hi in tiles:
        j0, j1, binding = window(tptr, lo, hi, use_max)
        bound = bound or binding
        chunks = 0
        for wave in range(W):
            for jb in range(j0 + 64 * wave, j1, 64 * W):
                chunks += 1
                j = jb + lanes
                gg = g[np.minimum(j, j1 - 1)]
                mine = (j < j1) & (gg >= lo) & ((gg <= hi) if closed else (gg < hi))
                np.add.at(count, j[mine], 1)
        most = max(most, chunks)
    return count, most, bound


def route_curve(g, tptr, tiles):
    """the curve kernels' copy: the lane's own observation, then j = j0 + lane, step 64, skipping what lies outside the tile"""
    count = route_first64(g, tiles)
    if g.size > 64:
        for lo, hi in tiles:
            j0, j1, _ = window(tptr, lo, hi)
            for k in range(j0, j1, 64):                       # (trip k of every lane at once: j = j0 + lane + 64 k)
                j = np.arange(k, min(k + 64, j1))
                gg = g[j]
                np.add.at(count, j[(gg >= lo) & (gg < hi)], 1)
    return count


def bound(z, mod, yerr, delta):
    """B(delta) per row: sum delta |z| |mod| / |yerr| + sum 8 eps (|z| |mod| / |yerr| + z^2) over the observations ([n_obs][rows])"""
    eps = 2.0 ** -52
    with np.errstate(all="ignore"):
        a = np.abs(z) * np.abs(mod) / np.abs(yerr)[:, None]
        a = np.where(np.isfinite(a), a, 0.0)
        return np.sum(delta * a + 8.0 * eps * (a + z * z), axis=0)
