"""Named cases for the four kernels of the autocorrelation monitor (magprop_amd/csrc/mp_acf.hip: acf_ingest_kernel,
acf_accumulate_kernel, acf_rho_kernel, acf_final_kernel).  numpy only, seeded and deterministic.  A case is one sample sequence
with its shape, max_lag and window constant, and a list of runs: ways to put that sequence through the monitor (chunking, ring
size and first row, junk rows in front of a chunk, finalisations between chunks), all of which must give the same answer.
tests/test_acf_cases_cpu.py runs every case through the restatement (tests/acf_restated.py), checks that it has the property its
name claims and holds the restatement against the textbook definition in long double; tests/test_gpu_acf_kernels.py runs the same
list through the kernels (libmp_probe_acf.so), so that no case exists on one side only."""
import zlib
from collections import namedtuple
from functools import lru_cache

import numpy as np

import acf_restated as ar

LAG_BLOCK, THREADS = 16, 256                       # kAcfLagBlock, kAcfThreads (mp_acf.h)
ACF_MAX_LAG, MAX_NDIM = 4096, 9                    # MP_ACF_MAX_LAG, MP_MAX_NDIM
ICANARY = -777                                     # window before a call
NAN_CANARY = np.array([0x7FF8C0FFEE15BAD1], dtype=np.uint64).view(np.float64)[0]   # a NaN no arithmetic makes
CHUNK_LENGTHS = (1, 2, 15, 16, 17, 31, 32, 33)
LEADS = (0, 1, 17)
# the kinds whose tau is not a number to compare (tests/test_acf_cases_cpu.py VALUE_EXCLUDED lists the cases by name)
DEGENERATE_KINDS = ("constant", "underflow", "overflow", "nan", "inf")

# x[n][n_ensembles * n_walkers][ndim]: a chain of the sampler.  base / poison: the case this one equals but for one sample, and
# that sample's (t, ensemble, walker, dimension).
Case = namedtuple("Case", "name kind x n_walkers n_ensembles ndim max_lag c runs base poison")
Run = namedtuple("Run", "name ring_rows head0 chunk_rows lead finalise_after c_mid")


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def kp_of(max_lag):
    return (max_lag + LAG_BLOCK - 1) // LAG_BLOCK * LAG_BLOCK


def n_series(c):
    return c.n_walkers * c.n_ensembles * c.ndim


def series(rng, n, nt, ndim, rho, scale=1.0, mean=3.0, start=None):
    """AR(1) series x[n][nt][ndim] of stationary standard deviation `scale` around `mean`; rho, scale, mean: scalars or
    [nt][ndim], one value per series.  start: the first sample's offset from the mean in standard deviations."""
    rho = np.broadcast_to(np.asarray(rho, dtype=np.float64), (nt, ndim))
    z = np.empty((n, nt, ndim))
    z[0] = rng.standard_normal((nt, ndim)) if start is None else start
    s = np.sqrt(1.0 - rho * rho)
    for t in range(1, n):
        z[t] = rho * z[t - 1] + s * rng.standard_normal((nt, ndim))
    return z * scale + mean


def own_rho_and_scale(nt, ndim, top=0.45):
    """One rho (0 to `top`: 0.45 keeps the window of the walker mean below 15 lags) and one scale per series, no two series
    alike: a swapped index changes the result by far more than rounding."""
    j = np.arange(nt * ndim, dtype=np.float64).reshape(nt, ndim)
    rho = np.array([0.0, 0.5, 0.9, 0.98])[(np.arange(nt * ndim) % 4).reshape(nt, ndim)] * (1.0 - 0.001 * (j % 7)) * (top / 0.98)
    return rho, 1.0 + 0.125 * (j % 23)


# ================================================================ runs
def chunkings(n, rng, lengths=CHUNK_LENGTHS, mixtures=3):
    """{name: chunk lengths summing to n}: the whole sequence, one row at a time, every length of `lengths` repeated, and seeded
    mixtures of them, one with empty chunks in between."""
    out = {"whole": [n], "ones": [1] * n}
    for L in lengths:
        if 1 < L < n:
            out[f"by{L}"] = [L] * (n // L) + ([n % L] if n % L else [])
    for i in range(mixtures):
        rows, left = [], n
        while left:
            rows.append(min(int(rng.choice(lengths)), left))
            left -= rows[-1]
            if i == 0 and rng.random() < 0.3:
                rows.append(0)
        out[f"mix{i}"] = ([0] + rows) if i == 0 else rows
    return out


def make_runs(name, n, max_lag, lengths=CHUNK_LENGTHS, mixtures=3, only=None):
    """The runs of one sequence.  ring_rows = kp + the longest chunk, the product's rule at its tightest; head0, the junk rows and
    the finalisations in between rotate over the runs, and the first mixture runs from all three heads."""
    r = _rng("runs-" + name)
    kp = kp_of(max_lag)
    runs = []
    todo = chunkings(n, r, lengths, mixtures)
    for i, (cname, rows) in enumerate(todo.items()):
        if only is not None and cname not in only:
            continue
        ring = kp + max(rows)
        heads = (0, ring - 1, ring // 2)
        for head0 in (heads if cname == "mix0" else (heads[i % 3],)):
            lead = [int(LEADS[(i + k) % 3]) for k in range(len(rows))] if i % 2 else [int(r.choice(LEADS)) for _ in rows]
            fin = [int(i % 3 == 0 and k % 2 == 0) for k in range(len(rows))]
            runs.append(Run(f"{cname}-h{head0}", ring, head0, rows, lead, fin, (5.0, 1.0e-3, 1.0e6)[i % 3]))
    # a chunk that ends exactly on the ring's last row, and one that straddles it (two chunks of L rows, then the rest)
    for L in (16, 17):
        if n > 2 * L and only is None:
            ring = kp + max(L, n - 2 * L)
            rows = [L, L, n - 2 * L]
            runs.append(Run(f"ends-on-last-row-{L}", ring, ring - 2 * L, rows, [0, 1, 17], [0, 1, 0], 5.0))
            runs.append(Run(f"straddles-last-row-{L}", ring, ring - L - L // 2, rows, [17, 0, 1], [1, 0, 0], 5.0))
    return runs


def heads_of(run):
    """The ring row of the first sample of every chunk, and the row behind the last chunk."""
    h = [run.head0]
    for rows in run.chunk_rows:
        h.append((h[-1] + rows) % run.ring_rows)
    return h


def wraps(run):
    """How many times the run passes the ring's last row."""
    return (run.head0 + sum(run.chunk_rows)) // run.ring_rows


# ================================================================ cases
def _cases():
    cases = []

    def add(name, kind, x, nw, ne, max_lag, c=5.0, base=None, poison=None, **kw):
        x = np.ascontiguousarray(x, dtype=np.float64)
        assert x.ndim == 3 and x.shape[1] == nw * ne and nw >= 2 and nw % 2 == 0 and 1 <= x.shape[2] <= MAX_NDIM
        cases.append(Case(name, kind, x, nw, ne, x.shape[2], max_lag, c, make_runs(base or name, len(x), max_lag, **kw), base, poison))     # (a poisoned case runs as its base does)

    few = dict(only=("whole", "ones", "by17", "mix0", "mix1"))
    # ---- geometry: every max_lag, 4 walkers x 2 ensembles x 3 dimensions, every series with its own rho and scale; n is three
    # rings of the longest chunking and more, so every chunked run wraps at least twice
    for K in (1, 2, 15, 16, 17, 31, 32, 33, 100):
        r = _rng(f"lag-{K}")
        rho, scale = own_rho_and_scale(8, 3, top=0.9 if K == 100 else 0.45)
        n = 3 * (kp_of(K) + 33) + 5 if K < 100 else 3 * (kp_of(K) + 17) + 5
        kw = {} if K in (17, 32) else dict(only=("whole", "by16", "by33", "mix0")) if K < 100 else dict(only=("whole", "by17", "mix0"))
        add(f"lag-{K}", "geometry", series(r, n, 8, 3, rho, scale), 4, 2, K, **kw)
    # ---- n_series: the sampler's smallest, and either side of and on one and two workgroups of the accumulate kernels
    for ns, nw, ne, nd in ((2, 2, 1, 1), (254, 2, 127, 1), (256, 32, 1, 8), (258, 86, 1, 3), (510, 34, 3, 5), (512, 64, 1, 8),
                           (514, 2, 257, 1), (72, 4, 2, MAX_NDIM)):
        r = _rng(f"series-{ns}")
        rho, scale = own_rho_and_scale(nw * ne, nd)
        add(f"series-{ns}-w{nw}-e{ne}-d{nd}", "n-series", series(r, 120, nw * ne, nd, rho, scale), nw, ne, 17,
            only=("whole", "by33", "mix0"))
    # ---- n: prefixes of one sequence at max_lag = 17 (kp = 32; the ring of the runs by 17 has 49 rows)
    r = _rng("length")
    rho, scale = own_rho_and_scale(4, 2)
    xs = series(r, 150, 4, 2, rho, scale)
    for n in (2, 15, 16, 17, 18, 32, 33, 48, 50, 147):
        add(f"length-{n}", "length", xs[:n], 4, 1, 17, **few)
    # ---- the CPU test's own cases, shortened: one rho for all series around mean 3; the pivot 30 sigma off
    for i, rho in enumerate((0.0, 0.5, 0.9, 0.98)):
        add(f"ar1-rho{rho}", "ar1", ar.ar1(_rng(f"ar1-{i}"), rho, 300, 8, 2, mean=3.0), 8, 1, 100, **few)
    for rho, off in ((0.9, 30.0), (0.5, -30.0)):
        add(f"ar1-rho{rho}-pivot{off:+.0f}sigma", "pivot", ar.ar1(_rng(f"pivot-{rho}"), rho, 300, 8, 2, mean=3.0, start=np.full((8, 2), off)),
            8, 1, 64, **few)
    # ---- values
    r = _rng("binades")
    rho, _ = own_rho_and_scale(12, 2)
    scale = 2.0 ** r.integers(-20, 21, (12, 2))                  # walkers spread over 40 binades
    add("walker-binades", "binades", series(r, 200, 12, 2, rho, scale, mean=0.0), 6, 2, 32, **few)
    # rho_k of the walkers differs in sign and size: the mean depends on the order of its sum
    add("walker-sum-order", "sum-order", series(_rng("sum-order"), 200, 6, 3, own_rho_and_scale(6, 3)[0]), 6, 1, 33, **few)
    rho, scale = own_rho_and_scale(4, 2)
    base = series(_rng("values"), 120, 4, 2, rho, scale, mean=0.0)
    add("values-base", "plain", base, 4, 1, 17, **few)
    add("mean-1e8", "mean", base + 1.0e8, 4, 1, 17, **few)
    add("scale-1e150", "scale", base * 1.0e150, 4, 1, 17, **few)
    add("scale-1e-150", "scale", base * 1.0e-150, 4, 1, 17, **few)
    add("scale-1e-170-underflows", "underflow", base * 1.0e-170, 4, 1, 17, **few)
    add("scale-1e160-overflows", "overflow", base * 1.0e160, 4, 1, 17, **few)
    add("all-constant", "constant", np.broadcast_to(base[:1], base.shape), 4, 1, 17, **few)
    stuck = base.copy()
    stuck[:, 2] = stuck[0, 2]
    add("one-stuck-walker", "stuck", stuck, 4, 1, 17, **few)
    late = base.copy()
    late[:-1, 1] = late[0, 1]
    late[-1, 1] += 0.75
    add("walker-moves-at-the-last-sample", "late", late, 4, 1, 17, **few)
    # one poisoned sample in a sequence of 2 ensembles x 4 walkers x 3 dimensions
    rho, scale = own_rho_and_scale(8, 3)
    clean = series(_rng("poison"), 120, 8, 3, rho, scale)
    add("poison-base", "plain", clean, 4, 2, 17, **few)
    for kind, v, at in (("nan", np.nan, (40, 1, 2, 1)), ("inf", np.inf, (40, 1, 2, 1)), ("nan", np.nan, (0, 0, 3, 2)), ("nan", np.nan, (119, 1, 0, 0))):
        x = clean.copy()
        t, e, w, d = at
        x[t, e * 4 + w, d] = v
        add(f"one-{kind}-at-t{t}-e{e}-w{w}-d{d}", kind, x, 4, 2, 17, base="poison-base", poison=at, **few)
    # ---- window rule (seeds chosen so that the claim holds in every dimension: tests/test_acf_cases_cpu.py asserts it)
    # n <= max_lag and no window below n - 1 whatever the rounding of the last lag: the answer is the last lag
    for K, n, seed in ((17, 16, WINDOW_SEEDS["last-lag-16"]), (17, 17, WINDOW_SEEDS["last-lag-17"]), (32, 32, WINDOW_SEEDS["last-lag-32"])):
        add(f"last-lag-n{n}-K{K}", "last-lag", series(np.random.default_rng(seed), n, 4, 1, 0.98), 4, 1, K, c=1.0e300, **few)
    # n == max_lag + 1 and none of the max_lag known lags is a window: NaN / -1
    for K, seed in ((17, WINDOW_SEEDS["none-18"]), (32, WINDOW_SEEDS["none-33"])):
        add(f"no-window-n{K + 1}-K{K}", "no-window", series(np.random.default_rng(seed), K + 1, 4, 1, 0.98), 4, 1, K, c=1.0e6, **few)
    # the first window lies in [max_lag, kp): lags the kernels compute and the estimator must not use
    for K, rho, seed in ((17, 0.7, WINDOW_SEEDS["pad-17"]), (33, 0.78, WINDOW_SEEDS["pad-33"])):
        add(f"window-in-the-padding-K{K}", "padding", series(np.random.default_rng(seed), 400, 4, 2, rho), 4, 1, K, **few)
    for c in (1.0e-3, 1.0, 1.0e6):
        add(f"window-constant-{c:g}", "c", series(_rng("c"), 150, 4, 2, 0.5), 4, 1, 100, c=c, **few)
    add("n2-K1", "n2", xs[:2], 4, 1, 1, only=("whole", "ones"))
    add("n2-K5", "n2", xs[:2], 4, 1, 5, only=("whole", "ones"))
    # ---- f[] of acf_final_kernel in LDS is sized by MP_ACF_MAX_LAG: every one of its lags, a handful of series
    add("max-lag-4096", "max-lag", series(_rng("max-lag"), ACF_MAX_LAG + 200, 2, 2, 0.5), 2, 1, ACF_MAX_LAG, lengths=(33, 1000),
        mixtures=1, only=("whole", "by1000", "mix0"))
    return cases


# seeds of the window-rule cases, the first that make the claim hold (tests/test_acf_cases_cpu.py asserts every claim)
WINDOW_SEEDS = {"last-lag-16": 8, "last-lag-17": 1, "last-lag-32": 2, "none-18": 1, "none-33": 2, "pad-17": 2, "pad-33": 2}

CASES = _cases()
BY_NAME = {c.name: c for c in CASES}


# ================================================================ expectations
def ensemble(c, e):
    return c.x[:, e * c.n_walkers:(e + 1) * c.n_walkers]


@lru_cache(maxsize=None)
def _expected(name):
    c = BY_NAME[name]
    n, ns, K, kp, ned = len(c.x), n_series(c), c.max_lag, kp_of(c.max_lag), c.n_ensembles * c.ndim
    lim = min(n, K)
    out = {"S": np.zeros((kp, ns)), "T": np.zeros(ns), "H": np.zeros((kp, ns)), "pivot": np.zeros(ns), "rho": np.zeros((kp, ns)),
           "f": np.full((ned, kp), NAN_CANARY), "tau": np.empty(ned), "window": np.empty(ned, dtype=np.int32)}
    w = c.n_walkers * c.ndim
    with np.errstate(all="ignore"):
        for e in range(c.n_ensembles):
            cols = slice(e * w, (e + 1) * w)
            wide = ar.Monitor(kp).feed(ensemble(c, e))           # every lag the kernels compute
            for key in ("S", "H"):
                out[key][:, cols] = getattr(wide, key).reshape(kp, w)
            out["T"][cols], out["pivot"][cols] = wide.T.ravel(), wide.pivot.ravel()
            rho = wide.finalise(c.c, with_rho=True)[3]
            out["rho"][:len(rho), cols] = rho.reshape(len(rho), w)
            tau, window, f = ar.Monitor(K).feed(ensemble(c, e)).finalise(c.c)      # the estimate: max_lag lags
            out["f"][e * c.ndim:(e + 1) * c.ndim, :lim] = f.T
            out["tau"][e * c.ndim:(e + 1) * c.ndim], out["window"][e * c.ndim:(e + 1) * c.ndim] = tau, window
    for v in out.values():
        v.flags.writeable = False
    return out


def expected(c):
    """What the device holds behind any run of case c, in its raw layouts, by the restatement: S, H, rho [kp][ns] (S and rho
    for all kp lags; H_k zero beyond k = n; rho zero from lag n on), T, pivot [ns], f [n_ensembles * ndim][kp] (the canary from
    lag min(n, max_lag) on), tau and window [n_ensembles * ndim].  Computed once per case and read-only."""
    return _expected(c.name)


def expected_hist(c, run):
    """The ring restated: y of the last min(n, ring_rows) samples at row (head0 + t) mod ring_rows, zeros elsewhere."""
    n, ns = len(c.x), n_series(c)
    x = c.x.reshape(n, ns)
    with np.errstate(all="ignore"):
        y = x - x[0]
    ring = np.zeros((run.ring_rows, ns))
    for t in range(max(0, n - run.ring_rows), n):
        ring[(run.head0 + t) % run.ring_rows] = y[t]
    return ring


def outputs(c, run):
    """The output buffers of one run as the caller hands them over: canaries everywhere."""
    ns, kp, ned = n_series(c), kp_of(c.max_lag), c.n_ensembles * c.ndim
    d = {"S": (kp, ns), "T": (ns,), "H": (kp, ns), "pivot": (ns,), "hist": (run.ring_rows, ns), "rho": (kp, ns), "f": (ned, kp), "tau": (ned,)}
    out = {k: np.full(s, NAN_CANARY) for k, s in d.items()}
    out["window"] = np.full(ned, ICANARY, dtype=np.int32)
    return out


def textbook(x, c, max_lag):
    """(tau, window, taus) of one ensemble x[n][n_walkers][ndim] by the definition, in np.longdouble: the autocovariance about
    the mean of the whole series, rho_k = c_k / c_0 (0 where c_0 = 0), the walker mean, the window rule of the header."""
    x = np.asarray(x, dtype=np.longdouble)
    n = len(x)
    lim = min(n, max_lag)
    d = x - x.sum(axis=0) / np.longdouble(n)
    ck = np.stack([(d[k:] * d[:n - k]).sum(axis=0) for k in range(lim)])
    with np.errstate(invalid="ignore", divide="ignore"):
        rho = np.where(ck[0] != 0, ck / ck[0], np.longdouble(0))
    f = rho.sum(axis=1) / np.longdouble(x.shape[1])
    taus = 2 * np.cumsum(f, axis=0) - 1
    tau, window = np.empty(x.shape[2], dtype=np.longdouble), np.empty(x.shape[2], dtype=np.int32)
    for j in range(x.shape[2]):
        stop = ~(np.arange(lim) < np.longdouble(c) * taus[:, j])
        if np.any(stop):
            window[j] = int(np.argmax(stop))
            tau[j] = taus[window[j], j]
        elif n <= max_lag:
            window[j], tau[j] = lim - 1, taus[lim - 1, j]
        else:
            window[j], tau[j] = -1, np.nan
    return tau, window, taus
