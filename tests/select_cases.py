"""Named cases for the kernels that decide which values a result is built from: band_transpose_kernel / band_select_kernel
(magprop_amd/csrc/mp_band.hip), nest_select_kernel (mp_nest.hip) and opt_reduce_kernel (mp_opt.hip).  numpy only, seeded and
deterministic.  tests/test_select_cases_cpu.py runs every case through the restatements and checks that it has the property its
name claims; tests/test_gpu_select.py runs the same lists through the kernels (libmp_probe_select.so), so that no case exists on
one side only.  The expectations (band_rule, nest_expected, opt_expected) are the restatements of the headers' rules:
mp_band.h's rank and lerp in Python floats, tests/nest_restated.py's select step, tests/de_restated.py's reduce."""
import zlib
from collections import namedtuple

import numpy as np

BAND_MAX_SAMPLES, BAND_MAX_Q = 16384, 16            # MP_BAND_MAX_SAMPLES, MP_BAND_MAX_Q
NEST_MIN_LIVE, NEST_MAX_LIVE = 16, 4096             # MP_NEST_MIN_LIVE, MP_NEST_MAX_LIVE
OPT_MIN_POP, OPT_MAX_POP = 5, 1024                  # mp_optimizer_create
MAX_NDIM = 9                                        # MP_MAX_NDIM
ICANARY = -777                                      # integer outputs before a call (doubles: NaN)

Q7 = np.array([0.0, 0.025, 0.16, 0.5, 0.84, 0.975, 1.0])          # the project's band quantiles (tests/test_gpu_band.py)
Q_BASIC = np.concatenate([Q7, [1.0 - 2.0 ** -53, 2.0 ** -1074, 0.25, 1.0 / 3.0, 0.999]])

_U = np.uint64
_SIGN = _U(1 << 63)


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


# ================================================================ band
def band_key(v):
    """mp_band.h band_key on an array of non-NaN doubles."""
    b = np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)
    return np.where(b >> _U(63) != 0, ~b, b | _SIGN)


def band_value(k):
    """mp_band.h band_value: the inverse of band_key."""
    k = np.ascontiguousarray(k, dtype=np.uint64)
    return np.where(k >> _U(63) != 0, k & ~_SIGN, ~k).view(np.float64)


def band_rank(m, q):
    """mp_band.h band_rank in Python floats: (lo, hi, gamma)."""
    h = float(m - 1) * float(q)
    if h >= float(m - 1):
        return m - 1, m - 1, h - (-1.0)
    lo = int(np.floor(h))
    return lo, lo + 1, h - float(lo)


def band_lerp(a, b, gamma):
    """mp_band.h band_lerp in Python floats, every step rounded."""
    a, b = float(a), float(b)
    d = b - a
    if gamma >= 0.5:
        return b - d * (1.0 - gamma)
    return a + d * gamma


def band_rule(col, q):
    """The quantiles q of one column by mp_band.h's rule: the NaNs dropped, the rest in key order (np.sort's order of the
    values, with -0.0 before +0.0), band_rank, band_lerp.  An all-NaN column gives NaN."""
    col = np.asarray(col, dtype=np.float64)
    v = band_value(np.sort(band_key(col[~np.isnan(col)])))
    if v.size == 0:
        return np.full(len(q), np.nan)
    out = np.empty(len(q))
    for j, qq in enumerate(q):
        lo, hi, gamma = band_rank(v.size, qq)
        out[j] = band_lerp(v[lo], v[hi], gamma)
    return out


def has_both_zeros(col):
    """True for the columns exempt from the sign comparison with np.nanquantile: they hold -0.0 and +0.0, whose order numpy's
    partition does not define (the kernel puts -0.0 first)."""
    z = col[col == 0.0]
    return bool(z.size and np.any(np.signbit(z)) and not np.all(np.signbit(z)))


def _nan_bits(rng, n):
    """n NaNs of either sign with non-default payloads (quiet and signalling patterns)."""
    b = _U(0x7FF0000000000000) | rng.integers(1, 1 << 52, n, dtype=np.uint64)
    b[rng.random(n) < 0.5] |= _SIGN
    return b.view(np.float64)


def _distinct(rng, n):
    while True:
        x = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4)
        if np.unique(x).size == n and (n < 2 or (x.min() < 0.0 < x.max())):
            return x


def _two_valued(n, c, a=-1.25, b=2.5, rng=None):
    """c copies of a and n - c of b, shuffled."""
    x = np.full(n, b)
    x[:c] = a
    return x if rng is None else rng.permutation(x)


def _boundary_counts(n, qs):
    """Counts c of the lower value that put the boundary between the two values below, on and above lo and hi of every q."""
    cs = {0, 1, n - 1, n}
    for q in qs:
        lo = band_rank(n, q)[0]
        cs.update(range(lo - 1, lo + 4))
    return sorted(c for c in cs if 0 <= c <= n)


def _low_byte(rng, n, negative):
    base = _U(0xC00921FB54442D00 if negative else 0x400921FB54442D00)          # +-pi with the lowest byte cleared
    return (base | rng.integers(0, 256, n, dtype=np.uint64)).view(np.float64)


def _top_byte(rng, n):
    """Values whose low 56 bits agree (second byte 0x35: never an infinity or a NaN) and whose sign / exponent byte varies."""
    top = rng.permutation(np.arange(256, dtype=np.uint64))[np.arange(n) % 256]
    return ((top << _U(56)) | _U(0x0035A5A5A5A5A5A5)).view(np.float64)


def _digit_level(rng, n, k):
    """Keys that share the digits above digit k (digit 7 is the most significant byte of the key), take every one of the 256
    values at digit k (n >= 256) and are random below it.  For k = 7 digit 6 is held at 0x55 so that no key maps to an infinity
    or a NaN; for k < 7 the shared digits are those of pi."""
    shift = _U(8 * k)
    digit = rng.permutation(np.concatenate([np.arange(256), rng.integers(0, 256, max(n - 256, 0))]).astype(np.uint64)[:n])
    if k == 7:
        low = _U(0x55) << _U(48) | rng.integers(0, 1 << 48, n, dtype=np.uint64)
        keys = digit << shift | low
    else:
        pi_key = _U(0xC00921FB54442D18)
        above = pi_key >> (shift + _U(8)) << (shift + _U(8))
        low = rng.integers(0, 1 << (8 * k), n, dtype=np.uint64) if k else np.zeros(n, dtype=np.uint64)
        keys = above | digit << shift | low
    return band_value(keys)


def _denormal(rng, n):
    b = rng.integers(1, 1 << 52, n, dtype=np.uint64)
    b[rng.random(n) < 0.5] |= _SIGN
    x = b.view(np.float64).copy()
    x[0] = 5e-324
    x[-1] = -5e-324
    if n > 2:
        x[n // 2] = 5e-324 if n % 2 else -5e-324
    return x


def _with_nans(rng, x, where):
    x = np.array(x, dtype=np.float64)
    where = np.asarray(where, dtype=int)
    x[where] = _nan_bits(rng, where.size)
    return x


BandCase = namedtuple("BandCase", "name kind cols q")       # cols[n_grid][n], q[nq]

BAND_NS = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1025, 7672, 7673, 16384)
BAND_LARGE = BAND_NS[-3:]
BAND_GRIDS = (1, 63, 64, 65, 200)
# Columns left out of the comparison with np.nanquantile, by case name and column index, with the reason.  None: on every generated
# column np.nanquantile (numpy 1.26 / 2.x) equals mp_band.h's rule, infinities and overflow included.
BAND_NOT_NANQUANTILE = {}


def _q_chunks(qs):
    qs = list(qs)
    return [np.array(qs[i:i + BAND_MAX_Q]) for i in range(0, len(qs), BAND_MAX_Q)]


def integer_h_quantiles(m):
    """Every j / (m - 1), j = 0 .. m - 1, for which h = (m - 1) q is the integer j exactly."""
    return [j / (m - 1) for j in range(m) if float(m - 1) * (j / (m - 1)) == float(j)]


def rounding_up_quantiles(m):
    """Quantiles just below j / (m - 1) whose h = (m - 1) q rounds (up) to the integer j."""
    out = []
    for j in range(1, m):
        q = np.nextafter(j / (m - 1), 0.0)
        if q < j / (m - 1) and float(m - 1) * float(q) == float(j):
            out.append(float(q))
    return out


def _band_cases():
    cases = []

    def add(name, kind, cols, q):
        cols = np.ascontiguousarray(np.atleast_2d(cols), dtype=np.float64)
        q = np.ascontiguousarray(q, dtype=np.float64)
        assert 1 <= q.size <= BAND_MAX_Q and 1 <= cols.shape[1] <= BAND_MAX_SAMPLES
        cases.append(BandCase(name, kind, cols, q))

    for n in BAND_NS:
        large = n in BAND_LARGE
        r = _rng(f"band-{n}")
        # ---- all distinct, both signs; the grid counts ride on n = 65 and 257 (more than one workgroup, odd sizes)
        for g in (BAND_GRIDS if n in (65, 257) else (4,) if large else (3,)):
            add(f"band-distinct-n{n}-g{g}", "distinct", [_distinct(r, n) for _ in range(g)], Q_BASIC)
        # ---- ties
        add(f"band-equal-n{n}", "equal", [np.full(n, v) for v in (-3.25, 7.0e-3, 1.0e300)], Q_BASIC)
        if large:
            cs = sorted({band_rank(n, q)[0] + d for q in (0.5, 0.975) for d in (0, 1, 2)} | {1, n - 1})
            add(f"band-two-valued-n{n}", "two-valued", [_two_valued(n, c, rng=r) for c in cs], Q7)
        else:
            cs = _boundary_counts(n, Q7)
            add(f"band-two-valued-n{n}", "two-valued", [_two_valued(n, c, rng=r) for c in cs], Q7)
        # ---- keys that differ in one digit only
        add(f"band-low-byte-n{n}", "low-byte", [_low_byte(r, n, False), _low_byte(r, n, True)], Q_BASIC)
        if n >= 256:
            add(f"band-digit-levels-n{n}", "digit-levels", [_digit_level(r, n, k) for k in range(8)], Q_BASIC)
        # ---- NaNs: 0, 1, n - 1 and n of them; first, last, at the wavefront boundary
        base = _distinct(r, n)
        cols = [base]
        for at in sorted({0, n - 1, min(63, n - 1), min(64, n - 1)}):
            cols.append(_with_nans(r, base, [at]))                                # one NaN
        for keep in sorted({0, n - 1, min(63, n - 1), min(64, n - 1)})[:2 if large else 4]:
            cols.append(_with_nans(r, base, np.delete(np.arange(n), keep)))       # n - 1 NaNs: m = 1
        cols.append(_with_nans(r, base, np.arange(n)))                            # all NaN
        add(f"band-nan-n{n}", "nan", cols[:8] if large else cols, Q_BASIC)
        if large:
            continue
        add(f"band-top-byte-n{n}", "top-byte", [_top_byte(r, n), _top_byte(r, n)], Q_BASIC)
        add(f"band-denormal-n{n}", "denormal", [_denormal(r, n), _denormal(r, n)], Q_BASIC)
        mixed = np.where(r.random(n) < 0.5, 0.0, -0.0)
        if n >= 2:
            mixed[0], mixed[-1] = 0.0, -0.0
        add(f"band-zeros-n{n}", "zeros", [np.full(n, 0.0), np.full(n, -0.0), mixed,
                                          np.where(r.random(n) < 0.3, mixed, r.choice([-1.5, 2.0], n))], Q_BASIC)
        fin = _distinct(r, n)
        inf_mix = np.where(r.random(n) < 0.4, r.choice([np.inf, -np.inf], n), fin)
        if n >= 3:
            inf_mix[:3] = [np.inf, -np.inf, fin[2]]
        add(f"band-inf-n{n}", "inf", [inf_mix, np.full(n, np.inf), np.full(n, -np.inf),
                                      np.where(r.random(n) < 0.5, np.inf, fin), np.where(r.random(n) < 0.5, -np.inf, fin)], Q_BASIC)
        big = np.finfo(np.float64).max
        dmax = r.choice([big, -big], n)
        if n >= 2:
            dmax[0], dmax[-1] = big, -big
        add(f"band-dbl-max-n{n}", "dbl-max", [dmax, np.where(r.random(n) < 0.5, dmax, fin)], Q_BASIC)
    # ---- quantiles whose h is an integer: every j for the small counts (m = n: no NaN in these columns); then quantiles just
    # below j / (m - 1) whose h rounds up to j
    for n in (2, 3, 63, 64, 65):
        r = _rng(f"band-q-{n}")
        cols = [_distinct(r, n), r.integers(-3, 4, n).astype(float) * 0.5]
        for c, q in enumerate(_q_chunks(integer_h_quantiles(n))):
            add(f"band-integer-h-n{n}-{c}", "integer-h", cols, q)
    # (rare: at these counts 1, 1, 1 and 244 of them; the first 16 of the last)
    for n in (7, 63, 255, 7673):
        r = _rng(f"band-q-up-{n}")
        add(f"band-rounds-up-n{n}", "rounds-up", [_distinct(r, n), r.integers(-3, 4, n).astype(float) * 0.5],
            rounding_up_quantiles(n)[:BAND_MAX_Q])
    # m = 1 after the NaNs beside full columns; nq = 1 and nq = MP_BAND_MAX_Q
    r = _rng("band-nq")
    cols = [_distinct(r, 257), _with_nans(r, _distinct(r, 257), np.arange(1, 257)), r.integers(-2, 3, 257).astype(float)]
    add("band-nq1", "nq", cols, [0.5])
    add("band-nq16", "nq", cols, np.concatenate([Q7, r.random(BAND_MAX_Q - 7)]))
    return cases


BAND_CASES = _band_cases()
# (n, n_grid) of the transpose: tiles of 64 x 64, so one short of, on and one past a tile edge in either direction
TRANSPOSE_SHAPES = [(n, g) for n in (1, 63, 64, 65, 257) for g in BAND_GRIDS] + [(7673, 3), (BAND_MAX_SAMPLES, 8), (1, 200), (200, 1)]


def transpose_input(n, n_grid):
    """src[n][n_grid] whose every element codes its own index."""
    return np.arange(n * n_grid, dtype=np.float64).reshape(n, n_grid) + 0.25


# ================================================================ nested select
NestCase = namedtuple("NestCase", "name kind nlive nbatch n_runs ndim mode slot chunk dlogz live lnl lnx lnz stopped nit")


def _nest_lnl(kind, r, n, K):
    base = -50.0 + 10.0 * r.standard_normal(n)
    while np.unique(base).size != n:
        base = -50.0 + 10.0 * r.standard_normal(n)
    if kind == "distinct":
        return base
    if kind == "equal":
        return np.full(n, -3.25)
    if kind == "all-minf":
        return np.full(n, -np.inf)
    if kind in ("minf-below", "minf-equal", "minf-above"):
        b = {"minf-below": K - 1, "minf-equal": K, "minf-above": K + max(1, K // 2)}[kind]
        base[r.permutation(n)[:b]] = -np.inf
        return base
    if kind == "nan":
        idx = r.permutation(n)
        base[idx[:3]] = _nan_bits(r, 3)
        base[idx[3:5]] = -np.inf
        return base
    if kind == "boundary-tie":
        # sorted ranks K - 2 .. K + 1 (clipped) share one value: the slots decide which of them die
        o = np.argsort(base)
        lo, hi = max(K - 2, 0), min(K + 2, n)
        base[o[lo:hi]] = base[o[K - 1]]
        return base
    raise ValueError(kind)


def _nest_cases():
    cases = []

    def add(name, kind, nlive, nbatch, n_runs=1, ndim=3, mode=0, slot=0, chunk=1, dlogz=0.01, lnl_kinds=None, lnx=None, lnz=None,
            stopped=None, nit=None):
        r = _rng(name)
        kinds = lnl_kinds or [kind] * n_runs
        lnl = np.stack([_nest_lnl(k, r, nlive, nbatch) for k in kinds])
        live = r.standard_normal((n_runs, nlive, ndim))
        lnx = np.zeros(n_runs) if lnx is None else np.array(lnx, dtype=np.float64)
        lnz = np.full(n_runs, -np.inf) if lnz is None else np.array(lnz, dtype=np.float64)
        stopped = np.zeros(n_runs, dtype=np.int32) if stopped is None else np.array(stopped, dtype=np.int32)
        nit = np.arange(3, 3 + n_runs, dtype=np.int32) if nit is None else np.array(nit, dtype=np.int32)
        cases.append(NestCase(name, kind, nlive, nbatch, n_runs, ndim, mode, slot, chunk, dlogz, live, lnl, lnx, lnz, stopped, nit))

    # ---- sizes x lnL kinds, first iteration (ln X = 0, ln Z = -inf)
    for n in (16, 17, 1000, 1023, 1024, 1025, 4096):
        for K in (1, 2, n // 2):
            add(f"nest-distinct-n{n}-k{K}", "distinct", n, K)
            add(f"nest-equal-n{n}-k{K}", "equal", n, K)
            add(f"nest-boundary-tie-n{n}-k{K}", "boundary-tie", n, K)
            if K >= 2 and n != 4096:
                for kind in ("minf-below", "minf-equal", "minf-above"):
                    add(f"nest-{kind}-n{n}-k{K}", kind, n, K)
        add(f"nest-nan-n{n}", "nan", n, 4)
        add(f"nest-all-minf-n{n}", "all-minf", n, n // 2)
    add("nest-minf-above-n4096-k2048", "minf-above", 4096, 2048)
    # ---- three runs, every kind side by side; a run in the middle of its life (finite ln Z)
    kinds3 = ["boundary-tie", "minf-above", "nan"]
    for n, K in ((17, 8), (1025, 2)):
        add(f"nest-three-runs-n{n}-k{K}", "three-runs", n, K, n_runs=3, lnl_kinds=kinds3, lnx=[0.0, -3.7, -0.5],
            lnz=[-np.inf, -61.5, -70.25])
    add("nest-mid-run-ndim9", "mid-run", 64, 8, ndim=MAX_NDIM, lnx=[-2.75], lnz=[-49.0], lnl_kinds=["distinct"])
    # ---- a stopped run beside live ones: all of its outputs keep what they held
    add("nest-stopped-beside-live", "stopped-beside", 1000, 2, n_runs=3, lnl_kinds=["equal", "distinct", "minf-equal"],
        stopped=[0, 1, 0], lnx=[0.0, -9.0, -1.0], lnz=[-np.inf, -20.0, -80.0])
    # ---- the stop rule fires: ln Z far above lnL_max + ln X (log1p(exp(-70)) < dlogz): only `stopped` is written
    add("nest-stop-fires", "stop-fires", 1023, 2, n_runs=3, lnl_kinds=["distinct", "distinct", "boundary-tie"],
        lnx=[-30.0, 0.0, -30.0], lnz=[40.0, -np.inf, 40.0])
    # ---- mode 1: the stop check only (no lists, nit unchanged); run 0 stops, the others go on
    add("nest-mode1", "mode1", 1025, 2, n_runs=3, mode=1, lnl_kinds=["distinct", "equal", "all-minf"],
        lnx=[-30.0, -1.0, 0.0], lnz=[40.0, -60.0, -np.inf])
    # ---- a chunk slot behind the first: the dead rows' offset (slot * n_runs + r) * nbatch
    add("nest-slot2-of-4", "slot", 17, 8, n_runs=3, slot=2, chunk=4, lnl_kinds=["distinct", "boundary-tie", "minf-below"])
    add("nest-slot3-of-4-n4096", "slot", 4096, 2048, n_runs=1, slot=3, chunk=4, lnl_kinds=["distinct"])
    return cases


NEST_CASES = _nest_cases()


def nest_outputs(c):
    """The output buffers of case c as the caller hands them over: canaries, and the run state."""
    return {"dead_slot": np.full((c.n_runs, c.nbatch), ICANARY, dtype=np.int32),
            "surv": np.full((c.n_runs, c.nlive - c.nbatch), ICANARY, dtype=np.int32),
            "lstar": np.full(c.n_runs, np.nan),
            "dead_pars": np.full((c.chunk, c.n_runs, c.nbatch, c.ndim), np.nan),
            "dead_lnl": np.full((c.chunk, c.n_runs, c.nbatch), np.nan),
            "dead_n": np.full((c.chunk, c.n_runs, c.nbatch), ICANARY, dtype=np.int32),
            "lnx": c.lnx.copy(), "lnz": c.lnz.copy(), "stopped": c.stopped.copy(), "nit": c.nit.copy()}


def nest_expected(c):
    """What one select launch leaves in nest_outputs(c), by tests/nest_restated.py."""
    import nest_restated as nr
    out = nest_outputs(c)
    for r in range(c.n_runs):
        if c.stopped[r]:
            continue
        if c.mode == 1:
            key = [nr._clean(v) for v in c.lnl[r]]
            if nr.stops(max(key), c.lnx[r], c.lnz[r], c.dlogz):
                out["stopped"][r] = 1
            continue
        sel = nr.select(c.lnl[r], c.lnx[r], c.lnz[r], c.nbatch, c.dlogz)
        if sel is None:
            out["stopped"][r] = 1
            continue
        dead, surv, lstar, dead_lnl, dead_n, lnx, lnz = sel
        out["dead_slot"][r], out["surv"][r], out["lstar"][r] = dead, surv, lstar
        out["dead_pars"][c.slot, r] = c.live[r, dead]
        out["dead_lnl"][c.slot, r], out["dead_n"][c.slot, r] = dead_lnl, dead_n
        out["lnx"][r], out["lnz"][r] = lnx, lnz
        out["nit"][r] += 1
    return out


# ================================================================ optimizer reduce
OptCase = namedtuple("OptCase", "name kind popsize n_pops ndim trial tol atol pop_cur pop_next lnp_cur lnp_next st_cur st_next "
                                "converged nit nfev")


def _opt_lnp(kind, r, n):
    if kind == "distinct":                       # spread wide: never converged
        x = -100.0 * r.random(n)
        while np.unique(x).size != n:
            x = -100.0 * r.random(n)
        return x
    if kind == "best-tie":                       # the largest value at members 2, n // 2 and n - 1
        x = _opt_lnp("distinct", r, n) - 1.0
        x[[2, n // 2, n - 1]] = -0.5
        return x
    if kind == "tight":                          # std(E) / |mean(E)| ~ 1e-9: converged at tol = 1e-6
        return -12.5 * (1.0 + 1.0e-9 * r.standard_normal(n))
    if kind == "tight-minf":                     # the same with one -inf member: not converged
        x = _opt_lnp("tight", r, n)
        x[n // 3] = -np.inf
        return x
    if kind == "equal":
        return np.full(n, -7.75)
    raise ValueError(kind)


def _opt_cases():
    cases = []

    def add(name, kind, popsize, kinds, trial=1, converged=None, ndim=4, tol=1.0e-6, atol=0.0):
        r = _rng(name)
        n_pops = len(kinds)
        lnp_next = np.stack([_opt_lnp(k, r, popsize) for k in kinds])
        shape = (n_pops, popsize)
        converged = np.zeros(n_pops, dtype=np.int32) if converged is None else np.array(converged, dtype=np.int32)
        cases.append(OptCase(name, kind, popsize, n_pops, ndim, trial, tol, atol, r.standard_normal(shape + (ndim,)),
                             r.standard_normal(shape + (ndim,)), -200.0 * r.random(shape), lnp_next,
                             r.integers(0, 4, shape).astype(np.int32), r.integers(4, 8, shape).astype(np.int32), converged,
                             np.arange(10, 10 + n_pops, dtype=np.int32), (1000 + 7 * np.arange(n_pops)).astype(np.int64)))

    for n in (5, 63, 64, 65, 200, 1024):
        for kind in ("distinct", "best-tie", "tight", "tight-minf", "equal"):
            add(f"opt-{kind}-p{n}", kind, n, [kind])
        add(f"opt-equal-gen0-p{n}", "equal-gen0", n, ["equal"], trial=0)
        add(f"opt-three-pops-p{n}", "three-pops", n, ["tight", "equal", "best-tie"], converged=[0, 1, 0], ndim=MAX_NDIM)
    add("opt-three-pops-gen0-p65", "three-pops-gen0", 65, ["tight", "best-tie", "equal"], trial=0)
    add("opt-atol-only-p64", "atol", 64, ["tight"], tol=0.0, atol=1.0e-3)
    add("opt-all-converged-p200", "all-converged", 200, ["tight", "distinct", "best-tie"], converged=[1, 1, 1])
    return cases


OPT_CASES = _opt_cases()


def opt_outputs(c):
    """Every buffer of case c as the caller hands it over (best: a canary)."""
    return {"pop_cur": c.pop_cur.copy(), "pop_next": c.pop_next.copy(), "lnp_cur": c.lnp_cur.copy(), "lnp_next": c.lnp_next.copy(),
            "st_cur": c.st_cur.copy(), "st_next": c.st_next.copy(), "best": np.full(c.n_pops, ICANARY, dtype=np.int32),
            "converged": c.converged.copy(), "nit": c.nit.copy(), "nfev": c.nfev.copy()}


def opt_expected(c):
    """What one reduce launch leaves in opt_outputs(c): tests/de_restated.py's reduce, nfev += popsize, nit += 1 behind a
    generation (trial = 1; generation 0 never converges), and the next buffers copied over the cur buffers of a population that
    has just converged.  A population that came in converged keeps everything."""
    import de_restated as de
    out = opt_outputs(c)
    for p in range(c.n_pops):
        if c.converged[p]:
            continue
        b, conv = de.reduce(c.lnp_next[p], c.tol, c.atol)
        conv = bool(conv and c.trial)
        out["best"][p] = b
        out["nfev"][p] += c.popsize
        out["nit"][p] += 1 if c.trial else 0
        out["converged"][p] = int(conv)
        if conv:
            out["pop_cur"][p], out["lnp_cur"][p], out["st_cur"][p] = c.pop_next[p], c.lnp_next[p], c.st_next[p]
    return out
