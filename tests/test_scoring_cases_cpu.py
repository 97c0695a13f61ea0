"""CPU checks of what tests/test_gpu_scoring.py rests on: the restated digest of a light curve (tests/pointwise_restated.py
digest, tile_ptr) against the definition of linear interpolation, the restated routes by which walker_eval scores an observation
(tests/scoring_cases.py) on every named case under many partitions of the grid into kept ranges, and the sensitivity of every
case: a slip of one index must move lnprob by at least 1 000 times the bound the GPU test grants.

Bounds (eps = 2^-52).  The restated model value ((Lb - La) * idt) * dx + La carries the roundings of Lb - La, idt, dx and of two
products, 5 eps / 2 relative to the product, which is at most |Lb - La| <= max(La, Lb) for a positive curve, and the rounding of
the sum, eps / 2 of a value between La and Lb: 3 eps max(La, Lb) against exact rational interpolation, and against scipy's
interp1d, which rounds likewise (its own slope form: another 3 eps max(La, Lb)).

Sensitivity is stated for the three walkers around the truth a case's y was drawn from (scoring_cases.own_walkers; the GPU test
gives every case at least one of them in every launch), on the C oracle's curves of those walkers, against B(1e-11), the widest
bound the GPU test grants (scoring_cases.bound).  The degenerate cases are left out: their lnprob is -inf or holds no bound."""
import bisect
from fractions import Fraction

import numpy as np
import pytest

import pointwise_restated as pr
import scoring_cases as sc

EPS = 2.0 ** -52
CASES = [c.name for c in sc.cases()]


@pytest.fixture(scope="module")
def partitions():
    """[(spl, tiles)]: random cuts and strides, uncut tiles of every stride, ends on multiples of 64, for both tile lengths"""
    out = []
    for spl in (2, 4):
        for seed in range(4):
            out.append((spl, sc.partition(np.random.default_rng(900 + 10 * spl + seed), spl)))
        for s in (1, 2, 4, 8):
            out.append((spl, sc.partition(np.random.default_rng(0), spl, cut=0.0, strides=(s,))))
        out.append((spl, sc.partition_aligned(spl)))
    return out


@pytest.fixture(scope="module")
def curves():
    """the C oracle's Ltot rows of the walkers, in units of 1e50"""
    P, lower, upper = sc.walkers()
    rows = []
    for p in P:
        st, lc = sc.oracle_curve(sc.unlog(p))
        assert st == 0 and np.all(np.isfinite(lc))
        rows.append(lc)
    return np.array(rows)


def test_case_list():
    cs = sc.cases()
    names = {c.name for c in cs}
    assert len(names) == len(cs) and len(sc.short_cases()) >= 20
    for n in sc.SIZES:
        assert sc.case(f"size_{n}").x.size == n
    for g in sc.ONE_G:
        for n in sc.ONE_N:
            assert f"one_g{g}_n{n}" in names
    for k in sc.ONE_HOT:
        assert f"one_hot_{k}" in names
    for name in ("bucket_boundaries", "split_same_interval", "bucket0_70", "first64_mid_bucket", "knots_interior", "knots_above",
                 "knots_below", "knots_ends", "knots_64k", "order_asc", "order_rev", "order_shuf", "ties_3"):
        assert name in names
    for n in (50, 65):
        for kind in ("yerr0", "yerrinf", "ynan", "yerrneg"):
            assert f"deg_{kind}_{n}" in names
    for c in cs:
        assert c.what and c.x.shape == c.y.shape == c.yerr.shape and all(0 <= d < c.x.size for d in c.deciding)


# ---------------------------------------------------------------- a. the digest against the definition
@pytest.mark.parametrize("name", CASES)
def test_digest_brackets_and_reaches_what_the_case_names(name):
    c = sc.case(name)
    t = sc.grid()
    order = np.argsort(c.x, kind="stable")
    g, dx, idt, y, yerr, tptr = sc.digested(c)
    xs = c.x[order]
    n = xs.size
    assert np.all(t[g] <= xs) and np.all(xs <= t[g + 1]) and g.min() >= 0 and g.max() <= sc.N_GRID - 2
    assert np.all((xs < t[g + 1]) | (g == sc.N_GRID - 2))                       # t[g] <= x < t[g + 1] but at the last knot
    assert np.all(np.diff(xs) >= 0.0) and np.all(np.diff(g) >= 0)
    # ties stay in the caller's order
    for j in range(n - 1):
        if xs[j] == xs[j + 1]:
            assert order[j] < order[j + 1]
    assert same_bits(y, c.y[order]) and same_bits(yerr, c.yerr[order])
    # the buckets
    assert tptr.size == sc.N_TILES + 1 and tptr[0] == 0 and tptr[-1] == n and np.all(np.diff(tptr) >= 0)
    assert np.array_equal(np.diff(tptr), np.bincount(g // 64, minlength=sc.N_TILES))
    # what the case names
    r = c.reach
    assert r["n"] == n
    if "g_all" in r:
        assert np.all(g == r["g_all"])
        if r["last_knot"]:
            assert xs[-1] == t[-1] and g[-1] == sc.N_GRID - 2 and dx[-1] == t[-1] - t[-2]
    if "g_list" in r:
        assert np.array_equal(g, r["g_list"]) and np.all(dx > 0.0)
        assert set(g % 64) == {63, 0}
    if r.get("same_63_64"):
        assert g[63] == g[64] and g[62] < g[63] < g[65]
    if "bucket" in r:
        b, lo, hi = r["bucket"]
        assert tptr[b] == lo < 64 < tptr[b + 1] == hi
    if "on_knots" in r:
        assert bool(np.all(dx == 0.0)) == r["on_knots"]                            # mp_capi.cpp append_dataset: kDsOnKnots
        if r["jitter"]:
            d, sign = r["jitter"]
            k = int(np.argmin(np.abs(t - xs[d])))
            assert np.all(np.delete(dx, d) == 0.0)
            if sign > 0:
                assert g[d] == k and 0.0 < dx[d] <= 2.0 * EPS * t[k]
            else:
                assert g[d] == k - 1 and t[k] - t[k - 1] - 2.0 * EPS * t[k] <= dx[d] <= t[k] - t[k - 1]
        if r["ends"]:
            assert xs[0] == t[0] and xs[-1] == t[-1] and np.all(dx[:-1] == 0.0) and dx[-1] == t[-1] - t[-2]
        if name == "knots_64k":
            assert np.all(g % 64 == 0) and {64, 128, 64 * (sc.N_INT // 64)} <= set(g)
    if "ties" in r:
        a, b, c3 = r["ties"]
        assert xs[a] == xs[b] == xs[c3] and len({y[a], y[b], y[c3]}) == 3 and a < 64 <= c3
    if "order_of" in r:
        ref = sc.digested(sc.case(r["order_of"]))
        assert all(same_bits(u, v) for u, v in zip(ref, (g, dx, idt, y, yerr, tptr)))
        assert np.unique(xs).size == n                                             # (no ties: the order cannot show)
    if "hot" in r:
        assert np.all(np.delete(yerr, r["hot"]) == 1.0e200) and 0.0 < yerr[r["hot"]] < 1.0e3
    if "degenerate" in r:
        kind, at = r["degenerate"]
        assert {"yerr0": yerr[at] == 0.0, "yerrinf": yerr[at] == np.inf, "ynan": np.isnan(y[at]), "yerrneg": yerr[at] < 0.0}[kind]
        assert np.all(np.isfinite(np.delete(y, at))) and np.all(np.delete(yerr, at) > 0.0)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _exact(t, L, x):
    """linear interpolation of the doubles (t, L) at the double x in rational arithmetic, the bracket found by bisection"""
    k = min(max(bisect.bisect_right(t, x) - 1, 0), len(t) - 2)
    ta, tb, la, lb, xf = (Fraction(float(v)) for v in (t[k], t[k + 1], L[k], L[k + 1], x))
    return la + (lb - la) * (xf - ta) / (tb - ta), max(float(L[k]), float(L[k + 1]))


def test_restated_model_value_against_exact_interpolation_and_scipy():
    from scipy.interpolate import interp1d
    t = sc.grid()
    rng = np.random.default_rng(31)
    L = np.exp(np.cumsum(0.05 * rng.standard_normal(t.size)))                   # a random positive curve
    tl = t.tolist()
    f = interp1d(t, L, bounds_error=True)
    worst = 0.0
    for name in ("size_321", "bucket_boundaries", "knots_above", "knots_below", "knots_ends", "one_g9999_n65", "one_g0_n65", "one_g31_n64", "ties_3"):
        g, dx, idt, y, yerr, _ = sc.digested(sc.case(name))
        xs = np.sort(sc.case(name).x)
        mod = ((L[g + 1] - L[g]) * idt) * dx + L[g]
        sp = f(xs)
        for j in range(xs.size):
            want, big = _exact(tl, L, xs[j])
            lim = 3.0 * EPS * big
            err = abs(Fraction(float(mod[j])) - want)
            assert err <= lim, (name, j, float(err), lim)
            assert abs(Fraction(float(sp[j])) - want) <= lim, (name, j)
            worst = max(worst, float(err) / lim)
    print(f"restated model value against exact interpolation: worst error / bound {worst:.3f}")
    # outside the grid: refused, as interp1d(bounds_error=True) and mp_set_dataset do
    for bad in (np.nextafter(t[0], 0.0), np.nextafter(t[-1], np.inf), np.nan):
        with pytest.raises(ValueError):
            pr.digest(t, np.array([10.0, bad]))
    for bad in (np.nextafter(t[0], 0.0), np.nextafter(t[-1], np.inf)):
        with pytest.raises(ValueError):
            f(np.array([10.0, bad]))


# ---------------------------------------------------------------- b. the routes
def test_partitions_cover_the_tile_shapes(partitions):
    full, ends_on, ends_off = set(), 0, 0
    for spl, tiles in partitions:
        assert tiles[0][0] == 0 and tiles[-1][1] == sc.N_INT and all(a[1] == b[0] for a, b in zip(tiles, tiles[1:]))
        assert any(hi == sc.PRE_FINE for lo, hi in tiles)                          # (no tile straddles the end of the start)
        for lo, hi in tiles:
            assert lo < hi
            full.add(hi - lo)
            if hi < sc.N_INT:
                ends_on += hi % 64 == 0
                ends_off += hi % 64 != 0
    assert {16, 32} | {64 * a * b for a in (1, 2, 4, 8) for b in (2, 4)} <= full
    assert ends_on > 50 and ends_off > 50
    assert min(full) == 1


@pytest.mark.parametrize("name", CASES)
def test_every_route_scores_every_observation_once(name, partitions):
    c = sc.case(name)
    g, _, _, _, _, tptr = sc.digested(c)
    n = g.size
    most, bound = 0, False
    for spl, tiles in partitions:
        first = sc.route_first64(g, tiles)
        assert np.all(first[:64] == 1) and np.all(first[64:] == 0), (spl, "first 64")
        for W in (1, 4):
            if W == 4 and spl != 4:
                continue                                                           # (a team's tile is 256 steps)
            cnt, m, b = sc.route_long(g, tptr, tiles, W)
            assert np.all(cnt[:64] == 0) and np.all(cnt[64:] == 1), (spl, W, np.nonzero(cnt[64:] != 1)[0][:5] + 64)
            most, bound = max(most, m), bound or b
        assert np.all(sc.route_curve(g, tptr, tiles) == 1), (spl, "curve")
    r = c.reach
    if "chunks" in r:
        assert most == r["chunks"], (most, r["chunks"])
    if r.get("binding"):
        assert bound
    if n <= 64:
        assert most == 0 and not bound
    else:
        assert most >= 1


def test_chunk_counts_one_w_and_w_plus_one(partitions):
    """chunk counts of 1, W = 4 and W + 1 per tile are reached (one_g*_n65, _n300, _n340), and some log-uniform set goes beyond"""
    assert sc.case("one_g5003_n65").reach["chunks"] == 1 and sc.case("one_g5003_n300").reach["chunks"] == 4
    assert sc.case("one_g5003_n340").reach["chunks"] == 5
    g, _, _, _, _, tptr = sc.digested(sc.case("size_1944"))
    assert max(sc.route_long(g, tptr, tiles, 4)[1] for spl, tiles in partitions if spl == 4) > 5


def test_route_mutants_are_seen_by_the_restatement(partitions):
    """j0 without the max scores observations below 64 twice where the first 64 end inside a bucket; g <= g_hi scores an
    observation twice where a tile ends on its interval"""
    for name in ("bucket0_70", "first64_mid_bucket", "split_same_interval", "size_65"):
        g, _, _, _, _, tptr = sc.digested(sc.case(name))
        for spl, tiles in partitions:
            cnt = sc.route_first64(g, tiles) + sc.route_long(g, tptr, tiles, 1, use_max=False)[0]
            assert np.all(cnt[64:] == 1) and np.any(cnt[:64] == 2), (name, spl)
    g, _, _, _, _, tptr = sc.digested(sc.case("one_g5003_n300"))
    tiles = [(0, 32), (32, 5003), (5003, sc.N_INT)]
    cnt = sc.route_long(g, tptr, tiles, 4, closed=True)[0]
    assert np.all(cnt[64:] == 2) and np.all(cnt[:64] == 0)
    assert np.all(sc.route_long(g, tptr, tiles, 4)[0][64:] == 1)


# ---------------------------------------------------------------- c. sensitivity
def _lnp(z, count=None):
    zz = z.astype(np.longdouble) ** 2
    if count is not None:
        zz = zz * count[:, None]
    return -0.5 * np.sum(zz, axis=0)


def _mutants(c, g, dx, idt, tptr):
    """[(label, g', dx', count')] of the digest of a case"""
    n = g.size
    one = np.ones(n, dtype=np.int64)
    out = []
    for d in c.deciding:
        for s in (1, -1):
            if 0 <= g[d] + s <= sc.N_GRID - 2:
                g2 = g.copy()
                g2[d] += s
                out.append((f"g{s:+d} at {d}", g2, dx, one))
    if c.swap is not None and dx[c.swap] != dx[c.swap + 1]:                      # (both on knots: nothing to exchange)
        d = c.swap
        dx2 = dx.copy()
        dx2[d], dx2[d + 1] = dx[d + 1], dx[d]
        out.append((f"dx of {d} and {d + 1} exchanged", g, dx2, one))
    hot = "hot" in c.reach
    for d in sorted(set(c.deciding[:1]) | (set() if hot else {j for j in (63, 64, n - 1) if j < n})):
        k = one.copy()
        k[d] = 0
        out.append((f"{d} dropped", g, dx, k))
    k = one.copy()
    k[c.deciding[0]] = 2
    out.append((f"{c.deciding[0]} twice", g, dx, k))
    if c.reach.get("binding"):
        tiles = sc.partition(np.random.default_rng(0), 4, cut=0.0, strides=(1,))
        k = sc.route_first64(g, tiles) + sc.route_long(g, tptr, tiles, 1, use_max=False)[0]
        assert k.max() == 2
        out.append(("j0 without the max", g, dx, k))
    return out


@pytest.mark.parametrize("name", [n for n in CASES if not n.startswith("deg_")])
def test_a_slip_moves_lnprob_by_a_thousand_bounds(name, curves):
    c = sc.case(name)
    g, dx, idt, y, yerr, tptr = sc.digested(c)
    own = sc.own_walkers(c)
    L = curves[own]
    st = np.zeros(len(own), dtype=np.int32)
    z = pr.cells(L, st, g, dx, idt, y, yerr)
    mod = y[:, None] - z * yerr[:, None]
    B = sc.bound(z, mod, yerr, 1.0e-11)
    base = _lnp(z)
    muts = _mutants(c, g, dx, idt, tptr)
    assert len(muts) >= 3
    worst = np.inf
    for label, g2, dx2, count in muts:
        z2 = pr.cells(L, st, g2, dx2, idt, y, yerr)
        move = np.abs(_lnp(z2, count) - base).astype(np.float64)
        worst = min(worst, float(np.min(move / B)))
        assert np.all(move >= 1000.0 * B), (label, move / B)
    print(f"{name}: the least move of lnprob over {len(muts)} mutants is {worst:.3g} bounds")
