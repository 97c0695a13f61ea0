"""The read-out of a kept tile on its own -- mp_eval.hpp hermite, hermite_d, hermite5, hermite_mdisc, dense_mdisc_qs, both forms of
image_state, mdot_fb / mdot_fb_d, tables_init -- and the tables mp_create builds and uploads for it (mp_capi.cpp build_tables),
reached through the probe library libmp_probe_dense.so (csrc/mp_probe_dense.hip), which is test infrastructure, no part of the
product's ABI, and reads the tables of a handle the product made: two handles, the synthetic grid and the "S" grid, no dataset.

Tables: against their exact values as functions of the double lnq (tests/golden/golden_dense.npz, mpmath at 400 bits) under the
bounds dense_restated.TABLE_C derives from libm's 1 ulp; the quadrature rows W5, whose cancellation has no simple bound, under twice
the error of their statement-by-statement restatement (math_restated.wtab) against the same exact values.  LDS copies: bit for bit.

Arithmetic: against exact arithmetic on the very doubles the device reads (tests/dense_restated.py: fractions.Fraction, Hermite
forms and Lagrange weights solved from their defining conditions), under the counts of roundings that module's docstring derives
from the operations of the source -- HERMITE_C = 41, HERMITE_D_C = 90, HERMITE5_C = 50 units of U = 2^-53 on
|y0| + |y1| + h (|d0| + |d1|) + h^2 (|e0| + |e1|), FALLBACK_*_C = 25 / 43 / 14 on the value, QS_*_C on the quasi-steady form -- which
allow for fp contraction (it only removes roundings from hermite's plain * and +).  An indexing slip -- a weight of the wrong
variant, a theta of the neighbouring kind, a node off by one, a clamp that bites a used value -- moves a state by 1e-9 and more
relative, five orders above these bounds.  No tolerance is taken from what the device returns; the largest |error| / bound of every
group is printed as a DENSE-MAX line (DESIGN.md section 5 records them).

At th = 0 the issue of hermite_d is fl(fl(h d0) / h), which is d0 itself only where nothing rounds: it is held to that double bit
for bit, and to d0 on steps whose length is a power of two.

tests/test_dense_cases_cpu.py checks the cases, the restatement (against the true solution) and the fixture themselves."""
from fractions import Fraction

import numpy as np
import pytest

import dense_cases as dc
import dense_probe
import dense_restated as dr
import math_restated as mr

pytestmark = pytest.mark.gpu

U = dr.U


@pytest.fixture(scope="module")
def probe():
    p = dense_probe.Probe()
    yield p
    for h in p.handles.values():
        h.close()


@pytest.fixture(scope="module")
def g():
    return np.load(dc.GOLDEN)


@pytest.fixture(scope="module")
def handles(probe):
    return {name: probe.handle(dc.grid(name)[0]) for name in dc.GRIDS}


@pytest.fixture(scope="module")
def tabs(probe, handles):
    """the tables the product built and uploaded, read back once"""
    return {name: probe.tables(handles[name]) for name in dc.GRIDS}


def test_probe_shares_the_restatement_constants_and_refuses_illegal_calls(probe, handles):
    L = probe.L
    assert (L.mpi_kinds(), L.mpi_wtab_size(), L.mpi_wtab_stride(), L.mpi_wtab_theta(), L.mpi_wtab_dense(), L.mpi_ttab_n(), L.mpi_ktab_n()) == \
        (dr.KINDS, dr.WTAB_SIZE, dr.WTAB_STRIDE, dr.WTAB_THETA, dr.WTAB_DENSE, dr.TTAB_N, dr.KTAB_N)
    h = handles["L"]
    tile = dc.tiles("L", 4, 4)[1]                               # 37 kept steps of 64 eighths
    end = tile["pos8"] + 37 * 64
    ok = np.array([tile["pos8"], end], dtype=np.int32)
    for G, over, p8 in ((4, {}, [end + 8]), (4, {}, [tile["pos8"] - 8]), (4, {}, [tile["pos8"] + 4]), (4, dict(keep=257), ok), (4, dict(keep=0), ok),
                        (4, dict(kind=5), ok), (4, dict(kind=-1), ok), (3, {}, ok), (4, dict(t_s=0.0), ok), (4, dict(t_s=np.inf), ok)):
        t = dict(tile, **over)
        if G != 4:
            t["img"] = np.zeros((5, 64 * G + 1))
        rc, out = probe.image_state_rc(h, G, t, p8=np.array(p8, dtype=np.int32))
        assert rc == -1 and np.all(out == dense_probe.CANARY), (G, over, p8)
    t2 = dict(tile, img=tile["img"][:, :129])
    rc, out = probe.image_state_rc(h, 2, dict(t2, keep=129), p8=ok)             # 129 kept steps do not fit the 128-step image
    assert rc == -1 and np.all(out == dense_probe.CANARY)
    k, w, E = np.zeros(dr.KTAB_N), np.zeros(dr.WTAB_SIZE), np.zeros(4 * 257)
    d = lambda a: a.ctypes.data_as(dense_probe._dp)                             # noqa: E731
    for G, NT in ((2, 128), (2, 256), (1, 64), (4, 512), (4, 32)):
        assert L.mpi_lds_tables(h._h, G, NT, d(k), d(w), d(E)) == -1
    assert L.mpi_lds_tables(None, 4, 64, d(k), d(w), d(E)) == -1 and L.mpi_tables(None, d(k), d(w), d(E), d(k)) == -1
    assert L.mpi_hermite(d(E), 0, d(E)) == -1 and L.mpi_hermite(d(E), L.mpi_max_n() + 1, d(E)) == -1
    assert L.mpi_fallback(3, d(k), d(k), d(k), 1, d(E)) == -1 and L.mpi_fallback(4, d(k), d(k), d(E), 0, d(E)) == -1
    assert not np.any(k) and not np.any(w) and not np.any(E)


# ---------------------------------------------------------------- the tables
@pytest.mark.parametrize("name", list(dc.GRIDS))
def test_product_tables_against_the_fixture(g, tabs, name):
    """What mp_create uploaded: lnQ of every kind the exact multiple of 8 lnq8, bit for bit, and lnq the double the fixture's exact
    values are functions of; inv_Q, one_m_invQ, theta_i, the 252 dense weights and the 1 028 Q^k within their bounds
    (dense_restated.TABLE_C) of the correctly rounded values; unused entries 0; the W5 rows within twice the restatement's own error
    against the exact rows (and whether they are the restatement's bit for bit: the node-weight tests of tests/test_gpu_math.py run
    on the restated table)."""
    T = tabs[name]
    tg, lnq = dc.grid(name)
    assert T["t0"] == tg[0] and T["pre_fine"] == 32
    assert 8.0 * T["lnq8"] == lnq == g[f"lnq_{name}"][0]
    assert mr.same_bits(T["sk"][:, 0], np.array([T["lnq8"], 8.0 * T["lnq8"], 16.0 * T["lnq8"], 32.0 * T["lnq8"], 64.0 * T["lnq8"]]))
    for label, ratio, c in dr.table_errors(T, g, name):
        print(f"DENSE-MAX product {name} {label}: {ratio:.3f} of the bound ({c:.3g} U)")
        assert ratio <= 1.0, label
    used = dr.used_wtab_mask()
    assert np.all(T["wtab"][~used] == 0.0) and np.all(T["ttab"][:, 0] == 1.0)
    R = dr.build_tables(lnq)
    ref_err = dr.w5_errors(R, g, name).max(axis=1, keepdims=True)
    err = dr.w5_errors(T, g, name)
    w5 = [kind * dr.WTAB_STRIDE + 6 * k + m for kind in range(dr.KINDS) for k in range(5) for m in range(5)]
    print(f"DENSE-MAX product {name} W5: {(err / (2.0 * ref_err)).max():.3f} of the bound (2 x the restatement's {ref_err.max():.3g}); "
          f"bit-equal to math_restated.wtab: {mr.same_bits(T['wtab'][w5], mr.wtab(lnq)[w5])}; "
          f"whole table bit-equal to dense_restated.build_tables: {all(mr.same_bits(T[k], R[k]) for k in ('sk', 'wtab', 'ttab'))}")
    assert np.all(err <= 2.0 * ref_err)


@pytest.mark.parametrize("G, NT", dc.LDS_INSTANCES)
@pytest.mark.parametrize("name", list(dc.GRIDS))
def test_lds_copies_equal_the_global_tables(probe, handles, tabs, name, G, NT):
    """tables_init<G, NT> in one workgroup of NT threads, the LDS tables poisoned before: g_ktab, every entry of g_wtab and
    tt.E[kind][0 .. 64 G] bit for bit what global memory (and kKtabInit) holds -- no chunk edge left uncopied."""
    ktab, wtab, E = probe.lds_tables(handles[name], G, NT)
    assert mr.same_bits(ktab, dr.KTAB)
    assert mr.same_bits(wtab, tabs[name]["wtab"])
    assert E.shape == (4, 64 * G + 1) and mr.same_bits(E, tabs[name]["ttab"][:, :64 * G + 1])


# ---------------------------------------------------------------- the Hermite forms
def _abc(e):
    th, h, z, y0, d0, e0, y1, d1, e1 = e
    return np.abs(y0) + np.abs(y1), h * (np.abs(d0) + np.abs(d1)), h * h * (np.abs(e0) + np.abs(e1))


def _hermite_ratios(e, out):
    """|device - exact| / bound of hermite, hermite_d, hermite5 for every element"""
    A, B, C = _abc(e)
    r = np.zeros((3, e.shape[1]))
    for q in range(e.shape[1]):
        th, h, z, y0, d0, e0, y1, d1, e1 = (float(v) for v in e[:, q])
        r[0, q] = dr.err(out[0, q], dr.hermite_exact(th, h, (y0, d0), (y1, d1))) / (dr.gamma(dr.HERMITE_C) * (A[q] + B[q]))
        r[1, q] = dr.err(out[1, q], dr.hermite_exact(th, h, (y0, d0), (y1, d1), deriv=True)) / (dr.gamma(dr.HERMITE_D_C) * (A[q] + B[q]) / h)
        r[2, q] = dr.err(out[2, q], dr.hermite_exact(th, h, (y0, d0, e0), (y1, d1, e1))) / (dr.gamma(dr.HERMITE5_C) * (A[q] + B[q] + C[q]))
    return r


def test_hermite_forms(probe, tabs):
    thetas = np.concatenate([T["wtab"][k * 40 + 33: k * 40 + 32 + dr.n_skip(k)] for T in tabs.values() for k in (2, 3, 4)])
    assert thetas.size == 22 and np.all((thetas > 0.0) & (thetas < 1.0))
    cases = dc.hermite_cases(thetas)
    # th = 0: y0 exactly from the three value forms; hermite_d the double fl(fl(h d0) / h), which is d0 where h is a power of two
    for name in ("th0", "th0_pow2"):
        e = cases[name]
        out = probe.hermite(e)
        for f in (0, 2, 3):
            assert mr.same_bits(out[f], e[3]), (name, f)
        assert mr.same_bits(out[1], (e[1] * e[4]) / e[1]), name
        assert np.all(np.abs(out[1] - e[4]) <= 2.0 * dr.gamma(1) * np.abs(e[4]) * 1.0000001)
    assert mr.same_bits(probe.hermite(cases["th0_pow2"])[1], cases["th0_pow2"][4])
    # th = 1: hermite5 is fl(fl(y1 - y0) + y0), hermite within its bound of y1
    e = cases["th1"]
    out = probe.hermite(e)
    A, B, _ = _abc(e)
    assert mr.same_bits(out[2], (e[6] - e[3]) + e[3])
    assert np.all(np.abs(out[0] - e[6]) <= dr.gamma(dr.HERMITE_C) * (A + B))
    # data of polynomials of degree <= 3 / <= 5, exact in doubles, are reproduced
    e, aux = cases["poly"], cases["poly_aux"]
    out = probe.hermite(e)
    A, B, C = _abc(e)
    worst = np.zeros(3)
    for q in range(e.shape[1]):
        deg, t0, c = int(aux[0, q]), Fraction(aux[1, q]), [Fraction(v) for v in aux[2:, q]]
        t = t0 + Fraction(e[0, q]) * Fraction(e[1, q])
        p = sum(ck * t ** k for k, ck in enumerate(c))
        dp = sum(k * ck * t ** (k - 1) for k, ck in enumerate(c) if k)
        b = (dr.gamma(dr.HERMITE_C) * (A[q] + B[q]), dr.gamma(dr.HERMITE_D_C) * (A[q] + B[q]) / e[1, q], dr.gamma(dr.HERMITE5_C) * (A[q] + B[q] + C[q]))
        if deg <= 3:
            worst[0], worst[1] = max(worst[0], dr.err(out[0, q], p) / b[0]), max(worst[1], dr.err(out[1, q], dp) / b[1])
        worst[2] = max(worst[2], dr.err(out[2, q], p) / b[2])
    print(f"DENSE-MAX hermite forms on polynomial data: {worst[0]:.3f} {worst[1]:.3f} {worst[2]:.3f} of the bounds")
    assert np.all(worst <= 1.0), worst
    # random and physically scaled data, every theta of the product's tables among the fractions
    for name in ("random", "physical"):
        e = cases[name]
        assert set(thetas.tolist()) <= set(e[0].tolist())
        out = probe.hermite(e)
        r = _hermite_ratios(e, out)
        print(f"DENSE-MAX hermite forms on {name} data: {r[0].max():.3f} {r[1].max():.3f} {r[2].max():.3f} of the bounds "
              f"({dr.HERMITE_C}, {dr.HERMITE_D_C}, {dr.HERMITE5_C} U)")
        assert np.all(r <= 1.0), (name, r.max(axis=1))
        assert mr.same_bits(out[3], np.where(e[2] < 1.0, out[2], out[0])), name
    # hermite_mdisc switches exactly at z = 1.0: the quintic one ulp below, the cubic at 1.0 and above
    e = cases["switch"]
    out = probe.hermite(e)
    assert np.all(out[0] != out[2])
    assert (e[2] == np.nextafter(1.0, 0.0)).sum() == 8 and (e[2] == 1.0).sum() == 8
    assert mr.same_bits(out[3], np.where(e[2] < 1.0, out[2], out[0]))


# ---------------------------------------------------------------- the fallback rate
@pytest.mark.parametrize("N", [1, 2, 4])
def test_fallback_rate(probe, N):
    """S, dS and iu of mdot_fb<N> / mdot_fb_d<N> against S_amp u^(-5/3), -(5/3) inv_tfb S / u and 1 / u at u = fma(t, inv_tfb, 1), the
    single rounding the source forms: 25, 43 and 14 U (dense_restated's docstring, from rcbrt_fast's 2 ulp).  The N slots of a
    thread hold different values; t = 0 and u = 2e7 are among them."""
    S_amp, inv_tfb, t = dc.fallback_case(N)
    out = probe.fallback(N, S_amp, inv_tfb, t)
    assert not np.any(np.isnan(out)) and not np.any(out == dense_probe.CANARY)
    u = mr.fma(t, inv_tfb[:, None], 1.0)
    assert np.all(out[:, 0] == np.array([S_amp[0], S_amp[0], (-5.0 / 3.0) * inv_tfb[0] * S_amp[0], 1.0])[:, None])   # u = 1: nothing rounds
    worst = np.zeros(4)
    for q in range(S_amp.size):
        for i in range(N):
            S, dS, iu = dr.fallback_exact(S_amp[q], inv_tfb[q], float(u[q, i]))
            for col, ref, cnt in ((0, S, dr.FALLBACK_S_C), (1, S, dr.FALLBACK_S_C), (2, dS, dr.FALLBACK_DS_C), (3, iu, dr.FALLBACK_IU_C)):
                worst[col] = max(worst[col], dr.err(out[col, q, i], ref) / (dr.gamma(cnt) * float(abs(ref))))
    print(f"DENSE-MAX fallback N = {N}: S of mdot_fb {worst[0]:.3f}, of mdot_fb_d {worst[1]:.3f}, dS {worst[2]:.3f}, iu {worst[3]:.3f} of the bounds "
          f"({dr.FALLBACK_S_C}, {dr.FALLBACK_S_C}, {dr.FALLBACK_DS_C}, {dr.FALLBACK_IU_C} U)")
    assert np.all(worst <= 1.0), worst


# ---------------------------------------------------------------- image_state
def _check_tile(probe, h, T, G, tile, res):
    """The device's (Mv, Wv) of a tile in the form of G against the restatement's results; returns them and the worst ratios by branch"""
    Mv, Wv = probe.image_state(h, G, tile)
    assert not np.any(np.isnan(Mv)) and not np.any(np.isnan(Wv)), (tile["name"], G)          # the clamps: no node beyond keep is used
    worst = {}
    for q, r in enumerate(res):
        if r["branch"] == "node":
            assert Mv[q] == tile["img"][2, r["J"]] and Wv[q] == tile["img"][0, r["J"]], (tile["name"], G, q)
            continue
        eM, eW = dr.err(Mv[q], r["Mv"]), dr.err(Wv[q], r["Wv"])
        assert eM <= r["bM"] and eW <= r["bW"], (tile["name"], G, int(tile["p8"][q]), r["branch"], r["J"], r["i"], r["variant"], eM / r["bM"], eW / r["bW"])
        worst[r["branch"]] = max(worst.get(r["branch"], 0.0), eM / r["bM"])
        worst["omega"] = max(worst.get("omega", 0.0), eW / r["bW"])
    return Mv, Wv, worst


def _widen(tile):
    """a tile of the 128-step image in the 256-step image: the same nodes, NaN behind them"""
    img = np.full((5, 257), np.nan)
    img[:, :129] = tile["img"]
    return dict(tile, img=img)


@pytest.mark.parametrize("kind", range(5))
@pytest.mark.parametrize("name", list(dc.GRIDS))
def test_image_state_against_the_restatement(probe, handles, tabs, name, kind):
    """Both forms (G = 2: read as you go; G = 4: batched, with its clamps) on the crafted tiles of dense_cases.tiles, every node beyond
    keep NaN: each (Mv, Wv) within the rounding bound of its branch of the exact-arithmetic restatement on the product's own table
    doubles; node hits exact; no NaN out; the tiles reach dense_cases.required(kind) on these tables; and the two forms on the same
    tile within the sum of their bounds, bit-equal at nodes and for kinds 0 and 1."""
    h, T = handles[name], tabs[name]
    worst = {}
    for G in (2, 4):
        tags = set()
        for tile in dc.tiles(name, kind, G):
            res = dc.restate(T, tile)
            tags |= dc.coverage(kind, G, tile, res)
            Mv, Wv, w = _check_tile(probe, h, T, G, tile, res)
            for k, v in w.items():
                worst[k] = max(worst.get(k, 0.0), v)
            if G == 2:                                   # the same tile through the batched form
                Mb, Wb, _ = _check_tile(probe, h, T, 4, _widen(tile), res)
                for q, r in enumerate(res):
                    if r["branch"] == "node" or kind < 2:
                        assert Mb[q] == Mv[q] and Wb[q] == Wv[q]
                    else:
                        assert abs(Mb[q] - Mv[q]) <= 2.0 * r["bM"] and abs(Wb[q] - Wv[q]) <= 2.0 * r["bW"], (tile["name"], q)
                worst["forms bit-equal"] = min(worst.get("forms bit-equal", 1.0), float(mr.same_bits(Mb, Mv) and mr.same_bits(Wb, Wv)))
        assert dc.required(kind) <= tags, (G, sorted(dc.required(kind) - tags))
    print(f"DENSE-MAX image_state {name} kind {kind}: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())) + " (of the bounds)")


@pytest.mark.parametrize("G", [2, 4])
def test_image_state_on_the_true_solution(probe, handles, tabs, g, G):
    """The fixture's trajectory cases (images of the true solution of the Mdisc equation and of an analytic omega, rounded once):
    the device's read-out at every grid point of the tile within rounding bound + method bound (dense_cases.METHOD_BOUNDS: twice
    what the exact-arithmetic read-out misses the truth by, measured on the CPU) of the true value; at the nodes the image itself."""
    worst = {}
    for tile in dc.golden_tiles(g, G):
        name = tile["name"][0]
        res = dc.restate(tabs[name], tile)
        Mv, Wv = probe.image_state(handles[name], G, tile)
        truth = [[Fraction(float(a)) + Fraction(float(b)) for a, b in zip(*tile[k])] for k in ("truth_M", "truth_W")]
        for q, r in enumerate(res):
            if r["branch"] == "node":
                assert Mv[q] == tile["truth_M"][0][q] and Wv[q] == tile["truth_W"][0][q]
                continue
            for key, got, tv, bound in ((r["branch"], Mv[q], truth[0][q], r["bM"]), ("omega", Wv[q], truth[1][q], r["bW"])):
                lim = bound + dc.METHOD_BOUNDS[(key, tile["kind"])] * float(abs(tv))
                e = dr.err(got, tv)
                assert e <= lim, (tile["name"], q, key, e / lim)
                worst[(key, tile["kind"])] = max(worst.get((key, tile["kind"]), 0.0), e / float(abs(tv)))
    assert set(worst) == set(dc.METHOD_BOUNDS)
    print(f"DENSE-MAX true solution G = {G}: " + ", ".join(f"{k[0]}{k[1]} {v:.2e}" for k, v in sorted(worst.items())) + " (relative)")
