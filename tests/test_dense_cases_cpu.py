"""The reference side of tests/test_gpu_dense_kernels.py, without a GPU: the fixture tests/golden/golden_dense.npz regenerates, the
restatement of the tile read-out (tests/dense_restated.py) is held to the true solution on the fixture's trajectory cases -- which
proves its index logic independently of the kernel: a wrong variant, theta or node shows as 1e-4, not 1e-10 -- the crafted tiles
(tests/dense_cases.py) reach every branch, and the probe library stays apart from the product's."""
import importlib.util
import json
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import dense_cases as dc
import dense_restated as dr
import math_restated as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def g():
    return np.load(dc.GOLDEN)


@pytest.fixture(scope="module")
def restated_tables():
    return {name: dr.build_tables(dc.grid(name)[1]) for name in dc.GRIDS}


def _generator():
    spec = importlib.util.spec_from_file_location("make_dense_golden", os.path.join(GOLDEN_DIR, "make_dense_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---------------------------------------------------------------- the fixture
@pytest.mark.parametrize("part", ["tables_L", "tables_S", "L3_quintic", "S4_cross", "S2_qs1"])
def test_fixture_regenerates(g, part):
    pytest.importorskip("mpmath")
    gen = _generator()
    arrays = gen.tables(part[-1]) if part.startswith("tables_") else gen.traj_case(part, check=True)
    assert arrays
    for key, want in arrays.items():
        assert mr.same_bits(g[key].ravel(), np.asarray(want, float).ravel()), key


def test_fixture_is_recorded_small_and_complete(g):
    man = json.load(open(os.path.join(GOLDEN_DIR, "MANIFEST.json")))["golden_dense.npz"]
    gen = _generator()
    assert man["generator"] == "tests/golden/make_dense_golden.py" and man["mpmath"] and man["precision_bits"] == gen.PREC == 400
    assert os.path.getsize(dc.GOLDEN) <= 356030            # golden_holdout.npz: no fixture may be larger
    assert gen.GRIDS == dc.GRIDS and gen.N_GRID == dc.N_GRID
    assert (gen.KINDS, gen.WTAB_STRIDE, gen.WTAB_THETA, gen.TTAB_N) == (dr.KINDS, dr.WTAB_STRIDE, dr.WTAB_THETA, dr.TTAB_N)
    assert {k[5:-5] for k in g.files if k.endswith("_meta")} == set(gen.CASES) and len(gen.CASES) == 42
    for name in dc.GRIDS:
        tg, lnq = dc.grid(name)
        assert g[f"lnq_{name}"][0] == lnq == gen.grid(name)[1]
        assert g[f"theta_{name}_hi"].shape == (40,) and g[f"dense_{name}_hi"].shape == (252,) and g[f"ttab_{name}_hi"].shape == (4 * 257,)
        assert g[f"w5_{name}_hi"].shape == (125,) and g[f"invq_{name}_hi"].shape == (5,) and g[f"omi_{name}_hi"].shape == (5,)
    for tile in dc.golden_tiles(g, 2):
        tg, _ = dc.grid(tile["name"][0])
        assert tile["t_s"] == tg[tile["pos8"] // 8] and 1 <= tile["keep"] <= 16
        assert tile["p8"].size == tile["keep"] * dr.n_skip(tile["kind"]) + 1 == tile["truth_M"][0].size


def test_double_double_pairs_are_valid(g):
    keys = [k[:-3] for k in g.files if k.endswith("_hi")]
    assert len(keys) >= 12 + 3 * 42
    for k in keys:
        hi, lo = g[k + "_hi"], g[k + "_lo"]
        assert np.all(np.isfinite(hi)) and np.all(np.isfinite(lo)) and np.all(np.abs(lo) <= 0.5 * mr.ulp(hi)), k


# ---------------------------------------------------------------- the restated tables and interpolants
@pytest.mark.parametrize("name", list(dc.GRIDS))
def test_restated_tables_against_the_fixture(g, restated_tables, name):
    """The statement-by-statement restatement of build_tables within the bounds the product's tables are held to
    (dense_restated.TABLE_C), its unused entries 0, lnQ the exact multiples of lnq."""
    T = restated_tables[name]
    lnq = dc.grid(name)[1]
    for label, ratio, c in dr.table_errors(T, g, name):
        print(f"DENSE-MAX restated {name} {label}: {ratio:.3f} of the bound ({c:.3g} U)")
        assert ratio <= 1.0, label
    used = dr.used_wtab_mask()
    assert used.sum() == 5 * 25 + (1 + 3 + 7) * 13 and np.all(T["wtab"][~used] == 0.0)
    assert np.all(T["wtab"][used & (np.arange(dr.WTAB_SIZE) % dr.WTAB_STRIDE >= dr.WTAB_THETA)] != 0.0) and np.all(T["wtab"][used][125:] != 0.0)
    assert [T["sk"][k, 0] for k in range(5)] == [lnq / 8.0, lnq, 2.0 * lnq, 4.0 * lnq, 8.0 * lnq]
    assert np.all(T["ttab"][:, 0] == 1.0)
    print(f"DENSE-MAX restated {name} W5 against exact: {dr.w5_errors(T, g, name).max():.3g} of the kind's largest weight")


@pytest.mark.parametrize("name", list(dc.GRIDS))
def test_dense_weights_reproduce_cubics_and_sum_to_one(g, restated_tables, name):
    """The 12 weights of every (kind, skipped point) in the table's layout [variant][node]: against the weights solved from the
    Vandermonde system of the four nodes (exact arithmetic on the table's theta and the double Q), which reproduce every cubic
    and sum to 1 by construction; and the table's own weights do so within their bound."""
    T = restated_tables[name]
    tol = dr.gamma(dr.TABLE_C["dense"])
    for kind in (2, 3, 4):
        Q = math.exp(T["sk"][kind, 0])
        for i in range(1, dr.n_skip(kind)):
            th = T["wtab"][kind * dr.WTAB_STRIDE + dr.WTAB_THETA + i]
            for v in range(3):
                nodes = dr.dense_nodes(Q, v)
                assert nodes[v] == 0 and nodes[v + 1] == 1                        # the step is interval `variant` of its four nodes
                w = dr.lagrange_weights(th, nodes)
                assert sum(w) == 1
                for c in ((1, 0, 0, 0), (0, 1, 0, 0), (2, -3, 5, 0), (-1, 4, 0, 7)):
                    p = lambda x: sum(ck * Fraction(x) ** k for k, ck in enumerate(c))    # noqa: E731
                    assert sum(wk * p(x) for wk, x in zip(w, nodes)) == p(th)
                base = dr.WTAB_DENSE + ((kind - 2) * 7 + (i - 1)) * 12 + v * 4
                tab = [Fraction(float(T["wtab"][base + k])) for k in range(4)]
                for wk, tk in zip(w, tab):
                    assert abs(tk - wk) <= tol * abs(wk), (kind, i, v)
                assert abs(sum(tab) - 1) <= tol * sum(abs(t) for t in tab)


def test_hermite_restatement_reproduces_monomials():
    """The interpolants solved from their end conditions return every monomial up to degree 3 (cubic) / 5 (quintic), and its time
    derivative, exactly, on a step that is not the unit interval."""
    t0, h = Fraction(7, 3), Fraction(5, 4)
    for m, top in ((2, 3), (3, 5)):
        for deg in range(top + 1):
            d = [lambda t, r=r: Fraction(math.perm(deg, r)) * (t ** (deg - r) if deg >= r else 0) for r in range(3)]
            left, right = [f(t0) for f in d[:m]], [f(t0 + h) for f in d[:m]]
            for th in (Fraction(0), Fraction(1, 3), Fraction(0.87439474), Fraction(1)):
                assert dr.hermite_exact(th, h, left, right) == d[0](t0 + th * h), (m, deg, th)
                assert dr.hermite_exact(th, h, left, right, deriv=True) == d[1](t0 + th * h), (m, deg, th)
    # one degree more is NOT reproduced: the interpolants are the cubic and the quintic, no more
    assert dr.hermite_exact(Fraction(1, 2), 1, (0, 0), (1, 4)) != Fraction(1, 16)
    assert dr.hermite_exact(Fraction(1, 2), 1, (0, 0, 0), (1, 6, 30)) != Fraction(1, 64)


def test_index_logic_on_hand_worked_queries():
    """Worked by hand from the comments of image_state and dense_mdisc_qs: a tile of kind 4 (64 eighths per step) at pos8 = 800."""
    ix = dr.index(4, 800, 10, 800 + 64 * 4 + 8 * 7)          # step 4, skipped point 7: nodes 3 .. 6, the middle interval
    assert (ix["sh8"], ix["J"], ix["rem"], ix["i"], ix["l0"], ix["variant"]) == (6, 4, 56, 7, 3, 1)
    assert ix["base"] == 200 + (2 * 7 + 6) * 12 + 4
    ix = dr.index(4, 800, 10, 800 + 8)                        # the first step: nodes 0 .. 3, the first interval
    assert (ix["J"], ix["i"], ix["l0"], ix["variant"]) == (0, 1, 0, 0) and ix["base"] == 200 + 14 * 12
    ix = dr.index(4, 800, 10, 800 + 64 * 9 + 16)              # the last step: nodes 7 .. 10, the last interval
    assert (ix["J"], ix["i"], ix["l0"], ix["variant"]) == (9, 2, 7, 2)
    ix = dr.index(2, 800, 3, 800 + 16 * 2 + 8)                # kind 2, keep 3: every step on nodes 0 .. 3
    assert (ix["sh8"], ix["J"], ix["i"], ix["l0"], ix["variant"]) == (4, 2, 1, 0, 2) and ix["base"] == 200 + 8
    assert dr.index(0, 5, 37, 5 + 37)["J"] == 37 and dr.index(0, 5, 37, 5 + 37)["rem"] == 0
    assert dr.legal(4, 800, 10, 800 + 640, 4) and not dr.legal(4, 800, 10, 800 + 648, 4) and not dr.legal(4, 800, 10, 804, 4)
    assert dr.legal(0, 5, 37, 6, 2) and not dr.legal(2, 800, 129, 800, 2) and dr.legal(2, 800, 129, 800, 4)


# ---------------------------------------------------------------- the crafted tiles
@pytest.mark.parametrize("G", [2, 4])
@pytest.mark.parametrize("kind", range(5))
@pytest.mark.parametrize("name", list(dc.GRIDS))
def test_crafted_tiles_reach_every_branch(restated_tables, name, kind, G):
    """Judged on the restatement alone: every query legal, no value read from a node beyond keep (those are NaN, which the exact
    arithmetic refuses), and between them the tiles reach dense_cases.required(kind)."""
    tags = set()
    for tile in dc.tiles(name, kind, G):
        assert tile["img"].shape == (5, 64 * G + 1) and np.all(np.isnan(tile["img"][:, tile["keep"] + 1:]))
        assert np.all(np.isfinite(tile["img"][:, :tile["keep"] + 1]))
        assert all(dr.legal(kind, tile["pos8"], tile["keep"], int(p), G) for p in tile["p8"]) and len(set(tile["p8"].tolist())) == tile["p8"].size
        res = dc.restate(restated_tables[name], tile)
        tags |= dc.coverage(kind, G, tile, res)
        if tile["name"] == "cross":
            zs = [r["z"] for r in res if r["z"] is not None]
            assert min(zs) < 1.0 <= max(zs)
    assert dc.required(kind) <= tags, sorted(dc.required(kind) - tags)


# ---------------------------------------------------------------- the read-out against the true solution
def _method_errors(g, T):
    """Largest relative error of the exact-arithmetic read-out against the true solution over the fixture's cases, per
    (branch, kind) for Mdisc and ("omega", kind); and of the plain cubic where the source makes a claim about it."""
    worst, cubic_qs, cubic_tr, quintic_tr = {}, {}, {}, {}
    for tile in dc.golden_tiles(g, 2):
        res = dc.restate(T[tile["name"][0]], tile)
        truth = [[Fraction(float(h)) + Fraction(float(l)) for h, l in zip(*tile[k])] for k in ("truth_M", "truth_W")]
        W, F, M, D, D2 = tile["img"]
        for q, r in enumerate(res):
            eM, eW = float(abs(r["Mv"] - truth[0][q]) / truth[0][q]), float(abs(r["Wv"] - truth[1][q]) / truth[1][q])
            if r["branch"] == "node":
                assert eM <= dr.U and eW <= dr.U                                    # the image is the truth rounded once
                continue
            worst[(r["branch"], tile["kind"])] = max(worst.get((r["branch"], tile["kind"]), 0.0), eM)
            worst[("omega", tile["kind"])] = max(worst.get(("omega", tile["kind"]), 0.0), eW)
            J = r["J"]
            cub = dr.hermite_exact(r["th"], r["h"], (float(M[J]), float(D[J])), (float(M[J + 1]), float(D[J + 1])))
            ec = float(abs(cub - truth[0][q]) / truth[0][q])
            gk = (tile["name"][0], tile["kind"])
            if tile["regime"] in ("qs", "qsdeep"):
                cubic_qs[gk] = max(cubic_qs.get(gk, 0.0), ec)
            if tile["regime"] == "quintic":
                cubic_tr[gk], quintic_tr[gk] = max(cubic_tr.get(gk, 0.0), ec), max(quintic_tr.get(gk, 0.0), eM)
    return worst, cubic_qs, cubic_tr, quintic_tr


def test_method_bounds_are_the_measured_ones(g, restated_tables):
    """The exact-arithmetic read-out of the trajectory cases agrees with the true solution to the figures recorded in
    dense_cases.METHOD_MEASURED (the GPU test allows twice them), which are what this test measures, rounded up to two digits.
    An index slip in the restatement -- a wrong variant, theta, node -- is 1e-4 and larger here."""
    worst, cubic_qs, cubic_tr, quintic_tr = _method_errors(g, restated_tables)
    assert set(worst) == set(dc.METHOD_MEASURED)
    for key in sorted(worst, key=str):
        print(f"DENSE-MAX method {key[0]} kind {key[1]}: {worst[key]:.3e} (recorded {dc.METHOD_MEASURED[key]:.1e})")
        assert worst[key] <= dc.METHOD_MEASURED[key] <= 1.11 * worst[key] + 1e-17, key
        assert dc.METHOD_BOUNDS[key] == 2.0 * dc.METHOD_MEASURED[key]
    assert max(dc.METHOD_MEASURED.values()) < 2.0e-8
    # the source's claims about the cubic (mp_eval.hpp above hermite5 / hermite_mdisc), measured on the same cases: on the synthetic
    # grid at stride 4 the quasi-steady figure is the source's; the transition of these cases (t = 5 tvisc) is milder than the worst
    # the source speaks of, and the quintic is three orders and more below the cubic in it
    for gk in sorted(cubic_qs):
        print(f"DENSE-MAX claim grid {gk[0]} kind {gk[1]}: plain cubic on quasi-steady tiles {cubic_qs[gk]:.3e}; in the transition "
              f"cubic {cubic_tr[gk]:.3e}, quintic {quintic_tr[gk]:.3e}")
        assert quintic_tr[gk] < 1e-3 * cubic_tr[gk]
    assert 0.1 * dc.CLAIM_CUBIC_QS < cubic_qs[("L", 3)] <= dc.CLAIM_CUBIC_QS
    assert max(cubic_tr[("L", 3)], cubic_tr[("S", 3)]) <= dc.CLAIM_CUBIC_TRANSITION


# ---------------------------------------------------------------- the probe library
def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_probe_library_is_separate():
    """After a build libmp_probe_dense.so exports the mpi_* functions and libmagprop_amd.so none of them; the ABI's binding and
    header do not name them."""
    from magprop_amd import _capi
    pkg = os.path.dirname(os.path.abspath(_capi.__file__))
    probe = _exports(os.path.join(pkg, "libmp_probe_dense.so"))
    assert {s for s in probe if s.startswith("mpi_")} == set(dr.PROBE_EXPORTS)
    assert not {s for s in probe if s.startswith("mp_")}
    product = _exports(os.path.join(pkg, "libmagprop_amd.so"))
    assert not {s for s in product if s.startswith("mpi_")}
    assert not [n for n in _capi.EXPORTS if n.startswith("mpi_")]
    assert "mpi_" not in open(os.path.join(ROOT, "include", "magprop_amd.h")).read()
