"""CPU tests of the bridge-sampling evidence with a Student-t proposal and with Warp-III (include/magprop_amd.h
mp_bridge_logz_warp, magprop_amd.bridge) through its numpy restatement (tests/bridge_warp_restated.py): closed forms under the four
variants, the invariances of the pairs, the rules of the t proposal, the crafted cases of tests/bridge_warp_cases.py, and the
argument checks and the Python mirror, which need no device."""
import contextlib
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import bridge_cases as bc
import bridge_restated as br
import bridge_warp_cases as wc
import bridge_warp_restated as bw
from conftest import ROOT
from magprop_amd import _capi, bridge


# ---------------------------------------------------------------- closed forms
@pytest.fixture(scope="module")
def closed():
    """out[0] of every closed case, variant and seed, computed once"""
    return {(name, var): np.array([wc.closed_run(name, var, seed)["out"][0] for seed in bc.CLOSED_SEEDS])
            for name in wc.CLOSED for var in wc.VARIANTS}


def rms_error(closed, name, var):
    return float(np.sqrt(np.mean((closed[(name, var)][:, br.LAMBDA] - wc.CLOSED[name]["truth"]) ** 2)))


@pytest.mark.parametrize("var", list(wc.VARIANTS))
@pytest.mark.parametrize("name", list(wc.CLOSED))
def test_closed_forms(closed, name, var):
    """|lambda - truth| < 4 dlnz for every seed, the rule of tests/test_bridge_cpu.py, for every target under every variant."""
    out, truth = closed[(name, var)], wc.CLOSED[name]["truth"]
    lam, dlnz = out[:, br.LAMBDA], out[:, br.DLNZ]
    print(name, var, "truth", truth, "lambda", lam, "dlnz", dlnz, "updates", out[:, br.NITER], "mirrors", out[:, bw.EST_MIRRORS],
          out[:, bw.DRAW_MIRRORS])
    assert np.all(out[:, br.STATUS] == br.OK)
    assert np.all(np.abs(lam - truth) < 4.0 * dlnz)
    warp = wc.VARIANTS[var][1]
    if not warp:
        assert np.all(out[:, bw.EST_MIRRORS] == 0) and np.all(out[:, bw.DRAW_MIRRORS] == 0)
    elif wc.CLOSED[name]["lower"] is None:
        assert np.all(out[:, bw.EST_MIRRORS] == bc.CLOSED_N) and np.all(out[:, bw.DRAW_MIRRORS] == bc.CLOSED_N)
    else:                                                # the half-normal: some mirrors leave the support, some stay
        assert np.all((out[:, bw.EST_MIRRORS] > 0) & (out[:, bw.EST_MIRRORS] < bc.CLOSED_N))
        assert np.all((out[:, bw.DRAW_MIRRORS] > 0) & (out[:, bw.DRAW_MIRRORS] < bc.CLOSED_N))


@pytest.mark.parametrize("name,better,plain", [("split3", "warped", "plain"), ("split6", "warped", "plain"), ("split3", "warped_t", "t"),
                                               ("t3_3", "t", "plain"), ("t3_6", "t", "plain"), ("t3_3", "warped_t", "warped")])
def test_each_remedy_is_not_worse_where_it_is_meant_to_help(closed, name, better, plain):
    """Warping on the skewed target and the t proposal on the heavy-tailed one: the RMS error of ln Z over the seeds is not above
    that of the variant without the remedy (what was seen: DESIGN.md section 8's table)."""
    e_better, e_plain = rms_error(closed, name, better), rms_error(closed, name, plain)
    print(f"{name}: rms error {better} {e_better:.5f}, {plain} {e_plain:.5f}, ratio {e_better / e_plain:.3f}")
    assert e_better <= e_plain


# ---------------------------------------------------------------- invariances
def test_pairs_are_symmetric_in_a_row_and_its_mirror():
    """a and b do not change when a row and its mirror are exchanged, to the bit, whichever of the two counts."""
    rng = np.random.default_rng(3)
    v, vm, lnq = 5.0 * rng.standard_normal(4000) - 40.0, 5.0 * rng.standard_normal(4000) - 40.0, rng.standard_normal(4000)
    ok, okm = rng.random(4000) < 0.7, rng.random(4000) < 0.7
    one, other = bw.pair(v, ok, vm, okm, lnq), bw.pair(vm, okm, v, ok, lnq)
    assert np.array_equal(one, other)
    assert np.array_equal(np.isneginf(one), ~ok & ~okm) and np.all(np.isfinite(one[ok | okm]))
    # a mirror that does not count leaves the row with half its mass
    alone = ok & ~okm
    assert np.array_equal(one[alone], ((v - bw.LN_2) - lnq)[alone])
    # and equal values are their own mean
    same = bw.pair(v, np.ones(4000, dtype=bool), v, np.ones(4000, dtype=bool), lnq)
    assert np.allclose(same, v - lnq, rtol=0, atol=1e-13)


@pytest.mark.parametrize("var", list(wc.VARIANTS))
@pytest.mark.parametrize("c", [1.0e6, 3.25])
def test_a_constant_added_to_every_lnprob_moves_lambda_by_it(var, c):
    """Beside the roundings of the shifted values themselves (every lnprob + c rounds at the ulp of c, 8 of them allowed) and
    the tolerance of the two fixed points."""
    case = wc.CLOSED["split3"]
    ulp = float(np.spacing(abs(c)))
    tol = max(1.0e-10, 8.0 * ulp)
    base = wc.closed_run("split3", var, 1, tol=tol)["out"][0]
    rng = np.random.default_rng(1)
    fit, est = case["sample"](rng, bc.CLOSED_N), case["sample"](rng, bc.CLOSED_N)
    proposal, warp = wc.VARIANTS[var]
    moved = bw.logz(fit, est, case["lnprob"](est) + c, n_draws=bc.CLOSED_N, seed=1, lnprob=lambda x: case["lnprob"](x) + c,
                    proposal=proposal, nu=wc.CLOSED_NU, warp=warp, tol=tol)["out"][0]
    assert moved[br.STATUS] == base[br.STATUS] == br.OK
    assert abs((moved[br.LAMBDA] - c) - base[br.LAMBDA]) <= 1e-12 + 8.0 * ulp + 2.0 * tol
    assert abs(moved[br.DLNZ] - base[br.DLNZ]) <= 1e-9 + 1e3 * ulp


@pytest.mark.parametrize("name", ["ndim_9", "box_cuts_the_draws", "terraces", "sizes_257"])
def test_normal_unwarped_is_the_plain_estimate_bit_for_bit(name):
    case = bc.CALLS[name]
    old = bc.call_expected(case)
    keys = ("lower", "upper", "n_draws", "n_rep", "seed", "neff", "max_iter", "tol", "target")
    new = bw.logz(case["x_fit"], case["x_est"], case["lnp_est"], proposal=bw.NORMAL, warp=False, **{k: case[k] for k in keys})
    for key in ("moments", "draws", "draw_lnp", "draw_lnq", "est_lnq", "a", "b"):
        assert np.array_equal(new[key], old[key], equal_nan=True), key
    assert np.array_equal(new["out"][:, :br.NOUT], old["out"], equal_nan=True) and np.all(new["out"][:, br.NOUT:] == 0.0)


# ---------------------------------------------------------------- the rules of the t proposal
@pytest.mark.parametrize("ndim,nu", [(1, 3), (3, 5), (6, 4), (9, 32)])
def test_t_density_against_scipy(ndim, nu):
    """lnq of the restated rule at random points against scipy.stats.multivariate_t.logpdf with the shape matrix L_t L_t^T.
    The value is a sum of five terms -- h log(1 + Q / nu), sum ln L_t,aa, (ndim / 2) ln(nu pi) and two lgamma -- of largest
    magnitude T.  Either implementation forms each term to about 2 ulp of it (a libm function and a product) and adds them with
    four roundings of half an ulp of at most T: 12 ulp(T) each, 24 between the two.  Q itself, a solve with a matrix of
    condition kappa, is good to about 2 ndim kappa eps relatively in either, which moves the first term by at most
    h Q / (nu + Q) times that: 2 h ndim kappa eps is allowed for it."""
    from scipy.stats import multivariate_t
    rng = np.random.default_rng(10 * ndim + nu)
    mix = rng.standard_normal((ndim, ndim)) + 2.0 * np.eye(ndim)
    x = rng.standard_normal((3000, ndim)) @ mix.T + 3.0 * rng.standard_normal(ndim)
    m, L, _ = br.factor(br.moments(x), x[0], x.shape[0], ndim)
    Lt, c_t, h = bw.student(L, ndim, nu)
    k = math.sqrt((nu - 2.0) / nu)
    assert np.array_equal(Lt, k * L) and h == 0.5 * (nu + ndim)
    shape = br.unpack(Lt, ndim) @ br.unpack(Lt, ndim).T
    pts = m + rng.standard_t(nu, size=(500, ndim)) @ br.unpack(Lt, ndim).T
    z, _ = bw.residuals(m, Lt, pts)
    got = bw.lnq_t(z, h, nu, c_t, br.NUMPY)
    want = multivariate_t(loc=m, shape=shape, df=nu).logpdf(pts)
    q = np.sum(z * z, axis=1)
    terms = [h * np.log1p(q / nu).max(), abs(float(np.sum(np.log(np.diag(br.unpack(Lt, ndim)))))), 0.5 * ndim * math.log(nu * math.pi),
             abs(math.lgamma(nu / 2.0)), abs(math.lgamma((nu + ndim) / 2.0))]
    tol = 24.0 * float(np.spacing(max(terms))) + 2.0 * h * ndim * float(np.linalg.cond(shape)) * np.finfo(float).eps
    err = float(np.max(np.abs(got - want)))
    print(f"ndim {ndim} nu {nu}: largest term {max(terms):.3f}, cond {np.linalg.cond(shape):.1f}, max |restated - scipy| {err:.3e}, allowed {tol:.3e}")
    assert err <= tol


def test_chi_square_normals_are_standard_normal_and_independent_of_z():
    n, nu = 20000, 5
    g = bw.chi_normals(7, n, 2, nu)
    _, _, z = br.draws(np.zeros(4), np.array([1.0, 0, 1, 0, 0, 1, 0, 0, 0, 1.0]), 0.0, 7, n, 2)
    assert g.shape == (2 * n, nu)
    sd = 1.0 / math.sqrt(2 * n)
    assert np.all(np.abs(g.mean(axis=0)) < 4.0 * sd) and np.all(np.abs(g.var(axis=0) - 1.0) < 4.0 * math.sqrt(2.0) * sd)
    both = np.corrcoef(np.hstack([g, z]).T)
    assert np.max(np.abs(both - np.eye(nu + 4))) < 4.5 * sd          # (36 coefficients: 4.5 sd for the largest of them)
    # an even nu uses both normals of every pair, an odd one all but the last: the first columns are the same normals
    assert np.array_equal(bw.chi_normals(7, 100, 1, 4), bw.chi_normals(7, 100, 1, 5)[:, :4])
    assert np.array_equal(bw.chi_normals(7, 100, 1, 6)[:, :5], bw.chi_normals(7, 100, 1, 5))


def test_scaled_draws_have_the_fit_rows_covariance():
    """x = m + sqrt(nu / w) L_t z has covariance nu / (nu - 2) L_t L_t^T = L L^T.  For the multivariate t the variance of a
    sample covariance C_ab over n draws is at most 3 (nu - 2) / (nu - 4) C_aa C_bb / n (its fourth moments are (nu - 2) / (nu - 4)
    times the Gaussian's): with nu = 8 and n = 40 000 each entry is held to 4 sd of that."""
    nd, nu, n = 3, 8, 40000
    rng = np.random.default_rng(2)
    rows = rng.standard_normal((2000, nd)) @ np.array([[1.0, 0, 0], [0.5, 2.0, 0], [-0.3, 0.4, 0.7]]).T + (1.0, -2.0, 0.5)
    m, L, _ = br.factor(br.moments(rows), rows[0], rows.shape[0], nd)
    Lt, c_t, h = bw.student(L, nd, nu)
    x, xm, lnq, z, scale = bw.draws(m, Lt, c_t, 11, n, 1, nu=nu, h=h, warp=True)
    cov, want = np.cov(x.T), br.unpack(L, nd) @ br.unpack(L, nd).T
    sd = np.sqrt(3.0 * (nu - 2.0) / (nu - 4.0) * np.outer(np.diag(want), np.diag(want)) / n)
    assert np.all(np.abs(cov - want) < 4.0 * sd), (cov, want)
    assert np.all(np.abs(x.mean(axis=0) - m) < 4.0 * np.sqrt(np.diag(want) / n))
    # the mirror is the draw reflected in m, and the density is that of the point by forward substitution
    assert np.allclose(x + xm, 2.0 * m, rtol=0, atol=1e-12 * (1.0 + np.abs(x).max()))
    back, _ = bw.residuals(m, Lt, x)
    assert np.allclose(bw.lnq_t(back, h, nu, c_t, br.NUMPY), lnq, rtol=0, atol=1e-9)
    assert np.allclose(bw.lnq_t(bw.residuals(m, Lt, xm)[0], h, nu, c_t, br.NUMPY), lnq, rtol=0, atol=1e-9)


# ---------------------------------------------------------------- the crafted calls
@pytest.mark.parametrize("name", list(wc.CALLS))
def test_whole_call_cases(name):
    case = wc.CALLS[name]
    res = wc.call_expected(case)
    n_rep, n_draws, nd = case["n_rep"], case["n_draws"], case["x_fit"].shape[1]
    assert res["draws"].shape == (n_rep, n_draws, nd) and res["out"].shape == (n_rep, bw.WARP_NOUT)
    assert np.all(np.isfinite(res["draw_lnq"])) and np.all(np.isfinite(res["est_lnq"])) and np.all(np.isfinite(res["a"]))
    assert np.array_equal(res["out"][:, br.NFINITE], np.count_nonzero(res["b"] > -np.inf, axis=1))
    if case["warp"]:
        inside = lambda x: np.all((x >= case["lower"]) & (x <= case["upper"]), axis=-1) if case["lower"] is not None else np.ones(x.shape[:-1], bool)
        assert np.array_equal(res["out"][:, bw.DRAW_MIRRORS], np.count_nonzero(inside(res["draw_mirrors"]), axis=1))
        assert np.all(res["out"][:, bw.EST_MIRRORS] == np.count_nonzero(inside(res["est_mirrors"])))
        assert np.array_equal(np.isneginf(res["b"]), ~inside(res["draws"]) & ~inside(res["draw_mirrors"]))
    if n_rep > 1:
        assert not np.array_equal(res["draws"][0], res["draws"][1])


def test_the_box_cases_are_what_their_names_say():
    half = wc.call_expected(wc.CALLS["box_cuts_half_the_mirrors"])["out"]
    assert np.all((half[:, bw.DRAW_MIRRORS] > 100) & (half[:, bw.DRAW_MIRRORS] < 200)) and np.all(half[:, br.STATUS] == br.OK)
    both = wc.call_expected(wc.CALLS["draw_and_mirror_both_outside"])
    assert 50 < np.count_nonzero(np.isneginf(both["b"])) < 250 and both["out"][0, br.STATUS] == br.OK
    none = wc.call_expected(wc.CALLS["no_draw_inside"])["out"]
    assert np.all(none[:, br.STATUS] == br.NO_OVERLAP) and np.all(none[:, br.NFINITE] == 0) and np.all(none[:, bw.DRAW_MIRRORS] == 0)


# ---------------------------------------------------------------- the argument checks and the Python mirror
def test_python_mirror_follows_the_header():
    hdr = open(os.path.join(ROOT, "include", "magprop_amd.h")).read()
    define = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, hdr).group(1))
    assert define("MP_BRIDGE_NORMAL") == _capi.BRIDGE_NORMAL == bw.NORMAL == 0
    assert define("MP_BRIDGE_STUDENT") == _capi.BRIDGE_STUDENT == bw.STUDENT == 1
    assert define("MP_BRIDGE_MAX_NU") == _capi.BRIDGE_MAX_NU == bw.MAX_NU == 32
    assert define("MP_BRIDGE_WARP_NOUT") == _capi.BRIDGE_WARP_NOUT == bw.WARP_NOUT == len(_capi.BRIDGE_WARP_COLUMNS)
    assert define("MP_BRIDGE_NOUT") == 12 and _capi.BRIDGE_WARP_COLUMNS[:12] == _capi.BRIDGE_COLUMNS
    assert re.search(r"enum\s*\{\s*MP_BRIDGE_EST_MIRRORS\s*=\s*12\s*,\s*MP_BRIDGE_DRAW_MIRRORS\s*\}", hdr)
    assert _capi.BRIDGE_WARP_COLUMNS[bw.EST_MIRRORS] == "est_mirrors" and _capi.BRIDGE_WARP_COLUMNS[bw.DRAW_MIRRORS] == "draw_mirrors"
    assert _capi.BRIDGE_PROPOSALS == {"normal": 0, "t": 1}
    assert _capi.ABI_VERSION == 5 and "mp_bridge_logz_warp" in _capi.EXPORTS and "mp_bridge_logz" in _capi.EXPORTS
    assert "0x42524701" in hdr and hex(bw.CTR_CHI) == "0x42524701"


def test_new_arguments_are_judged_before_a_device_is_touched():
    """Every new MP_EINVAL of mp_bridge_logz_warp on the library itself, with a handle that is no handle: a block of zeros the
    entry would have to read to reach a device, and returns before it does."""
    L = _capi.lib()
    fake = C.create_string_buffer(4096)
    rng = np.random.default_rng(1)
    x = np.ascontiguousarray(rng.standard_normal((64, 2)))
    lnp = np.ascontiguousarray(-0.5 * np.sum(x * x, axis=1))
    out = np.zeros((64, _capi.BRIDGE_WARP_NOUT))
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))

    def call(**kw):
        a = dict(n_draws=32, n_rep=1, target=1, proposal=0, nu=5, warp=0, x_fit=x, out=out, ndim=2)
        a.update(kw)
        return L.mp_bridge_logz_warp(C.cast(fake, C.c_void_p), dp(a["x_fit"]), 64, dp(x), dp(lnp), 64, a["ndim"], 0, None, None, a["n_draws"],
                                     a["n_rep"], C.c_uint64(3), C.c_double(64.0), 50, C.c_double(1e-8), a["target"], a["proposal"], a["nu"],
                                     a["warp"], dp(a["out"]), *([None] * 10))

    for kw in (dict(proposal=2), dict(proposal=-1), dict(proposal=1, nu=2), dict(proposal=1, nu=33), dict(proposal=1, nu=0), dict(warp=2),
               dict(warp=-1), dict(target=5), dict(target=-1), dict(warp=1, n_draws=(_capi.BRIDGE_MAX_ROWS >> 1) + 1),
               dict(warp=1, n_draws=1 << 20, n_rep=3), dict(x_fit=None), dict(out=None), dict(n_rep=65), dict(ndim=0)):
        assert call(**kw) == _capi.MP_EINVAL, kw
        assert "mp_bridge_logz_warp" in _capi.last_error(), kw
    # nu is read for the t proposal only; target 3 is not one of mp_bridge_logz's
    assert "nu must be" in (call(proposal=1, nu=2), _capi.last_error())[1]
    assert L.mp_bridge_logz(C.cast(fake, C.c_void_p), dp(x), 64, dp(x), dp(lnp), 64, 2, 0, None, None, 32, 1, C.c_uint64(3), C.c_double(64.0), 50,
                            C.c_double(1e-8), 3, dp(out), None, None, None, None, None) == _capi.MP_EINVAL


def test_front_end_arguments_are_judged_before_a_device_is_touched():
    class NoHandle:
        def bridge_logz(self, *a, **k):
            raise AssertionError("reached the handle")
    src = lambda ndim: contextlib.nullcontext((NoHandle(), 0, None))
    x = np.zeros((10, 3))
    for kw, what in ((dict(proposal="cauchy"), "proposal"), (dict(proposal="t", nu=2), "nu"), (dict(proposal="t", nu=33), "nu"),
                     (dict(proposal="t", nu=4.5), "nu"), (dict(warp=2), "warp"), (dict(proposal=2), "proposal")):
        with pytest.raises(ValueError, match=what):
            bridge.bridge_evidence(x, x, np.zeros(10), src, **kw)
    assert _capi.bridge_proposal("normal", nu=1000) == (0, 0, 0) and _capi.bridge_proposal("t", 7, True) == (1, 7, 1)
    assert _capi.bridge_proposal(_capi.BRIDGE_STUDENT, 3, 0) == (1, 3, 0)


def test_result_object_carries_the_proposal():
    out = np.zeros((2, _capi.BRIDGE_WARP_NOUT))
    out[:, 0], out[:, 12], out[:, 13] = (1.0, 3.0), (7.0, 7.0), (5.0, 6.0)
    r = bridge.BridgeResult(out, 10.0, 20, 30, "t", 5, True)
    assert (r.proposal, r.nu, r.warp, r.est_mirrors) == ("t", 5, True, 7) and r.draw_mirrors.tolist() == [5, 6]
    assert "t(5)" in repr(r) and "warp=True" in repr(r) and "draw_mirrors=[5, 6]" in repr(r)
    assert set(r.reps[0]) == set(_capi.BRIDGE_WARP_COLUMNS)
    plain = bridge.BridgeResult(np.zeros((1, _capi.BRIDGE_NOUT)), 10.0, 20, 30)
    assert (plain.proposal, plain.nu, plain.warp, plain.est_mirrors) == ("normal", None, False, 0) and plain.draw_mirrors.tolist() == [0]
    assert "warp" not in repr(plain) and "proposal" not in repr(plain) and set(plain.reps[0]) == set(_capi.BRIDGE_COLUMNS)
