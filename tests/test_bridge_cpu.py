"""CPU tests of the bridge-sampling evidence (include/magprop_amd.h mp_bridge_logz, magprop_amd.bridge) through its numpy
restatement (tests/bridge_restated.py): closed forms, the properties of the fixed point, the crafted cases of
tests/bridge_cases.py, the host's Cholesky rule, and the front end's pieces that need no device."""
import math
import os
import re

import numpy as np
import pytest

import bridge_cases as bc
import bridge_restated as br
from conftest import ROOT
from magprop_amd import _capi, bridge

# What the restatement gave on the closed cases over the seeds 1 .. 5 (N1 = N2 = n_fit = 4096 iid samples, numpy's libm), per
# case: the largest dlnz of a seed, and the ratio sd(lambda over the seeds) / mean(dlnz):
#     gauss3       dlnz <= 0.000709   ratio 0.561
#     gauss6       dlnz <= 0.001035   ratio 1.085
#     truncated3   dlnz <= 0.008930   ratio 0.429
#     laplace3     dlnz <= 0.006690   ratio 0.760
# The caps are the worst seed's dlnz x 1.5; the factor a case's ratio may lie off 1 by is its own excess max(r, 1 / r) x 1.5
# (five seeds estimate a standard deviation to about a third of itself).
DLNZ_CAP = {"gauss3": 1.5 * 0.000709, "gauss6": 1.5 * 0.001035, "truncated3": 1.5 * 0.008930, "laplace3": 1.5 * 0.006690}
SPREAD_FACTOR = {"gauss3": 1.5 / 0.561, "gauss6": 1.5 * 1.085, "truncated3": 1.5 / 0.429, "laplace3": 1.5 / 0.760}


@pytest.fixture(scope="module")
def closed():
    """out[0] of every closed case and seed, computed once"""
    return {name: np.array([bc.closed_run(name, seed)["out"][0] for seed in bc.CLOSED_SEEDS]) for name in bc.CLOSED}


@pytest.mark.parametrize("name", list(bc.CLOSED))
def test_closed_forms(closed, name):
    """|lambda - truth| < 4 dlnz for every seed; the scatter of lambda over the seeds agrees with the mean dlnz within the
    case's factor; dlnz stays under the case's cap (the figures: the comment at DLNZ_CAP)."""
    out, truth = closed[name], bc.CLOSED[name]["truth"]
    lam, dlnz = out[:, br.LAMBDA], out[:, br.DLNZ]
    print(name, "truth", truth, "lambda", lam, "dlnz", dlnz, "updates", out[:, br.NITER])
    assert np.all(out[:, br.STATUS] == br.OK)
    assert np.all(np.abs(lam - truth) < 4.0 * dlnz)
    ratio = np.std(lam, ddof=1) / np.mean(dlnz)
    print(name, "max dlnz", dlnz.max(), "sd / mean dlnz", ratio)
    assert 1.0 / SPREAD_FACTOR[name] < ratio < SPREAD_FACTOR[name]
    assert np.all(dlnz < DLNZ_CAP[name])
    # ln_volume is that of the box, and lnz the estimate without it
    c = bc.CLOSED[name]
    lv = 0.0 if c["lower"] is None else float(np.sum(np.log(c["upper"] - c["lower"])))
    assert np.allclose(out[:, br.LN_VOLUME], lv, rtol=0, atol=1e-14) and np.array_equal(out[:, br.LNZ], lam - out[:, br.LN_VOLUME])


def test_laplace_tails_are_heavier_than_the_proposal_and_still_counted(closed):
    """The plain importance-sampling start lambda_0 of the heavy-tailed case is biased low by the tails the Gaussian misses; the
    fixed point moves it to the truth."""
    out, truth = closed["laplace3"], bc.CLOSED["laplace3"]["truth"]
    assert np.all(np.abs(out[:, br.LAMBDA] - truth) < np.abs(out[:, br.LAMBDA0] - truth))


@pytest.fixture(scope="module")
def gauss3():
    return bc.closed_run("gauss3", 1)


def test_one_more_update_moves_the_result_by_no_more_than_tol(gauss3):
    o = gauss3["out"][0]
    k = br.constants(bc.CLOSED_N, bc.CLOSED_N, bc.CLOSED_N)
    nxt = br.update(o[br.LAMBDA], gauss3["a"], gauss3["b"][0], *k[:4])
    assert abs(nxt - o[br.LAMBDA]) <= 1.0e-10


def test_lambda0_is_the_importance_sampling_estimate(gauss3):
    b = gauss3["b"][0]
    want = np.log(np.mean(np.exp(b - b.max()))) + b.max()
    assert abs(gauss3["out"][0][br.LAMBDA0] - want) < 1e-12
    assert gauss3["out"][0][br.NFINITE] == np.count_nonzero(np.isfinite(b))


@pytest.mark.parametrize("c", [-1.0e9, 1.0e6, 3.25])
def test_a_constant_added_to_every_lnprob_moves_lambda_by_it(gauss3, c):
    """To 1e-12 beside the roundings of the shifted inputs themselves: a + c rounds every element at |c|'s ulp, so the run on
    a + c is held against the run on (a + c) - c, and that one against the unshifted run.  tol lies above the ulp of lambda
    (an absolute step of less than an ulp cannot be seen)."""
    k = br.constants(bc.CLOSED_N, bc.CLOSED_N, bc.CLOSED_N)
    ulp = float(np.spacing(abs(c)))
    tol = max(1.0e-10, 8.0 * ulp)
    base = br.fixed_point(gauss3["a"], gauss3["b"][0], *k, 1000, tol)
    moved = br.fixed_point(gauss3["a"] + c, gauss3["b"][0] + c, *k, 1000, tol)
    back = br.fixed_point((gauss3["a"] + c) - c, (gauss3["b"][0] + c) - c, *k, 1000, tol)
    assert moved[br.STATUS] == back[br.STATUS] == base[br.STATUS] == br.OK
    assert abs((moved[br.LAMBDA] - c) - back[br.LAMBDA]) <= 1e-12 + 8.0 * ulp
    assert abs(back[br.LAMBDA] - base[br.LAMBDA]) <= 1e-12 + 8.0 * ulp + tol
    assert abs(moved[br.DLNZ] - back[br.DLNZ]) <= 1e-9 + 1e3 * ulp


def test_the_moments_do_not_depend_on_the_chunks():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((2 * br.BLOCK + 1, 3)) * (1.0, 30.0, 1e-3) + (5.0, -2.0, 0.0)
    whole = br.moments(x)
    for chunk in (1, 2, 7):
        assert np.array_equal(br.moments(x, chunk), whole), chunk
    # and they are the sums about row 0
    d = x - x[0]
    assert np.allclose(whole[:3], d.sum(axis=0), rtol=1e-12)
    assert np.allclose(whole[3 + br.tri(2, 1)], np.sum(d[:, 2] * d[:, 1]), rtol=1e-10)


@pytest.mark.parametrize("ndim", [1, 2, 6, 9])
def test_cholesky_rule_against_numpy(ndim):
    rng = np.random.default_rng(ndim)
    mix = rng.standard_normal((ndim, ndim)) + 2.0 * np.eye(ndim)
    x = rng.standard_normal((5000, ndim)) @ mix.T + 10.0 * rng.standard_normal(ndim)
    m, L, c = br.factor(br.moments(x), x[0], x.shape[0], ndim)
    ref = np.linalg.cholesky(np.atleast_2d(np.cov(x.T)))
    got = br.unpack(L, ndim)
    assert np.max(np.abs(got - ref)) <= 1e-14 * np.max(np.abs(ref)) * 50     # (1e-14 relative, of a matrix of condition ~50)
    assert np.allclose(m, x.mean(axis=0), rtol=1e-13, atol=1e-13)
    assert abs(c - (np.sum(np.log(np.diag(ref))) + 0.5 * ndim * math.log(2.0 * math.pi))) < 1e-12


def test_constant_column_is_refused_with_its_dimension():
    with pytest.raises(ValueError, match="dimension 1"):
        bc.call_expected(bc.ERANGE_CALL)


@pytest.mark.parametrize("name", list(bc.FIXED))
def test_fixed_point_cases(name):
    case = bc.FIXED[name]
    out, _ = bc.fixed_expected(case)
    assert out.shape == (case["b"].shape[0], br.NOUT)
    assert np.all(out[:, br.STATUS] == case["expect"]), out[:, [br.STATUS, br.NITER]]
    if case["expect"] == br.NO_OVERLAP:
        assert np.all(np.isnan(out[:, br.LNZ])) and np.all(out[:, br.NITER] == 0) and np.all(out[:, br.NFINITE] == 0)
        return
    assert np.all(np.isfinite(out)) and np.all(out[:, br.NITER] >= 1)
    if case["expect"] == br.ITER_LIMIT:
        assert np.all(out[:, br.NITER] == case["max_iter"])


def test_offsets_of_any_size_are_harmless():
    lo, hi = bc.fixed_expected(bc.FIXED["offset_minus_1e9"])[0][0], bc.fixed_expected(bc.FIXED["offset_plus_1e6"])[0][0]
    assert abs((lo[br.LAMBDA] + 1.0e9) - (hi[br.LAMBDA] - 1.0e6)) < 1e-6      # (the ulp of 1e9 is 1.2e-7)
    assert abs(lo[br.DLNZ] - hi[br.DLNZ]) < 1e-6


def test_one_finite_draw():
    out = bc.fixed_expected(bc.FIXED["one_finite"])[0][0]
    assert out[br.NFINITE] == 1 and out[br.LAMBDA0] == 0.25 - math.log(300.0)


def test_neff_scales_the_error_of_the_estimator_rows():
    one, all_ = bc.fixed_expected(bc.FIXED["neff_1"])[0][0], bc.fixed_expected(bc.FIXED["neff_n1"])[0][0]
    assert one[br.DLNZ] > all_[br.DLNZ] > 0.0


@pytest.mark.parametrize("name", list(bc.CALLS))
def test_whole_call_cases(name):
    case = bc.CALLS[name]
    res = bc.call_expected(case)
    n_rep, n_draws, nd = case["n_rep"], case["n_draws"], case["x_fit"].shape[1]
    assert res["draws"].shape == (n_rep, n_draws, nd) and res["out"].shape == (n_rep, br.NOUT)
    assert np.all(np.isfinite(res["draw_lnq"])) and np.all(np.isfinite(res["est_lnq"]))
    # the two densities are one formula: the proposal density of a draw by forward substitution is its lnq
    back = br.est_lnq(res["m"], res["L"], res["c"], res["draws"].reshape(-1, nd))
    assert np.allclose(back, res["draw_lnq"].ravel(), rtol=0, atol=1e-6 * max(1.0, float(np.max(np.abs(back)))))
    if case["lower"] is not None:
        inside = np.all((res["draws"] >= case["lower"]) & (res["draws"] <= case["upper"]), axis=2)
        assert np.array_equal(np.isfinite(res["b"]), inside) and not np.all(inside)
    if n_rep > 1:
        assert not np.array_equal(res["draws"][0], res["draws"][1])


def test_draws_are_standard_normal():
    m, L = np.zeros(4), np.array([1.0, 0, 1, 0, 0, 1, 0, 0, 0, 1.0])
    x, lnq, z = br.draws(m, L, 0.0, 7, 20000, 2)
    assert np.array_equal(x.reshape(-1, 4), z) and np.allclose(lnq.ravel(), -0.5 * np.sum(z * z, axis=1))
    assert np.all(np.abs(z.mean(axis=0)) < 4.0 / math.sqrt(40000)) and np.all(np.abs(z.var(axis=0) - 1.0) < 4.0 * math.sqrt(2.0 / 40000))
    assert np.max(np.abs(np.corrcoef(z.T) - np.eye(4))) < 4.0 / math.sqrt(40000)


# ---------------------------------------------------------------- the front end's pieces
def test_split_and_reservoir_split():
    chain, lnp = np.arange(7 * 4 * 2, dtype=float).reshape(7, 4, 2), np.arange(28, dtype=float).reshape(7, 4)
    fit, est, le, ec = bridge.split(chain, lnp)
    assert fit.shape == (12, 2) and est.shape == (16, 2) and le.shape == (16,) and ec.shape == (4, 4, 2)
    assert np.array_equal(fit, chain[:3].reshape(-1, 2)) and np.array_equal(le, lnp[3:].ravel())
    with pytest.raises(ValueError):
        bridge.split(chain[:1], lnp[:1])
    s = {"x": np.arange(10.0)[:, None], "log_prob": -np.arange(10.0), "step": np.array([0, 0, 1, 2, 2, 3, 5, 5, 8, 9])}
    fit, est, le = bridge.reservoir_split(s)
    assert np.array_equal(fit[:, 0], np.arange(5.0)) and np.array_equal(le, -np.arange(5.0, 10.0))


def test_neff_from_tau_and_result_object():
    assert bridge.neff_from_tau(1000, [2.0, 5.0]) == (200.0, True)
    assert bridge.neff_from_tau(1000, [0.3]) == (1000.0, True)                 # clamped to N1
    assert bridge.neff_from_tau(1000, [np.nan]) == (1000.0, False) and bridge.neff_from_tau(10, None) == (10.0, False)
    assert bridge.neff_from_tau(100, [4.0], n_seen=10000.0) == (100.0, True)
    out = np.zeros((3, _capi.BRIDGE_NOUT))
    out[:, 0], out[:, 3], out[:, 7], out[:, 2] = (1.0, 3.0, 2.0), (0.1, 0.2, 0.3), (5.0, 5.0, 5.0), (1.0, 1.0, 1.0)
    r = bridge.BridgeResult(out, 10.0, 20, 30)
    lnz, dlnz = r
    assert lnz == 2.0 and abs(dlnz - 0.2) < 1e-15 and abs(r.dlnz_reps - np.std([1.0, 3.0, 2.0])) < 1e-15
    assert r.ok and list(r.lnz_is) == [4.0] * 3 and len(r.reps) == 3 and r.reps[1]["lnz"] == 3.0


def test_python_mirror_follows_the_header():
    hdr = open(os.path.join(ROOT, "include", "magprop_amd.h")).read()
    define = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, hdr).group(1))
    assert define("MP_BRIDGE_BLOCK") == _capi.BRIDGE_BLOCK == br.BLOCK
    assert define("MP_BRIDGE_MAX_REP") == _capi.BRIDGE_MAX_REP == br.MAX_REP
    assert define("MP_BRIDGE_MAX_ROWS") == _capi.BRIDGE_MAX_ROWS == br.MAX_ROWS
    assert define("MP_BRIDGE_NOUT") == _capi.BRIDGE_NOUT == br.NOUT == len(_capi.BRIDGE_COLUMNS)
    assert (define("MP_BRIDGE_OK"), define("MP_BRIDGE_ITER_LIMIT"), define("MP_BRIDGE_NO_OVERLAP")) == (br.OK, br.ITER_LIMIT, br.NO_OVERLAP)
    body = re.search(r"enum\s*\{\s*MP_BRIDGE_LNZ.*?\}", hdr, flags=re.S).group(0)
    names = [n.lower() for n in re.findall(r"MP_BRIDGE_([A-Z0-9_]+)", body)]
    assert [n.replace("nfinite", "n_finite") for n in names] == list(_capi.BRIDGE_COLUMNS)
    assert "mpb_" not in hdr                                   # (the probe is no part of the ABI)
    assert _capi.ABI_VERSION == 5 and "mp_bridge_logz" in _capi.EXPORTS


def test_bridge_arguments_are_judged_before_a_device_is_touched():
    class NoHandle:
        def bridge_logz(self, *a, **k):
            raise AssertionError("reached the handle")
    import contextlib
    src = lambda ndim: contextlib.nullcontext((NoHandle(), 0, None))
    x = np.zeros((10, 3))
    with pytest.raises(ValueError, match="expected"):
        bridge.bridge_evidence(x, x[:, :2], np.zeros(10), src)
    with pytest.raises(ValueError, match="finite"):
        bridge.bridge_evidence(x, x, np.full(10, -np.inf), src)
