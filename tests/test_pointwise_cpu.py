"""CPU checks of the pointwise scores' host side: magprop_amd/pointwise.py (PSIS-LOO from the split the device returns, WAIC,
summaries, comparison) against a full-matrix PSIS and a closed form, the column names against the header's indices,
fit_stats.ppc_pvalue against a simulation, and the entry point's argument checks without a device."""
import ctypes
import os
import re

import numpy as np
import pytest
from scipy.special import logsumexp
from scipy.stats import norm

from conftest import ROOT
from magprop_amd import _capi, fit_stats, pointwise

import pointwise_restated as pr

EPS = 2.0 ** -52


def split(ll):
    """(obs, tail) of a matrix ll[S][n_obs] of pointwise log-likelihoods <= 0, as the device would return them"""
    z = np.sqrt(-2.0 * np.asarray(ll, dtype=np.float64)).T
    return pr.pointwise(z), 0.5 * z * z


def full_matrix_psis(r):
    """PSIS-LOO of one observation from ALL its log importance ratios r[S] (ll = -r), the straightforward way: shift by the
    largest, take the M = ceil(min(S / 5, 3 sqrt(S))) largest above the (M + 1)-th as the tail, fit, replace them by the fitted
    distribution's expected order statistics truncated at the largest raw weight, normalise, weight the likelihoods."""
    S = r.size
    lw = r - np.max(r)
    order = np.argsort(lw, kind="stable")
    M = int(np.ceil(min(S / 5.0, 3.0 * np.sqrt(S))))
    khat = np.inf
    if S > M:
        cutoff = lw[order[-M - 1]]
        tail = order[lw[order] > cutoff]
        if tail.size >= 5:
            x = np.exp(lw[tail]) - np.exp(cutoff)
            k, sigma = pointwise.gpdfit(x)
            if np.isfinite(k):
                khat = k
                p = (np.arange(tail.size) + 0.5) / tail.size
                lw = lw.copy()
                lw[tail] = np.minimum(np.log(pointwise.gpdinv(p, k, sigma) + np.exp(cutoff)), 0.0)
    return logsumexp(lw - r) - logsumexp(lw), khat


def test_names_follow_the_header_indices():
    hdr = open(os.path.join(ROOT, "include", "magprop_amd.h")).read()
    defs = dict((k, int(v)) for k, v in re.findall(r"#define\s+MP_POINTWISE_([A-Z0-9_]+)\s+([0-9]+)\b", hdr))
    assert defs.pop("MAX_SAMPLES") == pointwise.MAX_SAMPLES == _capi.POINTWISE_MAX_SAMPLES == pr.MAX_SAMPLES == 262144
    assert defs.pop("MAX_CELLS") == pointwise.MAX_CELLS == _capi.POINTWISE_MAX_CELLS == pr.MAX_CELLS == 2 ** 28
    assert defs.pop("N") == len(pointwise.NAMES) == _capi.POINTWISE_N == pr.N == 12
    assert sorted(defs.values()) == list(range(12))
    assert [k.lower() for k, _ in sorted(defs.items(), key=lambda kv: kv[1])] == list(pointwise.NAMES)
    for k, v in defs.items():
        assert getattr(pr, k) == v == getattr(pointwise, k), k
    d = pointwise.as_dict(np.arange(24.0).reshape(2, 12))
    assert list(d) == list(pointwise.NAMES) and np.array_equal(d["cut"], [8.0, 20.0])
    with pytest.raises(ValueError, match="12 columns"):
        pointwise.as_dict(np.zeros((3, 11)))
    for n in list(range(-1, 300)) + [4096, 100000, 262144]:
        assert pointwise.tail_len(n) == pr.tail_len(n)


def test_gpdfit_recovers_a_generalised_pareto_sample():
    rng = np.random.default_rng(5)
    for k_true, sigma in ((0.1, 2.0), (0.5, 1.0), (1.0, 0.3)):
        u = rng.random(20000)
        x = np.sort(pointwise.gpdinv(u, k_true, sigma))
        k, s = pointwise.gpdfit(x)
        # the maximum-likelihood error of k is (1 + k) / sqrt(n); the prior moves it by 10 / n of its distance to 0.5
        assert abs(k - k_true) <= 5.0 * (1.0 + k_true) / np.sqrt(x.size) + 10.0 / x.size, (k_true, k)
        assert abs(s / sigma - 1.0) <= 0.1, (sigma, s)
    assert np.allclose(pointwise.gpdinv([0.0, 0.5], 0.0, 2.0), [0.0, 2.0 * np.log(2.0)])


def test_split_psis_is_the_full_matrix_psis():
    rng = np.random.default_rng(11)
    for S in (5, 26, 225, 1000, 4096):
        n_obs = 12
        scale = rng.uniform(0.2, 2.5, n_obs)
        ll = -0.5 * (rng.standard_normal((S, n_obs)) * scale + rng.uniform(-1, 1, n_obs)) ** 2
        ll[:, 0] = np.round(ll[:, 0] * 4.0) / 4.0             # ties, also at the cut
        (obs, tail), r = split(ll)
        got = pointwise.psis_loo(obs, tail)
        for j in range(n_obs):
            want, k = full_matrix_psis(r[j])
            # the two differ in how the S weights and the S weighted likelihoods are summed: (S - 1) eps relative on each of the
            # two sums, hence 2 (S - 1) eps on the difference of their logs; the exps, logs and the shift add a few eps times
            # the magnitudes involved
            lim = 2.0 * (S - 1) * EPS + 16.0 * EPS * (1.0 + abs(want) + np.max(r[j]))
            assert abs(got["elpd_loo"][j] - want) <= lim, (S, j, got["elpd_loo"][j] - want, lim)
            assert (got["khat"][j] == k) or abs(got["khat"][j] - k) <= 1e-9 * (1 + abs(k)), (S, j, got["khat"][j], k)
            assert got["lppd"][j] == pytest.approx(logsumexp(ll[:, j]) - np.log(S), abs=(S + 16) * EPS * (1 + np.max(r[j])))
        assert np.allclose(got["p_loo"], got["lppd"] - got["elpd_loo"], rtol=0, atol=0)
        w = pointwise.waic(obs)
        assert np.allclose(w["p_waic"], np.var(ll, axis=0, ddof=1) if S > 1 else np.nan, rtol=1e-11)
        assert np.array_equal(w["elpd_waic"], w["lppd"] - w["p_waic"]) and np.array_equal(w["lppd"], got["lppd"])


def test_normal_mean_toy_against_the_closed_form():
    """y_j ~ N(theta, 1), flat prior: theta | y ~ N(ybar, 1 / n) and p(y_j | y_-j) = N(ybar_-j, 1 + 1 / (n - 1)) in closed form.
    Observed (seed 0): largest gap per point and on the total, largest khat -- printed below."""
    rng = np.random.default_rng(0)
    n, S = 50, 4096
    y = rng.standard_normal(n)
    theta = y.mean() + rng.standard_normal(S) / np.sqrt(n)
    ll = -0.5 * (y[None, :] - theta[:, None]) ** 2            # the project's unnormalised lnlike term, yerr = 1
    (obs, tail), r = split(ll)
    loo = pointwise.psis_loo(obs, tail)
    ybar_minus = (y.sum() - y) / (n - 1)
    exact = norm.logpdf(y, ybar_minus, np.sqrt(1.0 + 1.0 / (n - 1))) - pointwise.normalisation(np.ones(n))
    gap = np.abs(loo["elpd_loo"] - exact)
    # Monte-Carlo standard error of plain importance sampling: elpd = -log mean(w), w = exp(r), so se = sd(w) / (mean(w) sqrt(S))
    w = np.exp(r - r.max(axis=1, keepdims=True))
    se = w.std(axis=1, ddof=1) / (w.mean(axis=1) * np.sqrt(S))
    print(f"normal-mean toy: largest gap {gap.max():.3e} (largest gap / se {np.max(gap / se):.2f}), total gap "
          f"{abs(loo['elpd_loo'].sum() - exact.sum()):.3e} (se {np.sqrt(np.sum(se ** 2)):.3e}), largest khat {loo['khat'].max():.3f}")
    assert np.all(gap <= 5.0 * se), (gap / se).max()
    assert np.all(loo["khat"] < 0.7), loo["khat"].max()
    s = pointwise.summarize({**pointwise.waic(obs), **loo})
    assert s["n_bad"] == 0 and s["n_obs"] == n
    assert s["elpd_loo"] == pytest.approx(loo["elpd_loo"].sum()) and s["elpd_loo_se"] == pytest.approx(np.sqrt(n * np.var(loo["elpd_loo"], ddof=1)))
    assert abs(s["elpd_waic"] - s["elpd_loo"]) < 0.05 and 0.5 < s["p_loo"] < 1.5 and 0.5 < s["p_waic"] < 1.5   # one parameter


def test_heavy_tail_is_flagged_and_short_tails_fall_back():
    rng = np.random.default_rng(3)
    S = 2000
    ll = -0.5 * rng.standard_normal((S, 6)) ** 2 * 0.05
    ll[:, 2] = -1.5 * rng.exponential(size=S)                 # importance ratios exp(1.5 E): Pareto of shape 1.5
    (obs, tail), r = split(ll)
    loo = pointwise.psis_loo(obs, tail)
    assert loo["khat"][2] > 0.7 and np.all(np.delete(loo["khat"], 2) < 0.7), loo["khat"]
    s = pointwise.summarize(loo, worst=3)
    assert s["n_bad"] == 1 and s["worst"][0] == 2 and len(s["worst"]) == 3
    # four values or fewer above the cut: no fit, khat = inf, plain importance sampling
    for S in (1, 2, 5, 20):
        ll = -0.5 * rng.standard_normal((S, 3)) ** 2
        (obs, tail), r = split(ll)
        assert np.all(obs[:, pr.N_USED] - obs[:, pr.NONTAIL_COUNT] <= 4)
        loo = pointwise.psis_loo(obs, tail)
        assert np.all(loo["khat"] == np.inf)
        plain = np.log(S) - logsumexp(r, axis=1)
        assert np.allclose(loo["elpd_loo"], plain, rtol=0, atol=(S + 16) * EPS * (1 + np.abs(plain).max()))
    # ties: a constant column has nothing above its cut
    (obs, tail), r = split(np.full((300, 2), -0.75))
    loo = pointwise.psis_loo(obs, tail)
    assert np.all(loo["khat"] == np.inf) and np.allclose(loo["elpd_loo"], -0.75, atol=1e-13) and np.allclose(loo["p_loo"], 0, atol=1e-13)
    # a sample that gives a point zero likelihood, and a point no sample reached
    obs0 = obs.copy()
    obs0[0, pr.R_MAX] = np.inf
    obs0[1, :] = np.nan
    obs0[1, pr.N_USED] = 0
    loo = pointwise.psis_loo(obs0, tail)
    assert loo["elpd_loo"][0] == -np.inf and loo["khat"][0] == np.inf and np.isnan(loo["elpd_loo"][1]) and np.isnan(loo["khat"][1])
    with pytest.raises(ValueError, match="2-D"):
        pointwise.psis_loo(obs[0], tail)
    with pytest.raises(ValueError, match="tail"):
        pointwise.psis_loo(obs, tail[:1])


def test_compare_and_normalisation():
    rng = np.random.default_rng(4)
    a, b = rng.standard_normal(40), rng.standard_normal(40)
    assert pointwise.compare(a, a) == (0.0, 0.0)
    d, se = pointwise.compare(a, b)
    assert d == pytest.approx(np.sum(a) - np.sum(b)) and se == pytest.approx(np.sqrt(40 * np.var(a - b, ddof=1)))
    assert pointwise.compare({"elpd_loo": a}, {"elpd_loo": b}) == (d, se) and pointwise.compare({"elpd_waic": a}, b) == (d, se)
    assert pointwise.compare(b, a)[0] == -d
    with pytest.raises(ValueError, match="one length"):
        pointwise.compare(a, b[:-1])
    yerr = np.array([0.5, 1.0, 2.0])
    assert np.allclose(pointwise.normalisation(yerr), norm.logpdf(0.0, 0.0, yerr), rtol=1e-15)


def test_ppc_pvalue_against_a_simulation():
    rng = np.random.default_rng(6)
    n_obs, S, R = 30, 400, 500
    lnlike = -0.5 * rng.chisquare(n_obs, S) * rng.uniform(0.7, 1.6)
    lnlike[::50] = -np.inf                                    # failed models take no part
    p = fit_stats.ppc_pvalue(lnlike, n_obs)
    fin = np.isfinite(lnlike)
    rep = rng.chisquare(n_obs, (R, int(fin.sum())))           # replicated datasets: chi^2_rep ~ chi^2_n for every sample
    sim = np.mean(rep >= -2.0 * lnlike[fin][None, :])
    assert 0.0 < p < 1.0 and abs(p - sim) <= 5.0 * np.sqrt(p * (1.0 - p) / rep.size), (p, sim)
    assert fit_stats.ppc_pvalue([-0.5 * 1e-9], 5) == pytest.approx(1.0) and fit_stats.ppc_pvalue([-5000.0], 5) < 1e-300
    assert np.isnan(fit_stats.ppc_pvalue([-np.inf, np.nan], 5))
    with pytest.raises(ValueError, match="n_obs"):
        fit_stats.ppc_pvalue([-1.0], 0)


def test_entry_point_refuses_bad_arguments_without_a_device():
    L = _capi.lib()
    assert {"mp_model_pointwise", "mp_pointwise_tail_len"} <= set(_capi.EXPORTS)
    assert [L.mp_pointwise_tail_len(n) for n in (-3, 0, 1, 2, 6, 225, 4096, 262144)] == [0, 0, 2, 2, 3, 46, 193, 1537]
    dp = ctypes.POINTER(ctypes.c_double)
    p, out = np.zeros((4, 6)), np.empty((50, 12))
    pp, po = p.ctypes.data_as(dp), out.ctypes.data_as(dp)
    call = lambda n, ndim, ds: L.mp_model_pointwise(None, pp, n, ndim, 0, ds, po, None, None, None, None)   # noqa: E731
    assert call(4, 6, 0) == _capi.MP_EINVAL and "mp_model_pointwise" in _capi.last_error() and "NULL" in _capi.last_error()
    for n in (0, -1, 262145):
        assert call(n, 6, 0) == _capi.MP_EINVAL and "n must be 1..262144" in _capi.last_error(), n
    assert call(4, 5, 0) == _capi.MP_EINVAL and "ndim" in _capi.last_error()
    assert call(4, 10, 0) == _capi.MP_EINVAL
    for ds in (-1, _capi.MAX_DATASETS):
        assert call(4, 6, ds) == _capi.MP_EINVAL and "ds_id" in _capi.last_error()


def test_product_code_imports_no_test_or_oracle_module():
    pkg = os.path.join(ROOT, "magprop_amd")
    for name in ("pointwise.py", "fit_stats.py", "synth.py", "mcmc_eqns.py", "ensemble.py", "_capi.py"):
        src = open(os.path.join(pkg, name)).read()
        assert not re.search(r"^\s*(from|import)\s+(oracle|tests|pointwise_restated|pointwise_cases)\b", src, flags=re.M), name
