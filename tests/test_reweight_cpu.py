"""CPU checks of the importance reweighting above the kernels: the refusals of mp_model_reweight that need no handle, the column
names against the header, the host functions of magprop_amd/reweight.py against direct numpy on the same log weights, two closed
forms, the Student-t constant, and summaries.reweight over a recording stand-in for the Handle.  No device."""
import contextlib
import os
import re

import numpy as np
import pytest
from scipy.integrate import quad
from scipy.special import logsumexp

from conftest import ROOT

import pointwise_restated as pr
import reweight_restated as rr
from magprop_amd import _capi, pointwise, reweight, summaries
from raw_abi import dp, ip


def _header():
    return open(os.path.join(ROOT, "include", "magprop_amd.h")).read()


def test_names_follow_the_header():
    hdr = _header()
    defs = dict(re.findall(r"#define\s+MP_REWEIGHT_([A-Z0-9_]+)\s+(\d+)", hdr))
    assert int(defs.pop("N")) == len(reweight.NAMES) == _capi.REWEIGHT_N == rr.N == 12
    assert int(defs.pop("MAX_ALT")) == reweight.MAX_ALT == _capi.REWEIGHT_MAX_ALT == rr.MAX_ALT == 64
    assert (int(defs.pop("GAUSS")), int(defs.pop("STUDENT"))) == (reweight.GAUSS, reweight.STUDENT) == (rr.GAUSS, rr.STUDENT) == (0, 1)
    assert sorted(defs, key=lambda k: int(defs[k])) == [n.upper() for n in reweight.NAMES] and sorted(map(int, defs.values())) == list(range(12))
    for k, name in enumerate(reweight.NAMES):
        assert getattr(reweight, name.upper()) == getattr(rr, name.upper()) == k


def test_refusals_without_a_handle():
    """h = NULL: the sizes are judged first, in the order n, ndim, ds_id, n_alt, then the NULL arguments."""
    L = _capi.lib()
    p, kind, alt, out = np.zeros((2, 6)), np.zeros(1, dtype=np.int32), np.array([[1.0, 0.0, 0.0]]), np.zeros((1, 12))

    def call(n=2, ndim=6, ds_id=0, n_alt=1, pars=p, kind=kind, alt=alt, out=out):
        rc = L.mp_model_reweight(None, dp(pars), n, ndim, 0, ds_id, n_alt, ip(kind), dp(alt), None, None, dp(out), None, None, None)
        return rc, _capi.last_error()

    for kw, word in ((dict(n=0, ndim=5, ds_id=-1, n_alt=0), "MP_POINTWISE_MAX_SAMPLES"), (dict(n=_capi.POINTWISE_MAX_SAMPLES + 1), "MP_POINTWISE_MAX_SAMPLES"),
                     (dict(ndim=5, ds_id=-1, n_alt=0), "ndim"), (dict(ndim=10), "ndim"), (dict(ds_id=-1, n_alt=0), "ds_id"),
                     (dict(ds_id=_capi.MAX_DATASETS, n_alt=65), "ds_id"), (dict(n_alt=0, pars=None), "MP_REWEIGHT_MAX_ALT"),
                     (dict(n_alt=65), "MP_REWEIGHT_MAX_ALT"), (dict(), "NULL argument"), (dict(kind=None), "NULL argument")):
        rc, msg = call(**kw)
        assert rc == _capi.MP_EINVAL and "mp_model_reweight" in msg and word in msg, (kw, msg)
    # a bad alternative comes behind the NULL arguments
    rc, msg = call(alt=np.array([[0.0, 0.0, 0.0]]))
    assert rc == _capi.MP_EINVAL and "NULL argument" in msg


def test_constructors():
    g = reweight.gaussian()
    assert (g.kind, g.scale, g.jitter) == (0, 1.0, 0.0) and reweight.observation_weights(g, 5) is None
    t = reweight.student_t(4, scale=1.3, jitter=0.1, power=0.5)
    assert (t.kind, t.scale, t.jitter, t.nu) == (1, 1.3, 0.1, 4.0) and np.array_equal(reweight.observation_weights(t, 3), [0.5] * 3)
    assert np.array_equal(reweight.observation_weights(reweight.gaussian(leave_out=[1, 3]), 4), [1, 0, 1, 0])
    assert np.array_equal(reweight.observation_weights(reweight.gaussian(leave_out=np.array([True, False, False])), 3), [0, 1, 1])
    assert np.array_equal(reweight.observation_weights(reweight.gaussian(weights=[2.0, 0.5], leave_out=[0], power=2.0), 2), [0.0, 1.0])
    assert np.array_equal(reweight.observation_weights(reweight.gaussian(leave_out=[]), 3), [1, 1, 1])     # nothing left out
    assert np.array_equal(reweight.observation_weights(reweight.gaussian(leave_out=np.zeros(0, dtype=bool)), 0), [])
    for bad in (dict(scale=0.0), dict(scale=np.inf), dict(jitter=-0.1), dict(jitter=np.nan), dict(weights=[-1.0]), dict(weights=[np.nan]),
                dict(power=-1.0), dict(leave_out=[0.5]), dict(weights=[[1.0]])):
        with pytest.raises(ValueError):
            reweight.gaussian(**bad)
    for nu in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="nu"):
            reweight.student_t(nu)
    with pytest.raises(ValueError, match="shape"):
        reweight.observation_weights(reweight.gaussian(weights=[1.0, 2.0]), 3)
    with pytest.raises(ValueError, match="alternatives"):
        reweight.pack([], 3)
    with pytest.raises(ValueError, match="alternatives"):
        reweight.pack([g] * 65, 3)
    # pack: the library's order of the observations
    kind, alt, w = reweight.pack([g, reweight.gaussian(1.2, weights=[1.0, 2.0, 3.0])], 3, order=np.array([1, 2, 0]))
    assert kind.dtype == np.int32 and alt.shape == (2, 3) and np.array_equal(w, [[1, 1, 1], [2, 3, 1]])
    assert reweight.pack(g, 3)[2] is None


def test_student_t_constant_integrates_to_one():
    for nu in (1.0, 2.5, 30.0, 1.0e6):
        t = reweight.student_t(nu)
        total, err = quad(lambda x: np.exp(reweight.shape_constant(t, 1.0) - 0.5 * (nu + 1.0) * np.log1p(x * x / nu)), -np.inf, np.inf, epsabs=1e-12)
        assert abs(total - 1.0) < 1e-8 + 10.0 * err, (nu, total, err)
    total, _ = quad(lambda x: np.exp(reweight.shape_constant(reweight.gaussian(), 1.0) - 0.5 * x * x), -np.inf, np.inf)
    assert abs(total - 1.0) < 1e-10
    assert reweight.shape_constant(reweight.gaussian(), 7.5) == 7.5 * reweight.shape_constant(reweight.gaussian(), 1.0)


def test_host_functions_against_direct_numpy():
    rng = np.random.default_rng(3)
    n = 1500
    lw = np.stack([rng.standard_normal(n), 3.0 * rng.standard_normal(n) - 40.0, 0.2 * rng.standard_normal(n) + 700.0, np.zeros(n)])
    lw[:, ::17] = np.nan                                     # samples that did not finish
    table, tail = rr.cols(lw)
    used = ~np.isnan(lw[0])
    m = int(used.sum())
    v = lw[:, used]
    alts = [reweight.gaussian(1.3), reweight.student_t(3.0, leave_out=[0, 1]), reweight.gaussian(power=0.5), reweight.gaussian()]
    n_obs = 10
    want_lmw = logsumexp(v, axis=1) - np.log(m)
    want_neff = np.exp(2.0 * logsumexp(v, axis=1) - logsumexp(2.0 * v, axis=1))
    assert np.allclose(reweight.log_mean_weight(table), want_lmw, rtol=1e-12, atol=0)
    assert np.allclose(reweight.n_eff(table), want_neff, rtol=1e-12, atol=0) and abs(reweight.n_eff(table)[3] - m) < 1e-9 * m
    c_g = -0.5 * np.log(2.0 * np.pi)
    from math import lgamma
    c_t = lgamma(2.0) - lgamma(1.5) - 0.5 * np.log(3.0 * np.pi)
    const = np.array([0.0, 8 * c_t - 10 * c_g, 5 * c_g - 10 * c_g, 0.0])
    ratio, err = reweight.log_evidence_ratio(table, alts, n_obs)
    assert np.allclose(ratio, want_lmw + const, rtol=1e-12, atol=1e-12)
    w = np.exp(v - v.max(axis=1, keepdims=True))
    want_err = np.sqrt(np.mean(w * w, axis=1) / np.mean(w, axis=1) ** 2 - 1.0) / np.sqrt(m)
    assert np.allclose(err[:3], want_err[:3], rtol=1e-12, atol=0)
    assert err[3] == 0.0                                     # the identity alternative: n_eff = N_USED, no error
    # weights and sensitivity
    for k in range(4):
        wk = reweight.weights(lw, k)
        assert wk.shape == (n,) and np.all(wk[~used] == 0.0) and abs(wk.sum() - 1.0) < 1e-12
        assert np.allclose(wk[used], w[k] / w[k].sum(), rtol=1e-12)
    x = rng.standard_normal((n, 3)) + np.array([1.0, -2.0, 0.5])
    s = reweight.sensitivity(x, lw)
    assert np.allclose(s["mean"], x[used].mean(axis=0), rtol=1e-12) and np.allclose(s["std"], x[used].std(axis=0), rtol=1e-12)
    for k in range(4):
        wk = w[k] / w[k].sum()
        mean = (wk[:, None] * x[used]).sum(axis=0)
        assert np.allclose(s["weighted_mean"][k], mean, rtol=1e-12)
        assert np.allclose(s["weighted_std"][k], np.sqrt((wk[:, None] * (x[used] - mean) ** 2).sum(axis=0)), rtol=1e-12)
        assert np.isclose(s["n_eff"][k], want_neff[k], rtol=1e-12)
        assert np.allclose(s["weighted_mean_err"][k], np.sqrt((wk[:, None] ** 2 * (x[used] - mean) ** 2).sum(axis=0)), rtol=1e-12)
    assert np.allclose(s["weighted_mean"][3], s["mean"], rtol=1e-12) and np.allclose(s["mean_err"], x[used].std(axis=0) / np.sqrt(m), rtol=1e-12)
    assert np.allclose(s["weighted_mean_err"][3], s["mean_err"], rtol=1e-12)     # equal weights: the two errors are one
    # psis: nothing to smooth in a constant column; a fitted shape elsewhere, and the smoothed normaliser near the raw one
    ps = reweight.psis(table, tail)
    assert ps["khat"][3] == np.inf and abs(ps["log_mean_weight"][3]) < 1e-12
    assert np.all(np.isfinite(ps["khat"][:3])) and np.all(np.abs(ps["log_mean_weight"][[0, 2]] - want_lmw[[0, 2]]) < 1e-2)
    assert ps["khat"][2] < ps["khat"][0] < reweight.KHAT_BAD < ps["khat"][1]    # (log weights of sd 0.2, 1 and 3: the last is beyond repair)
    empty = rr.cols(np.full((1, 8), np.nan))
    assert np.isnan(reweight.psis(*empty)["khat"][0]) and np.isnan(reweight.n_eff(empty[0])[0])
    with pytest.raises(ValueError, match="weight 0"):
        reweight.weights(np.full((1, 4), -np.inf))


def full_column_psis(col):
    """(khat, ln mean of the smoothed weights) of ALL the log weights col[n] of one alternative, the straightforward way
    (tests/test_pointwise_cpu.py full_matrix_psis for a column of log weights): drop the NaN, shift by the largest, take the M =
    ceil(min(S / 5, 3 sqrt(S))) largest above the (M + 1)-th as the tail, fit, replace them by the fitted distribution's expected
    order statistics truncated at the largest raw weight, and average."""
    v = col[~np.isnan(col)]
    S = v.size
    if S == 0:
        return np.nan, np.nan
    top = np.max(v)
    if not np.isfinite(top):
        return np.inf, top
    lw = v - top
    order = np.argsort(lw, kind="stable")
    M = int(np.ceil(min(S / 5.0, 3.0 * np.sqrt(S))))
    khat = np.inf
    if S > M:
        cutoff = lw[order[-M - 1]]
        tail = order[lw[order] > cutoff]
        if tail.size >= 5:
            x = np.exp(lw[tail]) - np.exp(cutoff)
            if x[0] > 0.0 and np.isfinite(x[-1]):
                k, sigma = pointwise.gpdfit(x)
                if np.isfinite(k):
                    khat = k
                    p = (np.arange(tail.size) + 0.5) / tail.size
                    lw = lw.copy()
                    lw[tail] = np.minimum(np.log(pointwise.gpdinv(p, k, sigma) + np.exp(cutoff)), 0.0)
    return khat, top + logsumexp(lw) - np.log(S)


def test_psis_is_the_full_column_psis():
    """reweight.psis works from the table and the tail row alone; held to the full-column computation on the same log weights to
    1e-12 relative: columns of every size around the tail rule, with failed samples, with ties that straddle the cut (so that
    fewer values lie above it than the tail is long), with fewer than MIN_TAIL values above the cut (no fit: khat = inf, the raw
    mean), constant, with -inf entries, empty."""
    rng = np.random.default_rng(17)
    for n in (5, 26, 224, 225, 226, 1500, 4096):
        lw = np.stack([rng.standard_normal(n), 3.0 * rng.standard_normal(n) - 40.0, 0.2 * rng.standard_normal(n) + 700.0,
                       np.round(2.0 * rng.standard_normal(n)) / 2.0, np.zeros(n), rng.standard_normal(n), rng.standard_normal(n),
                       np.full(n, np.nan)])
        lw[0, ::7] = np.nan                                  # samples that did not finish
        lw[5, rng.random(n) < 0.3] = -np.inf
        top = np.argsort(lw[6])[-4:]                         # four values far above a sea of ties: fewer than MIN_TAIL above the cut
        lw[6] = -1.0
        lw[6, top] = np.array([0.5, 1.0, 1.5, 2.0])[:top.size]
        table, tail = rr.cols(lw)
        got = reweight.psis(table, tail)
        fitted = 0
        for k in range(lw.shape[0]):
            khat, lmw = full_column_psis(lw[k])
            assert (np.isnan(khat) and np.isnan(got["khat"][k])) or got["khat"][k] == khat or \
                abs(got["khat"][k] - khat) <= 1e-12 * abs(khat), (n, k, got["khat"][k], khat)
            assert (np.isnan(lmw) and np.isnan(got["log_mean_weight"][k])) or \
                abs(got["log_mean_weight"][k] - lmw) <= 1e-12 * max(1.0, abs(lmw)), (n, k, got["log_mean_weight"][k], lmw)
            fitted += bool(np.isfinite(khat))
        assert got["khat"][4] == np.inf and got["khat"][6] == np.inf and np.isnan(got["khat"][7])
        assert abs(got["log_mean_weight"][4]) <= 1e-12
        if n >= 224:
            assert fitted >= 4 and np.isfinite(got["khat"][3])          # the tied column is fitted too
            used3 = int(table[3, rr.N_USED] - table[3, rr.NONTAIL_COUNT])
            assert 5 <= used3 < pr.tail_len(n) - 1                      # ... from fewer values than the tail is long: ties at the cut


@pytest.mark.parametrize("s", [0.7, 1.1])
def test_closed_form_gaussian_to_gaussian(s):
    """x ~ N(0, 1) reweighted to N(0, s^2) through the restated kernels: one observation y = 0 with error 1, the model value of
    sample i being x_i, and the alternative gaussian(scale=s).  The weights' fourth moment exists for s^2 < 4 / 3, so both
    estimators have delta-method errors: log_evidence_ratio -> 0 (its own reported error) and n_eff / n -> s sqrt(2 - s^2) (the
    error of m1^2 / m2 from the sample covariance of (w, w^2)); each within 5 standard errors."""
    n = 65536
    x = np.random.default_rng(20231 + int(10 * s)).standard_normal(n)
    ltot = np.repeat(x[:, None], 2, axis=1)
    alts = [reweight.gaussian(scale=s)]
    kind, alt, _ = reweight.pack(alts, 1)
    lw = rr.rows(ltot, np.zeros(n, dtype=np.int32), np.zeros(1, dtype=np.int32), np.zeros(1), np.ones(1), np.zeros(1), np.ones(1), kind, alt)
    assert np.allclose(lw[0], -np.log(s) - 0.5 * x * x / (s * s) + 0.5 * x * x, rtol=1e-12, atol=1e-12)
    table, _ = rr.cols(lw)
    ratio, err = reweight.log_evidence_ratio(table, alts, 1)
    w = np.exp(lw[0])
    m1, m2 = w.mean(), (w * w).mean()
    grad = np.array([2.0 * m1 / m2, -m1 * m1 / (m2 * m2)])
    se_r = float(np.sqrt(grad @ np.cov(np.stack([w, w * w])) @ grad / n))
    got_r, want_r = reweight.n_eff(table)[0] / n, s * np.sqrt(2.0 - s * s)
    print(f"s = {s}: log_evidence_ratio {ratio[0]:+.3e} (se {err[0]:.3e}), n_eff / n {got_r:.6f} against {want_r:.6f} (se {se_r:.3e})")
    assert abs(ratio[0]) < 5.0 * err[0] and abs(got_r - want_r) < 5.0 * se_r
    assert err[0] < 0.01 and se_r < 0.01


class FakeHandle:
    """Handle.model_reweight and dataset_size: the call recorded, the restated columns of seeded log weights returned"""

    def __init__(self, n_obs):
        self.n_obs, self.calls = n_obs, []

    def dataset_size(self, ds_id):
        return self.n_obs

    def model_reweight(self, pars, kind, alt, obs_w=None, ds_id=0, physical=False):
        self.calls.append(dict(pars=np.array(pars), kind=np.array(kind), alt=np.array(alt), obs_w=None if obs_w is None else np.array(obs_w),
                               ds_id=ds_id, physical=physical))
        n = len(pars)
        lw = np.random.default_rng(5).standard_normal((len(kind), n))
        st = np.zeros(n, dtype=np.int32)
        st[2::7] = _capi.STATUS_FLAG
        lw[:, st != 0] = np.nan
        table, tail = rr.cols(lw)
        self.ret = (lw, table, tail, st, int(np.sum(st == 0)))
        return self.ret


def test_summaries_reweight_over_a_fake_handle():
    x = np.array([30.0, 10.0, 20.0, 10.0])                   # (not sorted, with a tie: the library's order is stable)
    h = FakeHandle(4)
    rows = np.random.default_rng(6).standard_normal((120, 6))
    alts = [reweight.gaussian(1.2), reweight.student_t(5.0, weights=[1.0, 2.0, 3.0, 4.0]), reweight.gaussian(leave_out=[0])]
    entered = []

    def source(ndim):
        entered.append(ndim)
        return contextlib.nullcontext((h, 3, x))

    out = summaries.reweight(source, rows, alts, width=6)
    assert entered == [6] and len(h.calls) == 1
    c = h.calls[0]
    assert np.array_equal(c["pars"], rows) and c["ds_id"] == 3 and c["physical"] is False
    assert np.array_equal(c["kind"], [0, 1, 0]) and np.array_equal(c["alt"], [[1.2, 0, 0], [1, 0, 5.0], [1, 0, 0]])
    assert np.array_equal(c["obs_w"], [[1, 1, 1, 1], [2, 4, 3, 1], [1, 1, 1, 0]])      # times 10, 10, 20, 30: indices 1, 3, 2, 0
    lw, table, tail, st, used = h.ret
    assert set(out) == {"lw", "table", "tail", "status", "n_used", "n_eff", "khat", "log_evidence_ratio", "log_evidence_ratio_err"}
    assert out["lw"] is lw and out["table"] is table and out["tail"] is tail and out["status"] is st and out["n_used"] == used
    ratio, err = reweight.log_evidence_ratio(table, alts, 4)
    assert np.array_equal(out["log_evidence_ratio"], ratio) and np.array_equal(out["log_evidence_ratio_err"], err)
    assert np.array_equal(out["n_eff"], reweight.n_eff(table)) and np.array_equal(out["khat"], reweight.psis(table, tail)["khat"])
    # without times the dataset's size is the handle's and nothing is permuted; one alternative need not be a list
    out1 = summaries.reweight(summaries.on(h, 2), rows, reweight.gaussian(power=0.5))
    assert h.calls[-1]["ds_id"] == 2 and np.array_equal(h.calls[-1]["obs_w"], [[0.5] * 4]) and out1["lw"].shape == (1, 120)
    assert summaries.reweight(summaries.on(h), rows, reweight.gaussian(1.1))["lw"].shape == (1, 120) and h.calls[-1]["obs_w"] is None
    # a bad request touches no handle
    n_calls = len(h.calls)
    with pytest.raises(ValueError, match="samples must be 2-D"):
        summaries.reweight(source, rows[:, :5], alts, width=6)
    with pytest.raises(ValueError, match="alternatives"):
        summaries.reweight(source, rows, [], width=6)
    with pytest.raises(ValueError, match="shape"):
        summaries.reweight(source, rows, [reweight.gaussian(weights=[1.0, 2.0])], width=6)
    assert len(h.calls) == n_calls
