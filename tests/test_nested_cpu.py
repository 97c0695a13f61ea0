"""CPU tests of the nested sampler: the estimator (magprop_amd.nested: add_live, estimate, resample_equal) against an exact-draw
nested sampler in numpy, the numpy restatement of the device scheme (tests/nest_restated.py), and the Python front end's
argument checks, which run before any device is touched."""
import math
import os
import re

import numpy as np
import pytest
from scipy.special import erf

import nest_restated as nr
from conftest import ROOT


def _radial_lnz(sig, half, ndim):
    """ln Z of L = exp(-r^2 / (2 sig^2)) under the uniform prior on [-half, half]^ndim."""
    one = sig * math.sqrt(2.0 * math.pi) * erf(half / (sig * math.sqrt(2.0)))
    return ndim * math.log(one / (2.0 * half))


def _exact_runs(n_seeds, nlive, nbatch, sig=0.15, half=1.0, ndim=2, dlogz=0.01, seed=0):
    """Nested sampling with batch removal where the constrained prior is drawn exactly: L depends on r alone, so {L > L*} in the
    box is the ball r < r* cut by the box (rejection from the box while the ball pokes out, uniform in the ball after).  All
    seeds advance together; each stops by the device's rule.  Returns the list of (dead lnL, dead n, live lnL) per seed."""
    rng = np.random.default_rng(seed)

    def lnl_of(r2):
        return -r2 / (2.0 * sig * sig)

    def draw_box(k):
        return np.sum((half * (2.0 * rng.random((k, ndim)) - 1.0)) ** 2, axis=1)

    def draw_constrained(r2max, k):
        rmax = math.sqrt(r2max)
        if rmax <= half:                                   # the ball lies inside the box: exact uniform draw in the ball
            u = rng.random(k) ** (1.0 / ndim)
            return (rmax * u) ** 2
        out = np.empty(0)
        while out.size < k:
            r2 = draw_box(4 * k)
            out = np.concatenate([out, r2[r2 < r2max]])
        return out[:k]

    res = []
    for _ in range(n_seeds):
        live = lnl_of(draw_box(nlive))
        dead_l, dead_n = [], []
        lnx, lnz = 0.0, -math.inf
        while not nr.stops(np.max(live), lnx, lnz, dlogz):
            o = np.argsort(live, kind="stable")
            dead = o[:nbatch]
            for k, j in enumerate(dead):
                inv = 1.0 / (nlive - k)
                lnw = live[j] + lnx + math.log(-math.expm1(-inv))
                lnx -= inv
                lnz = nr.logaddexp(lnz, lnw)
                dead_l.append(live[j])
                dead_n.append(nlive - k)
            lstar = live[dead[-1]]
            live[dead] = lnl_of(draw_constrained(-2.0 * sig * sig * lstar, nbatch))
        res.append((np.array(dead_l), np.array(dead_n), live.copy()))
    return res


@pytest.mark.parametrize("nbatch", [1, 16, 32])
def test_estimator_is_unbiased_and_its_error_matches_the_scatter(nbatch):
    """N = 64 live points, 200 seeds per batch size: the mean of ln Z over the seeds lies within 3 standard errors of the
    closed form, and the scatter of ln Z over the seeds matches the mean logzerr = sqrt(H / N) within 30 %."""
    from magprop_amd import nested
    nlive, ndim, sig = 64, 2, 0.15
    truth = _radial_lnz(sig, 1.0, ndim)
    runs = _exact_runs(200, nlive, nbatch, sig=sig, ndim=ndim, seed=nbatch)
    est = [nested.estimate(dl, dn, ll, nlive) for dl, dn, ll in runs]
    lnz = np.array([e["logz"] for e in est])
    err = np.array([e["logzerr"] for e in est])
    h = np.mean([e["information"] for e in est])
    se = lnz.std(ddof=1) / math.sqrt(lnz.size)
    assert abs(lnz.mean() - truth) < 3.0 * se, (lnz.mean(), truth, se)
    assert 0.7 < lnz.std(ddof=1) / err.mean() < 1.3, (lnz.std(ddof=1), err.mean())
    # H of this likelihood: ln(V / (2 pi sig^2)) - 1 in 2-d (the ball lies well inside the box)
    assert abs(h - (math.log(4.0 / (2.0 * math.pi * sig * sig)) - 1.0)) < 0.1, h


def test_add_live_volumes_and_weights():
    from magprop_amd import nested
    lnl = np.array([-1.0, -3.0, -2.0, -3.0])
    order, lnx, lnw = nested.add_live(-2.5, lnl)
    assert order.tolist() == [1, 3, 2, 0]                              # ascending lnL, slot on ties
    assert np.allclose(np.exp(lnx), np.exp(-2.5) * (1.0 - np.arange(1, 5) / 5.0))
    # the live points share X_final equally: X_{j-1} - X_j = X_final / (N + 1)
    assert np.allclose(lnw, lnl[order] - 2.5 - math.log(5.0))
    # dead sequence: ln X_i = ln X_{i-1} - 1 / n_i
    lx, lw = nested.dead_weights([-5.0, -4.0, -4.5], [4, 3, 4])
    assert np.allclose(lx, -np.cumsum([1 / 4, 1 / 3, 1 / 4]))
    assert np.isclose(lw[1], -4.0 + lx[0] + math.log(1.0 - math.exp(-1.0 / 3.0)))


def test_estimate_of_a_constant_likelihood_is_exact():
    """L = e^{-2} everywhere: Z = e^{-2} (1 - X_final / (N + 1)) (the live points' volumes stop at X_final / (N + 1): dynesty's
    convention), H = -ln(1 - X_final / (N + 1)), and the f_valid term adds with its error."""
    from magprop_amd import nested, tempering
    nlive = 32
    dead_n = np.tile(np.arange(nlive, nlive - 8, -1), 20)
    e = nested.estimate(np.full(dead_n.size, -2.0), dead_n, np.full(nlive, -2.0), nlive)
    x_final = math.exp(-np.sum(1.0 / dead_n))
    assert abs(e["logz"] - (-2.0 + math.log1p(-x_final / (nlive + 1)))) < 1e-12
    assert abs(e["information"] + math.log1p(-x_final / (nlive + 1))) < 1e-12 and e["logzerr"] < 2e-3
    lnf, dlnf = tempering.validity_term(300, 400)
    e2 = nested.estimate(np.full(dead_n.size, -2.0), dead_n, np.full(nlive, -2.0), nlive, lnf, dlnf)
    assert abs(e2["logz"] - (e["logz"] + math.log(0.75))) < 1e-12
    assert abs(e2["logzerr"] - math.sqrt(e["logzerr"] ** 2 + dlnf ** 2)) < 1e-15
    assert abs(dlnf - math.sqrt(0.25 / 300.0)) < 1e-15


def test_resample_equal_follows_the_weights():
    from magprop_amd import nested
    samples = np.arange(4.0)[:, None]
    w = np.array([0.1, 0.2, 0.3, 0.4])
    out = np.concatenate([nested.resample_equal(np.repeat(samples, 250, axis=0), np.log(np.repeat(w, 250)), s) for s in range(20)])
    frac = np.array([(out[:, 0] == k).mean() for k in range(4)])
    assert np.allclose(frac, w / w.sum() * 1.0, atol=0.002)
    # systematic resampling: each row appears floor(n w) or ceil(n w) times
    one = nested.resample_equal(samples, np.log(w), 3)
    counts = np.bincount(one[:, 0].astype(int), minlength=4)
    assert np.all(np.abs(counts - 4 * w) < 1.0)
    with pytest.raises(ValueError):
        nested.resample_equal(samples, np.log(w[:3]))


def test_restatement_samples_the_gaussian_evidence():
    """The restated device scheme (DE walks of 25 steps from the survivors) on the unit Gaussian in an asymmetric 3-d box: ln Z
    within 3 logzerr of the closed form, and the counters add up."""
    from magprop_amd import nested
    lo, hi = np.array([-2.0, -1.0, -4.0]), np.array([3.0, 2.5, 1.5])
    nlive, nbatch = 64, 16
    live0 = lo + (hi - lo) * np.random.default_rng(1).random((1, nlive, 3))
    s = nr.start(live0, nr.gaussian)
    nr.run(s, 400, nbatch, 12345, 25, 0.0, 0.1, 0.01, lo, hi, nr.gaussian_one)
    assert s.stopped[0] and s.nit[0] < 400
    e = nested.estimate(s.dead_lnl[0], s.dead_n[0], s.lnl[0], nlive)
    truth = sum(math.log(math.sqrt(math.pi / 2.0) * (erf(h / math.sqrt(2.0)) - erf(l / math.sqrt(2.0))) / (h - l))
                for l, h in zip(lo, hi))
    assert abs(e["logz"] - truth) < 3.0 * e["logzerr"], (e["logz"], truth, e["logzerr"])
    assert abs(e["logz"] - s.lnz[0]) < 0.2                              # (the running ln Z lacks the live points only)
    assert len(s.dead_lnl[0]) == nbatch * s.nit[0]
    assert 0 < s.nacc[0] <= s.ncall[0] <= 25 * nbatch * s.nit[0]
    assert s.nacc[0] >= s.acc[0].sum()
    assert s.dead_lnl[0][-1] <= np.min(s.lnl[0])


def test_restatement_dead_points_rise_and_walks_respect_the_constraint():
    """Inside an iteration the dead leave in ascending lnL; across iterations L* never falls; every live point after an
    iteration lies in the box above that iteration's L*."""
    lo, hi = np.full(2, -3.0), np.full(2, 3.0)
    live0 = lo + (hi - lo) * np.random.default_rng(2).random((2, 32, 2))
    s = nr.start(live0, nr.gaussian)
    for _ in range(30):
        nr.iteration(s, 8, 7, 10, 0.0, 0.1, 1e-12, lo, hi, nr.gaussian_one)
        for r in range(2):
            assert np.min(s.lnl[r]) >= s.dead_lnl[r][-1]
            assert np.all((s.live[r] >= lo) & (s.live[r] <= hi))
    for r in range(2):
        d = np.array(s.dead_lnl[r])
        assert np.all(np.diff(d) >= 0.0)
        assert s.dead_n[r][:8] == list(range(32, 24, -1))


def assert_states_equal(a, b, extra=()):
    """Two restated States field by field: arrays and dead lists with np.array_equal, ln X and ln Z with ==."""
    for k in ("live", "lnl", "status", "acc", "nit", "stopped", "ncall", "nacc", "nzero") + tuple(extra):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    for r in range(len(a.nit)):
        assert np.array_equal(np.array(a.dead_pars[r]), np.array(b.dead_pars[r]))
        assert np.array_equal(np.array(a.dead_lnl[r]), np.array(b.dead_lnl[r]))
        assert a.dead_n[r] == b.dead_n[r]
    assert np.all(a.lnx == b.lnx) and np.all(a.lnz == b.lnz)


class RecordingGaussian:
    """evaluate(rows, runs) of the unit Gaussian that keeps every call's arguments."""

    def __init__(self):
        self.calls = []

    def __call__(self, rows, runs):
        self.calls.append((np.array(rows), np.array(runs)))
        return nr.gaussian(rows)


def test_rounds_leave_the_state_of_the_one_at_a_time_path():
    """3 runs on the unit Gaussian, N = 32, K = 8, 6 iterations as run(2) + run(4): the round-batched driver and the
    one-at-a-time path leave identical States; the driver hands every row's run through (a row of run r is a point of a walk
    of run r: the walks of different runs start from different live sets) and the live set's rows carry their run."""
    lo, hi = np.array([-2.0, -1.0, -4.0]), np.array([3.0, 2.5, 1.5])
    live0 = lo + (hi - lo) * np.random.default_rng(11).random((3, 32, 3))
    kw = dict(walks=10, g0=0.0, sigma=0.1, dlogz=1e-6, lower=lo, upper=hi)
    a = nr.start(live0, nr.gaussian)
    rec = RecordingGaussian()
    b = nr.start(live0, rec, with_runs=True)
    assert len(rec.calls) == 1 and np.array_equal(rec.calls[0][1], np.repeat(np.arange(3), 32))
    assert np.array_equal(rec.calls[0][0], live0.reshape(-1, 3))
    for n in (2, 4):
        nr.run(a, n, 8, 77, evaluate_one=nr.gaussian_one, **kw)
        nr.run(b, n, 8, 77, evaluate=rec, **kw)
    assert_states_equal(a, b)
    assert np.all(a.nit == 6) and np.all(a.nacc > 0) and np.all(a.ncall > a.nacc)
    rows = sum(len(c[1]) for c in rec.calls[1:])
    assert rows == a.ncall.sum()                                       # every evaluation went through a round, once
    for r in range(3):
        assert sum(int(np.sum(c[1] == r)) for c in rec.calls[1:]) == a.ncall[r]
    assert all(np.all(np.diff(c[1]) >= 0) and set(c[1]) <= {0, 1, 2} for c in rec.calls[1:])
    assert 6 < len(rec.calls) - 1 <= 6 * 10                            # at most `walks` rounds an iteration


def test_the_round_driver_calls_evaluate_once_per_round_of_the_longest_walk():
    """The walks of one iteration of 3 runs driven together: as many evaluate calls as the longest walk has evaluations, each
    with one row per walk still going, and the results of the walks driven one at a time."""
    lo, hi = np.array([-2.0, -1.0, -4.0]), np.array([3.0, 2.5, 1.5])
    live0 = lo + (hi - lo) * np.random.default_rng(12).random((3, 32, 3))
    s = nr.start(live0, nr.gaussian)
    g0, s3 = nr.resolve(0.0, 0.1, 3)
    jobs = nr.retire(s, 8, 1e-6)

    def gens():
        return [nr.walk_rounds(s, r, j, t, surv, lstar, 5, 10, g0, s3, lo, hi) for r, dead, surv, lstar, t in jobs for j in dead]

    runs = [r for r, dead, *_ in jobs for _ in dead]
    rec = RecordingGaussian()
    out = nr.in_rounds(gens(), runs, rec)
    one = [nr.one_at_a_time(g, nr.gaussian_one) for g in gens()]
    assert len(out) == 24 and out == one
    evals = np.array([o[4] for o in out])
    assert len(rec.calls) == evals.max() and evals.min() < evals.max()
    for k, (rows, rr) in enumerate(rec.calls):
        assert len(rows) == np.sum(evals > k) and rr.tolist() == [runs[i] for i in np.nonzero(evals > k)[0]]
    assert nr.in_rounds([], [], rec) == [] and len(rec.calls) == evals.max()


def test_stop_rule():
    assert not nr.stops(-1.0, 0.0, -np.inf, 0.01)
    assert not nr.stops(-np.inf, 0.0, -np.inf, 0.01)
    assert nr.stops(-10.0, -5.0, 0.0, 0.01)                 # log1p(e^-15) = 3e-7
    assert not nr.stops(-10.0, -5.0, -15.0, 0.01)           # log1p(1) = 0.69


@pytest.mark.parametrize("kw, match", [
    ({"nlive": 8}, "nlive"),
    ({"nlive": 5000}, "nlive"),
    ({"nlive": 64, "nbatch": 33}, "nbatch"),
    ({"nbatch": 0}, "nbatch"),
    ({"walks": 0}, "walks"),
    ({"walks": 5000}, "walks"),
    ({"sigma": 0.6}, "sigma"),
    ({"g0": np.inf}, "g0"),
    ({"n_runs": 0}, "n_runs"),
    ({"n_runs": 65}, "at most"),
    ({"variant": "other"}, "variant"),
    ({"ndim": 7}, "6 parameters"),
    ({"variant": "lib", "ndim": 10}, "6 to 9"),
    ({"bounds": [(1.0, 0.0)] * 6}, "lower < upper"),
    ({"bounds": [(0.0, 1.0)] * 5}, "pairs"),
    ({"target": "other"}, "target"),
    ({"target": "gaussian"}, "bounds"),
])
def test_argument_checks_raise_before_any_device_is_touched(monkeypatch, kw, match):
    from magprop_amd import _capi, nested

    def no_device(*a, **k):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(_capi, "lib", no_device)
    monkeypatch.setattr(_capi, "Handle", no_device)
    monkeypatch.setattr(_capi, "cfg_synth", no_device)
    monkeypatch.setattr(_capi, "cfg_lib", no_device)
    x = np.linspace(1.0, 10.0, 5)
    with pytest.raises(ValueError, match=match):
        nested.NestedSampler(x, x, x, **kw)


def test_run_arguments_are_checked_before_any_device_is_touched(monkeypatch):
    from magprop_amd import _capi, nested

    def no_device(*a, **k):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(_capi, "lib", no_device)
    monkeypatch.setattr(_capi, "Handle", no_device)
    x = np.linspace(1.0, 10.0, 5)
    s = nested.NestedSampler(x, x, x, nlive=64)
    for bad in (dict(dlogz=0.0), dict(dlogz=np.nan), dict(maxiter=-1), dict(maxiter=2.5)):
        with pytest.raises(ValueError):
            s.run_nested(**bad)
    with pytest.raises(ValueError, match="run_nested first"):
        s.resample_equal()
    with pytest.raises(ValueError, match="dataset"):
        nested.NestedSampler()


def test_header_states_the_limits_and_the_library_exports_the_entry_points():
    from magprop_amd import _capi
    hdr = open(os.path.join(ROOT, "include", "magprop_amd.h")).read()
    for name, val in (("MP_NEST_MIN_LIVE", _capi.NEST_MIN_LIVE), ("MP_NEST_MAX_LIVE", _capi.NEST_MAX_LIVE),
                      ("MP_NEST_MAX_WALKS", _capi.NEST_MAX_WALKS)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, hdr).group(1)) == val
    for name in ("mp_nested_create", "mp_nested_set_live", "mp_nested_run", "mp_nested_get_dead", "mp_nested_get_state",
                 "mp_nested_destroy"):
        assert name in _capi.EXPORTS and hasattr(_capi.lib(), name)
    import magprop_amd
    assert magprop_amd.NestedSampler is magprop_amd.nested.NestedSampler
