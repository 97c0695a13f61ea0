"""The bridge-sampling evidence on the device (include/magprop_amd.h mp_bridge_logz, magprop_amd.bridge,
EnsembleSampler.log_evidence(method="bridge")): the posterior target held to mp_lnprob_batch bit for bit, the brute-force
evidence of tests/test_gpu_tempering.py, the reservoir path, repetitions, the argument codes, and the unchanged default of
log_evidence."""
import ctypes as C
import math

import numpy as np
import pytest

from conftest import TRUTHS
from raw_abi import dp, synth_handle

pytestmark = pytest.mark.gpu

EVIDENCE_INFLATION = 10.0                 # tests/test_gpu_tempering.py: Humped with yerr x 10 ...
BRUTE_FORCE, BRUTE_ESS = -5.5046, 160641  # ... its brute-force ln Z and the effective sample size behind it


def box_start(lp, n, rng):
    """n uniform draws of the prior box at which the model succeeds"""
    from magprop_amd import synth
    lo, hi = synth.PRIOR_LOWER, synth.PRIOR_UPPER
    start = lo + (hi - lo) * rng.random((4 * n, 6))
    start = start[np.isfinite(lp(start))][:n]
    assert start.shape[0] == n
    return start


@pytest.mark.parametrize("ds", [0, 1], ids=["short", "long"])
def test_posterior_draws_are_lnprob_batch_bit_for_bit(gsynth, glonglc, ds):
    """draw_lnp of target 0 equals mp_lnprob_batch of the returned draws, row for row in a batch of the call's size: 256 rows
    (the team regime) and 2 048; ds 1 is a light curve of 112 points (the LONG build)."""
    h = synth_handle()
    lo, hi = gsynth["prior_lower"], gsynth["prior_upper"]
    h.set_prior(lo, hi, 0b111100)
    h.set_dataset(0, gsynth["Humped_x"], gsynth["Humped_y"], gsynth["Humped_yerr"])
    h.set_dataset(1, *glonglc["synth112_ds"])
    rng = np.random.default_rng(50 + ds)
    rows = np.clip(np.array(TRUTHS["Humped"]) + 0.05 * rng.standard_normal((600, 6)), lo + 1e-6, hi - 1e-6)
    lnp = h.lnprob_batch(rows, ds_id=ds)
    ok = np.isfinite(lnp)
    fit, est, lnp_est = rows[:300], rows[300:][ok[300:]], lnp[300:][ok[300:]]
    assert est.shape[0] >= 200
    try:
        for n_draws, n_rep in ((256, 1), (1024, 2)):
            res = h.bridge_logz(fit, est, lnp_est, lo, hi, ds_id=ds, n_draws=n_draws, n_rep=n_rep, seed=9, tol=1e-8, details=True)
            draws = res["draws"].reshape(-1, 6)
            want = h.lnprob_batch(draws, ds_id=ds)
            assert np.array_equal(res["draw_lnp"].ravel(), want, equal_nan=True), (ds, n_draws)
            assert np.count_nonzero(np.isfinite(want)) > 0
            inside = np.all((draws >= lo) & (draws <= hi), axis=1)
            assert res["out"][:, 6].sum() == np.count_nonzero(inside & np.isfinite(want))
            assert np.all(np.isfinite(res["out"][:, 0]))
    finally:
        h.close()


def test_humped_evidence_against_brute_force(gsynth):
    """Humped with yerr x 10, the brute-force case of tests/test_gpu_tempering.py (-5.5046 from an effective sample size of
    160 641): 8 sampler seeds, each 512 walkers with the KDE move for 400 steps from box draws, the first 100 discarded, and
    log_evidence(method="bridge") of each; the mean ln Z within 4 sigma, sigma^2 = sd^2 / 8 + 1 / 160 641, as
    tests/test_gpu_smc.py holds the SMC sampler."""
    from magprop_amd import EnsembleSampler, KDEMove, LogProb
    x, y, yerr = gsynth["Humped_x"], gsynth["Humped_y"], gsynth["Humped_yerr"] * EVIDENCE_INFLATION
    lp = LogProb(x, y, yerr)
    res = []
    for seed in range(8):
        s = EnsembleSampler(512, 6, x, y, yerr, seed=1000 + seed, moves=KDEMove())
        s.run_mcmc(box_start(lp, 512, np.random.default_rng(2000 + seed)), 400)
        res.append(s.log_evidence(method="bridge", discard=100))
        s.close()
    lnz = np.array([r.lnz for r in res])
    sd = np.std(lnz, ddof=1)
    sigma = math.sqrt(sd ** 2 / 8.0 + 1.0 / BRUTE_ESS)
    print(f"Humped yerr x 10: brute force {BRUTE_FORCE}, bridge mean {lnz.mean():.4f}, sd over seeds {sd:.4f}, mean dlnz "
          f"{np.mean([r.dlnz for r in res]):.4f}, sigma {sigma:.4f}, difference {lnz.mean() - BRUTE_FORCE:+.4f} = "
          f"{(lnz.mean() - BRUTE_FORCE) / sigma:+.2f} sigma; updates {[int(r.niter[0]) for r in res]}, neff "
          f"{[round(r.neff) for r in res]} of {res[0].n_est}, finite draws {[int(r.n_finite[0]) for r in res]}, importance sampling "
          f"{np.round([r.lnz_is[0] for r in res], 4).tolist()}, lnz {np.round(lnz, 4).tolist()}")
    assert all(r.ok for r in res)
    assert abs(lnz.mean() - BRUTE_FORCE) < 4.0 * sigma


def test_reservoir_path_agrees_with_the_stored_chain(gsynth):
    """An unstored run_mcmc_until with monitor_samples(4096) ends with an evidence (source="reservoir") that agrees with the
    stored-chain estimate of the same run (the same seed and start, stored) within 4 x their combined dlnz."""
    from magprop_amd import EnsembleSampler, KDEMove, LogProb
    x, y, yerr = gsynth["Humped_x"], gsynth["Humped_y"], gsynth["Humped_yerr"] * EVIDENCE_INFLATION
    start = box_start(LogProb(x, y, yerr), 256, np.random.default_rng(31))
    out = {}
    for store in (False, True):
        s = EnsembleSampler(256, 6, x, y, yerr, seed=32, moves=KDEMove())
        s.run_mcmc(start, 100, store=False)
        s.monitor_autocorr(256)
        s.monitor_samples(4096)
        s.run_mcmc_until(None, 300, check_every=100, store=store)
        if store:
            out["chain"] = s.log_evidence(method="bridge")
            assert s.get_chain().shape[0] == s.iteration - 100
        else:
            assert s.get_chain() is None
            out["reservoir"] = s.log_evidence(method="bridge", source="reservoir")
            with pytest.raises(ValueError, match="reservoir"):
                s.log_evidence(method="bridge", source="reservoir", discard=5)
            with pytest.raises(ValueError, match="chain is empty"):
                s.log_evidence(method="bridge")
        s.close()
    a, b = out["reservoir"], out["chain"]
    print(f"reservoir {a!r}\nchain     {b!r}")
    assert a.ok and b.ok and a.n_est >= 2048 and a.neff <= a.n_est
    assert abs(a.lnz - b.lnz) < 4.0 * math.hypot(a.dlnz, b.dlnz)


def test_repetitions_and_seeds():
    """repetitions=4 returns four statuses OK; the same seed gives the same bits, another seed other draws; the repetitions differ
    by their draws alone."""
    from magprop_amd import EnsembleSampler, bridge, summaries
    s = EnsembleSampler(64, 6, target="gaussian", seed=8)
    s.run_mcmc(np.random.default_rng(7).standard_normal((64, 6)), 300)
    try:
        r = s.log_evidence(method="bridge", discard=100, repetitions=4, seed=5)
        again = s.log_evidence(method="bridge", discard=100, repetitions=4, seed=5)
        other = s.log_evidence(method="bridge", discard=100, repetitions=4, seed=6)
        assert r.status.tolist() == [0, 0, 0, 0] and r.ok and len(r.reps) == 4
        assert np.array_equal(r.out, again.out) and not np.array_equal(r.out[:, 0], other.out[:, 0])
        assert len(set(r.lnz_reps.tolist())) == 4 and r.lnz == np.median(r.lnz_reps) and r.dlnz_reps == np.std(r.lnz_reps)
        lnz, dlnz = r
        truth = 3.0 * math.log(2.0 * math.pi)
        print(f"unit Gaussian, d = 6: truth {truth:.4f}, {r!r}, spread over the repetitions {r.dlnz_reps:.4f}")
        assert lnz == r.lnz and dlnz == r.dlnz and abs(lnz - truth) < 0.5          # (a sanity band, not the test of the estimate)
        # the front end is bridge_evidence on the two halves of the chain
        fit, est, lnp, _ = bridge.split(s.get_chain()[100:], s.get_log_prob()[100:])
        by_hand, det = bridge.bridge_evidence(fit, est, lnp, summaries.on(s.handle), repetitions=4, seed=5, neff=r.neff, target=1,
                                              details=True)
        assert np.array_equal(by_hand.out, r.out)
        _, det6 = bridge.bridge_evidence(fit, est, lnp, summaries.on(s.handle), repetitions=4, seed=6, neff=r.neff, target=1, details=True)
        assert not np.array_equal(det["draws"], det6["draws"]) and not np.array_equal(det["draws"][0], det["draws"][1])
        assert np.array_equal(det["moments"], det6["moments"]) and np.array_equal(det["est_lnq"], det6["est_lnq"])
        with pytest.raises(ValueError, match="method"):
            s.log_evidence(method="laplace")
        with pytest.warns(RuntimeWarning, match="autocorrelation"):
            s.log_evidence(method="bridge", discard=296)
    finally:
        s.close()


def test_argument_codes(gsynth):
    """Every MP_EINVAL and MP_ESTATE case of the header."""
    from magprop_amd import _capi, engine
    L = _capi.lib()
    h = synth_handle()
    lo, hi = np.ascontiguousarray(gsynth["prior_lower"]), np.ascontiguousarray(gsynth["prior_upper"])
    h.set_prior(lo, hi, 0b111100)
    h.set_dataset(0, gsynth["Humped_x"], gsynth["Humped_y"], gsynth["Humped_yerr"])
    rng = np.random.default_rng(1)
    x6 = np.ascontiguousarray(np.clip(np.array(TRUTHS["Humped"]) + 0.01 * rng.standard_normal((64, 6)), lo, hi))
    lnp6 = h.lnprob_batch(x6)
    assert np.all(np.isfinite(lnp6))
    x2 = np.ascontiguousarray(rng.standard_normal((64, 2)))
    lnp2 = -0.5 * np.sum(x2 * x2, axis=1)
    out = np.zeros((64, _capi.BRIDGE_NOUT))

    def call(handle=h, target=0, **kw):
        x, lnp = (x6, lnp6) if target == 0 else (x2, lnp2)
        a = dict(x_fit=x, n_fit=64, x_est=x, lnp_est=lnp, n_est=64, ndim=x.shape[1], ds_id=0, lower=lo if target == 0 else None,
                 upper=hi if target == 0 else None, n_draws=32, n_rep=1, neff=64.0, max_iter=50, tol=1e-8, out=out)
        a.update(kw)
        return L.mp_bridge_logz(handle._h if handle is not None else None, dp(a["x_fit"]), a["n_fit"], dp(a["x_est"]), dp(a["lnp_est"]),
                                a["n_est"], a["ndim"], a["ds_id"], dp(a["lower"]), dp(a["upper"]), a["n_draws"], a["n_rep"],
                                C.c_uint64(3), C.c_double(a["neff"]), a["max_iter"], C.c_double(a["tol"]), target, dp(a["out"]),
                                None, None, None, None, None)

    try:
        assert call() == _capi.MP_OK and call(target=1) == _capi.MP_OK and call(target=2) == _capi.MP_OK, _capi.last_error()
        bad_row, bad_lnp, bad_box = x6.copy(), lnp6.copy(), hi.copy()
        bad_row[5, 2], bad_lnp[7], bad_box[1] = np.nan, -np.inf, lo[1]
        inf_box = hi.copy()
        inf_box[0] = np.inf
        einval = [dict(n_fit=7), dict(target=1, n_fit=3), dict(n_est=0), dict(n_draws=0), dict(n_rep=0), dict(n_rep=65),
                  dict(target=1, ndim=0), dict(target=1, ndim=10), dict(ndim=5), dict(x_fit=bad_row), dict(x_est=bad_row),
                  dict(lnp_est=bad_lnp), dict(neff=0.0), dict(neff=64.5), dict(neff=np.nan), dict(tol=-1e-3), dict(tol=np.nan),
                  dict(tol=np.inf), dict(max_iter=0), dict(lower=None, upper=None), dict(upper=None), dict(target=1, lower=lo[:2]),
                  dict(upper=bad_box), dict(upper=inf_box), dict(n_draws=_capi.BRIDGE_MAX_ROWS + 1), dict(n_draws=1 << 20, n_rep=8),
                  dict(n_fit=_capi.BRIDGE_MAX_ROWS + 1), dict(n_est=_capi.BRIDGE_MAX_ROWS + 1), dict(target=3), dict(target=-1),
                  dict(ds_id=-1), dict(ds_id=64), dict(x_fit=None), dict(x_est=None), dict(lnp_est=None), dict(out=None), dict(handle=None)]
        for kw in einval:
            assert call(**kw) == _capi.MP_EINVAL, (kw.keys(), _capi.last_error())
        assert call(ds_id=5) == _capi.MP_ESTATE                                   # an unset dataset
        multi = _capi.Handle(_capi.cfg_synth(), engine.grid(None), device=[0])
        try:
            multi.set_prior(lo, hi, 0b111100)
            multi.set_dataset(0, gsynth["Humped_x"], gsynth["Humped_y"], gsynth["Humped_yerr"])
            assert call(handle=multi) == _capi.MP_ESTATE and call(handle=multi, target=1) == _capi.MP_ESTATE
        finally:
            multi.close()
        torque = synth_handle(dipole_torque=1)
        try:
            torque.set_prior(lo, hi, 0b111100)
            torque.set_dataset(0, gsynth["Humped_x"], gsynth["Humped_y"], gsynth["Humped_yerr"])
            assert call(handle=torque) == _capi.MP_ESTATE and call(handle=torque, target=1) == _capi.MP_OK
        finally:
            torque.close()
    finally:
        h.close()


def test_default_log_evidence_is_unchanged(gsynth):
    """log_evidence() without method on a small tempered run is tempering's estimator on the stored chain plus the validity
    term of the same box draws, to the bit; method="bridge" of a tempered sampler takes its cold chain."""
    from magprop_amd import EnsembleSampler, bridge, summaries, synth, tempering
    x, y, yerr = gsynth["Humped_x"], gsynth["Humped_y"], gsynth["Humped_yerr"] * EVIDENCE_INFLATION
    betas = tempering.geometric_ladder(4, 1e-2)
    s = EnsembleSampler(16, 6, x, y, yerr, seed=13, betas=betas)
    try:
        s.run_mcmc(np.array(TRUTHS["Humped"]) + 1.0e-3 * np.random.default_rng(3).standard_normal((4 * 16, 6)), 60)
        got = s.log_evidence(discard=20, prior_draws=4096)
        lnl = s.get_log_prob()[20:].reshape(-1, 1, 4, 16)[:, 0]
        ti, dti = tempering.ti_log_evidence(betas, lnl.transpose(1, 0, 2).reshape(4, -1).mean(axis=1))
        lo, hi = synth.PRIOR_LOWER, synth.PRIOR_UPPER
        lp = s.handle.lnprob_batch(lo + (hi - lo) * np.random.default_rng(13).random((4096, 6)), ds_id=0)
        lnf, dlnf = tempering.validity_term(int(np.count_nonzero(np.isfinite(lp))), 4096)
        assert got == (ti + lnf, float(np.hypot(dti, dlnf)))
        assert s.log_evidence(20, 0, 4096, False) == got and s.log_evidence(discard=20, prior_draws=4096, method="ti") == got
        r = s.log_evidence(method="bridge", discard=20, seed=3, neff=40.0)
        fit, est, lnp, _ = bridge.split(s.get_chain(temp=0)[20:], s.get_log_prob(temp=0)[20:])
        by_hand = bridge.bridge_evidence(fit, est, lnp, summaries.on(s.handle), lo, hi, seed=3, neff=40.0)
        assert np.array_equal(r.out, by_hand.out, equal_nan=True) and r.n_est == 20 * 16
    finally:
        s.close()
