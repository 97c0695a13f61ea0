"""The bridge-sampling evidence with a Student-t proposal and with Warp-III on the device (include/magprop_amd.h
mp_bridge_logz_warp, magprop_amd.bridge, EnsembleSampler.log_evidence(method="bridge", proposal=, nu=, warp=)): the posterior
target held to mp_lnprob_batch bit for bit in the batches the header states, the brute-force evidence of
tests/test_gpu_tempering.py under the four variants, the argument codes, and the front end with and without the new arguments."""
import ctypes as C
import math

import numpy as np
import pytest

import bridge_restated as br
import bridge_warp_restated as bw
from conftest import TRUTHS
from raw_abi import dp, synth_handle
from test_gpu_bridge import BRUTE_ESS, BRUTE_FORCE, EVIDENCE_INFLATION, box_start
from test_gpu_bridge_warp_kernels import raw_warp

pytestmark = pytest.mark.gpu

VARIANTS = {"plain": dict(proposal="normal", warp=False), "warped": dict(proposal="normal", warp=True),
            "t": dict(proposal="t", nu=5, warp=False), "warped_t": dict(proposal="t", nu=5, warp=True)}


@pytest.mark.parametrize("ds", [0, 1], ids=["short", "long"])
def test_posterior_draws_and_mirrors_are_lnprob_batch_bit_for_bit(gsynth, glonglc, ds):
    """Target 0 with warp: draw_lnp and draw_mirror_lnp equal mp_lnprob_batch of the returned draws followed by the returned
    mirrors, in one batch of 2 n_rep n_draws rows; est_mirror_lnp equals mp_lnprob_batch of the estimator rows' mirrors
    m - (x - m) in one batch (n_est lies under a chunk): 256 draws x 1 (the team regime) under the Gaussian, 1 024 x 2 under
    t(5); ds 1 is a light curve of 112 points (the LONG build).  The mirror counts and n_finite equal numpy counts."""
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
    counted = lambda x, v: np.all((x >= lo) & (x <= hi), axis=1) & np.isfinite(v)
    try:
        for n_draws, n_rep, proposal in ((256, 1, "normal"), (1024, 2, "t")):
            res = h.bridge_logz(fit, est, lnp_est, lo, hi, ds_id=ds, n_draws=n_draws, n_rep=n_rep, seed=9, tol=1e-8, details=True,
                                proposal=proposal, nu=5, warp=True)
            draws, mirrors = res["draws"].reshape(-1, 6), res["draw_mirrors"].reshape(-1, 6)
            want = h.lnprob_batch(np.concatenate([draws, mirrors]), ds_id=ds)
            assert np.array_equal(res["draw_lnp"].ravel(), want[:draws.shape[0]], equal_nan=True), (ds, n_draws)
            assert np.array_equal(res["draw_mirror_lnp"].ravel(), want[draws.shape[0]:], equal_nan=True), (ds, n_draws)
            m, _, _ = br.factor(res["moments"], fit[0], fit.shape[0], 6)
            est_m = m - (est - m)
            want_est = h.lnprob_batch(est_m, ds_id=ds)
            assert np.array_equal(res["est_mirror_lnp"], want_est, equal_nan=True), (ds, n_draws)
            c_d, c_m = counted(draws, want[:draws.shape[0]]), counted(mirrors, want[draws.shape[0]:])
            out = res["out"]
            assert np.array_equal(out[:, bw.DRAW_MIRRORS], np.count_nonzero(c_m.reshape(n_rep, n_draws), axis=1))
            assert np.all(out[:, bw.EST_MIRRORS] == np.count_nonzero(counted(est_m, want_est)))
            assert np.array_equal(out[:, br.NFINITE], np.count_nonzero((c_d | c_m).reshape(n_rep, n_draws), axis=1))
            assert np.array_equal(np.isneginf(res["b"]).ravel(), ~(c_d | c_m)) and out[:, bw.DRAW_MIRRORS].sum() > 0
            assert np.all(np.isfinite(out[:, 0])) and np.all(np.isfinite(res["a"]))
            # the mirrors are the draws reflected in m
            assert np.allclose(draws + mirrors, 2.0 * m, rtol=0, atol=1e-12)
    finally:
        h.close()


def test_parity_with_the_old_entry_on_the_posterior(gsynth):
    """proposal = 0, warp = 0 through mp_bridge_logz_warp equals mp_bridge_logz on target 0, bit for bit."""
    h = synth_handle()
    lo, hi = gsynth["prior_lower"], gsynth["prior_upper"]
    h.set_prior(lo, hi, 0b111100)
    h.set_dataset(0, gsynth["Humped_x"], gsynth["Humped_y"], gsynth["Humped_yerr"])
    rng = np.random.default_rng(60)
    rows = np.clip(np.array(TRUTHS["Humped"]) + 0.05 * rng.standard_normal((600, 6)), lo + 1e-6, hi - 1e-6)
    lnp = h.lnprob_batch(rows)
    ok = np.isfinite(lnp)
    case = dict(x_fit=rows[:300], x_est=rows[300:][ok[300:]], lnp_est=lnp[300:][ok[300:]], lower=lo, upper=hi, n_draws=300, n_rep=2, seed=4,
                neff=None, max_iter=200, tol=1e-8, target=0)
    try:
        old = h.bridge_logz(case["x_fit"], case["x_est"], case["lnp_est"], lo, hi, n_draws=300, n_rep=2, seed=4, max_iter=200, tol=1e-8,
                            details=True)
        new = raw_warp(h, case, bw.NORMAL, 0, False)
        for key in ("moments", "draws", "draw_lnp", "draw_lnq", "est_lnq"):
            assert np.array_equal(new[key].ravel(), old[key].ravel(), equal_nan=True), key
        assert np.array_equal(new["out"][:, :br.NOUT], old["out"], equal_nan=True) and np.all(new["out"][:, br.NOUT:] == 0.0)
    finally:
        h.close()


def test_humped_evidence_against_brute_force_under_the_four_variants(gsynth):
    """Humped with yerr x 10 (brute force -5.5046 from an effective sample size of 160 641, as tests/test_gpu_bridge.py): that
    test's 8 sampler seeds, each run once, and the four variants taken from the same chain with the same neff; the mean ln Z of
    each variant within 4 sigma, sigma^2 = sd^2 / 8 + 1 / 160 641."""
    from magprop_amd import EnsembleSampler, KDEMove, LogProb
    x, y, yerr = gsynth["Humped_x"], gsynth["Humped_y"], gsynth["Humped_yerr"] * EVIDENCE_INFLATION
    lp = LogProb(x, y, yerr)
    res = {v: [] for v in VARIANTS}
    for seed in range(8):
        s = EnsembleSampler(512, 6, x, y, yerr, seed=1000 + seed, moves=KDEMove())
        s.run_mcmc(box_start(lp, 512, np.random.default_rng(2000 + seed)), 400)
        plain = s.log_evidence(method="bridge", discard=100)
        res["plain"].append(plain)
        for v in ("warped", "t", "warped_t"):
            res[v].append(s.log_evidence(method="bridge", discard=100, neff=plain.neff, **VARIANTS[v]))
        s.close()
    for v, rs in res.items():
        lnz = np.array([r.lnz for r in rs])
        sd = np.std(lnz, ddof=1)
        sigma = math.sqrt(sd ** 2 / 8.0 + 1.0 / BRUTE_ESS)
        print(f"Humped yerr x 10, {v}: brute force {BRUTE_FORCE}, mean {lnz.mean():.4f}, sd over seeds {sd:.4f}, mean dlnz "
              f"{np.mean([r.dlnz for r in rs]):.4f}, difference {lnz.mean() - BRUTE_FORCE:+.4f} = {(lnz.mean() - BRUTE_FORCE) / sigma:+.2f} "
              f"sigma; updates {[int(r.niter[0]) for r in rs]}, finite draws {[int(r.n_finite[0]) for r in rs]}, mirrors est "
              f"{[r.est_mirrors for r in rs]} draws {[int(r.draw_mirrors[0]) for r in rs]} of {rs[0].n_est}, lnz {np.round(lnz, 4).tolist()}")
        assert all(r.ok for r in rs), v
        assert abs(lnz.mean() - BRUTE_FORCE) < 4.0 * sigma, v
        assert all((r.proposal, r.warp) == (VARIANTS[v]["proposal"], VARIANTS[v]["warp"]) for r in rs)


def test_argument_codes(gsynth):
    """Every MP_EINVAL case the header adds, those mp_bridge_logz hands down, and its MP_ESTATE cases, on mp_bridge_logz_warp."""
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
    out = np.zeros((64, _capi.BRIDGE_WARP_NOUT))

    def call(handle=h, target=0, **kw):
        x, lnp = (x6, lnp6) if target == 0 else (x2, lnp2)
        a = dict(x_fit=x, n_fit=64, x_est=x, lnp_est=lnp, n_est=64, ndim=x.shape[1], ds_id=0, lower=lo if target == 0 else None,
                 upper=hi if target == 0 else None, n_draws=32, n_rep=1, neff=64.0, max_iter=50, tol=1e-8, out=out, proposal=1, nu=5, warp=1)
        a.update(kw)
        return L.mp_bridge_logz_warp(handle._h if handle is not None else None, dp(a["x_fit"]), a["n_fit"], dp(a["x_est"]), dp(a["lnp_est"]),
                                     a["n_est"], a["ndim"], a["ds_id"], dp(a["lower"]), dp(a["upper"]), a["n_draws"], a["n_rep"],
                                     C.c_uint64(3), C.c_double(a["neff"]), a["max_iter"], C.c_double(a["tol"]), target, a["proposal"],
                                     a["nu"], a["warp"], dp(a["out"]), *([None] * 10))

    try:
        for target in range(5):
            for proposal, warp in ((0, 0), (0, 1), (1, 0), (1, 1)):
                assert call(target=target, proposal=proposal, warp=warp) == _capi.MP_OK, (target, proposal, warp, _capi.last_error())
        assert call(target=1, proposal=0, nu=-4) == _capi.MP_OK                      # nu is read for the t proposal only
        assert call(target=1, nu=3) == _capi.MP_OK and call(target=1, nu=32) == _capi.MP_OK
        assert call(target=1, warp=1, n_draws=_capi.BRIDGE_MAX_ROWS >> 1, proposal=0) == _capi.MP_OK   # 2 n_rep n_draws at the cap
        added = [dict(proposal=2), dict(proposal=-1), dict(nu=2), dict(nu=33), dict(nu=-1), dict(warp=2), dict(warp=-1), dict(target=5),
                 dict(target=-1), dict(target=1, n_draws=(_capi.BRIDGE_MAX_ROWS >> 1) + 1), dict(target=1, n_draws=1 << 20, n_rep=3)]
        bad_row, bad_lnp, bad_box = x6.copy(), lnp6.copy(), hi.copy()
        bad_row[5, 2], bad_lnp[7], bad_box[1] = np.nan, -np.inf, lo[1]
        inf_box = hi.copy()
        inf_box[0] = np.inf
        handed_down = [dict(n_fit=7), dict(target=1, n_fit=3), dict(n_est=0), dict(n_draws=0), dict(n_rep=0), dict(n_rep=65),
                       dict(target=1, ndim=0), dict(target=1, ndim=10), dict(ndim=5), dict(x_fit=bad_row), dict(x_est=bad_row),
                       dict(lnp_est=bad_lnp), dict(neff=0.0), dict(neff=64.5), dict(neff=np.nan), dict(tol=-1e-3), dict(tol=np.nan),
                       dict(tol=np.inf), dict(max_iter=0), dict(lower=None, upper=None), dict(upper=None), dict(target=3, lower=lo[:2]),
                       dict(upper=bad_box), dict(upper=inf_box), dict(n_draws=_capi.BRIDGE_MAX_ROWS + 1, warp=0),
                       dict(n_draws=1 << 20, n_rep=8, warp=0), dict(n_fit=_capi.BRIDGE_MAX_ROWS + 1), dict(n_est=_capi.BRIDGE_MAX_ROWS + 1),
                       dict(ds_id=-1), dict(ds_id=64), dict(x_fit=None), dict(x_est=None), dict(lnp_est=None), dict(out=None), dict(handle=None)]
        for kw in added + handed_down:
            assert call(**kw) == _capi.MP_EINVAL, (kw.keys(), _capi.last_error())
        assert call(ds_id=5) == _capi.MP_ESTATE                                   # an unset dataset
        multi = _capi.Handle(_capi.cfg_synth(), engine.grid(None), device=[0])
        try:
            multi.set_prior(lo, hi, 0b111100)
            multi.set_dataset(0, gsynth["Humped_x"], gsynth["Humped_y"], gsynth["Humped_yerr"])
            assert call(handle=multi) == _capi.MP_ESTATE and call(handle=multi, target=4) == _capi.MP_ESTATE
        finally:
            multi.close()
        torque = synth_handle(dipole_torque=1)
        try:
            torque.set_prior(lo, hi, 0b111100)
            torque.set_dataset(0, gsynth["Humped_x"], gsynth["Humped_y"], gsynth["Humped_yerr"])
            assert call(handle=torque) == _capi.MP_ESTATE and call(handle=torque, target=3) == _capi.MP_OK
        finally:
            torque.close()
    finally:
        h.close()


def test_front_end_with_and_without_the_new_arguments():
    """log_evidence(method="bridge") without the new arguments is mp_bridge_logz on the two halves of the chain, to the bit, with
    rows of MP_BRIDGE_NOUT columns; with warp=True, proposal="t" it returns ok on the unit Gaussian inside the sanity band of
    tests/test_gpu_bridge.py, and is bridge_evidence with those arguments."""
    from magprop_amd import EnsembleSampler, _capi, bridge, summaries
    s = EnsembleSampler(64, 6, target="gaussian", seed=8)
    s.run_mcmc(np.random.default_rng(7).standard_normal((64, 6)), 300)
    try:
        r = s.log_evidence(method="bridge", discard=100, repetitions=2, seed=5)
        fit, est, lnp, _ = bridge.split(s.get_chain()[100:], s.get_log_prob()[100:])
        fit, est, lnp = (np.ascontiguousarray(v, dtype=np.float64) for v in (fit, est, lnp))
        tol = max(1.0e-10, 8.0 * float(np.spacing(np.max(np.abs(lnp)))))
        raw = np.zeros((2, _capi.BRIDGE_NOUT))
        rc = _capi.lib().mp_bridge_logz(s.handle._h, dp(fit), fit.shape[0], dp(est), dp(lnp), est.shape[0], 6, 0, None, None, est.shape[0], 2,
                                        C.c_uint64(5), C.c_double(r.neff), 1000, C.c_double(tol), 1, dp(raw), None, None, None, None, None)
        assert rc == _capi.MP_OK, _capi.last_error()
        assert r.out.shape == (2, _capi.BRIDGE_NOUT) and np.array_equal(r.out, raw)
        assert (r.proposal, r.nu, r.warp, r.est_mirrors) == ("normal", None, False, 0)
        w = s.log_evidence(method="bridge", discard=100, repetitions=2, seed=5, warp=True, proposal="t", neff=r.neff)
        truth = 3.0 * math.log(2.0 * math.pi)
        print(f"unit Gaussian, d = 6: truth {truth:.4f}, plain {r!r}, warped t {w!r}")
        assert w.ok and abs(w.lnz - truth) < 0.5 and w.out.shape == (2, _capi.BRIDGE_WARP_NOUT)
        assert (w.proposal, w.nu, w.warp) == ("t", 5, True) and w.est_mirrors == w.n_est and w.draw_mirrors.tolist() == [w.n_draws] * 2
        by_hand = bridge.bridge_evidence(fit, est, lnp, summaries.on(s.handle), repetitions=2, seed=5, neff=r.neff, target=1, proposal="t",
                                         nu=5, warp=True)
        assert np.array_equal(by_hand.out, w.out)
        with pytest.raises(ValueError, match="nu"):
            s.log_evidence(method="bridge", discard=100, proposal="t", nu=2)
    finally:
        s.close()
