"""GPU tests of the weighted band (mp_model_band_weighted, run with -m gpu on an MI355X): the device reduction against the
restatement (tests/wband_restated.py) applied to the curves the existing entry points return for the same rows, bit for bit."""
import warnings

import numpy as np
import pytest

import wband_restated as wr
from conftest import TRUTHS

pytestmark = pytest.mark.gpu

Q7 = np.array([0.0, 0.025, 0.16, 0.5, 0.84, 0.975, 1.0])
Q3 = np.array([0.025, 0.5, 0.975])


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a), np.signbit(b))


@pytest.fixture(scope="module")
def humped(tarr, gsynth):
    from magprop_amd import _capi, synth
    h = _capi.Handle(_capi.cfg_synth(), tarr)
    h.set_dataset(0, gsynth["Humped_x"], gsynth["Humped_y"], gsynth["Humped_yerr"])
    h.set_prior(synth.PRIOR_LOWER, synth.PRIOR_UPPER, synth.LOG_MASK)
    yield h
    h.close()


def _rows(gflag, n, seed):
    """n rows in sampler coordinates: near the truth and prior-wide, and from n = 2 on a fifth of them flagged rows of the flag
    scan and an eighth outside the prior, shuffled"""
    from magprop_amd import synth
    rng = np.random.default_rng(seed)
    flag = gflag["pars"][gflag["status"] == 1]
    n_flag, n_out = min(len(flag), (n + 3) // 5 if n > 1 else 0), n // 8
    n_near = (n - n_flag - n_out + 1) // 2
    near = np.array(TRUTHS["Humped"]) + 0.02 * rng.standard_normal((n_near, 6))
    wide = synth.PRIOR_LOWER + (synth.PRIOR_UPPER - synth.PRIOR_LOWER) * rng.random((n - n_flag - n_out - n_near, 6))
    out = np.array(TRUTHS["Humped"]) + np.zeros((n_out, 6))
    out[:, 5] = 3.5
    P = np.concatenate([near, wide, out, flag[:n_flag]])
    assert P.shape == (n, 6)
    return P[rng.permutation(n)], rng.permutation(np.exp(3.0 * rng.standard_normal(n)))


@pytest.mark.parametrize("n", [1, 2, 65, 300])
def test_weighted_ltot_band_is_the_restatement_of_lnprob_batch_curves(humped, gflag, n):
    from magprop_amd import _capi
    P, w = _rows(gflag, n, 10 + n)
    band, st, used = humped.model_band(P, Q7, weights=w)
    _, st_ref, lt = humped.lnprob_batch(P, ds_id=0, want_status=True, want_ltot=True)
    assert np.array_equal(st, st_ref) and used == int(np.sum(st_ref == _capi.STATUS_OK)) and used >= 1
    if n >= 65:
        assert np.sum(st_ref == _capi.STATUS_FLAG) >= 12 and np.sum(st_ref == _capi.STATUS_PRIOR) >= 8
    elif n == 2:
        assert np.sum(st_ref == _capi.STATUS_FLAG) == 1
    assert np.all(np.isnan(lt[st_ref != _capi.STATUS_OK]))
    units = _capi.band_weight_units(w)
    assert np.array_equal(units, wr.weight_units(w))
    assert band.shape == (1, 7, humped.tgrid.size) and _same(band[0], wr.weighted_band(lt.T, units, Q7))
    assert not np.any(np.isnan(band))


def test_weighted_lprop_ldip_band_matches_model_lc(humped, gflag):
    rng = np.random.default_rng(2)
    S = np.concatenate([np.array(TRUTHS["Humped"]) + 0.05 * rng.standard_normal((58, 6)), gflag["pars"][gflag["status"] == 1][:7]])
    S = S[rng.permutation(65)]
    Pphys = S.copy()
    Pphys[:, 2:] = 10.0 ** S[:, 2:]
    w = np.exp(3.0 * rng.standard_normal(65))
    band, st, used = humped.model_band(Pphys, Q3, ("Ltot", "Lprop", "Ldip"), physical=True, weights=w)
    curves = np.empty((3, 65, humped.tgrid.size))
    for i in range(65):
        s, out = humped.model_lc(Pphys[i])
        assert s == st[i]
        curves[:, i] = out[1:4] if s == 0 else np.nan
    assert used == int(np.sum(st == 0)) and 50 <= used < 65
    units = wr.weight_units(w)
    for k in range(3):
        assert _same(band[k], wr.weighted_band(curves[k].T, units, Q3)), k


def test_equal_weights_are_inverted_cdf_and_the_unweighted_band_is_unchanged(humped, gflag):
    P, _ = _rows(gflag, 300, 5)
    _, st_ref, lt = humped.lnprob_batch(P, ds_id=0, want_status=True, want_ltot=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        want_w = np.nanquantile(lt, Q7, axis=0, method="inverted_cdf")
        want_u = np.nanquantile(lt, Q7, axis=0)
    for weights in (np.ones(300), np.full(300, 0.3)):
        band, st, _ = humped.model_band(P, Q7, weights=weights)
        assert np.array_equal(st, st_ref) and _same(band[0], want_w)
    plain, st, used = humped.model_band(P, Q7)                 # what it was: numpy's method "linear"
    assert np.array_equal(st, st_ref) and used == int(np.sum(st_ref == 0)) and _same(plain[0], want_u)
    assert not np.array_equal(plain[0], want_w)


def test_no_finished_row_and_no_weight_on_the_finished_rows(humped, gflag):
    P = np.array(TRUTHS["Humped"]) + np.zeros((64, 6))
    P[:, 0] = 50.0                                            # B outside the prior
    band, st, used = humped.model_band(P, Q3, ("Ltot", "Ldip"), weights=np.arange(1.0, 65.0))
    assert used == 0 and np.all(st == 3)
    assert band.shape == (2, 3, humped.tgrid.size) and np.all(np.isnan(band))
    # every unit on rows that fail
    P, w = _rows(gflag, 65, 6)
    st = humped.lnprob_batch(P, ds_id=0, want_status=True)[1]
    w[st == 0] = 0.0
    w[np.nonzero(st == 0)[0][:3]] = np.max(w) * 2.0 ** -32    # (weight, but below one unit)
    band, st2, used = humped.model_band(P, Q3, weights=w)
    assert np.array_equal(st, st2) and used == int(np.sum(st == 0)) > 0 and np.all(np.isnan(band))
    with pytest.raises(ValueError, match="finite"):
        humped.model_band(P, Q3, weights=np.zeros(65))
    with pytest.raises(ValueError, match="shape"):
        humped.model_band(P, Q3, weights=np.ones(64))


def test_repeat_is_bitwise(humped, gflag):
    P, w = _rows(gflag, 300, 8)
    a = humped.model_band(P, Q7, ("Ltot", "Ldip"), weights=w)
    b = humped.model_band(P, Q7, ("Ltot", "Ldip"), weights=w)
    assert _same(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


def test_sampler_and_module_wiring(gsynth):
    from magprop_amd import EnsembleSampler, _capi, summaries, synth
    x, y, yerr = gsynth["Humped_x"], gsynth["Humped_y"], gsynth["Humped_yerr"]
    rng = np.random.default_rng(4)
    p0 = np.array(TRUTHS["Humped"]) + 1e-3 * rng.standard_normal((32, 6))
    s = EnsembleSampler(32, 6, x, y, yerr, seed=5)
    s.run_mcmc(p0, 10)
    rows = s.get_chain()[2::2].reshape(-1, 6)
    w = np.exp(rng.standard_normal(rows.shape[0]))
    got = s.get_model_band(discard=2, thin=2, weights=w)
    want = synth.model_band(rows, weights=w)
    assert got["n_used"] == want["n_used"] == rows.shape[0] and _same(got["Ltot"], want["Ltot"]) and np.array_equal(got["t"], want["t"])
    assert got["n_eff"] == want["n_eff"] == float(np.sum(w)) ** 2 / float(np.sum(w * w))
    assert "n_eff" not in s.get_model_band(discard=2, thin=2)
    with pytest.raises(ValueError, match="shape"):
        s.get_model_band(discard=2, thin=2, weights=w[:-1])
    direct = summaries.band(summaries.on(s.handle), rows, Q3, ("Ltot",), w)
    assert _same(direct["Ltot"], got["Ltot"])
    s.close()
    # the library variant: mcmc_eqns.model_band is the handle's band under the variant's prior box
    from magprop_amd import engine, mcmc_eqns
    S = np.array(TRUTHS["Humped"]) + 0.01 * np.abs(rng.standard_normal((16, 6)))
    wl = np.exp(rng.standard_normal(16))
    a = mcmc_eqns.model_band(S, "L", q=Q3, components=("Ltot", "Ldip"), weights=wl)
    lo, hi = mcmc_eqns._bounds(6)
    with engine.use(_capi.cfg_lib(), "L", -1) as eng:
        eng.set_prior(lo, hi, mcmc_eqns.LIB_LOG_MASK)
        b = summaries.band(summaries.on(eng.handle), S, Q3, ("Ltot", "Ldip"), wl)
    assert a["n_used"] == b["n_used"] >= 1 and a["n_eff"] == b["n_eff"] and _same(a["Ltot"], b["Ltot"]) and _same(a["Ldip"], b["Ldip"])
    assert set(mcmc_eqns.model_band(S, "L", q=Q3)) == {"t", "Ltot", "n_used"}


def test_nested_sampler_exact_band(gsynth):
    """A short nested run (the smallest live set the nested tests use): weights="exact" is summaries.band on the documented row
    selection, a function of the run alone; the default call is what it was."""
    from magprop_amd import NestedSampler, _capi, nested, summaries
    x, y, yerr = gsynth["Humped_x"], gsynth["Humped_y"], gsynth["Humped_yerr"]
    s = NestedSampler(x, y, yerr, nlive=64, nbatch=16, seed=3)
    res = s.run_nested(dlogz=0.5, maxiter=30)
    got = s.get_model_band(weights="exact")
    w = np.exp(res.logwt - np.max(res.logwt))
    keep = np.floor(w * 2.0 ** 31) > 0
    assert 1 <= keep.sum() <= len(w) <= _capi.BAND_MAX_SAMPLES
    rows, wsel, dropped = nested.band_exact_selection(res.samples, res.logwt)
    assert np.array_equal(rows, res.samples[keep]) and np.array_equal(wsel, w[keep]) and dropped == 0.0
    want = summaries.band(summaries.on(s.handle), res.samples[keep], Q3, ("Ltot",), w[keep])
    assert _same(got["Ltot"], want["Ltot"]) and got["n_used"] == want["n_used"] > 0 and got["n_eff"] == want["n_eff"] > 0.0
    assert got["weight_dropped"] == 0.0 and got["Ltot"].shape == (3, 10001)
    assert _same(s.get_model_band(weights="exact")["Ltot"], got["Ltot"])
    # the default: the equal-weight resample, as before
    default = s.get_model_band()
    eq = s.resample_equal()
    old = summaries.band(summaries.on(s.handle), eq, Q3, ("Ltot",))
    assert set(default) == {"t", "Ltot", "n_used"} and _same(default["Ltot"], old["Ltot"]) and default["n_used"] == old["n_used"]
    assert _same(s.get_model_band(weights="resample")["Ltot"], default["Ltot"])
    s.close()
