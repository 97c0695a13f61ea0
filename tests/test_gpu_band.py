"""GPU tests of the posterior-predictive band (mp_model_band, run with -m gpu on an MI355X): the device reduction against
np.nanquantile over the curves the existing entry points return for the same rows, bit for bit."""
import warnings

import numpy as np
import pytest

from conftest import TRUTHS

pytestmark = pytest.mark.gpu

Q7 = np.array([0.0, 0.025, 0.16, 0.5, 0.84, 0.975, 1.0])
Q3 = np.array([0.025, 0.5, 0.975])


def _nanq(curves, q):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)       # all-NaN columns
        return np.nanquantile(curves, q, axis=0)


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
    """near-truth rows, prior-wide rows, 20 outside the prior and the flagged rows of the flag scan"""
    from magprop_amd import synth
    rng = np.random.default_rng(seed)
    flag = gflag["pars"][gflag["status"] == 1]
    n_out = 20
    n_near = (n - len(flag) - n_out) // 2
    near = np.array(TRUTHS["Humped"]) + 0.02 * rng.standard_normal((n_near, 6))
    wide = synth.PRIOR_LOWER + (synth.PRIOR_UPPER - synth.PRIOR_LOWER) * rng.random((n - len(flag) - n_out - n_near, 6))
    out = np.array(TRUTHS["Humped"]) + np.zeros((n_out, 6))
    out[:, 5] = 3.5
    P = np.concatenate([near, wide, out, flag])
    return P[rng.permutation(len(P))]


def test_ltot_band_matches_nanquantile_of_lnprob_batch_curves(humped, gflag):
    from magprop_amd import _capi
    P = _rows(gflag, 1500, 1)
    band, st, used = humped.model_band(P, Q7)
    _, st_ref, lt = humped.lnprob_batch(P, ds_id=0, want_status=True, want_ltot=True)
    assert np.array_equal(st, st_ref)
    assert used == int(np.sum(st_ref == _capi.STATUS_OK))
    assert np.sum(st_ref == _capi.STATUS_FLAG) >= 12 and np.sum(st_ref == _capi.STATUS_PRIOR) >= 20
    assert _same(band[0], _nanq(lt, Q7))


def test_lprop_ldip_band_matches_model_lc(humped):
    rng = np.random.default_rng(2)
    S = np.array(TRUTHS["Humped"]) + 0.05 * rng.standard_normal((200, 6))
    Pphys = S.copy()
    Pphys[:, 2:] = 10.0 ** S[:, 2:]
    band, st, used = humped.model_band(Pphys, Q3, ("Ltot", "Lprop", "Ldip"), physical=True)
    curves = np.empty((3, 200, humped.tgrid.size))
    for i in range(200):
        s, out = humped.model_lc(Pphys[i])
        assert s == st[i]
        curves[:, i] = out[1:4] if s == 0 else np.nan
    assert used == int(np.sum(st == 0)) and used > 150
    for k in range(3):
        assert _same(band[k], _nanq(curves[k], Q3)), k


def test_band_at_the_cap(humped, gflag):
    from magprop_amd import _capi
    n = _capi.BAND_MAX_SAMPLES
    P = _rows(gflag, n, 3)
    band, st, used = humped.model_band(P, Q3)
    _, st_ref, lt = humped.lnprob_batch(P, ds_id=0, want_status=True, want_ltot=True)
    assert np.array_equal(st, st_ref) and used == int(np.sum(st_ref == 0))
    cols = np.arange(0, humped.tgrid.size, 37)
    assert _same(band[0][:, cols], _nanq(lt[:, cols], Q3))
    with pytest.raises(ValueError, match="16384"):
        humped.model_band(np.zeros((n + 1, 6)), Q3)
    L = _capi.lib()
    P1 = np.ascontiguousarray(np.repeat(P[:1], n + 1, axis=0))
    out = np.empty(humped.tgrid.size)
    q = np.array([0.5])
    assert L.mp_model_band(humped._h, _capi._dptr(P1), n + 1, 6, 0, _capi._dptr(q), 1, 1, _capi._dptr(out), None, None) == _capi.MP_EINVAL


def test_all_rows_fail(humped):
    P = np.array(TRUTHS["Humped"]) + np.zeros((64, 6))
    P[:, 0] = 50.0                                            # B outside the prior
    band, st, used = humped.model_band(P, Q3, ("Ltot", "Ldip"))
    assert used == 0 and np.all(st == 3)
    assert band.shape == (2, 3, humped.tgrid.size) and np.all(np.isnan(band))


def test_sampler_wiring(gsynth):
    from magprop_amd import EnsembleSampler, synth
    x, y, yerr = gsynth["Humped_x"], gsynth["Humped_y"], gsynth["Humped_yerr"]
    rng = np.random.default_rng(4)
    p0 = np.array(TRUTHS["Humped"]) + 1e-3 * rng.standard_normal((64, 6))
    s = EnsembleSampler(64, 6, x, y, yerr, seed=5)
    s.run_mcmc(p0, 200)
    got = s.get_model_band(discard=100, thin=5)
    rows = s.get_chain()[100::5].reshape(-1, 6)
    want = synth.model_band(rows)
    assert got["n_used"] == want["n_used"] > 0
    assert np.array_equal(got["t"], want["t"]) and _same(got["Ltot"], want["Ltot"])
    assert got["Ltot"].shape == (3, 10001)
    s.close()
    # two ensembles: ensemble=1 takes the second dataset's walkers
    xc, yc, ec = gsynth["Classic_x"], gsynth["Classic_y"], gsynth["Classic_yerr"]
    s2 = EnsembleSampler(32, 6, datasets=[(x, y, yerr), (xc, yc, ec)], seed=6)
    p2 = np.concatenate([np.array(TRUTHS["Humped"]) + 1e-3 * rng.standard_normal((32, 6)),
                         np.array(TRUTHS["Classic"]) + 1e-3 * rng.standard_normal((32, 6))])
    s2.run_mcmc(p2, 20)
    b1 = s2.get_model_band(q=(0.5,), ensemble=1)
    want1 = synth.model_band(s2.get_chain()[:, 32:].reshape(-1, 6), q=(0.5,))
    assert _same(b1["Ltot"], want1["Ltot"])
    b0 = s2.get_model_band(q=(0.5,), ensemble=0)
    assert not np.array_equal(b0["Ltot"], b1["Ltot"], equal_nan=True)
    s2.close()
    g = EnsembleSampler(8, 2, target="gaussian")
    g.run_mcmc(rng.standard_normal((8, 2)), 5)
    with pytest.raises(ValueError, match="gaussian"):
        g.get_model_band()
    g.close()


def test_multi_device_handle_matches_single(tarr, gflag):
    from magprop_amd import _capi, synth
    P = _rows(gflag, 600, 7)
    out = []
    for dev in (0, [0, 0]):
        h = _capi.Handle(_capi.cfg_synth(), tarr, device=dev)
        h.set_prior(synth.PRIOR_LOWER, synth.PRIOR_UPPER, synth.LOG_MASK)
        out.append(h.model_band(P, Q3, ("Ltot", "Lprop")))
        h.close()
    assert _same(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and out[0][2] == out[1][2]


def test_repeat_is_bitwise(humped, gflag):
    P = _rows(gflag, 700, 8)
    a = humped.model_band(P, Q7, ("Ltot", "Ldip"))
    b = humped.model_band(P, Q7, ("Ltot", "Ldip"))
    assert _same(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
