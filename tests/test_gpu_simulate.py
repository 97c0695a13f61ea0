"""GPU tests of the simulated light curves end to end (mp_simulate, run with -m gpu on an MI355X): the reference's recipe on the
four canonical parameter sets against mp_model_lc bit for bit; independence of the chunking; the noise against the restatement
(tests/simulate_restated.py, with the device runtime's log, cos, sin and sqrt) and against the normal law; a failed row; every
return code; the front ends, the CSV and the sampler.

How a row keeps its index when it is simulated alone.  A row's noise is keyed by its index i in the call, its model is not.  So
every row of the big call is simulated alone at index 0 and its model and error are compared; its normals are compared with the
restatement under index i (a function of seed, i and j alone); and rows 1, n_simd - 1 and n_simd -- the last of the first chunk
and the first of the second -- are simulated again at their own index in a call padded in front with i copies of one fixed row,
all outputs compared."""
import ctypes as C
import os

import numpy as np
import pytest
from scipy import stats

from conftest import CANON, TRUTHS, TYPES

import simulate_restated as sr
from raw_abi import dp, ip
from test_gpu_simulate_kernels import libm, same  # noqa: F401  (libm: the device runtime's functions, a module fixture)

pytestmark = pytest.mark.gpu

FLAGS = [1.8171068, 3.68147895, -2.61786801, 1.99840102, -0.33083576, 2.95613803]   # sampler coordinates: reaches break-up


def _unlog(S):
    P = np.array(S, dtype=np.float64, ndmin=2)
    P[:, 2:6] = 10.0 ** P[:, 2:6]
    return P


@pytest.fixture(scope="module")
def handle(tarr):
    from magprop_amd import _capi, synth
    h = _capi.Handle(_capi.cfg_synth(), tarr)
    h.set_prior(synth.PRIOR_LOWER, synth.PRIOR_UPPER, synth.LOG_MASK)
    yield h
    h.close()


def test_reference_recipe_on_the_canonical_sets(handle, tarr):
    """grid-index times: the model is mp_model_lc's Ltot at those indices and yerr = 0.25 * model, bit for bit"""
    inx = np.sort(np.random.default_rng(3).integers(0, tarr.size, 50))
    inx[0], inx[-1] = 0, tarr.size - 1                                   # both ends of the grid
    P = np.array([CANON[t] for t in TYPES])
    out = handle.simulate(P, tarr[inx], seed=5, physical=True)
    assert out["n_ok"] == 4 and not np.any(out["status"])
    for k, t in enumerate(TYPES):
        st, lc = handle.model_lc(P[k])
        assert st == 0
        assert same(out["model"][k], lc[1][inx]), t
        assert same(out["yerr"][k], 0.25 * lc[1][inx]), t
        assert same(out["y"][k], out["model"][k] + out["yerr"][k] * out["z"][k]), t
    # per-row times (each set at its own indices) give the same cells as four calls
    rows = np.stack([np.sort(np.random.default_rng(10 + k).integers(0, tarr.size, 50)) for k in range(4)])
    per = handle.simulate(P, tarr[rows], seed=5, physical=True)
    for k in range(4):
        assert same(per["model"][k], handle.model_lc(P[k])[1][1][rows[k]])
        assert same(per["z"][k], out["z"][k])                            # the noise is keyed by row and observation, not by the times


def test_nothing_depends_on_the_chunking(handle, tarr, libm):  # noqa: F811
    n_simd = handle.n_simd
    n, n_obs, seed = n_simd + 1, 9, 77
    rng = np.random.default_rng(8)
    P = np.array(TRUTHS["Humped"]) + 0.02 * rng.standard_normal((n, 6))
    x = np.exp(rng.uniform(np.log(tarr[0]), np.log(tarr[-1]), n_obs))
    x[3] = tarr[1234]
    big = handle.simulate(P, x, seed=seed)
    assert big["n_ok"] == n
    for i in range(n):                                                   # alone, at index 0: model and error
        one = handle.simulate(P[i:i + 1], x, seed=seed)
        assert same(one["model"][0], big["model"][i]) and same(one["yerr"][0], big["yerr"][i]), i
        if i == 0:
            assert same(one["y"][0], big["y"][0]) and same(one["z"][0], big["z"][0])
    want = np.stack([sr.normals(seed, i, n_obs, libm) for i in range(n)])   # the normals under the row's index
    assert same(big["z"], want)
    assert same(big["y"], big["model"] + big["yerr"] * big["z"])
    for i in (1, n_simd - 1, n_simd):                                    # alone at its own index, behind i copies of a fixed row
        pad = handle.simulate(np.concatenate([np.repeat(P[:1], i, axis=0), P[i:i + 1]]), x, seed=seed)
        for k in ("y", "yerr", "model", "z"):
            assert same(pad[k][i], big[k][i]), (i, k)
    # per-row times and given errors: the whole call against the two chunks as calls of their own is not possible (the index), so
    # against the shared-times call row by row where the times agree
    xr = np.repeat(x[None, :], n, axis=0)
    ye = rng.uniform(0.1, 1.0, (n, n_obs))
    per = handle.simulate(P, xr, yerr=ye, seed=seed)
    assert same(per["model"], big["model"]) and same(per["z"], big["z"]) and same(per["yerr"], ye)
    assert same(per["y"], big["model"] + ye * big["z"])


def test_noise_is_standard_normal(handle, tarr):
    n, n_obs = 2048, 50
    rng = np.random.default_rng(1)
    P = np.array(TRUTHS["Humped"]) + 0.02 * rng.standard_normal((n, 6))
    x = tarr[np.sort(rng.integers(0, tarr.size, n_obs))]
    a = handle.simulate(P, x, seed=123)
    ok = a["status"] == 0
    r = ((a["y"] - a["model"]) / a["yerr"])[ok].ravel()
    N = r.size
    assert N >= 100000
    ks = stats.kstest(r, "norm").statistic
    print(f"noise: N {N}, mean {r.mean():.2e}, var - 1 {r.var() - 1.0:.2e}, KS {ks:.2e}")
    assert abs(r.mean()) < 5.0 / np.sqrt(N) and abs(r.var() - 1.0) < 5.0 * np.sqrt(2.0 / N)
    assert ks < stats.kstwo.ppf(0.999, N)
    assert np.max(np.abs(r - a["z"][ok].ravel())) < 1.0e-12              # (y - model) / yerr gives z back to rounding
    b = handle.simulate(P[:64], x, seed=123)
    c = handle.simulate(P[:64], x, seed=124)
    assert same(b["y"], a["y"][:64]) and same(b["z"], a["z"][:64])
    assert not np.any(c["z"] == b["z"]) and same(c["model"], b["model"])


def test_a_failed_row_is_nan_with_its_status(handle, tarr):
    from magprop_amd import _capi
    P = np.array([TRUTHS["Humped"], FLAGS, TRUTHS["Classic"], [50.0, 5.0, -3.0, 2.0, -1.0, 0.0]])
    out = handle.simulate(P, tarr[[0, 10, 5000, 10000]], seed=1)
    assert list(out["status"]) == [_capi.STATUS_OK, _capi.STATUS_FLAG, _capi.STATUS_OK, _capi.STATUS_PRIOR] and out["n_ok"] == 2
    for k in ("y", "yerr", "model", "z"):
        assert np.all(np.isnan(out[k][[1, 3]])) and np.all(np.isfinite(out[k][[0, 2]]))
    phys = handle.simulate(_unlog([TRUTHS["Humped"], FLAGS]), tarr[[0, 10]], seed=1, physical=True)
    assert list(phys["status"]) == [_capi.STATUS_OK, _capi.STATUS_FLAG]


def test_return_codes(handle, tarr):
    from magprop_amd import _capi, synth
    L = _capi.lib()
    P = np.ascontiguousarray(np.array([TRUTHS["Humped"]] * 2))
    x = np.ascontiguousarray(tarr[[5, 50]])
    y = np.empty((2, 2))
    st, ok = np.empty(2, dtype=np.int32), C.c_int64(0)

    def call(h=handle._h, pars=P, n=2, ndim=6, xx=x, n_obs=2, x_rows=1, yerr=None, frac=0.25, yo=y):
        return L.mp_simulate(h, dp(pars), n, ndim, 0, dp(xx), n_obs, x_rows, dp(yerr), frac, C.c_uint64(1), dp(yo), None, None, None, ip(st),
                             C.byref(ok))
    assert call() == _capi.MP_OK and ok.value == 2
    for bad in (dict(h=None), dict(pars=None), dict(xx=None), dict(yo=None), dict(n=0), dict(n=-1), dict(n=_capi.SIM_MAX_ROWS + 1),
                dict(n_obs=0), dict(n_obs=-3), dict(n=2, n_obs=_capi.SIM_MAX_CELLS // 2 + 1), dict(ndim=5), dict(ndim=10),
                dict(x_rows=0), dict(x_rows=3), dict(frac=0.0), dict(frac=-0.25), dict(frac=np.nan), dict(frac=np.inf),
                dict(yerr=np.array([0.1, 0.0])), dict(yerr=np.array([0.1, -1.0])), dict(yerr=np.array([np.nan, 0.1])),
                dict(yerr=np.array([0.1, np.inf]))):
        assert call(**bad) == _capi.MP_EINVAL, bad
        assert b"mp_simulate" in L.mp_last_error()
    for t in (tarr[0] - 1.0e-9, tarr[-1] + 1.0, np.nan, np.inf):
        assert call(xx=np.array([5.0, t])) == _capi.MP_ERANGE, t
    assert call(x_rows=2, xx=np.ascontiguousarray(tarr[[5, 50, 7, 70]])) == _capi.MP_OK
    assert call(yerr=np.array([0.1, 0.2]), frac=np.nan) == _capi.MP_OK   # frac_err is not looked at when yerr is given
    # no state of the handle is refused: a multi-device handle runs on its first device, the alternative dipole torque is served
    with _capi.Handle(_capi.cfg_synth(dipole_torque=1), tarr) as h1:
        h1.set_prior(synth.PRIOR_LOWER, synth.PRIOR_UPPER, synth.LOG_MASK)
        assert call(h=h1._h) == _capi.MP_OK and ok.value == 2


def test_generate_data_round_trips_through_the_csv_and_the_sampler(tmp_path, handle, tarr):
    from magprop_amd import EnsembleSampler, mcmc_eqns, mcmc_io, synth
    d = synth.generate_data(grb="Humped", seed=4)
    assert d["status"] == 0 and d["x"].shape == d["y"].shape == (50,)
    assert np.array_equal(d["x"], tarr[np.sort(np.random.default_rng(4).integers(0, tarr.size, 50))])   # the reference's draw of the times
    st, lc = handle.model_lc(CANON["Humped"])
    assert same(d["model"], lc[1][np.searchsorted(tarr, d["x"])]) and same(d["yerr"], 0.25 * d["model"])
    again = synth.generate_data(pars=_unlog([TRUTHS["Humped"]])[0], physical=True, seed=4)
    assert same(again["y"], d["y"])
    path = os.path.join(tmp_path, "Humped.csv")
    mcmc_io.write_dataset(path, d["x"], d["y"], d["yerr"])
    x, y, yerr = mcmc_io.read_dataset(path)
    assert np.allclose(x, d["x"], rtol=1e-15) and np.allclose(y, d["y"], rtol=1e-15) and np.allclose(yerr, d["yerr"], rtol=1e-15)
    es = EnsembleSampler(16, 6, x, y, yerr, seed=2)
    pos = np.array(TRUTHS["Humped"]) + 1.0e-4 * np.random.default_rng(0).standard_normal((16, 6))
    es.run_mcmc(pos, 20)
    lnp = es.get_log_prob()
    es.close()
    assert np.all(np.isfinite(lnp)) and lnp.max() > -0.5 * 50 * 9.0         # a fit near the truth: chi^2 per point far below 9
    many = synth.generate_data(pars=np.array([TRUTHS[t] for t in TYPES]), n_obs=20, seed=9)
    assert many["y"].shape == (4, 20) and many["x"].shape == (20,) and many["n_ok"] == 4
    with pytest.raises(ValueError):
        synth.generate_data()
    with pytest.raises(ValueError):
        synth.generate_data(grb="Bumpy")
    # the library variant, on the "S" grid, at times of the caller's
    t_s = np.array([2.0e-3, 0.5, 30.0, 4.0e4])
    lib = mcmc_eqns.generate_data([1.0, 5.0, -2.0, 2.0, 0.0, 0.0], "S", times=t_s, seed=3)
    assert lib["status"] == 0 and lib["y"].shape == (4,) and np.all(lib["yerr"] == 0.25 * np.abs(lib["model"]))
    with pytest.raises(Exception):
        mcmc_eqns.generate_data([1.0, 5.0, -2.0, 2.0, 0.0, 0.0], "L", times=t_s)      # 2e-3 s lies before the "L" grid
