"""GPU tests of the pointwise scores end to end (mp_model_pointwise, run with -m gpu on an MI355X): the cell matrix against the
numpy restatement (tests/pointwise_restated.py) of the curve mp_model_lc returns for the same rows one by one, bit for bit; the
table and the tail rows against the restatement of the returned cells; the sum of a row's cells against the likelihood kernel;
independence of the chunking; a light curve of 1 944 points; the front ends; the error paths.

As in tests/test_gpu_derived.py the bit-for-bit comparisons with mp_model_lc run on a handle whose prior box is in physical units
with no log mask (`phys`): mp_model_lc takes physical parameters, and the device's 10^x and numpy's need not agree to the bit."""
import numpy as np
import pytest

from conftest import TRUTHS

import pointwise_restated as pr
from test_gpu_derived import PHYS_LOWER, PHYS_UPPER, _unlog
from test_pointwise_cases_cpu import lse_bound, lse_error, same

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
L = np.longdouble


def _sorted(x, y, yerr):
    order = np.argsort(x, kind="stable")
    return np.asarray(x)[order], np.asarray(y)[order], np.asarray(yerr)[order]


@pytest.fixture(scope="module")
def phys(tarr, gsynth):
    from magprop_amd import _capi
    h = _capi.Handle(_capi.cfg_synth(), tarr)
    h.set_prior(PHYS_LOWER, PHYS_UPPER, 0)
    h.set_dataset(0, gsynth["Humped_x"], gsynth["Humped_y"], gsynth["Humped_yerr"])
    yield h
    h.close()


def _host_cells(h, P, inside, x, y, yerr):
    """(z[n_obs][n], status) of mp_model_lc row by row and the restatement; rows outside the prior: status 3"""
    xs, ys, es = _sorted(x, y, yerr)
    g, dx, idt = pr.digest(h.tgrid, xs)
    z = np.full((xs.size, len(P)), np.nan)
    st = np.full(len(P), 3, dtype=np.int32)
    for i in np.nonzero(inside)[0]:
        s, lc = h.model_lc(P[i])
        st[i] = s
        if s == 0:
            z[:, i] = pr.cells(lc[1][None, :], np.zeros(1, dtype=np.int32), g, dx, idt, ys, es)[:, 0]
    return z, st


def check_table(obs, tail, z):
    """the table and the tail rows against the restatement of the cells z; returns the worst log-sum-exp error / bound"""
    want_obs, want_tail = pr.pointwise(z)
    assert tail.shape == want_tail.shape and same(tail, want_tail)
    for col in pr.EXACT:
        assert same(obs[:, col], want_obs[:, col]), (col, obs[:, col], want_obs[:, col])
    d = pr.definition(z)
    worst = 0.0
    for mcol, scol, key in ((pr.LPPD_M, pr.LPPD_S, "lppd"), (pr.NONTAIL_M, pr.NONTAIL_S, "nontail")):
        for j in range(z.shape[0]):
            want = d[key][j]
            err = lse_error(obs[j, mcol], obs[j, scol], want)
            lim = lse_bound(z.shape[1], float(want)) if np.isfinite(want) else 0.0
            assert err <= lim, (key, j, err, lim)
            if lim:
                worst = max(worst, err / lim)
    return worst


def test_synthetic_case_against_model_lc_and_the_likelihood_kernel(phys, gsynth, gcorners):
    x, y, yerr = gsynth["Humped_x"], gsynth["Humped_y"], gsynth["Humped_yerr"]
    rng = np.random.default_rng(21)
    ball = _unlog(np.array(TRUTHS["Humped"]) + 0.02 * rng.standard_normal((96, 6)))
    out = _unlog(np.array([TRUTHS["Humped"]]))
    out[0, 0] = 50.0                                          # B above the box
    # a break-up corner of the prior box, which the model flags (10 ** log10(50) lands an ulp outside the physical box: clipped onto it)
    corners = np.clip(_unlog(gcorners["pars"][gcorners["status"] == 1]), PHYS_LOWER, PHYS_UPPER)
    assert len(corners) >= 1
    P = np.concatenate([ball[:40], out, ball[40:70], corners[:1], ball[70:]])
    inside = np.all((P >= PHYS_LOWER) & (P <= PHYS_UPPER), axis=1)
    assert len(P) == 98 and int((~inside).sum()) == 1
    z_want, st_want = _host_cells(phys, P, inside, x, y, yerr)
    obs, tail, st, used, z = phys.model_pointwise(P, ds_id=0, cells=True)
    lnp, st_batch = phys.lnprob_batch(P, ds_id=0, want_status=True)
    assert np.array_equal(st, st_batch) and np.array_equal(st, st_want)
    assert st[40] == 3 and st[71] == 1 and used == 96 == int(np.sum(st == 0))
    assert z.shape == (50, 98) and tail.shape == (50, pr.tail_len(98))
    bad = np.argwhere(~((z == z_want) | (np.isnan(z) & np.isnan(z_want))))
    assert bad.size == 0 and same(z, z_want), (bad[:5], [(z[j, s], z_want[j, s]) for j, s in bad[:5]])
    worst = check_table(obs, tail, z)
    assert np.all(obs[:, pr.N_USED] == 96)
    print(f"synthetic case: device log-sum-exp worst/bound {worst:.3f}")
    # Per row, the sum of its cells' ll against the likelihood kernel's lnlike (inside the box the prior adds 0).  The two paths
    # differ only in where the division by 1e50 and the FMA round: per cell the model value moves by a few eps |mod|, which
    # moves z by that over yerr and ll = -z^2 / 2 by |z| times that, and the square and the halving round: about
    # 8 eps (|z| |mod| / yerr + z^2) per cell, summed over the row's cells.  (The sum here is formed in long double.)
    xs, ys, es = _sorted(x, y, yerr)
    ratio = 0.0
    for i in np.nonzero(st == 0)[0]:
        zi = z[:, i].astype(L)
        mod = ys - z[:, i] * es
        lim = float(np.sum(8.0 * EPS * (np.abs(z[:, i]) * np.abs(mod) / es + z[:, i] ** 2)))
        err = float(abs(np.sum(-0.5 * zi * zi) - L(lnp[i])))
        ratio = max(ratio, err / lim)
        assert err <= lim, (i, err, lim)
    print(f"synthetic case: |sum ll - lnlike| worst/bound {ratio:.3f}")
    # without the cell matrix the results are the same
    obs2, tail2, st2, used2 = phys.model_pointwise(P, ds_id=0)
    assert same(obs2, obs) and same(tail2, tail) and np.array_equal(st2, st) and used2 == used


def test_chunking_does_not_show(phys):
    n = phys._L.mp_n_simd(phys._h) + 1
    rng = np.random.default_rng(22)
    P = _unlog(np.array(TRUTHS["Humped"]) + 0.02 * rng.standard_normal((n, 6)))
    P[n // 2, 1] = 0.1                                        # one row outside the box, inside the first chunk
    obs, tail, st, used, z = phys.model_pointwise(P, ds_id=0, cells=True)
    assert st[n // 2] == 3 and used == int(np.sum(st == 0)) >= n - 8
    assert np.array_equal(np.isnan(z), np.broadcast_to(st != 0, z.shape))
    check_table(obs, tail, z)
    # the last row sits alone in the second chunk: its cells are those of a call of its own, and of a call it opens
    one = phys.model_pointwise(P[-1:], ds_id=0, cells=True)[4]
    head = phys.model_pointwise(P[-1:-66:-1], ds_id=0, cells=True)[4]
    assert same(one[:, 0], z[:, -1]) and same(head[:, 0], z[:, -1]) and same(head[:, 64], z[:, -65])


def test_long_light_curve(tarr, glonglc):
    from magprop_amd import _capi
    x, y, yerr = glonglc["synth1944_ds"]
    P = np.clip(_unlog(glonglc["synth1944_pars"][:8]), PHYS_LOWER, PHYS_UPPER)
    h = _capi.Handle(_capi.cfg_synth(), tarr)
    try:
        h.set_prior(PHYS_LOWER, PHYS_UPPER, 0)
        h.set_dataset(3, x, y, yerr)
        z_want, st_want = _host_cells(h, P, np.ones(8, dtype=bool), x, y, yerr)
        obs, tail, st, used, z = h.model_pointwise(P, ds_id=3, cells=True)
        g, dx, _ = pr.digest(tarr, np.sort(x))
        assert z.shape == (1944, 8) and np.any(dx > 0.0) and np.unique(g).size > 64
        assert np.array_equal(st, st_want) and used == int(np.sum(st == 0)) >= 6
        assert same(z, z_want)
        check_table(obs, tail, z)
    finally:
        h.close()


def test_front_ends(gsynth):
    from magprop_amd import EnsembleSampler, pointwise, synth
    x, y, yerr = gsynth["Humped_x"], gsynth["Humped_y"], gsynth["Humped_yerr"]
    rev = np.arange(x.size)[::-1]                             # the caller's order is not the library's
    rng = np.random.default_rng(23)
    s = EnsembleSampler(32, 6, x[rev], y[rev], yerr[rev], seed=5)
    p0 = np.array(TRUTHS["Humped"]) + 1.0e-3 * rng.standard_normal((32, 6))
    s.run_mcmc(p0, 6)
    a = s.get_pointwise()
    flat = s.get_chain(flat=True)
    b = synth.model_pointwise(flat, x[rev], y[rev], yerr[rev])
    assert a["n_used"] == b["n_used"] == 192 and np.array_equal(a["status"], b["status"])
    assert same(a["obs"], b["obs"]) and same(a["tail"], b["tail"])
    for k in ("elpd_loo", "khat", "p_loo", "lppd"):
        assert same(a["loo"][k], b["loo"][k]), k
    assert a["obs"].shape == (50, 12) and a["summary"]["n_obs"] == 50 and np.all(np.isfinite(a["loo"]["elpd_loo"]))
    # per-point arrays follow the caller's order of x
    c = synth.model_pointwise(flat, x, y, yerr, cells=True)
    assert same(c["obs"][rev], b["obs"]) and same(c["tail"][rev], b["tail"]) and c["z"].shape == (50, 192)
    w = pointwise.waic(c["obs"])
    assert same(w["elpd_waic"], c["waic"]["elpd_waic"]) and pointwise.compare(c["loo"], a["loo"]["elpd_loo"][rev]) == (0.0, 0.0)
    s2 = s.get_pointwise(discard=2, thin=2)
    assert s2["n_used"] == 64
    with pytest.raises(ValueError, match="samples must be 2-D"):
        synth.model_pointwise(flat[:, :5], x, y, yerr)


def test_error_paths(phys, tarr):
    from magprop_amd import _capi
    P = _unlog(np.array([TRUTHS["Humped"]] * 4))
    with pytest.raises(_capi.MagpropAmdError, match="unset dataset 7"):
        phys.model_pointwise(P, ds_id=7)
    with pytest.raises(ValueError, match="MP_POINTWISE_MAX_SAMPLES"):
        phys.model_pointwise(np.zeros((_capi.POINTWISE_MAX_SAMPLES + 1, 6)), ds_id=0)
    # n * n_obs over the cell limit: 2^28 / 1 944 < 138 085 rows <= MP_POINTWISE_MAX_SAMPLES (refused before anything is allocated)
    h = _capi.Handle(_capi.cfg_synth(), tarr)
    try:
        xs = np.linspace(tarr[0], tarr[-1], 1944)
        h.__dict__["_ds_size"] = {}
        assert h._L.mp_set_dataset(h._h, 1, _capi._dptr(xs), _capi._dptr(xs), _capi._dptr(xs), 1944) == 0
        p = np.zeros((138085, 6))
        o = np.empty((1944, 12))
        rc = h._L.mp_model_pointwise(h._h, _capi._dptr(p), 138085, 6, 0, 1, _capi._dptr(o), None, None, None, None)
        assert rc == _capi.MP_EINVAL and "MP_POINTWISE_MAX_CELLS" in _capi.last_error()
    finally:
        h.close()
    with pytest.raises(ValueError, match="2-D"):
        phys.model_pointwise(np.zeros(6))
