"""GPU tests of the sampler's posterior monitor (include/magprop_amd.h mp_sampler_set_posterior): every accumulator bit for bit
against the numpy restatement (tests/post_restated.py) over the stored chain and stored lnprob, no change of the chain, store
and split invariance, the autocorrelation monitor beside it, discard, restart, tempering, a move table, half-step launches, the
refusals, and the Python front end on the Humped posterior."""
import ctypes as C

import numpy as np
import pytest

import post_restated as pr
from conftest import TRUTHS
from raw_abi import RawSampler, dp, lp
from test_gpu_autocorr import Raw as AcfRaw

pytestmark = pytest.mark.gpu

NDIM, BINS, BINS2 = 3, 256, 64
LOWER, UPPER = np.full(NDIM, -1.5), np.full(NDIM, 2.0)      # a unit Gaussian leaves samples below and above
KEYS = ("hist1", "below", "above", "nonfinite", "hist2", "outside2", "sum1", "sum2", "pivot", "n_finite", "best_x", "best_lnp", "best_idx", "n")


class Raw(AcfRaw):
    """The unit-Gaussian sampler of tests/test_gpu_autocorr.py with the posterior monitor and its read-outs.  post: None, or
    (bins1, bins2, discard); setup(r): settings that go before set_positions (temperatures, moves, whole step)."""

    def __init__(self, n_walkers, n_ens, seed, post=(BINS, BINS2, 0), max_lag=0, setup=None, ndim=NDIM):
        RawSampler.__init__(self, n_walkers, n_ens, ndim, seed)
        self.K = max_lag
        if setup is not None:
            setup(self)
        if max_lag:
            self.set_autocorr(max_lag, 0)
        self.post = post
        if post is not None:
            self._ok(self.set_posterior(*post))
        self.set_positions(np.random.default_rng(seed).standard_normal((self.nt, ndim)))

    def set_posterior(self, bins1, bins2, discard, lower=LOWER, upper=UPPER):
        return self.L.mp_sampler_set_posterior(self.sp, bins1, bins2, dp(np.ascontiguousarray(lower)), dp(np.ascontiguousarray(upper)), discard)

    def read(self, e):
        """Every read-out of ensemble e, keyed as the restatement keys them."""
        b1, b2 = self.post[0], self.post[1]
        nd, npairs = self.ndim, self.ndim * (self.ndim - 1) // 2
        o = {"hist1": np.empty((nd, b1), dtype=np.int64), "sum1": np.empty(nd), "sum2": np.empty((nd, nd)), "pivot": np.empty(nd), "best_x": np.empty(nd)}
        o.update({k: np.empty(nd, dtype=np.int64) for k in ("below", "above", "nonfinite")})
        n, nf, bi, bl = C.c_int64(-5), C.c_int64(-5), C.c_int64(-5), C.c_double(0.0)
        self._ok(self.L.mp_sampler_get_posterior_hist1(self.sp, e, lp(o["hist1"]), lp(o["below"]), lp(o["above"]), lp(o["nonfinite"]), C.byref(n)))
        o["hist2"] = o["outside2"] = None
        if b2:
            o["hist2"], o["outside2"] = np.empty((npairs, b2, b2), dtype=np.int64), np.empty(npairs, dtype=np.int64)
            self._ok(self.L.mp_sampler_get_posterior_hist2(self.sp, e, lp(o["hist2"]), lp(o["outside2"])))
        self._ok(self.L.mp_sampler_get_posterior_moments(self.sp, e, dp(o["sum1"]), dp(o["sum2"]), dp(o["pivot"]), C.byref(nf)))
        self._ok(self.L.mp_sampler_get_posterior_best(self.sp, e, dp(o["best_x"]), C.byref(bl), C.byref(bi)))
        o.update(n=n.value, n_finite=nf.value, best_lnp=bl.value, best_idx=bi.value)
        return o


def _same(got, want, what=""):
    for k in KEYS:
        a, b = got[k], want[k]
        if a is None or b is None:
            assert a is None and b is None, (what, k)
        else:
            assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True), (what, k, a, b)


def _restated(r, chain, lnp, e, lower=LOWER, upper=UPPER):
    s = slice(e * r.nw, (e + 1) * r.nw)
    return pr.accumulate(chain[:, s], lnp[:, s], r.post[0], r.post[1], lower, upper)


def _check_all(r, chain, lnp, what=""):
    for e in range(r.ne):
        _same(r.read(e), _restated(r, chain, lnp, e), (what, e))


@pytest.mark.parametrize("n_ens,n_walkers", [(1, 32), (4, 32), (1, 512)])
def test_accumulators_bit_equal_to_the_restatement_whatever_the_store_and_the_split(n_ens, n_walkers):
    """600 steps: every accumulator of every ensemble equals the restatement over the stored chain and stored lnprob; the
    same run without a host chain and the same run split into six calls hold the same accumulators; and the chain with the
    monitor on is the chain with it off."""
    seed = 300 + n_ens + n_walkers
    on, off, quiet, split = (Raw(n_walkers, n_ens, seed, post=p) for p in ((BINS, BINS2, 0), None, (BINS, BINS2, 0), (BINS, BINS2, 0)))
    chain, lnp = on.run(600)
    c0, l0 = off.run(600)
    assert np.array_equal(chain, c0) and np.array_equal(lnp, l0)
    quiet.run(600, store=False)
    cs, ls, _ = split.run_chunks([1, 15, 16, 17, 251, 300])
    assert np.array_equal(cs, chain) and np.array_equal(ls, lnp)
    for e in range(n_ens):
        want = _restated(on, chain, lnp, e)
        assert want["below"].all() and want["above"].all() and want["outside2"].all() and want["n"] == 600 * n_walkers
        for r, what in ((on, "stored"), (quiet, "store=False"), (split, "split")):
            _same(r.read(e), want, (what, e))
    for r in (on, off, quiet, split):
        r.close()


def test_both_monitors_together():
    K = 256
    both, acf, post = Raw(32, 2, 7, max_lag=K), Raw(32, 2, 7, post=None, max_lag=K), Raw(32, 2, 7)
    chain, lnp = both.run(600)
    acf.run(600, store=False)
    post.run(600, store=False)
    t, w, n = both.tau()
    t1, w1, n1 = acf.tau()
    assert np.array_equal(t, t1) and np.array_equal(w, w1) and n == n1 == 600
    for e in range(2):
        a, b = both.sums(e), acf.sums(e)
        assert all(np.array_equal(a[k], b[k]) for k in ("S", "T", "H", "tail", "pivot")) and a["n"] == b["n"]
        _same(both.read(e), post.read(e), e)
    _check_all(both, chain, lnp)
    for r in (both, acf, post):
        r.close()


def test_discard_and_restart():
    r = Raw(32, 2, 9, post=(BINS, BINS2, 100))
    assert r.read(0)["n"] == 0 and r.read(0)["best_idx"] == -1                 # nothing yet: zeros, best = none
    c1, l1 = r.run(60)
    assert r.read(1)["n"] == 0 and np.isnan(r.read(1)["best_x"]).all() and r.read(1)["best_lnp"] == -np.inf
    c2, l2 = r.run(540)
    chain, lnp = np.concatenate([c1, c2]), np.concatenate([l1, l2])
    assert r.read(0)["n"] == 500 * 32
    _check_all(r, chain[100:], lnp[100:], "discard")
    # set_positions in mid-run restarts the monitor, and the discard applies again
    r.set_positions(np.random.default_rng(10).standard_normal((r.nt, NDIM)))
    assert r.read(0)["n"] == 0 and not r.read(0)["hist1"].any() and r.read(0)["best_idx"] == -1
    c3, l3 = r.run(150)
    assert r.read(0)["n"] == 50 * 32
    _check_all(r, c3[100:], l3[100:], "restart")
    r.close()


def _tempered(r):
    r.set_temperatures([1.0, 0.5, 0.25])


def _de_table(r):
    from magprop_amd.moves import MOVE_DE, MOVE_STRETCH
    r.set_moves([(MOVE_DE, 1.0, 0.0, 1.0e-5), (MOVE_STRETCH, 0.5, 2.0, 0.0)])


def _half_steps(r):
    r.set_whole_step(0)


@pytest.mark.parametrize("setup,n_ens", [(_tempered, 6), (_de_table, 2), (_half_steps, 2)], ids=["tempered-2x3", "de-table", "half-steps"])
def test_sampler_variants(setup, n_ens):
    """A tempered sampler of 2 groups x 3 temperatures (every ensemble against its own rows), a move table with a DE move and
    one launch per half-step."""
    r = Raw(32, n_ens, 21, setup=setup)
    chain, lnp = r.run(300)
    _check_all(r, chain, lnp, setup.__name__)
    r.close()


def test_refusals_and_error_codes():
    from magprop_amd import _capi
    r = Raw(16, 1, 1, post=None)
    L, sp = r.L, r.sp
    EINVAL, ESTATE, OK = _capi.MP_EINVAL, _capi.MP_ESTATE, _capi.MP_OK
    out = np.empty(NDIM * BINS, dtype=np.int64)
    reads = (lambda e: L.mp_sampler_get_posterior_hist1(sp, e, None, None, None, None, None),
             lambda e: L.mp_sampler_get_posterior_hist2(sp, e, None, None),
             lambda e: L.mp_sampler_get_posterior_moments(sp, e, None, None, None, None),
             lambda e: L.mp_sampler_get_posterior_best(sp, e, None, None, None))
    for get in reads:
        assert get(0) == ESTATE and "monitor is off" in _capi.last_error()
    nan_lo, inf_hi, empty, huge = LOWER.copy(), UPPER.copy(), UPPER.copy(), UPPER.copy()
    nan_lo[1], inf_hi[2], empty[0], huge[0] = np.nan, np.inf, LOWER[0], 1.7e308
    for args, word in (((-1, 0, 0), "bins1"), ((_capi.POST_MAX_BINS + 1, 0, 0), "bins1"), ((16, -1, 0), "bins2"),
                       ((16, _capi.POST_MAX_BINS2 + 1, 0), "bins2"), ((16, 8, -1), "discard")):
        assert r.set_posterior(*args) == EINVAL and word in _capi.last_error(), args
    for kw in (dict(lower=nan_lo), dict(upper=inf_hi), dict(upper=empty), dict(lower=UPPER, upper=LOWER), dict(lower=-huge, upper=huge)):
        assert r.set_posterior(16, 8, 0, **kw) == EINVAL and "range" in _capi.last_error(), kw
    assert L.mp_sampler_set_posterior(sp, 16, 8, None, None, 0) == EINVAL
    assert reads[0](0) == ESTATE                                              # a refused call leaves the monitor off
    assert r.set_posterior(16, 0, 0) == OK
    assert reads[0](0) == OK and reads[2](0) == OK and reads[3](0) == OK       # every pointer NULL, no sample yet
    assert reads[1](0) == ESTATE and "bins2 = 0" in _capi.last_error()
    for get in reads:
        for e in (-1, 1):
            assert get(e) == EINVAL and "ensemble" in _capi.last_error(), e
    assert r.set_posterior(16, 8, 0) == OK and reads[1](-1) == EINVAL and reads[1](0) == OK
    assert r.set_posterior(BINS, 0, 0) == OK and L.mp_sampler_get_posterior_hist1(sp, 0, lp(out), None, None, None, None) == OK and not out.any()
    # the walker-sharded entry points do not feed the monitor
    for rc in (L.mp_sampler_halfstep_shard(sp, 0, 0, 1, None, None), L.mp_sampler_halfstep_apply(sp, 0, C.c_void_p(8), None, None, None),
               L.mp_sampler_step_shard(sp, 0, 1, None, None), L.mp_sampler_step_apply(sp, C.c_void_p(8), None, None, None)):
        assert rc == ESTATE and "mp_sampler_set_posterior" in _capi.last_error()
    assert L.mp_sampler_set_posterior(sp, 0, 0, None, None, 0) == OK          # off again: the monitor is gone
    assert reads[0](0) == ESTATE and "monitor is off" in _capi.last_error()
    r.close()
    # accumulators beyond MP_POST_MAX_BYTES: 256 ensembles x 36 pairs x 128^2 cells x 8 bytes = 1.2 GB
    big = Raw(2, 256, 2, post=None, ndim=9)
    lo9, hi9 = np.full(9, -1.0), np.full(9, 1.0)
    assert big.set_posterior(4096, 128, 0, lo9, hi9) == EINVAL and "MP_POST_MAX_BYTES" in _capi.last_error()
    assert big.set_posterior(256, 64, 0, lo9, hi9) == OK
    big.close()


def test_front_end_on_humped(gsynth):
    """64 walkers on the Humped posterior: 100 steps of burn-in, monitor_posterior(range="ensemble"), 200 stored steps.
    get_posterior equals the restatement over the stored chain; best_x / best_lnprob are the stored chain's first argmax;
    get_quantiles lies within one bin width of np.quantile over the same rows (both lie in the bin that holds rank q n or beside
    it: tests/test_post_cases_cpu.py)."""
    from magprop_amd import EnsembleSampler, posterior
    x, y, yerr = gsynth["Humped_x"], gsynth["Humped_y"], gsynth["Humped_yerr"]
    s = EnsembleSampler(64, 6, x, y, yerr, seed=7)
    with pytest.raises(ValueError, match="needs positions"):
        s.monitor_posterior(range="ensemble")
    with pytest.raises(_capi_error(), match="monitor is off"):
        s.get_posterior()
    s.run_mcmc(np.array(TRUTHS["Humped"]) + 1.0e-4 * np.random.default_rng(6).standard_normal((64, 6)), 100, store=False)
    pos = s.get_last_sample()[0]
    s.monitor_posterior(range="ensemble")
    bins, bins2, lo, hi = s._post
    elo, ehi = posterior.ensemble_range(pos, *s._prior)
    assert (bins, bins2) == (256, 64) and np.array_equal(lo, elo) and np.array_equal(hi, ehi)
    s.run_mcmc(None, 200)
    chain, lnp = s.get_chain(), s.get_log_prob()
    assert chain.shape == (200, 64, 6)
    want = pr.accumulate(chain, lnp, 256, 64, lo, hi)
    got = s.get_posterior()
    for k in ("hist1", "below", "above", "nonfinite", "hist2", "outside2", "best_x"):
        assert np.array_equal(got[k], want[k]), k
    assert got["n"] == want["n"] == 200 * 64 and got["n_finite"] == want["n_finite"] and got["pairs"] == pr.pairs(6)
    mean, cov = posterior.mean_cov(want["sum1"], want["sum2"], want["pivot"], want["n_finite"])
    assert np.array_equal(got["mean"], mean) and np.array_equal(got["cov"], cov)
    assert np.array_equal(got["edges1"], posterior.edges(lo, hi, 256)) and np.array_equal(got["edges2"], posterior.edges(lo, hi, 64))
    i = int(np.argmax(lnp.ravel()))
    assert got["best_index"] == i and got["best_lnprob"] == lnp.ravel()[i] and np.array_equal(got["best_x"], chain.reshape(-1, 6)[i])
    q = s.get_quantiles()
    ref = np.quantile(chain.reshape(-1, 6), (0.16, 0.5, 0.84), axis=0)
    widths = (hi - lo) / 256
    print("quantiles off by (bin widths):", np.abs(q - ref) / widths)
    assert q.shape == (3, 6) and np.all(np.abs(q - ref) <= widths)
    s.monitor_posterior(bins=0)
    with pytest.raises(_capi_error(), match="monitor is off"):
        s.get_quantiles()
    s.close()


def test_front_end_selects_the_temperature():
    from magprop_amd import EnsembleSampler
    t = EnsembleSampler(32, 2, target="gaussian", seed=12, betas=(1.0, 0.5, 0.25))
    box = np.array([[-4.0, 4.0], [-4.0, 4.0]])
    t.monitor_posterior(bins=64, bins2=16, range=box, discard=10)
    t.run_mcmc(np.random.default_rng(3).standard_normal((96, 2)), 210)
    for temp in range(3):
        got = t.get_posterior(0, temp=temp)
        want = pr.accumulate(t.get_chain(temp=temp)[10:], t.get_log_prob(temp=temp)[10:], 64, 16, box[:, 0], box[:, 1])
        for k in ("hist1", "below", "above", "hist2", "outside2", "best_x"):
            assert np.array_equal(got[k], want[k]), (temp, k)
        assert got["n"] == 200 * 32 and got["best_index"] == want["best_idx"]
    assert np.array_equal(t.get_posterior(1)["hist1"], t.get_posterior(0, temp=1)["hist1"])
    with pytest.raises(ValueError, match="temp must be"):
        t.get_posterior(0, temp=3)
    t.close()


def _capi_error():
    from magprop_amd import _capi
    return _capi.MagpropAmdError
