"""GPU tests of the sampler's autocorrelation monitor (include/magprop_amd.h mp_sampler_set_autocorr): the accumulators bit for
bit against the numpy restatement (tests/acf_restated.py) over the stored chain, tau and window against the restatement and
against the host estimator (magprop_amd.mcmc_io.integrated_time), no change of the chain, split and store invariance, discard,
restart, tempering, run_mcmc_until and the refusals."""
import ctypes as C

import numpy as np
import pytest

import acf_restated as ar
from conftest import TRUTHS
from raw_abi import RawSampler, dp, ip
from test_autocorr_cpu import MEASURED_DISCREPANCY

pytestmark = pytest.mark.gpu

# against the restatement: division and the order of the scan may differ by rounding
RESTATED_RTOL = 1e-12
# against the host's FFT estimator: 10 x the restatement-vs-FFT discrepancy measured in tests/test_autocorr_cpu.py (7.9e-12); the
# margin covers the longer real chains
HOST_RTOL = 10.0 * MEASURED_DISCREPANCY


class Raw(RawSampler):
    """A unit-Gaussian sampler of n_ens ensembles through the C ABI, started at standard-normal positions drawn from its seed,
    with the read-outs of the monitor."""

    def __init__(self, n_walkers, n_ens, ndim, seed, max_lag=0, discard=0):
        super().__init__(n_walkers, n_ens, ndim, seed)
        self.K = max_lag
        if max_lag:
            self.set_autocorr(max_lag, discard)
        self.set_positions(np.random.default_rng(seed).standard_normal((self.nt, ndim)))

    def sums(self, e):
        w = (self.nw, self.ndim)
        out = {k: np.empty((self.K,) + w) for k in ("S", "H", "tail")}
        out.update({k: np.empty(w) for k in ("T", "pivot")})
        n = C.c_int64(0)
        self._ok(self.L.mp_sampler_get_autocorr_sums(self.sp, e, *(dp(out[k]) for k in ("S", "T", "H", "tail", "pivot")), C.byref(n)))
        out["n"] = n.value
        return out

    def tau(self, c=5.0):
        tau, win = np.empty((self.ne, self.ndim)), np.empty((self.ne, self.ndim), dtype=np.int32)
        n = C.c_int64(0)
        self._ok(self.L.mp_sampler_get_autocorr(self.sp, C.c_double(c), dp(tau), ip(win), C.byref(n)))
        return tau, win, n.value


def _same_sums(a, b):
    for key in ("S", "T", "H", "tail", "pivot"):
        assert np.array_equal(a[key], b[key]), key
    assert a["n"] == b["n"]


@pytest.mark.parametrize("n_ens,n_walkers", [(1, 32), (1, 512), (4, 32), (4, 512)])
def test_accumulators_bit_equal_to_the_restatement(n_ens, n_walkers):
    """3 000 stored steps of the unit-Gaussian target: every accumulator of every ensemble equals the restatement over the
    stored chain bit for bit; tau agrees to 1e-12, the window exactly; and both agree with the host's FFT estimator on the
    same chain within HOST_RTOL."""
    K, ndim = 384, 3      # (tau is about 35 here: windows near 180)
    r = Raw(n_walkers, n_ens, ndim, seed=100 + n_ens + n_walkers, max_lag=K)
    chain, _ = r.run(3000)
    tau, win, n = r.tau()
    assert n == 3000
    for e in range(n_ens):
        x = chain[:, e * n_walkers:(e + 1) * n_walkers]
        m = ar.Monitor(K).feed(x)
        _same_sums(r.sums(e), m.sums())
        rt, rw, rf = m.finalise(5.0)
        assert np.array_equal(win[e], rw) and np.all(rw > 0)
        rel = np.max(np.abs(tau[e] / rt - 1.0))
        ht, hw = ar.host_tau_window(x, 5.0)
        rel_host = np.max(np.abs(tau[e] / ht - 1.0))
        print(f"ensemble {e}: tau {tau[e]}, window {win[e]}, vs restatement {rel:.2e} (bit-equal: {np.array_equal(tau[e], rt)}), vs host {rel_host:.2e}")
        assert rel <= RESTATED_RTOL
        # the device rounds every operation of the finalisation once, IEEE, in the restatement's order (the unfused helpers, the
        # correctly rounded fp64 division of a build without fast-math flags, the running sum by one lane): no bit may differ
        assert np.array_equal(tau[e], rt)
        assert np.array_equal(win[e], hw) and rel_host <= HOST_RTOL
        f = np.empty((K, ndim))
        rows = r.L.mp_sampler_get_acf(r.sp, e, K, dp(f))
        assert rows == K and np.allclose(f, rf, rtol=0, atol=1e-13) and np.all(f[0] == 1.0)
    r.close()


@pytest.mark.parametrize("moves", ["stretch", "kde"])
def test_humped_posterior_against_the_host_estimator(gsynth, moves):
    from magprop_amd import EnsembleSampler, KDEMove
    x, y, yerr = gsynth["Humped_x"], gsynth["Humped_y"], gsynth["Humped_yerr"]
    s = EnsembleSampler(64, 6, x, y, yerr, seed=7, moves=None if moves == "stretch" else KDEMove())
    s.monitor_autocorr(max_lag=2048, discard=500)
    s.run_mcmc(np.array(TRUTHS["Humped"]) + 1.0e-4 * np.random.default_rng(6).standard_normal((64, 6)), 3500)
    tau, win, n = s.get_autocorr_device()
    assert n == 3000
    ht, hw = ar.host_tau_window(s.get_chain()[500:], 5.0)
    rel = np.max(np.abs(tau / ht - 1.0))
    print(f"Humped, {moves}: tau {tau}, window {win}, vs host {rel:.2e}")
    assert np.array_equal(win, hw)
    assert rel <= HOST_RTOL
    assert np.array_equal(s.get_autocorr_time(device=True, quiet=True), tau)
    s.close()


def test_monitor_changes_nothing_and_splits_do_not_matter():
    K = 512
    off, on, split, quiet = (Raw(32, 2, 3, seed=5, max_lag=k) for k in (0, K, K, K))
    c0, l0 = off.run(600)
    c1, l1 = on.run(600)
    assert np.array_equal(c0, c1) and np.array_equal(l0, l1)          # same chain and lnprob bit for bit with the monitor on
    parts = [split.run(n) for n in (1, 7, 592)]
    assert np.array_equal(np.concatenate([p[0] for p in parts]), c0)
    quiet.run(600, store=False)                                        # no host chain at all
    t1, w1, n1 = on.tau()
    for other in (split, quiet):
        for e in range(2):
            _same_sums(on.sums(e), other.sums(e))
        t, w, n = other.tau()
        assert np.array_equal(t, t1) and np.array_equal(w, w1) and n == n1 == 600 and np.all(w1 > 0)
    for r in (off, on, split, quiet):
        r.close()


def test_discard_restart_and_tempering():
    from magprop_amd import EnsembleSampler
    rng = np.random.default_rng(3)
    s = EnsembleSampler(32, 2, target="gaussian", seed=11)
    s.monitor_autocorr(max_lag=1024, discard=200)
    s.run_mcmc(rng.standard_normal((32, 2)), 150)                      # still inside the discard
    with pytest.raises(Exception, match="2 or more"):
        s.get_autocorr_device()
    s.run_mcmc(None, 2050)
    tau, win, n = s.get_autocorr_device()
    ht, hw = ar.host_tau_window(s.get_chain()[200:], 5.0)
    assert n == 2000 and np.array_equal(win, hw) and np.max(np.abs(tau / ht - 1.0)) <= HOST_RTOL
    assert tau.shape == (2,)
    # set_positions restarts the monitor (and its discard)
    first_len = len(s.get_chain())
    s.run_mcmc(rng.standard_normal((32, 2)), 1200)
    tau2, win2, n2 = s.get_autocorr_device()
    ht2, hw2 = ar.host_tau_window(s.get_chain()[first_len + 200:], 5.0)
    assert n2 == 1000 and np.array_equal(win2, hw2) and np.max(np.abs(tau2 / ht2 - 1.0)) <= HOST_RTOL
    # quiet=False raises on a chain shorter than tol tau, as the host path does
    with pytest.raises(RuntimeError, match="shorter than"):
        s.get_autocorr_time(device=True, tol=10 ** 6)
    # max_lag too small for the window: NaN, which raises (quiet=False) or warns (quiet=True)
    s.monitor_autocorr(max_lag=4)
    s.run_mcmc(None, 500)
    with pytest.raises(RuntimeError, match="max_lag"):
        s.get_autocorr_time(device=True)
    with pytest.warns(RuntimeWarning, match="max_lag"):
        assert np.all(np.isnan(s.get_autocorr_time(device=True, quiet=True)))
    s.monitor_autocorr(max_lag=0)
    with pytest.raises(Exception, match="monitor is off"):
        s.get_autocorr_device()
    s.close()
    # a tempered sampler reports its beta = 1 ensemble
    t = EnsembleSampler(32, 2, target="gaussian", seed=12, betas=(1.0, 0.5, 0.25))
    t.monitor_autocorr(max_lag=1024)
    t.run_mcmc(rng.standard_normal((96, 2)), 2000)
    tau, win, n = t.get_autocorr_device()
    ht, hw = ar.host_tau_window(t.get_chain(temp=0), 5.0)
    assert tau.shape == (2,) and np.array_equal(win, hw) and np.max(np.abs(tau / ht - 1.0)) <= HOST_RTOL
    assert np.max(np.abs(t.get_autocorr_time(device=True, quiet=True) / t.get_autocorr_time(quiet=True) - 1.0)) <= HOST_RTOL
    t.close()


def test_run_mcmc_until():
    from magprop_amd import EnsembleSampler
    from magprop_amd.ensemble import autocorr_converged
    pos = np.random.default_rng(21).standard_normal((64, 2))
    s = EnsembleSampler(64, 2, target="gaussian", seed=22)
    out = s.run_mcmc_until(pos, 20000, check_every=100)
    chain = s.get_chain()
    n = len(chain)
    assert s.converged and n % 100 == 0 and 0 < n < 20000 and s.iteration == n
    assert np.array_equal(out, chain[-1]) and [h[0] for h in s.tau_history] == list(range(100, n + 1, 100))
    # the criterion, recomputed on the host from the stored chain: holds at the stop, did not hold at the check before
    host = {m: ar.host_tau_window(chain[:m], 5.0)[0] for m in (n - 200, n - 100, n)}
    assert autocorr_converged(host[n], host[n - 100], n)
    assert not autocorr_converged(host[n - 100], host[n - 200], n - 100)
    assert np.max(np.abs(s.tau_history[-1][1] / host[n] - 1.0)) <= HOST_RTOL
    print(f"run_mcmc_until stopped after {n} steps, tau {s.tau_history[-1][1]}")
    assert s._chain.shape[0] == n and s._chain.base is None      # trimmed: the rows of the early stop, not a view of max_steps
    # without a host chain it stops at the same step
    q = EnsembleSampler(64, 2, target="gaussian", seed=22)
    q.run_mcmc_until(pos, 20000, check_every=100, store=False)
    assert q.converged and q.iteration == n and q.get_chain() is None
    assert np.array_equal(q.tau_history[-1][1], s.tau_history[-1][1])
    # max_steps too small: not converged, exactly max_steps steps
    u = EnsembleSampler(64, 2, target="gaussian", seed=22)
    u.run_mcmc_until(pos, 250, check_every=100)
    assert not u.converged and u.iteration == 250 and len(u.get_chain()) == 250
    assert np.array_equal(u.get_chain(), chain[:250])
    for x in (s, q, u):
        x.close()


def test_run_mcmc_until_inside_the_discard():
    """Checks that fall inside the monitor's discard are skipped without an estimate; any other failure of the estimate
    propagates instead of letting the loop run on to max_steps."""
    from magprop_amd import EnsembleSampler, _capi
    pos = np.random.default_rng(31).standard_normal((32, 2))
    s = EnsembleSampler(32, 2, target="gaussian", seed=32)
    s.monitor_autocorr(max_lag=256, discard=250)
    assert s.get_autocorr_device(wait=True) == (None, None, 0)
    with pytest.raises(_capi.MagpropAmdError, match="2 or more"):
        s.get_autocorr_device()
    s.run_mcmc_until(pos, 500, check_every=100)
    # the checks after 100 and 200 steps see no sample; those after 300, 400 and 500 see 50, 150 and 250
    assert [h[0] for h in s.tau_history] == [50, 150, 250] and s.iteration == 500 and not s.converged
    ht, _ = ar.host_tau_window(s.get_chain()[250:], 5.0)
    assert np.max(np.abs(s.tau_history[-1][1] / ht - 1.0)) <= HOST_RTOL
    with pytest.raises(ValueError, match="c must be"):
        s.run_mcmc_until(None, 100, check_every=100, c=-1.0)
    s.close()


def test_refusals_carry_a_message():
    from magprop_amd import _capi
    r = Raw(16, 1, 2, seed=1)
    L, sp = r.L, r.sp
    for bad in (-1, _capi.ACF_MAX_LAG + 1):
        assert L.mp_sampler_set_autocorr(sp, bad, 0) == _capi.MP_EINVAL and "max_lag" in _capi.last_error()
    assert L.mp_sampler_set_autocorr(sp, 16, -1) == _capi.MP_EINVAL and "discard" in _capi.last_error()
    tau, win = np.empty((1, 2)), np.empty((1, 2), dtype=np.int32)
    get = lambda: L.mp_sampler_get_autocorr(sp, C.c_double(5.0), dp(tau), ip(win), None)   # noqa: E731
    assert get() == _capi.MP_ESTATE and "monitor is off" in _capi.last_error()
    assert L.mp_sampler_get_acf(sp, 0, 4, dp(tau)) == _capi.MP_ESTATE
    assert L.mp_sampler_get_autocorr_sums(sp, 0, None, None, None, None, None, None) == _capi.MP_ESTATE
    assert L.mp_sampler_set_autocorr(sp, 16, 0) == _capi.MP_OK
    assert get() == _capi.MP_ESTATE and "2 or more" in _capi.last_error()
    r.run(1)
    assert get() == _capi.MP_ESTATE and "2 or more" in _capi.last_error()
    r.run(1)
    assert get() == _capi.MP_OK
    # the walker-sharded entry points do not feed the monitor
    for rc in (L.mp_sampler_halfstep_shard(sp, 0, 0, 1, None, None), L.mp_sampler_halfstep_apply(sp, 0, C.c_void_p(8), None, None, None),
               L.mp_sampler_step_shard(sp, 0, 1, None, None), L.mp_sampler_step_apply(sp, C.c_void_p(8), None, None, None)):
        assert rc == _capi.MP_ESTATE and "mp_sampler_set_autocorr" in _capi.last_error()
    assert L.mp_sampler_set_autocorr(sp, 0, 0) == _capi.MP_OK          # off again: the monitor is gone
    assert get() == _capi.MP_ESTATE and "monitor is off" in _capi.last_error()
    r.close()
    # accumulators beyond MP_ACF_MAX_BYTES: 4 x 4 096 lags x 16 384 walkers x 9 dimensions x 8 bytes = 19 GB
    big = Raw(16384, 1, 9, seed=2)
    assert big.L.mp_sampler_set_autocorr(big.sp, 4096, 0) == _capi.MP_EINVAL and "MP_ACF_MAX_BYTES" in _capi.last_error()
    assert big.L.mp_sampler_set_autocorr(big.sp, 64, 0) == _capi.MP_OK
    big.close()
