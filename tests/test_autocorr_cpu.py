"""CPU checks of the autocorrelation monitor's definition (include/magprop_amd.h mp_sampler_set_autocorr) through its numpy
restatement (tests/acf_restated.py), and of run_mcmc_until's stopping rule.  No GPU.

Measured restatement-vs-FFT discrepancy (test_restatement_agrees_with_the_host_estimator): the largest relative difference of tau
between the moment-form restatement and magprop_amd.mcmc_io.integrated_time over the cases below is 7.8e-12 (the series whose
first sample, the pivot, sits 30 standard deviations from its mean; 8e-14 or less on the stationary ones), against the bound 1e-9
above which the pivoted moment form would not be doing its job.  tests/test_gpu_autocorr.py bounds the device against the host estimator by 10 x the measured figure."""
import numpy as np
import pytest

import acf_restated as ar
from magprop_amd import _capi
from magprop_amd.ensemble import autocorr_converged

# (rho, nsteps, nwalkers, ndim, max_lag, seed, first sample's offset in standard deviations)
CASES = [
    (0.0, 500, 8, 2, 500, 1, 0.0),
    (0.0, 5000, 64, 1, 256, 2, 0.0),
    (0.5, 500, 16, 3, 512, 3, 0.0),
    (0.5, 20000, 8, 2, 128, 4, 0.0),
    (0.9, 2000, 32, 2, 512, 5, 0.0),
    (0.9, 20000, 16, 1, 1024, 6, 0.0),
    (0.98, 5000, 64, 1, 2048, 7, 0.0),
    (0.98, 20000, 8, 2, 2048, 8, 0.0),
    (0.9, 5000, 16, 2, 1024, 9, 30.0),      # the pivot x_0 sits 30 standard deviations from the mean of the series
    (0.5, 2000, 8, 2, 256, 10, -30.0),
]
MEASURED_DISCREPANCY = 7.9e-12   # the module docstring; tests/test_gpu_autocorr.py takes its bound from here
DISCREPANCY_BOUND = 1e-9


def _case(rho, nsteps, nwalkers, ndim, seed, offset):
    rng = np.random.default_rng(seed)
    start = None if offset == 0.0 else np.full((nwalkers, ndim), offset)
    return ar.ar1(rng, rho, nsteps, nwalkers, ndim, mean=3.0, start=start)


def test_restatement_agrees_with_the_host_estimator():
    """Windows equal in every case and tau within DISCREPANCY_BOUND of the FFT estimator; the largest difference seen is the
    measured discrepancy of the module docstring (printed; no seed here lands on a rounding tie of M >= c taus_M)."""
    worst = 0.0
    for rho, nsteps, nwalkers, ndim, K, seed, offset in CASES:
        x = _case(rho, nsteps, nwalkers, ndim, seed, offset)
        tau, window, _ = ar.Monitor(K).feed(x).finalise(5.0)
        host_tau, host_window = ar.host_tau_window(x, 5.0)
        assert np.array_equal(window, host_window), (rho, nsteps, window, host_window)
        rel = np.max(np.abs(tau / host_tau - 1.0))
        print(f"rho={rho} n={nsteps} walkers={nwalkers} K={K} offset={offset}: window {window}, tau {tau}, rel diff {rel:.2e}")
        worst = max(worst, rel)
    print(f"measured restatement-vs-FFT discrepancy: {worst:.2e}")
    assert worst <= DISCREPANCY_BOUND
    # the figure the GPU tests build their bound on still holds; 2 x, because the FFT side's rounding is numpy's own and another
    # pocketfft build may move it (DISCREPANCY_BOUND above is the requirement, this line only guards the recorded figure)
    assert worst <= 2.0 * MEASURED_DISCREPANCY


def test_cap_rule():
    assert _capi.ACF_MAX_LAG == 4096
    rng = np.random.default_rng(11)
    # n <= K: every lag is known and the monitor never answers NaN / -1.  (All n autocovariances of a series sum to zero, so
    # taus_{n-1} = 0 up to rounding and the last lag ends the search however large c is: whether the window test or the
    # fallback picks it depends on that rounding, and both estimators answer the last lag.)
    x = ar.ar1(rng, 0.98, 40, 8, 2)
    for c in (5.0, 1.0e6):
        tau, window, _ = ar.Monitor(64).feed(x).finalise(c)
        host_tau, host_window = ar.host_tau_window(x, c)
        print(f"n = 40 <= K = 64, c = {c}: window {window} (host {host_window}), tau {tau} (host {host_tau})")
        assert np.array_equal(window, host_window) and np.all(window >= 0)
        assert np.max(np.abs(tau - host_tau)) < DISCREPANCY_BOUND
    assert np.array_equal(window, [39, 39])
    # n > K without a window below K: NaN / -1, never a truncated sum
    x = ar.ar1(rng, 0.98, 5000, 8, 2)
    tau, window, _ = ar.Monitor(32).feed(x).finalise(5.0)
    assert np.all(np.isnan(tau)) and np.array_equal(window, [-1, -1])
    # a window below K: the same tau for every K above it, bit for bit
    x = ar.ar1(rng, 0.5, 3000, 16, 2)
    ref_tau, ref_window, _ = ar.Monitor(3000).feed(x).finalise(5.0)
    assert np.all(ref_window < 40)
    for K in (int(ref_window.max()) + 1, 64, 1000):
        tau, window, _ = ar.Monitor(K).feed(x).finalise(5.0)
        assert np.array_equal(window, ref_window) and np.array_equal(tau, ref_tau), K


def test_accumulators_do_not_depend_on_chunking():
    rng = np.random.default_rng(12)
    x = ar.ar1(rng, 0.9, 700, 6, 3, mean=-2.0)
    K = 128
    whole = ar.Monitor(K).feed(x)
    one = ar.sums_oneshot(x, K)
    ws = whole.sums()
    for key in ("S", "T", "H", "pivot"):
        assert np.array_equal(ws[key], one[key]), key
    assert np.array_equal(ws["tail"], (x - x[0])[-K:])
    for trial in range(5):
        cuts = np.sort(rng.choice(np.arange(1, len(x)), size=int(rng.integers(1, 40)), replace=False))
        m = ar.Monitor(K)
        for part in np.split(x, cuts):
            m.feed(part)
        ps = m.sums()
        for key in ("S", "T", "H", "tail", "pivot"):
            assert np.array_equal(ps[key], ws[key]), (trial, key)
        assert ps["n"] == ws["n"] == len(x)
        for a, b in zip(m.finalise(5.0), whole.finalise(5.0)):
            assert np.array_equal(a, b) and not np.any(np.isnan(a))
    # fewer samples than lags: unknown lags stay zero, H_k = T beyond n, the tail is zero before sample 0
    short = ar.Monitor(K).feed(x[:10]).sums()
    assert np.all(short["S"][10:] == 0.0) and np.array_equal(short["H"][11], short["T"]) and np.all(short["tail"][:K - 10] == 0.0)


def test_convergence_rule():
    tau = np.array([10.0, 12.0])
    assert not autocorr_converged(tau, None, 10 ** 6)                                 # no previous estimate
    assert autocorr_converged(tau, tau * 1.005, 601, tol=50, rtol=0.01)
    assert not autocorr_converged(tau, tau * 1.005, 600, tol=50, rtol=0.01)           # 50 x 12 < 600 is false
    assert not autocorr_converged(tau, tau * np.array([1.0, 1.02]), 5000, rtol=0.01)  # one dimension still moving
    assert autocorr_converged(tau, tau * np.array([1.0, 1.02]), 5000, rtol=0.05)
    assert not autocorr_converged(np.array([10.0, np.nan]), tau, 5000)                # NaN: max_lag too small
    assert not autocorr_converged(tau, np.array([10.0, np.nan]), 5000)
    assert autocorr_converged(np.array([[10.0, 12.0], [11.0, 9.0]]), np.array([[10.0, 12.0], [11.0, 9.0]]), 601)   # several ensembles
    hist = [(100, 8.0), (200, 11.0), (300, 12.5), (400, 12.9), (500, 12.95), (600, 12.96), (700, 12.97)]
    stop = [n for (n, t), (_, tp) in zip(hist[1:], hist[:-1]) if autocorr_converged(np.array([t]), np.array([tp]), n)]
    assert stop == [700]                                                              # 50 x 12.96 = 648 > 600
