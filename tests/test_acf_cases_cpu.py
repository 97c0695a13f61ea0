"""CPU side of tests/acf_cases.py: every case runs through the restatement (tests/acf_restated.py) and has the property its name
claims; every run of a case (chunking, intermediate finalisations) gives the same sums and estimates; a NaN or an infinity
poisons its own (ensemble, dimension) only; and the restatement is held against the textbook definition in np.longdouble
(acf_cases.textbook: the autocovariance about the full-series mean, the walker mean, the header's window rule).
tests/test_gpu_acf_kernels.py holds the kernels to the restatement bit for bit on the same cases, so the comparison below is what
says that the restatement itself is right.

Measured restatement-vs-long-double discrepancy (test_restatement_agrees_with_the_long_double_definition; x86-64, 80-bit long
double): the largest |tau - tau_ld| / max(1, |tau_ld|) over the compared cases is 1.06e-12, at `ar1-rho0.5-pivot-30sigma`, whose
pivot sits 30 standard deviations from the mean so that the moment form cancels three digits; next come `mean-1e8` with 2.4e-13
and one ensemble of `series-254-w2-e127-d1` with 8.2e-14, every other case is below 6e-14.  All of it is far below DISCREPANCY_BOUND = 1e-9, which every
compared case is required to meet; MEASURED_LD_DISCREPANCY records the figure and the test guards it with a factor of 2.
The difference is taken relative to max(1, |tau|) because taus_M = 2 (f_0 + ... + f_M) - 1 is a sum of terms of size f_0 = 1:
where it cancels to about zero (a chain no longer than max_lag: all n autocovariances sum to zero) its rounding error is that of
the terms, not of the result.  At mean 1e8 the restatement and the FFT estimator differ by 7e-10, the restatement and the long-
double definition by 2.4e-13: the 7e-10 is the FFT estimator's, which subtracts a mean of 1e8 in double.  (Of the 2.4e-13 a
good part is the long-double side's own: one unit of its last place at 1e8 is 7e-12, and x - mean carries that as a common
shift; the restatement's y = x - x_0 is exact.)

Cases left out of the comparison of values, all degenerate (their tau is NaN, or -1 from rho = 0 everywhere): VALUE_EXCLUDED
below, by name.  Every other case is compared."""
import numpy as np
import pytest

import acf_cases as ac
import acf_restated as ar
from test_autocorr_cpu import DISCREPANCY_BOUND

CASES = ac.CASES
VALUE_EXCLUDED = ("scale-1e-170-underflows", "scale-1e160-overflows", "all-constant", "one-nan-at-t40-e1-w2-d1", "one-inf-at-t40-e1-w2-d1",
                  "one-nan-at-t0-e0-w3-d2", "one-nan-at-t119-e1-w0-d0")
MEASURED_LD_DISCREPANCY = 1.1e-12   # the module docstring
TIE_MARGIN = 1.0e-6             # |M - c taus_M| / max(1, M) at the window and the lag before it: 1000 x DISCREPANCY_BOUND


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    """The same bits everywhere but in NaNs, and NaNs at the same places."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != np.float64:
        return a.dtype == b.dtype and np.array_equal(a, b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(_bits(a)[~np.isnan(a)], _bits(b)[~np.isnan(b)])


def restated_taus(c, e, K=None):
    """(tau, window, taus[lim][ndim]) of ensemble e by the restatement with K lags (default: the case's max_lag)."""
    with np.errstate(all="ignore"):
        tau, window, f = ar.Monitor(c.max_lag if K is None else K).feed(ac.ensemble(c, e)).finalise(c.c)
        return tau, window, 2.0 * np.cumsum(f, axis=0) - 1.0


def test_the_list_covers_what_it_promises():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    for c in CASES:
        assert len({r.name for r in c.runs}) == len(c.runs) >= 2, c.name
    assert {c.max_lag for c in CASES} >= {1, 2, 15, 16, 17, 31, 32, 33, 100, ac.ACF_MAX_LAG}
    assert {ac.n_series(c) for c in CASES} >= {2, ac.THREADS - 2, ac.THREADS, ac.THREADS + 2, 2 * ac.THREADS - 2, 2 * ac.THREADS, 2 * ac.THREADS + 2}
    assert {c.ndim for c in CASES} >= {1, ac.MAX_NDIM} and {c.n_ensembles for c in CASES} >= {1, 2, 3, 127}
    assert {c.c for c in CASES} >= {1.0e-3, 1.0, 5.0, 1.0e6}
    assert {c.kind for c in CASES} >= set(ac.DEGENERATE_KINDS)
    assert {c.name for c in CASES if c.kind in ac.DEGENERATE_KINDS} == set(VALUE_EXCLUDED)
    # small: the GPU module runs in seconds
    for c in CASES:
        big = c.max_lag == ac.ACF_MAX_LAG
        assert (len(c.x) <= 400 and ac.n_series(c) <= 514 and c.max_lag <= 128) or (big and ac.n_series(c) <= 4), c.name
    K, kp = 17, 32
    lengths = {len(c.x) for c in CASES if c.kind == "length"}
    assert lengths == {2, 15, 16, 17, K + 1, kp, kp + 1, kp + 17 - 1, kp + 17 + 1, 3 * (kp + 17)}       # ring of the runs by 17: 49
    assert K - 1 in lengths and K in lengths
    runs = [(c, r) for c in CASES for r in c.runs]
    for c, r in runs:
        kp = ac.kp_of(c.max_lag)
        assert sum(r.chunk_rows) == len(c.x) and len(r.lead) == len(r.finalise_after) == len(r.chunk_rows)
        assert r.ring_rows == kp + max(r.chunk_rows) and 0 <= r.head0 < r.ring_rows and min(r.chunk_rows) >= 0
        assert set(r.lead) <= set(ac.LEADS)
    for c in CASES:
        rings = [r.ring_rows for r in c.runs]
        assert {r.head0 for r in c.runs} >= {0} and any(r.head0 == r.ring_rows - 1 for r in c.runs), c.name
        assert any(0 < r.head0 < r.ring_rows - 1 for r in c.runs) or max(rings) <= 2 or len(c.runs) == 2, c.name
        assert any(any(r.finalise_after) for r in c.runs) and any(not any(r.finalise_after) for r in c.runs), c.name
        assert any(r.chunk_rows == [len(c.x)] for r in c.runs), c.name
        assert len(c.runs) < 4 or {x for r in c.runs for x in r.lead} == set(ac.LEADS), c.name
    assert {x for _, r in runs for x in r.chunk_rows} >= set(ac.CHUNK_LENGTHS) | {0}
    assert any(set(r.chunk_rows) == {1} for _, r in runs)
    # every geometry case has a chunked run that wraps its ring at least twice, many of them far more often
    for c in CASES:
        if c.kind == "geometry":
            assert max(ac.wraps(r) for r in c.runs) >= 2 + (c.max_lag < 100), c.name
    assert max(ac.wraps(r) for _, r in runs) >= 9
    # chunks that end exactly on the ring's last row, and chunks that straddle it
    for c, r in runs:
        h = ac.heads_of(r)
        if r.name.startswith("ends-on-last-row"):
            assert h[1] != 0 and h[2] == 0 and r.chunk_rows[1] > 0
        if r.name.startswith("straddles-last-row"):
            assert 0 < h[2] < h[1] and h[2] < r.chunk_rows[1]
    assert sum(r.name.startswith("ends-on-last-row") for _, r in runs) >= 2 and sum(r.name.startswith("straddles") for _, r in runs) >= 2


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_case_has_the_property_its_name_claims(case):
    c, x, n, K, kp = case, case.x, len(case.x), case.max_lag, ac.kp_of(case.max_lag)
    want = ac.expected(c)
    tau, window = want["tau"].reshape(c.n_ensembles, c.ndim), want["window"].reshape(c.n_ensembles, c.ndim)
    lim = min(n, K)
    # what is defined and what is not, in every case
    assert np.all(_bits(want["f"][:, lim:]) == _bits(ac.NAN_CANARY)) and not np.any(_bits(want["f"][:, :lim]) == _bits(ac.NAN_CANARY))
    assert np.all(want["rho"][min(n, kp):] == 0.0) and np.all(want["H"][min(n, kp - 1) + 1:] == 0.0)
    assert same(want["pivot"], x[0].ravel())
    if c.kind not in ac.DEGENERATE_KINDS:
        assert np.all(np.isfinite(x))
    if c.kind in ("geometry", "n-series", "binades", "sum-order"):
        # no two series alike: every series has its own c_0 and its own rho_1
        s0 = want["S"][0]
        assert np.unique(s0).size == s0.size and (K <= 2 or np.mean(np.isfinite(tau) & (window > 0)) >= (0.75 if c.n_walkers == 2 else 1.0))
        if kp > 1 and n > 1:
            assert np.unique(want["rho"][1]).size == s0.size
    if c.kind in ("binades", "sum-order"):
        # the walker mean in reverse order gives other bits
        for e in range(c.n_ensembles):
            with np.errstate(all="ignore"):
                rho = ar.Monitor(K).feed(ac.ensemble(c, e)).finalise(c.c, with_rho=True)[3]
            fwd = np.cumsum(rho, axis=1)[:, -1]
            rev = np.cumsum(rho[:, ::-1], axis=1)[:, -1]
            assert np.any(fwd != rev), e
        if c.kind == "binades":
            sd = x.std(axis=0)
            assert sd.max() / sd.min() > 2.0 ** 30
    if c.kind == "pivot":
        assert np.all(np.abs(x[0] - x.mean(axis=0)) > 20.0 * x[50:].std(axis=0))
    if c.kind == "mean":
        assert np.all(np.abs(x.mean(axis=0)) > 0.99e8) and np.all(np.isfinite(tau))
    if c.kind == "scale":
        assert np.all(np.isfinite(tau)) and np.all(window > 0)
        s = want["S"][0]
        assert s.max() < 1.0e-290 or s.min() > 1.0e290
    if c.kind in ("underflow", "constant"):
        assert np.all(want["S"] == 0.0) and np.all(want["rho"] == 0.0)
        assert np.all(tau == -1.0) and np.all(window == 0)
        assert (c.kind == "constant") == bool(np.all(want["T"] == 0.0))
    if c.kind == "overflow":
        assert np.all(np.isinf(want["S"][0])) and np.all(np.isnan(tau))
    if c.kind == "stuck":
        stuck = np.all(x == x[0], axis=0)
        assert stuck.sum() == c.ndim and np.all(stuck[2]) and np.all(np.isfinite(tau))
        assert np.all(want["rho"].reshape(kp, -1, c.ndim)[:, 2] == 0.0) and np.all(want["f"][:, 0] == 0.75)
    if c.kind == "late":
        assert np.all(x[:-1, 1] == x[0, 1]) and np.all(x[-1, 1] != x[0, 1]) and np.all(np.isfinite(tau))
        assert np.all(want["S"].reshape(kp, -1, c.ndim)[1:, 1] == 0.0) and np.all(want["S"].reshape(kp, -1, c.ndim)[0, 1] > 0.0)
    if c.kind in ("nan", "inf"):
        t, e, w, d = c.poison
        bad = x[t, e * c.n_walkers + w, d]
        assert (np.isnan(bad) if c.kind == "nan" else bad == np.inf) and np.sum(~np.isfinite(x)) == 1
    if c.kind == "last-lag":
        # n <= max_lag, and M < c taus_M holds at every known lag: the window is the fallback's, whatever c
        assert n <= K
        for e in range(c.n_ensembles):
            _, win, taus = restated_taus(c, e)
            assert np.all(np.arange(n)[:, None] < c.c * taus) and np.all(win == n - 1)
        assert np.all(np.isfinite(tau)) and np.all(window == n - 1)
    if c.kind == "no-window":
        assert n == K + 1 and np.all(np.isnan(tau)) and np.all(window == -1)
        for e in range(c.n_ensembles):
            assert np.all(np.arange(K)[:, None] < c.c * restated_taus(c, e)[2])
    if c.kind == "padding":
        assert K % ac.LAG_BLOCK and n > kp and np.all(np.isnan(tau)) and np.all(window == -1)
        for e in range(c.n_ensembles):
            wide_tau, wide_window, _ = restated_taus(c, e, K=kp)
            assert np.all((wide_window >= K) & (wide_window < kp)) and np.all(np.isfinite(wide_tau))
    if c.kind == "c":
        assert np.all(window == 1) if c.c == 1.0e-3 else np.all(window > 0) if c.c == 1.0 else np.all(window == -1)
    if c.kind == "n2":
        assert n == 2
        if K == 1:
            assert np.all(np.isnan(tau)) and np.all(window == -1)
        else:
            assert np.all(window == 1) and np.all(np.isfinite(tau))
    if c.kind == "max-lag":
        assert K == ac.ACF_MAX_LAG and n > K and np.all(np.isfinite(tau)) and np.all(window > 0)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_every_run_gives_the_same_sums_and_estimates(case):
    """The restatement fed in the chunks of every run, finalised in between where the run says so, against the expectation
    (which is fed the whole sequence at once): S, T, H, pivot, rho, f, tau and window, NaNs equal by position; and the ring of
    every run holds the last samples where the header says."""
    c, n, K, kp = case, len(case.x), case.max_lag, ac.kp_of(case.max_lag)
    want = ac.expected(c)
    w = c.n_walkers * c.ndim
    y = c.x.reshape(n, -1) - c.x.reshape(n, -1)[0] if np.all(np.isfinite(c.x[0])) else None
    for r in c.runs:
        with np.errstate(all="ignore"):
            for e in range(c.n_ensembles):
                wide, est = ar.Monitor(kp), ar.Monitor(K)
                t = 0
                for rows, fin in zip(r.chunk_rows, r.finalise_after):
                    for m in (wide, est):
                        m.feed(ac.ensemble(c, e)[t:t + rows])
                    t += rows
                    if fin and t >= 2:
                        est.finalise(r.c_mid)
                cols = slice(e * w, (e + 1) * w)
                assert same(wide.S.reshape(kp, w), want["S"][:, cols]) and same(wide.H.reshape(kp, w), want["H"][:, cols]), r.name
                assert same(wide.T.ravel(), want["T"][cols]) and same(wide.pivot.ravel(), want["pivot"][cols]), r.name
                rho = wide.finalise(c.c, with_rho=True)[3]
                assert same(rho.reshape(len(rho), w), want["rho"][:len(rho), cols]), r.name
                tau, window, f = est.finalise(c.c)
                dims = slice(e * c.ndim, (e + 1) * c.ndim)
                assert same(tau, want["tau"][dims]) and same(window, want["window"][dims]) and same(f.T, want["f"][dims, :len(f)]), r.name
                # the lags below max_lag do not depend on how many lags are kept
                assert same(wide.finalise(c.c)[2][:len(f)], f), r.name
        ring = ac.expected_hist(c, r)
        held = min(n, r.ring_rows)
        assert ring.shape == (r.ring_rows, ac.n_series(c))
        if y is not None:
            assert same(ring[(r.head0 + n - 1) % r.ring_rows], y[n - 1]) and same(ring[(r.head0 + n - held) % r.ring_rows], y[n - held])
            rows = (r.head0 + np.arange(n - held, n)) % r.ring_rows
            assert same(ring[rows], y[n - held:]) and np.all(np.delete(ring, rows, axis=0) == 0.0)


@pytest.mark.parametrize("case", [c for c in CASES if c.poison], ids=lambda c: c.name)
def test_a_nan_or_an_infinity_poisons_its_own_dimension_only(case):
    got, clean = ac.expected(case), ac.expected(ac.BY_NAME[case.base])
    t, e, w, d = case.poison
    one = e * case.ndim + d
    assert np.isnan(got["tau"][one]) and np.all(np.isnan(got["f"][one, :min(len(case.x), case.max_lag)]))
    others = np.delete(np.arange(case.n_ensembles * case.ndim), one)
    assert np.all(np.isfinite(clean["tau"]))
    for key in ("tau", "window", "f"):
        assert same(got[key][others], clean[key][others]), key
    j = (e * case.n_walkers + w) * case.ndim + d
    series = np.delete(np.arange(ac.n_series(case)), j)
    for key in ("S", "H", "rho"):
        assert same(got[key][:, series], clean[key][:, series]), key
    for key in ("T", "pivot"):
        assert same(got[key][series], clean[key][series]), key
    assert np.any(np.isnan(got["rho"][:, j]))


def test_restatement_agrees_with_the_long_double_definition():
    """tau of the restatement against the textbook definition in long double on every case but VALUE_EXCLUDED; windows equal on
    every one of them, none sitting on a rounding tie of M < c taus_M (the margin at the window and at the lag before it is
    checked; the last lag of a chain with n <= max_lag is exempt from the margin, not from the equality: all n autocovariances
    sum to zero, so taus_{n-1} is rounding, and the window test and the fallback both answer n - 1)."""
    assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble is no wider than double here: the reference needs its 64 bits"
    worst = 0.0
    for c in CASES:
        if c.name in VALUE_EXCLUDED:
            continue
        n, K = len(c.x), c.max_lag
        for e in range(c.n_ensembles):
            tau, window, taus = restated_taus(c, e)
            ld_tau, ld_window, _ = ac.textbook(ac.ensemble(c, e), c.c, K)
            assert np.array_equal(window, ld_window), (c.name, e, window, ld_window)
            for d in range(c.ndim):
                M = int(window[d])
                for k in ((M - 1, M) if M >= 0 else (min(n, K) - 1,)):
                    if k < 0 or (n <= K and k == n - 1):
                        continue
                    assert abs(k - c.c * taus[k, d]) > TIE_MARGIN * max(1.0, k), (c.name, e, d, k)
            assert np.array_equal(np.isnan(tau), np.isnan(ld_tau)), c.name
            ok = ~np.isnan(tau)
            rel = float(np.max(np.abs(tau[ok] - ld_tau[ok]) / np.maximum(1.0, np.abs(ld_tau[ok])), initial=0.0))
            worst = max(worst, rel)
            if rel > 6e-14 or c.kind == "mean":
                print(f"{c.name} ensemble {e}: window {window}, tau {tau}, differs from long double by {rel:.2e}")
    print(f"measured restatement-vs-long-double discrepancy: {worst:.2e}")
    assert worst <= DISCREPANCY_BOUND
    assert worst <= 2.0 * MEASURED_LD_DISCREPANCY        # 2 x: another libm or numpy build may move the recorded figure
