"""The summary functions of magprop_amd.calibration on a conjugate model where calibration is exact, without a GPU: theta ~ N(0, 1),
y ~ N(theta, 1), so the posterior is N(y / 2, 1 / 2); 6 independent parameters, 500 posterior draws per dataset, 256 datasets.

The thresholds come from the KS law, not from the draws: a calibrated set of PIT values exceeds kstwo.ppf(0.999, 256) = 0.1210
with probability 1e-3 per parameter; a posterior narrowed to half its sd has PIT values u = Phi(2 z) whose law lies 0.16 from
the uniform one (at u = 0.1: Phi(-0.64) - 0.1), a posterior shifted by 0.7 sd 0.27 (Phi(0.7 / 2) - Phi(-0.7 / 2)).  Checked on
the CPU at the seed used here (20260101) and at seeds 0 .. 49: the calibrated case stays below 0.109 on every parameter, the
narrowed case never falls below 0.137, the shifted case never below 0.205."""
import numpy as np
import pytest
from scipy import stats

from magprop_amd import calibration as cal

N_DATASETS, NDIM, DRAWS, SEED = 256, 6, 500, 20260101
SD = np.sqrt(0.5)


def _study(seed=SEED, narrow=1.0, shift=0.0, n=N_DATASETS):
    """(truths (n, NDIM), posterior draws (n, DRAWS, NDIM)): the exact posterior, its sd scaled by narrow, its mean moved by shift sd"""
    rng = np.random.default_rng(seed)
    theta = rng.standard_normal((n, NDIM))
    y = theta + rng.standard_normal((n, NDIM))
    return theta, y[:, None, :] / 2.0 + shift * SD + narrow * SD * rng.standard_normal((n, DRAWS, NDIM))


@pytest.fixture(scope="module")
def exact():
    theta, draws = _study()
    return theta, draws, cal.pit_from_samples(draws, theta)


def test_the_calibrated_case_passes_on_every_parameter(exact):
    theta, draws, pit = exact
    assert pit.shape == (N_DATASETS, NDIM)
    ks, pv = cal.uniformity(pit)
    crit = stats.kstwo.ppf(0.999, N_DATASETS)
    print("calibrated KS", ks, "critical", crit)
    assert np.all(ks < crit) and np.all(pv > 1.0e-3)
    s = cal.summarize(pit, (draws.mean(axis=1) - theta) / draws.std(axis=1, ddof=1), 1.0 - draws.var(axis=1, ddof=1) / 1.0)
    assert np.all(s["calibrated"]) and np.allclose(s["ks"], ks) and np.allclose(s["ks_critical"], crit)
    assert np.all(np.abs(s["z_mean"]) < 5.0 / np.sqrt(N_DATASETS)) and np.all(np.abs(s["z_sd"] - 1.0) < 0.25)
    assert np.all(np.abs(s["contraction_median"] - 0.5) < 0.05)           # var_post / var_prior = 1 / 2
    for c in s["coverage"]:
        assert np.all(c["inside"]), c


def test_a_narrowed_posterior_is_flagged_on_every_parameter():
    theta, draws = _study(narrow=0.5)
    ks, pv = cal.uniformity(cal.pit_from_samples(draws, theta))
    print("narrowed KS", ks)
    assert np.all(ks > stats.kstwo.ppf(0.999, N_DATASETS)) and np.all(pv < 1.0e-3)
    cov = cal.coverage(cal.pit_from_samples(draws, theta))
    assert all(not np.any(c["inside"]) and np.all(c["observed"] < c["level"]) for c in cov)     # the intervals hold the truth too rarely


def test_a_shifted_posterior_is_flagged_on_every_parameter():
    theta, draws = _study(shift=0.7)
    pit = cal.pit_from_samples(draws, theta)
    ks, pv = cal.uniformity(pit)
    print("shifted KS", ks)
    assert np.all(ks > stats.kstwo.ppf(0.999, N_DATASETS)) and np.all(pv < 1.0e-3)
    assert not np.any(cal.summarize(pit)["calibrated"])
    assert np.all(np.mean(pit, axis=0) < 0.4)                             # the truths sit low in posteriors that sit high


def test_pit_from_histogram_agrees_to_the_mass_of_the_truths_bin(exact):
    theta, draws, pit = exact
    lo, hi, bins = -6.0, 6.0, 64
    worst = 0.0
    for i in range(0, N_DATASETS, 8):
        edges = np.linspace(lo, hi, bins + 1)
        hist = np.stack([np.histogram(draws[i, :, d], edges)[0] for d in range(NDIM)])
        below, above = (draws[i] < lo).sum(axis=0), (draws[i] >= hi).sum(axis=0)
        u, res = cal.pit_from_histogram(hist, below, above, lo, hi, theta[i])
        k = np.clip(np.floor((theta[i] - lo) / (hi - lo) * bins).astype(int), 0, bins - 1)
        assert np.allclose(res, hist[np.arange(NDIM), k] / DRAWS)
        assert np.all(np.abs(u - pit[i]) <= res + 1.0e-12), (i, u, pit[i], res)
        worst = max(worst, float(np.max(np.abs(u - pit[i]))))
    print("histogram PIT: worst difference", worst)
    # a finer histogram is a better PIT; one bin per sample at most is the sample PIT to 1 / n
    fine = np.stack([np.histogram(draws[0, :, d], np.linspace(lo, hi, 100001))[0] for d in range(NDIM)])
    u, res = cal.pit_from_histogram(fine, np.zeros(NDIM), np.zeros(NDIM), lo, hi, theta[0])
    assert np.all(np.abs(u - pit[0]) <= 1.0 / DRAWS + 1.0e-12)
    # a truth outside the range has no PIT; the mass on its side is reported
    u, res = cal.pit_from_histogram(fine, np.full(NDIM, 25), np.zeros(NDIM), lo, hi, np.full(NDIM, -7.0))
    assert np.all(np.isnan(u)) and np.allclose(res, 25.0 / (DRAWS + 25))


def test_pit_from_samples_shapes():
    assert cal.pit_from_samples(np.array([1.0, 2.0, 3.0, 4.0]), 2.5) == pytest.approx(0.5)
    s = np.arange(12.0).reshape(6, 2)
    assert np.allclose(cal.pit_from_samples(s, [4.0, 100.0]), [2.0 / 6.0, 1.0])
    assert cal.pit_from_samples(np.stack([s, s]), np.array([[4.0, 100.0], [-1.0, 5.0]])).tolist() == [[2.0 / 6.0, 1.0], [0.0, 2.0 / 6.0]]


def test_coverage_on_hand_made_pit_values():
    pit = np.array([0.5, 0.17, 0.83, 0.15, 0.85, 0.03, 0.97, 0.02, 0.98, np.nan])
    c68, c95 = cal.coverage(pit)
    assert c68["n"][0] == 9 and c68["count"][0] == 3 and c68["observed"][0] == pytest.approx(3.0 / 9.0)     # 0.5, 0.17, 0.83 lie in [0.16, 0.84]
    assert c95["count"][0] == 7 and c95["observed"][0] == pytest.approx(7.0 / 9.0)                          # all but 0.02, 0.98
    lo, hi = stats.binom.interval(0.95, 9, 0.68)
    assert c68["expected"][0][0] == pytest.approx(lo / 9.0) and c68["expected"][1][0] == pytest.approx(hi / 9.0)
    assert bool(c68["inside"][0]) == (lo <= 3 <= hi)
    two = cal.coverage(np.column_stack([np.full(100, 0.5), np.linspace(0.0, 1.0, 100)]), levels=(0.5,))[0]
    assert two["count"].tolist() == [100, 50] and two["inside"].tolist() == [False, True]


def test_rank_histogram():
    counts, (lo, hi) = cal.rank_histogram(np.column_stack([np.linspace(0.0, 1.0, 200), np.full(200, 0.999)]), bins=10)
    assert counts.shape == (2, 10) and counts[0].sum() == 200 and counts[1].tolist() == [0] * 9 + [200]
    assert np.all((counts[0] >= lo[0]) & (counts[0] <= hi[0])) and counts[0, -1] == 20     # u = 1 goes into the last bin
