"""CPU checks of the posterior monitor's definition: the numpy restatement (tests/post_restated.py) against numpy's own
histograms, moments and argmax where both are defined alike, the corners of the bin rule, the named cases of
tests/post_cases.py (each has the property its name claims), and the host-side summaries of magprop_amd/posterior.py."""
import warnings

import numpy as np
import pytest

import post_cases as pc
import post_restated as pr
from magprop_amd import posterior


# ---------------------------------------------------------------- the restatement against numpy
@pytest.fixture(scope="module")
def inside():
    """1 500 steps of 8 walkers in 3 dimensions, every sample inside [-6, 6) (no sample on or above `upper`)."""
    rng = np.random.default_rng(11)
    chain = np.clip(rng.standard_normal((1500, 8, 3)) * [1.0, 0.5, 2.0] + [0.0, 1.0, -1.0], -5.9, 5.9)
    lnp = -0.5 * np.sum(chain * chain, axis=2)
    return chain, lnp, pr.accumulate(chain, lnp, 50, 20, np.full(3, -6.0), np.full(3, 6.0))


def test_histograms_equal_numpys(inside):
    chain, _, acc = inside
    flat = chain.reshape(-1, 3)
    for d in range(3):
        assert np.array_equal(acc["hist1"][d], np.histogram(flat[:, d], bins=50, range=(-6.0, 6.0))[0])
    assert not acc["below"].any() and not acc["above"].any() and not acc["nonfinite"].any() and acc["n"] == len(flat)
    for p, (a, b) in enumerate(pr.pairs(3)):
        h = np.histogram2d(flat[:, a], flat[:, b], bins=20, range=[(-6.0, 6.0), (-6.0, 6.0)])[0]
        assert np.array_equal(acc["hist2"][p], h.astype(np.int64))
    assert not acc["outside2"].any()


def test_moments_within_the_first_order_bound_of_any_summation_order(inside):
    """mean and covariance from the sequential sums against np.mean / np.cov: |delta| <= n 2^-52 sum|terms| per entry, the
    first-order bound of the difference of two summation orders of the same n terms."""
    chain, _, acc = inside
    flat = chain.reshape(-1, 3)
    n = len(flat)
    assert acc["n_finite"] == n
    y = flat - acc["pivot"]
    u = n * 2.0 ** -52
    assert np.all(np.abs(acc["sum1"] - y.sum(axis=0)) <= u * np.abs(y).sum(axis=0))
    prod = y[:, :, None] * y[:, None, :]
    assert np.all(np.abs(acc["sum2"] - prod.sum(axis=0)) <= u * np.abs(prod).sum(axis=0))
    mean, cov = posterior.mean_cov(acc["sum1"], acc["sum2"], acc["pivot"], n)
    assert np.all(np.abs(mean - flat.mean(axis=0)) <= u * np.abs(y).sum(axis=0) / n + 4e-16 * np.abs(mean))
    ref = np.cov(flat.T)
    # the covariance subtracts s1 s1 / n from s2: both carry the bound above, relative to the sums of absolute terms
    bound = u * (np.abs(prod).sum(axis=0) + np.outer(np.abs(y).sum(axis=0), np.abs(y).sum(axis=0)) / n) / (n - 1)
    assert np.all(np.abs(cov - ref) <= 4.0 * bound)
    assert np.array_equal(acc["sum2"], acc["sum2"].T)


def test_best_sample_equals_numpys_first_argmax(inside):
    chain, lnp, acc = inside
    i = int(np.argmax(lnp.ravel()))
    assert acc["best_idx"] == i and acc["best_lnp"] == lnp.ravel()[i] and np.array_equal(acc["best_x"], chain.reshape(-1, 3)[i])
    assert pr.holder_loop(lnp) == (acc["best_lnp"], acc["best_idx"])


# ---------------------------------------------------------------- the bin rule
def test_bin_rule_corners():
    inv = 256 / 10.0
    code = lambda v: int(pr.bin_code(np.array([v]), -5.0, 5.0, inv, 256)[0])   # noqa: E731
    assert np.floor((pc.BELOW5 + 5.0) * inv) == 256.0        # the clamp matters: without it this sample has no bin
    assert code(pc.BELOW5) == 255
    assert code(-5.0) == 0 and code(np.nextafter(-5.0, -np.inf)) == 256 and code(5.0) == 257 and code(1e300) == 257 and code(-1e300) == 256
    assert code(np.nan) == code(np.inf) == code(-np.inf) == 258
    assert code(0.0) == code(-0.0) == 128
    zero = lambda v: int(pr.bin_code(np.array([v]), 0.0, 1.0, 7.0, 7)[0])     # noqa: E731
    assert zero(-0.0) == 0 and zero(0.0) == 0 and zero(5e-324) == 0 and zero(-5e-324) == 7 and zero(np.nextafter(1.0, 0.0)) == 6
    inv1, inv2, pivot = pr.params(256, 64, [-5.0, 0.0], [5.0, 1.0])
    assert np.array_equal(inv1, [25.6, 256.0]) and np.array_equal(inv2, [6.4, 64.0]) and np.array_equal(pivot, [0.0, 0.5])


# ---------------------------------------------------------------- the named cases
@pytest.mark.parametrize("case", pc.cases(), ids=lambda c: c.name)
def test_case_runs_through_the_restatement(case):
    """Every sample lands in exactly one 1-D counter per dimension and in one 2-D cell or `outside2` per pair; the best sample
    obeys the holder rule one sample at a time; the runs cover the sequence."""
    n = len(case.chain)
    assert case.chain.shape == (n, case.n_walkers * case.n_ensembles, case.ndim) and case.lnp.shape == case.chain.shape[:2]
    assert 1 <= case.bins1 <= pc.MAX_BINS and 0 <= case.bins2 <= pc.MAX_BINS2 and 1 <= case.ndim <= pc.MAX_NDIM
    assert all(sum(rows) == n for rows in case.runs.values())
    for e, acc in enumerate(pc.expected(case.name)):
        total = n * case.n_walkers
        assert np.all(acc["hist1"].sum(axis=1) + acc["below"] + acc["above"] + acc["nonfinite"] == total) and acc["n"] == total
        if case.bins2:
            assert np.all(acc["hist2"].sum(axis=(1, 2)) + acc["outside2"] == total) and len(acc["outside2"]) == case.ndim * (case.ndim - 1) // 2
        chain, lnp = pc.ensemble(case, e)
        assert pr.holder_loop(lnp) == (acc["best_lnp"], acc["best_idx"])
        assert acc["n_finite"] == np.count_nonzero(np.all(np.isfinite(chain), axis=2))
    lay = pc.device_layout(case)
    assert lay["hist1"].shape == (case.n_ensembles, case.ndim, case.bins1 + 3) and lay["mom"].shape[1] == case.chain.shape[1]


def test_cases_have_the_property_their_name_claims():
    acc = pc.expected("one-bin-70000")[0]
    assert acc["n"] == 70000 > 2 ** 16 and np.all(acc["hist1"][:, 135] == 70000) and acc["hist2"][0, 33, 33] == 70000
    e = pc.expected("edges")[0]
    # dimension 0: -5 -> bin 0, 5 -> above, the largest double below 5 -> bin 255 by the clamp, just below -5 -> below
    assert e["hist1"][0, 0] == 2 and e["hist1"][0, 255] == 2 and e["above"][0] == 1 and e["below"][0] == 1 and e["hist1"][0, 128] == 2
    # dimension 1: -0.0, 0.0 and the smallest subnormal -> bin 0; minus the subnormal -> below; 1 -> above
    assert e["hist1"][1, 0] == 3 and e["below"][1] == 1 and e["above"][1] == 1 and e["hist1"][1, 255] == 1
    one, every = pc.expected("nonfinite-one-coordinate")[0], pc.expected("nonfinite-all-coordinates")[0]
    assert one["nonfinite"].tolist() == [0, 0, 3] and one["n_finite"] == one["n"] - 3 and one["outside2"][0] < one["outside2"][1]
    assert every["nonfinite"].tolist() == [4, 4, 4] and every["n_finite"] == every["n"] - 4
    assert np.all(np.isfinite(one["mom"])) and np.all(np.isfinite(every["mom"]))
    for acc in pc.expected("lnprob-all-minus-inf"):
        assert acc["best_idx"] == -1 and acc["best_lnp"] == -np.inf and np.all(np.isnan(acc["best_x"]))
    assert [a["best_idx"] for a in pc.expected("lnprob-nan-among-finite")][0] == 2 * 6 + 1
    assert all(a["best_idx"] == 70 * 34 + 5 and a["best_lnp"] == 1.0 for a in pc.expected("lnprob-tie"))
    last = pc.expected("lnprob-max-in-last-row")
    assert last[0]["best_idx"] == last[2]["best_idx"] == 193 * 34 - 1 and last[1]["best_idx"] < 193 * 34 - 34
    assert {c.n_walkers for c in pc.cases()} >= {2, 34, 64, 66} and {c.ndim for c in pc.cases()} >= {1, 6, 9}
    assert {c.bins1 for c in pc.cases()} >= {1, 7, 4096} and {c.bins2 for c in pc.cases()} >= {0, 1, 128}
    assert any(c.ndim == 9 and c.bins2 == 128 for c in pc.cases()) and {c.n_ensembles for c in pc.cases()} >= {1, 3}
    assert any(r == pc.SPLIT for c in pc.cases() for r in c.runs.values()) and pc.by_name("one-row").runs == {"whole": [1]}


# ---------------------------------------------------------------- magprop_amd/posterior.py
@pytest.mark.parametrize("n", [2000, 100000])
def test_hist_quantiles_within_one_bin_width_of_numpys(n):
    """Standard normals in 256 bins over [-5, 5): the interpolated quantile and np.quantile both lie in the bin that holds rank
    q n or beside it, so they differ by less than one bin width (the worst seen over 20 seeds was 0.21 of a width)."""
    q = (0.16, 0.5, 0.84)
    width = 10.0 / 256
    worst = 0.0
    for seed in range(20):
        x = np.random.default_rng(seed).standard_normal(n)
        acc = pr.accumulate(x.reshape(n // 2, 2, 1), np.zeros((n // 2, 2)), 256, 0, [-5.0], [5.0])
        got = posterior.hist_quantiles(acc["hist1"], acc["below"], acc["above"], [-5.0], [5.0], q)
        assert got.shape == (3, 1)
        worst = max(worst, float(np.max(np.abs(got[:, 0] - np.quantile(x, q)))) / width)
    print(f"n = {n}: worst |hist_quantiles - np.quantile| = {worst:.3f} bin widths")
    assert worst <= 1.0


def test_hist_quantiles_of_a_flat_histogram_and_a_too_narrow_range():
    h = np.array([[10, 10, 10, 10]])
    got = posterior.hist_quantiles(h, [0], [0], [0.0], [4.0], (0.0, 0.25, 0.5, 0.625, 1.0))
    assert np.allclose(got[:, 0], [0.0, 1.0, 2.0, 2.5, 4.0], rtol=0, atol=1e-15)
    assert posterior.hist_quantiles(h[0], 0, 0, 0.0, 4.0, 0.5).shape == (1,)
    # 30 % of the samples below the range, 20 % above: 0.16 and 0.84 cannot be placed
    two = np.array([[25, 25], [50, 50]])
    with pytest.warns(RuntimeWarning, match="dimension 0") as rec:
        got = posterior.hist_quantiles(two, [30, 0], [20, 0], [0.0, 0.0], [1.0, 1.0], (0.16, 0.5, 0.84))
    assert len(rec) == 2 and "below" in str(rec[0].message) and "above" in str(rec[1].message)
    assert np.isnan(got[0, 0]) and np.isnan(got[2, 0]) and got[1, 0] == pytest.approx(0.4) and np.allclose(got[:, 1], (0.16, 0.5, 0.84))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert np.all(np.isnan(posterior.hist_quantiles(np.zeros((1, 4)), [0], [0], [0.0], [1.0], (0.5,))))      # empty: NaN, no warning
    with pytest.raises(ValueError, match="quantile"):
        posterior.hist_quantiles(h, [0], [0], [0.0], [4.0], (1.5,))


def test_hist2_levels_on_a_hand_made_table():
    h = np.array([[1, 2, 1], [2, 40, 30], [1, 20, 3]])          # total 100; downwards: 40 30 20 3 2 2 1 1 1
    assert posterior.hist2_levels(h, (0.393, 0.865)).tolist() == [40.0, 20.0]
    assert posterior.hist2_levels(h, (0.4, 0.41, 0.9, 0.931, 1.0)).tolist() == [40.0, 30.0, 20.0, 2.0, 1.0]
    assert np.all(np.isnan(posterior.hist2_levels(np.zeros((3, 3)))))


def test_edges_and_mean_cov():
    assert np.array_equal(posterior.edges(-1.0, 1.0, 4), [-1.0, -0.5, 0.0, 0.5, 1.0])
    e = posterior.edges([0.0, -5.0], [1.0, 5.0], 256)
    assert e.shape == (2, 257) and np.array_equal(e[:, 0], [0.0, -5.0]) and np.array_equal(e[:, -1], [1.0, 5.0]) and e[1, 128] == 0.0
    x = np.array([[1.0, 2.0], [3.0, 5.0], [2.0, 2.0], [6.0, 3.0]])
    y = x - [3.0, 3.0]
    mean, cov = posterior.mean_cov(y.sum(axis=0), y.T @ y, [3.0, 3.0], 4)
    assert np.allclose(mean, x.mean(axis=0), rtol=0, atol=1e-15) and np.allclose(cov, np.cov(x.T), rtol=0, atol=1e-14)
    assert np.allclose(posterior.mean_cov(y.sum(axis=0), y.T @ y, [3.0, 3.0], 4, ddof=0)[1], np.cov(x.T, ddof=0), rtol=0, atol=1e-14)
    assert np.all(np.isnan(posterior.mean_cov(np.zeros(2), np.zeros((2, 2)), np.zeros(2), 0)[0]))


def test_ensemble_range_arithmetic():
    pos = np.array([[0.0, 10.0, -1.0], [1.0, 14.0, -3.0], [0.5, 12.0, -2.0]])
    lo, hi = posterior.ensemble_range(pos, [-10.0, 9.0, -4.5], [10.0, 17.0, 0.0])
    # [min - span, max + span]: [-1, 2], [6, 18], [-5, 1], clipped to the box
    assert np.array_equal(lo, [-1.0, 9.0, -4.5]) and np.array_equal(hi, [2.0, 17.0, 0.0])
    lo, hi = posterior.ensemble_range(pos.reshape(3, 1, 3), np.full(3, -100.0), np.full(3, 100.0))
    assert np.array_equal(lo, [-1.0, 6.0, -5.0]) and np.array_equal(hi, [2.0, 18.0, 1.0])
    stuck = pos.copy()
    stuck[:, 1] = 12.0
    with pytest.raises(ValueError, match="differ in every dimension"):
        posterior.ensemble_range(stuck, np.full(3, -100.0), np.full(3, 100.0))
    with pytest.raises(ValueError, match="outside the box"):
        posterior.ensemble_range(pos, [5.0, 9.0, -4.5], [10.0, 17.0, 0.0])
