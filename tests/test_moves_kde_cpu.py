"""CPU checks of the KDE move (include/magprop_amd.h MP_MOVE_KDE): KDEMove's arguments and table codes, the restatement
(tests/kde_restated.py) against scipy.stats.gaussian_kde, and that it samples a correlated 6-d Gaussian in the restated step
loop (tests/sampler_restated.py) -- and fails to with its Hastings term zeroed."""
import math

import numpy as np
import pytest

from kde_restated import KDE, bandwidth, correlated_gaussian_nd, fit, log_kernel_sum
from sampler_restated import run

# 6-d Gaussian, unit variances, correlation 0.4 between neighbours
COV6 = np.eye(6) + 0.4 * (np.eye(6, k=1) + np.eye(6, k=-1))
# 64 walkers x 800 steps, the first 200 discarded (~38 000 draws; tau of a few steps): mean within 0.1, variance within 10 %,
# neighbour correlation within 0.05
MEAN_TOL, VAR_TOL, CORR_TOL = 0.1, 0.1, 0.05


def test_kde_move_arguments_and_codes():
    from magprop_amd import DEMove, KDEMove, moves
    import magprop_amd
    assert "KDEMove" in magprop_amd.__all__
    assert KDEMove.kind == moves.MOVE_KDE == KDE == 3
    assert KDEMove().params(6) == (0.0, 0.0) and KDEMove("scott").params(6) == (0.0, 0.0)
    assert KDEMove("silverman").params(6) == (-1.0, 0.0)
    assert KDEMove(0.5).params(6) == (0.5, 0.0) and KDEMove(2).params(3) == (2.0, 0.0)
    assert KDEMove() == KDEMove("scott") and KDEMove() != KDEMove("silverman") and KDEMove(0.5) == KDEMove(0.5)
    assert KDEMove() != DEMove() and "silverman" in repr(KDEMove("silverman"))
    for bad in ("walk", "Scott", "", 0.0, -0.5, float("nan"), float("inf"), True, [1.0], object()):
        with pytest.raises(ValueError):
            KDEMove(bad)
    assert moves.parse_spec("kde:0.5,de:0.5") == [(KDEMove(), 0.5), (DEMove(), 0.5)]
    assert moves.parse_spec("kde") == [(KDEMove(), 1.0)]
    with pytest.raises(ValueError):
        moves.parse_spec("walk:1")
    kinds, weights, params = moves.move_table([(KDEMove("silverman"), 0.8), (DEMove(), 0.2)], 6)
    assert kinds == [3, 1] and weights == [0.8, 0.2] and params == [(-1.0, 0.0), (0.0, 1.0e-5)]
    assert moves.move_table(KDEMove(0.3), 6) == ([3], [1.0], [(0.3, 0.0)])


@pytest.mark.parametrize("bw", [None, "silverman", 0.35])
def test_restated_kernel_density_against_scipy(bw):
    """factor, kernel covariance and ln KDE(x) - ln KDE(q) of the restatement against scipy.stats.gaussian_kde, to 1e-12."""
    from scipy.stats import gaussian_kde
    rng = np.random.default_rng(11)
    for n, d in ((32, 6), (7, 6), (200, 2)):
        pts = rng.normal(size=(n, d)) @ np.linalg.cholesky(COV6[:d, :d]).T + 0.3
        k = gaussian_kde(pts.T, bw_method=bw)
        p0 = {None: 0.0, "silverman": -1.0}.get(bw, bw)
        f = bandwidth(p0, n, d)
        assert abs(f - k.factor) <= 1e-12 * k.factor
        sigma, L = fit(pts, f)
        assert np.allclose(sigma, k.covariance, rtol=1e-12, atol=1e-12 * np.abs(k.covariance).max())
        assert np.allclose(L @ L.T, k.covariance, rtol=1e-12, atol=1e-12 * np.abs(k.covariance).max())
        for _ in range(5):
            x, q = rng.normal(size=d), rng.normal(size=d) * 2.0
            want = float(k.logpdf(x)[0] - k.logpdf(q)[0])
            got = log_kernel_sum(x, pts, L) - log_kernel_sum(q, pts, L)
            assert abs(got - want) <= 1e-12 * max(1.0, abs(want)), (n, d, got, want)


def test_degenerate_points_have_no_factor():
    pts = np.random.default_rng(2).normal(size=(10, 3))
    pts[:, 1] = 0.25                                 # one shared coordinate: S singular
    assert fit(pts, bandwidth(0.0, 10, 3))[1] is None
    assert fit(pts[:3], 1.0)[1] is None              # n_comp = ndim: rank ndim - 1 at most


def _moments(table, zero_hastings=False):
    rng = np.random.default_rng(21)
    pos = rng.normal(size=(64, 6))
    r = run(pos, 800, 4242, table, lnprob_fn=correlated_gaussian_nd(COV6), zero_hastings=zero_hastings)
    x = r.chain[200:].reshape(-1, 6)
    c = np.corrcoef(x.T)
    return x.mean(axis=0), x.var(axis=0), np.array([c[i, i + 1] for i in range(5)]), r.acc.mean() / 800


def _within(m, v, c):
    return bool(np.all(np.abs(m) < MEAN_TOL) and np.all(np.abs(v - 1.0) < VAR_TOL) and np.all(np.abs(c - 0.4) < CORR_TOL))


def test_restated_kde_samples_a_correlated_6d_gaussian():
    m, v, c, af = _moments([(KDE, 1.0, 0.0, 0.0)])
    assert _within(m, v, c), (m, v, c)
    assert 0.2 < af < 0.95, af


def test_kde_without_its_hastings_term_fails_the_same_check():
    """The check has power: without the Hastings term the chain follows the product of target and KDE, which is narrower."""
    m, v, c, _ = _moments([(KDE, 1.0, 0.0, 0.0)], zero_hastings=True)
    assert not _within(m, v, c), (m, v, c)
    assert np.all(v < 1.0 - VAR_TOL), v


def test_set_moves_kde_argument_checks_on_the_built_library():
    import ctypes as C
    from magprop_amd import _capi
    L = _capi.lib()
    k = (C.c_int32 * 1)(KDE)
    w = (C.c_double * 1)(1.0)
    p = (C.c_double * 2)(0.0, 0.0)
    assert L.mp_sampler_set_moves(None, 1, k, w, p) == _capi.MP_EINVAL
    assert math.isclose(bandwidth(-1.0, 16, 6), (16 * 8 / 4.0) ** (-0.1))
