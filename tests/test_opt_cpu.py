"""CPU tests of the differential-evolution optimizer: the numpy restatement of the device scheme (tests/de_restated.py) minimises,
its trial rules hold, and the Python front end (magprop_amd.optimize) checks its arguments before it touches a device."""
import os
import re

import numpy as np
import pytest

import de_restated as de
from conftest import ROOT


def _rosenbrock(P):
    P = np.asarray(P)
    f = np.sum(100.0 * (P[:, 1:] - P[:, :-1] ** 2) ** 2 + (1.0 - P[:, :-1]) ** 2, axis=1)
    return -f, np.zeros(len(P), dtype=np.int32)


@pytest.mark.parametrize("strategy", [de.BEST1BIN, de.RAND1BIN])
def test_restatement_minimises_a_shifted_gaussian_in_a_box(strategy):
    """Unit Gaussian, box [0.5, 4]^4: the optimum is the corner (0.5, ...), lnprob = -0.5; two populations converge there."""
    ndim, popsize = 4, 20
    lo, hi = np.full(ndim, 0.5), np.full(ndim, 4.0)
    pop0 = lo + (hi - lo) * np.random.default_rng(1).random((2, popsize, ndim))
    s = de.run(pop0, 400, de.gaussian, 77, strategy, 0.5, 1.0, 0.7, 1e-6, 0.0, lo, hi)
    for p in range(2):
        b = s.best[p]
        assert s.converged[p] and s.lnp[p, b] > -0.5 - 1e-3
        assert np.all(np.abs(s.pop[p, b] - 0.5) < 0.03)
        assert s.nfev[p] == popsize * (s.nit[p] + 1)
        assert np.all((s.pop[p] >= lo) & (s.pop[p] <= hi))


def test_restatement_minimises_rosenbrock_6d():
    ndim, popsize = 6, 60
    lo, hi = np.full(ndim, -2.0), np.full(ndim, 2.0)
    pop0 = lo + (hi - lo) * np.random.default_rng(2).random((1, popsize, ndim))
    s = de.run(pop0, 1500, _rosenbrock, 5, de.BEST1BIN, 0.5, 1.0, 0.9, 1e-10, 1e-10, lo, hi)
    b = s.best[0]
    assert -s.lnp[0, b] < 1e-3, -s.lnp[0, b]
    assert np.allclose(s.pop[0, b], 1.0, atol=0.05)


def test_partners_are_distinct_and_never_the_member():
    for popsize in (5, 6, 17):
        for i in range(popsize):
            for gen in range(1, 30):
                r = de.partners(11, gen, 2, i, popsize)
                assert len(set(r)) == 3 and i not in r and all(0 <= v < popsize for v in r)


def test_fill_point_is_always_taken_and_crossover_rate_zero_changes_one_coordinate():
    """cr = 0: a trial differs from its member in the fill point only (inside a wide box nothing is resampled)."""
    ndim, popsize = 6, 12
    X = np.random.default_rng(3).random((popsize, ndim))
    lo, hi = np.full(ndim, -100.0), np.full(ndim, 100.0)
    for gen in range(1, 20):
        for i in range(popsize):
            t = de.trial(X, 0, 9, gen, 0, i, de.RAND1BIN, 0.8, 0.0, lo, hi)
            fill = de.fill_point(9, gen, 0, i, ndim)
            changed = np.nonzero(t != X[i])[0]
            assert list(changed) == [fill]


def test_out_of_box_coordinates_are_resampled_inside():
    """F = 1.9 from members at the box's edges pushes mutants out: every trial coordinate still lies in the box, and a
    resampled one is lower + u (upper - lower) with the u of its slot."""
    ndim, popsize = 3, 8
    lo, hi = np.zeros(ndim), np.ones(ndim)
    X = np.where(np.random.default_rng(4).random((popsize, ndim)) < 0.5, 0.0, 1.0)
    n_resampled = 0
    for gen in range(1, 40):
        for i in range(popsize):
            t = de.trial(X, 0, 3, gen, 0, i, de.RAND1BIN, 1.9, 1.0, lo, hi)
            assert np.all((t >= lo) & (t <= hi))
            r0, r1, r2 = de.partners(3, gen, 0, i, popsize)
            mut = X[r0] + 1.9 * (X[r1] - X[r2])
            out = (mut < lo) | (mut > hi)
            for d in np.nonzero(out)[0]:
                assert t[d] == lo[d] + de.uniform(3, gen, 0, i, 4 + ndim + d) * (hi[d] - lo[d])
            n_resampled += int(out.sum())
    assert n_resampled > 50


def test_reduce_ties_go_to_the_lower_index_and_inf_never_converges():
    assert de.reduce([-3.0, -1.0, -2.0, -1.0], 0.01, 0.0)[0] == 1
    assert de.reduce([-1.0] * 5, 0.01, 0.0) == (0, True)
    assert de.reduce([-np.inf] + [-1.0] * 4, 0.01, 0.0) == (1, False)
    assert de.reduce([-np.inf] * 5, 0.01, 0.0) == (0, False)
    # std(E) = 0.5 against atol + tol |mean(E)| = 0.01 x 10: not converged; tol = 0.1 converges
    assert de.reduce([-9.5, -10.5], 0.01, 0.0) == (0, False)
    assert de.reduce([-9.5, -10.5], 0.05, 0.0) == (0, True)


@pytest.mark.parametrize("kw, match", [
    ({"strategy": "best2bin"}, "strategy"),
    ({"popsize": 0}, "popsize"),
    ({"popsize": 200}, "members"),
    ({"mutation": (1.0, 0.5)}, "mutation"),
    ({"mutation": 2.5}, "mutation"),
    ({"recombination": 1.5}, "recombination"),
    ({"tol": -1.0}, "tol"),
    ({"maxiter": -3}, "maxiter"),
    ({"bounds": [(0.0, 1.0)] * 5}, "6 parameters"),
    ({"bounds": [(1.0, 0.0)] * 6}, "lower < upper"),
    ({"bounds": [(0.0, np.inf)] * 6}, "finite"),
    ({"variant": "lib", "bounds": [(0.0, 1.0)] * 10}, "6 to 9"),
    ({"variant": "other"}, "variant"),
    ({"n_starts": 0}, "n_starts"),
    ({"n_starts": 65}, "at most"),
    ({"init": "sobol"}, "init"),
    ({"init": np.zeros((3, 6))}, "init must have shape"),
])
def test_argument_checks_raise_before_any_device_is_touched(monkeypatch, kw, match):
    from magprop_amd import _capi, optimize

    def no_device(*a, **k):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(_capi, "lib", no_device)
    monkeypatch.setattr(_capi, "Handle", no_device)
    monkeypatch.setattr(_capi, "cfg_synth", no_device)
    monkeypatch.setattr(_capi, "cfg_lib", no_device)
    x = np.linspace(1.0, 10.0, 5)
    with pytest.raises(ValueError, match=match):
        optimize.differential_evolution(x, x, x, **kw)


def test_a_dataset_is_required():
    from magprop_amd import optimize
    with pytest.raises(ValueError, match="dataset"):
        optimize.differential_evolution()


def test_latin_hypercube_fills_every_slice():
    from magprop_amd import optimize
    lo, hi = np.array([0.0, -2.0]), np.array([1.0, 2.0])
    P = optimize.latin_hypercube(np.random.default_rng(0), 10, lo, hi)
    for j in range(2):
        slots = np.floor((P[:, j] - lo[j]) / (hi[j] - lo[j]) * 10).astype(int)
        assert sorted(slots) == list(range(10))


def test_initial_ball_is_clipped_into_the_box():
    from magprop_amd import optimize
    res = optimize.OptimizeResult(x=np.array([1.0, 0.0]), bounds=np.array([[0.0, 1.0], [-1.0, 1.0]]))
    P = optimize.initial_ball(res, 64, scale=1e-4, seed=1)
    assert P.shape == (64, 2) and np.all(P[:, 0] <= 1.0) and np.any(P[:, 0] == 1.0)
    assert np.all(np.abs(P - res.x) <= 5e-4)


def test_header_states_the_strategy_codes():
    from magprop_amd import _capi
    hdr = open(os.path.join(ROOT, "include", "magprop_amd.h")).read()
    assert int(re.search(r"#define\s+MP_DE_BEST1BIN\s+(\d+)", hdr).group(1)) == _capi.DE_BEST1BIN
    assert int(re.search(r"#define\s+MP_DE_RAND1BIN\s+(\d+)", hdr).group(1)) == _capi.DE_RAND1BIN
    for name in ("mp_optimizer_create", "mp_optimizer_set_population", "mp_optimizer_run", "mp_optimizer_get_state",
                 "mp_optimizer_destroy"):
        assert name in _capi.EXPORTS and hasattr(_capi.lib(), name)
