"""CPU tests of the ladder adaptation's rule and of the thermodynamic monitor's sums on their restatement (tests/ladder_restated.py),
over the named cases the device kernels are held to (tests/ladder_cases.py), and of the host-only pieces in
magprop_amd/tempering.py.  The GPU tests (tests/test_gpu_ladder_kernels.py, tests/test_gpu_ladder.py) hold the device to the same
restatement bit for bit, so what is shown here of the rule holds for the device's ladders."""
import math

import numpy as np
import pytest

import ladder_cases as lc
import ladder_restated as lr
import sampler_restated
from magprop_amd import tempering
from moves_restated import STRETCH

EPS = 2.0 ** -52


def _state(case, g):
    if case.gap is None:
        gap, span, _ = lr.init(case.betas[g], case.prev[g])
        return gap, span
    return case.gap[g], case.span[g]


@pytest.mark.parametrize("n_temps", lc.N_TEMPS)
def test_updates_keep_the_ends_and_a_strictly_decreasing_ladder(n_temps):
    for case in lc.adapt_cases(n_temps):
        for g in range(case.betas.shape[0]):
            gap, span = _state(case, g)
            assert np.all(gap > 0.0) and span == -np.log(case.betas[g, -1])
            b, new_gap, prev, taken = lr.adapt(case.betas[g], gap, span, case.prev[g], case.swaps[g], case.n_walkers, case.kappa)
            assert taken, case.name
            assert b[0] == 1.0 and b[-1] == case.betas[g, -1] and np.all(np.diff(b) < 0.0), case.name
            assert np.all(new_gap > 0.0) and np.array_equal(prev, case.swaps[g]), case.name
            A = (case.swaps[g] - case.prev[g]) / case.n_walkers
            if np.all(A == A[0]) or case.kappa < 1e-200:
                # equal acceptance (or exp = 1): h = g, c = L / G with G a sum of T - 1 terms and L the rounded log of beta_{T-1}:
                # each g'_i = c g_i is off by (T - 1) ulp of the sum's rounding, one of the quotient and one of the product at most
                assert np.all(np.abs(new_gap - gap) <= 2 * (n_temps - 1) * EPS * gap), case.name
            else:
                # direction: the pair that swapped most widens, the one that swapped least narrows
                assert new_gap[np.argmax(A)] > gap[np.argmax(A)] and new_gap[np.argmin(A)] < gap[np.argmin(A)], case.name


def test_a_ladder_with_equal_acceptance_is_a_fixed_point_over_many_updates():
    b = lc.ladder(1.0e-6, 12)
    gap, span, prev = lr.init(b, np.zeros(11, dtype=np.int64))
    g0, swaps = gap.copy(), np.zeros(11, dtype=np.int64)
    for t in range(50):
        swaps = swaps + 9
        b, gap, prev, taken = lr.adapt(b, gap, span, prev, swaps, 16, tempering.adaptation_rate(t, 20.0, 5.0))
        assert taken
    assert np.all(np.abs(gap - g0) <= 50 * 2 * 11 * EPS * g0)


def test_dropped_updates_leave_the_state_and_advance_prev():
    for case in lc.dropped_cases():
        for g in range(case.betas.shape[0]):
            b, gap, prev, taken = lr.adapt(case.betas[g], case.gap[g], case.span[g], case.prev[g], case.swaps[g], case.n_walkers,
                                           case.kappa)
            assert not taken, case.name
            assert np.array_equal(b, case.betas[g]) and np.array_equal(gap, case.gap[g]), case.name
            assert np.array_equal(prev, case.swaps[g]) and not np.array_equal(prev, case.prev[g]), case.name


def test_adaptation_rate_and_the_host_pieces():
    for t, lag, time in ((0, 10000.0, 100.0), (1, 10000.0, 100.0), (119, 20.0, 5.0), (10 ** 9, 3.0, 0.7)):
        assert tempering.adaptation_rate(t, lag, time) == lag / (time * (float(t) + lag))
    assert tempering.adaptation_rate(0, 10000.0, 100.0) == 0.01                        # 1 / time at the start
    assert tempering.adaptation_rate(10 ** 12, 10000.0, 100.0) < 1e-10                 # diminishing
    g = tempering.ladder_gaps(tempering.geometric_ladder(9, 1e-4))
    assert np.allclose(g, g[0], rtol=1e-12) and g.shape == (8,)
    lin = np.linspace(1.0, 0.01, 8)
    assert abs(tempering.ladder_gaps(lin).max() / tempering.ladder_gaps(lin).min() - 17.8) < 0.05
    assert tempering.ladder_gaps(np.array([lin, lin])).shape == (2, 7)
    assert tempering.swap_spread([0.2, 0.9, 0.5]) == 0.9 - 0.2
    assert np.array_equal(tempering.swap_spread([[0.5, 0.5], [0.0, 1.0]]), [0.0, 1.0])
    assert tempering.adaptation_settings(300) == (300, 10000.0, 100.0, False)
    assert tempering.adaptation_settings({"steps": 5, "lag": 2, "time": 3, "history": 1}) == (5, 2.0, 3.0, True)
    for bad in ({"lag": 3.0}, {"steps": 3, "rate": 1.0}, 2.5):
        with pytest.raises(ValueError):
            tempering.adaptation_settings(bad)


@pytest.mark.parametrize("n_walkers", lc.THERMO_WALKERS)
def test_thermo_sums_against_fsum(n_walkers):
    """The monitor's sum of an ensemble against the exactly rounded sum of its finite cells: every finite lnL of a Gaussian target
    has one sign, so a sum of n terms in any order is within n eps |sum| of it."""
    lnp = lc.thermo_rows(n_walkers)
    s, nf, nn = lr.thermo(lnp)
    half = lr.thermo(lnp[3:], *lr.thermo(lnp[:3]))
    assert all(np.array_equal(x, y) for x, y in zip((s, nf, nn), half))
    for e in range(lnp.shape[1]):
        cells = lnp[:, e].ravel()
        fin = cells[np.isfinite(cells)]
        assert nf[e] == fin.size and nn[e] == cells.size - fin.size and nn[e] > 0
        exact = math.fsum(fin)
        assert abs(s[e] - exact) <= fin.size * EPS * abs(exact), (e, s[e], exact)


# Gaussian target, 3 dimensions, 16 walkers, 8 temperatures, start ladder linear in beta from 1 to 0.01 (max g / min g = 17.8),
# 300 adapting steps with lag = 100, time = 10, then 300 steps on the frozen ladder.  For a Gaussian the swap acceptance of a pair
# depends on beta_{i+1} / beta_i alone, so the ladder of equal acceptance is the geometric one: gap ratio 1, spread 0.
# The restated loop over the seeds 1 .. 5 gave
#     max g / min g of the frozen ladder     1.1228  1.1121  1.0567  1.0685  1.1681
#     swap_spread over the frozen window     0.0617  0.0396  0.0131  0.0477  0.0665
# (the fixed ladder over the same window: 0.859, 0.861, 0.853, 0.866, 0.852).  The bounds are the worst seed's excess x 1.5.
GAP_RATIO_BOUND = 1.0 + 1.5 * 0.1681
SPREAD_BOUND = 1.5 * 0.0665


def test_the_rule_equalises_the_acceptances_of_a_gaussian_ladder():
    T, nw, nd, n_adapt, n_frozen = 8, 16, 3, 300, 300
    start = np.linspace(1.0, 0.01, T)
    table = [(STRETCH, 1.0, 2.0, 0.0)]
    fixed_ratio = tempering.ladder_gaps(start).max() / tempering.ladder_gaps(start).min()
    fixed_spread = None
    for seed in (5,):                                 # (the worst of the five)
        rng = np.random.default_rng(seed)
        pos = rng.normal(size=(T * nw, nd)) / np.sqrt(np.repeat(start, nw))[:, None]
        r = lr.run_adaptive(pos.copy(), n_adapt + n_frozen, seed, table, 1, start, n_adapt, 100.0, 10.0)
        assert r.n_updates == n_adapt and r.dropped[0] == 0 and len(r.history) == n_adapt
        assert np.array_equal(r.history[-1], r.betas) and r.betas[0, 0] == 1.0 and r.betas[0, -1] == 0.01
        g = tempering.ladder_gaps(r.betas[0])
        acc = r.step_swaps[n_adapt:].sum(axis=0)[0] / (n_frozen * nw)
        ratio, spread = g.max() / g.min(), tempering.swap_spread(acc)
        print(f"seed {seed}: max g / min g {ratio:.4f}, swap_spread {spread:.4f}, acceptances {np.round(acc, 3)}")
        assert ratio <= GAP_RATIO_BOUND and spread <= SPREAD_BOUND, (seed, ratio, spread)
        if fixed_spread is None:                      # the fixed ladder over the same window
            p = pos.copy()
            a = sampler_restated.run(p, n_adapt, seed, table, n_ensembles=T, n_temps=T, betas=start)
            b = sampler_restated.run(p, n_frozen, seed, table, n_ensembles=T, n_temps=T, betas=start, step0=n_adapt,
                                     lnp=a.lnp[-1].copy(), acc=a.acc)
            fixed_spread = tempering.swap_spread(b.swaps[0] / (n_frozen * nw))
    assert GAP_RATIO_BOUND < fixed_ratio / 4.0 and SPREAD_BOUND < fixed_spread / 4.0, (fixed_ratio, fixed_spread)
