"""CPU checks of the Gaussian (Metropolis) and walk moves (include/magprop_amd.h MP_MOVE_GAUSSIAN, MP_MOVE_WALK): the front end's
constructors, tables and command-line names, and the numpy restatement (tests/normal_moves_restated.py) -- its Philox over arrays
against the oracle's, Floyd's subsets, the covariance of the walk proposal, a Gaussian chain on a correlated target, the tune
rule from both sides, and the step loop against itself (continued runs, mixtures, tempering)."""
import math

import numpy as np
import pytest

import normal_moves_restated as nm
from moves_restated import DE, STRETCH, correlated_gaussian
from oracle.stretch_oracle import philox4x32_10, u01
from slice_move_restated import autocorr_time

# the bounds of tests/test_moves_cpu.py on 32 walkers x 1 500 steps with the first 300 discarded: at the tau of 10 to 20 steps
# a Metropolis chain with the optimal scale has in 2 dims, ~2 500 independent draws, so the standard errors are 0.02 (mean),
# 0.03 (variance) and 0.004 (correlation at rho = 0.9): the bounds are 3.5 to 7 of them
RHO, MEAN_TOL, VAR_TOL, CORR_TOL = 0.9, 0.1, 0.1, 0.03
# The tuning case of the issue: 3 dims, 64 walkers, target 0.25, 300 tuning steps, then 200 steps on the frozen scales.  Shared
# with tests/test_gpu_moves_normal.py, which runs the same two cases on the device.
TUNE_CASE = dict(n_walkers=64, ndim=3, tune=300, after=200, target=0.25, seed=20261201)
ACCEPT_BRACKET = (0.1, 0.5)


# ---------------------------------------------------------------- the front end
def test_constructors_tables_and_names():
    from magprop_amd import DEMove, GaussianMove, KDEMove, WalkMove, moves
    assert WalkMove().s is None and WalkMove(3).s == 3 and WalkMove(np.int64(4)).s == 4
    assert moves.move_table(WalkMove(), 6) == ([6], [1.0], [(0.0, 0.0)])
    assert moves.move_table([(WalkMove(s=3), 0.3), (DEMove(), 0.7)], 6) == ([6, 1], [0.3, 0.7], [(3.0, 0.0), (0.0, 1.0e-5)])
    assert moves.parse_spec("awalk:0.3,de:0.7") == [(WalkMove(), 0.3), (DEMove(), 0.7)]
    assert WalkMove(3) == WalkMove(3) and WalkMove(3) != WalkMove() and hash(WalkMove(3)) == hash(WalkMove(3))
    for bad in (1, 0, -2, 2.5, True, "3"):
        with pytest.raises(ValueError):
            WalkMove(bad)
    for spec in ("walk:1", "gaussian", "mh"):
        with pytest.raises(ValueError, match="awalk"):
            moves.parse_spec(spec)
    g = GaussianMove(0.25)
    assert (g.mode, g.scale, g.tune, g.target_accept) == ("vector", 1.0, 0, 0.25)
    assert np.array_equal(g.factor(3), 0.5 * np.eye(3)) and np.array_equal(g.packed_factor(2), [0.5, 0.0, 0.5])
    assert GaussianMove([1.0, 4.0], mode="random").target_accept == 0.44 == GaussianMove([1.0, 4.0], mode="sequential").target_accept
    assert np.array_equal(GaussianMove([1.0, 4.0]).factor(2), np.diag([1.0, 2.0]))
    cov = np.array([[4.0, 1.2], [1.2, 1.0]])
    f = GaussianMove(cov, scale=0.5, tune=20, target_accept=0.3)
    assert np.allclose(f.factor(2) @ f.factor(2).T, cov, rtol=1e-15) and f.factor(2)[0, 1] == 0.0
    assert np.array_equal(f.packed_factor(2), np.linalg.cholesky(cov)[np.tril_indices(2)])
    assert moves.move_table(f, 2) == ([5], [1.0], [(0.5, 20.0)])
    assert f == GaussianMove(cov, scale=0.5, tune=20, target_accept=0.3) and f != GaussianMove(cov, scale=0.5, tune=20)
    assert moves.gaussian_move(moves.parse_moves([(KDEMove(), 0.8), (f, 0.2)])) is f and moves.gaussian_move(moves.parse_moves(g)) is g
    assert moves.gaussian_move(moves.parse_moves(WalkMove())) is None
    with pytest.raises(ValueError, match="coordinates"):
        f.factor(3)
    x = np.random.default_rng(1).normal(size=(500, 3)) * [1.0, 2.0, 0.5]
    s = GaussianMove.from_samples(x, tune=5)
    assert np.allclose(s.factor(3) @ s.factor(3).T, np.cov(x.T) * 2.38 ** 2 / 3, rtol=1e-12) and s.tune == 5
    for ctor in (lambda: GaussianMove(0.0), lambda: GaussianMove(-1.0), lambda: GaussianMove([1.0, 0.0]), lambda: GaussianMove(float("nan")),
                 lambda: GaussianMove([[1.0, 2.0], [2.0, 1.0]]),                       # not positive definite
                 lambda: GaussianMove([[1.0, 0.5], [0.4, 1.0]]),                       # not symmetric
                 lambda: GaussianMove(np.ones((2, 3))), lambda: GaussianMove(np.ones((2, 2, 2))),
                 lambda: GaussianMove(cov, mode="random"), lambda: GaussianMove(cov, mode="sequential"),   # emcee's rule
                 lambda: GaussianMove(1.0, mode="axis"), lambda: GaussianMove(1.0, scale=0.0), lambda: GaussianMove(1.0, scale=float("inf")),
                 lambda: GaussianMove(1.0, tune=-1), lambda: GaussianMove(1.0, tune=0.5), lambda: GaussianMove(1.0, tune=2 ** 31),
                 lambda: GaussianMove(1.0, target_accept=0.0), lambda: GaussianMove(1.0, target_accept=1.0),
                 lambda: GaussianMove.from_samples(np.ones((1, 3))),
                 lambda: moves.parse_moves([(g, 0.5), (f, 0.5)])):                     # two Gaussian moves
        with pytest.raises(ValueError):
            ctor()
    with pytest.raises(TypeError):
        GaussianMove(1.0, factor=2.0)                                                  # emcee's factor= is not offered
    assert not hasattr(moves, "MHMove")
    import magprop_amd
    assert magprop_amd.WalkMove is WalkMove and magprop_amd.GaussianMove is GaussianMove


def test_sampler_refuses_a_covariance_of_the_wrong_size():
    from magprop_amd import EnsembleSampler, GaussianMove
    with pytest.raises(ValueError, match="coordinates"):
        EnsembleSampler(8, 3, target="gaussian", moves=GaussianMove(np.eye(2)))


def test_library_refuses_null_samplers():
    from magprop_amd import _capi
    L = _capi.lib()
    assert L.mp_sampler_set_gaussian(None, None, 0, 0.25) == _capi.MP_EINVAL
    assert "mp_sampler_set_gaussian" in _capi.last_error()
    assert L.mp_sampler_get_gaussian(None, None, None, None, None) == _capi.MP_EINVAL
    assert "mp_sampler_get_gaussian" in _capi.last_error()


# ---------------------------------------------------------------- the restatement's parts
def test_philox_over_arrays_is_the_oracles():
    seed = 0x1234567890ABCDEF
    ks, cs = np.array([0, 1, 77, 2 ** 20 + 3]), np.array([nm.WALK_CTR, nm.GAUSS_CTR + 2, nm.WALK_NORMAL_CTR + 511])
    got = nm.philox_batch(seed, 4_000_000_123, 1, ks[:, None], cs[None, :])
    for i, k in enumerate(ks):
        for j, c in enumerate(cs):
            want = philox4x32_10(seed & nm.M32, seed >> 32, 4_000_000_123 & nm.M32, 1, int(k), int(c))
            assert tuple(int(w[i, j]) for w in got) == want
            assert nm.u01_batch(got[0], got[1])[i, j] == u01(want[0], want[1])


@pytest.mark.parametrize("n_comp,s", [(5, 3), (65, 64), (64, 2)])
def test_floyd_draws_distinct_members_uniformly(n_comp, s):
    n = 4000
    count = np.zeros(n_comp, dtype=np.int64)
    for k in range(n):
        mem = nm.floyd(99, 3, k & 1, k, n_comp, s)
        assert len(mem) == s == len(set(mem)) and all(0 <= m < n_comp for m in mem)
        count[mem] += 1
    p = s / n_comp
    assert np.all(np.abs(count - n * p) <= 5.0 * math.sqrt(n * p * (1.0 - p))), count


def _walk_case(n_comp, ndim, s, n, seed):
    """n restated proposals of walkers at the origin from one fixed other half: q - x_k and the member sets."""
    rng = np.random.default_rng(seed)
    other = rng.normal(size=(n_comp, ndim)) @ rng.normal(size=(ndim, ndim))
    pos = np.concatenate([other, np.zeros((n, ndim))])
    q, logu, mem = nm.walk_proposals(pos, np.arange(n_comp, n_comp + n), list(range(n_comp)), seed, 5, 0, s)
    assert np.all(np.isfinite(q)) and np.all(logu <= 0.0)
    return other, q, mem


def _assert_covariance(d, members):
    n = len(d)
    S = np.atleast_2d(np.cov(members.T))
    got = (d.T @ d) / n                      # (the proposal's mean is 0 by construction)
    se = np.sqrt((np.outer(np.diag(S), np.diag(S)) + S * S) / n)
    assert np.all(np.abs(got - S) <= 5.0 * se), np.max(np.abs(got - S) / se)
    assert np.all(np.abs(d.mean(axis=0)) <= 5.0 * np.sqrt(np.diag(S) / n))


@pytest.mark.parametrize("n_comp,ndim,s", [(16, 3, 16), (3, 6, 3), (2, 3, 2)])
def test_walk_proposal_has_the_members_sample_covariance(n_comp, ndim, s):
    """All of the other half; s = 3 members in 6 dims (a covariance of rank 2: no factorisation would exist); two members (n_comp = s = 2, the smallest ensemble)."""
    other, q, mem = _walk_case(n_comp, ndim, s, 20000, 20261202)
    assert np.all(mem == np.arange(n_comp))
    _assert_covariance(q, other)
    if s < ndim + 1:
        assert np.linalg.matrix_rank(np.cov(other.T)) == s - 1 < ndim
        assert np.linalg.matrix_rank(q, tol=1e-9) == s - 1                     # the proposals stay in the members' plane


def test_walk_subsets_propose_with_their_own_covariance():
    """s = 3 of 5 in 6 dims by Floyd: conditioned on each of the 10 member sets, the covariance is that set's."""
    other, q, mem = _walk_case(5, 6, 3, 40000, 20261203)
    sets = {}
    for i, m in enumerate(mem):
        sets.setdefault(frozenset(m.tolist()), []).append(i)
    assert len(sets) == 10 and min(len(v) for v in sets.values()) > 3000
    for members, rows in sets.items():
        _assert_covariance(q[rows], other[sorted(members)])


def test_kernel_order_sums_agree_with_member_order_to_rounding():
    rng = np.random.default_rng(7)
    pos = rng.normal(size=(300, 3))
    comp, ks = list(range(257)), np.arange(257, 300)
    plain = nm.walk_proposals(pos, ks, comp, 11, 2, 1, 257)[0]
    for waves in (1, 4):
        got = nm.walk_proposals(pos, ks, comp, 11, 2, 1, 257, waves=waves)[0]
        assert np.allclose(got, plain, rtol=0.0, atol=1e-13) and not np.array_equal(got, plain)


def test_tune_rule():
    assert nm.tune(2.0, 0, 16, 64, 0.25) == 2.0                                # at the target nothing moves
    assert nm.tune(2.0, 0, 0, 64, 0.25) == 1.0 and nm.tune(2.0, 8, 0, 64, 0.25) == 1.5   # f = 1/2; the gain 8 / (8 + n)
    assert nm.tune(2.0, 0, 64, 64, 0.25) == 5.0                                # f = (1 + t) / (2 t) = 2.5


# ---------------------------------------------------------------- chains of the restatement
@pytest.mark.parametrize("mode", [nm.VECTOR, nm.RANDOM, nm.SEQUENTIAL])
def test_restated_gaussian_move_samples_a_correlated_gaussian(mode):
    cov = np.array([[1.0, RHO], [RHO, 1.0]])
    L = np.linalg.cholesky(cov * 2.38 ** 2 / 2) if mode == nm.VECTOR else np.diag([1.0, 1.0]) * 2.38 * math.sqrt(1.0 - RHO * RHO)
    steps = 1500 if mode == nm.VECTOR else 6000       # (one axis at a time against rho = 0.9 mixes slowly)
    pos = np.random.default_rng(5).normal(size=(32, 2))
    r = nm.run(pos, steps, 7005, [(nm.GAUSSIAN, 1.0, 1.0, 0.0)], gauss=nm.Gauss(L, mode), lnprob_fn=correlated_gaussian(RHO))
    x = r.chain[steps // 5:].reshape(-1, 2)
    m, v, c = x.mean(axis=0), x.var(axis=0), np.corrcoef(x.T)[0, 1]
    print(f"mode {mode}: acceptance {r.acc.mean() / steps:.3f}, tau {autocorr_time(r.chain[steps // 5:, :, 0]):.1f}, mean {m}, var {v}, corr {c:.4f}")
    assert 0.1 < r.acc.mean() / steps < 0.9
    assert np.all(np.abs(m) < MEAN_TOL) and np.all(np.abs(v - 1.0) < VAR_TOL) and abs(c - RHO) < CORR_TOL, (m, v, c)
    assert np.all(r.sigma == 1.0) and np.all(r.state.n_tuned == 0) and r.state.n_proposed[0] == steps * 32


def test_restated_walk_move_samples_a_correlated_gaussian():
    for s in (0, 3):
        pos = np.random.default_rng(6).normal(size=(32, 2))
        r = nm.run(pos, 1500, 7006, [(nm.WALK, 1.0, float(s), 0.0)], lnprob_fn=correlated_gaussian(RHO))
        x = r.chain[300:].reshape(-1, 2)
        m, v, c = x.mean(axis=0), x.var(axis=0), np.corrcoef(x.T)[0, 1]
        print(f"s {s}: acceptance {r.acc.mean() / 1500:.3f}, tau {autocorr_time(r.chain[300:, :, 0]):.1f}, mean {m}, var {v}, corr {c:.4f}")
        assert 0.1 < r.acc.mean() / 1500 < 0.9
        assert np.all(np.abs(m) < MEAN_TOL) and np.all(np.abs(v - 1.0) < VAR_TOL) and abs(c - RHO) < CORR_TOL, (s, m, v, c)
        assert r.state is None and np.all(np.isnan(r.sigma))


def tune_case(scale0):
    """The restated run of TUNE_CASE from scale0: (sigma behind the tuning, acceptance of the steps behind it, the Run)."""
    c = TUNE_CASE
    pos = np.random.default_rng(c["seed"]).normal(size=(c["n_walkers"], c["ndim"]))
    r = nm.run(pos, c["tune"] + c["after"], c["seed"], [(nm.GAUSSIAN, 1.0, scale0, float(c["tune"]))],
               gauss=nm.Gauss(np.eye(c["ndim"]), nm.VECTOR, c["target"]))
    return r.sigma[-1, 0], r.accepted[c["tune"]:].mean(), r


def test_tuning_from_both_sides_meets():
    lo, acc_lo, r_lo = tune_case(1.0e-3)
    hi, acc_hi, r_hi = tune_case(1.0e3)
    print(f"sigma {lo:.4f} (from 1e-3, acceptance {acc_lo:.3f}), {hi:.4f} (from 1e3, acceptance {acc_hi:.3f})")
    for r in (r_lo, r_hi):
        c = TUNE_CASE
        assert r.state.n_tuned[0] == c["tune"] and np.all(r.sigma[c["tune"] - 1:, 0] == r.sigma[-1, 0]) and r.sigma[0, 0] != r.sigma[1, 0]
        assert r.state.n_proposed[0] == (c["tune"] + c["after"]) * c["n_walkers"] and r.state.n_accepted[0] == r.acc.sum()
    assert ACCEPT_BRACKET[0] < acc_lo < ACCEPT_BRACKET[1] and ACCEPT_BRACKET[0] < acc_hi < ACCEPT_BRACKET[1]
    assert 0.5 < lo / hi < 2.0


# ---------------------------------------------------------------- the step loop against itself
MIXTURE = [(nm.GAUSSIAN, 0.3, 0.7, 10.0), (nm.WALK, 0.3, 3.0, 0.0), (STRETCH, 0.2, 2.0, 0.0), (DE, 0.2, 0.0, 1.0e-5)]


@pytest.mark.parametrize("tempered", [False, True])
def test_continued_run_equals_one_run(tempered):
    """40 steps equal 15 + 25 continued through step0 / lnp / acc / state on the four-move mixture (16 walkers x 3 ensembles x 3
    dims; tempered: ladder (1, 0.5, 0.25) with its swap sweep); every move is drawn and the Gaussian steps alone tune."""
    kw = dict(n_ensembles=3, gauss=nm.Gauss(np.linalg.cholesky(np.array([[1.0, 0.3, 0.0], [0.3, 1.0, 0.2], [0.0, 0.2, 1.0]]))))
    if tempered:
        kw.update(betas=[1.0, 0.5, 0.25], n_temps=3)
    pos = np.random.default_rng(4).normal(size=(3 * 16, 3)) * 1.5
    whole = nm.run(pos.copy(), 40, 13, MIXTURE, **kw)
    p = pos.copy()
    first = nm.run(p, 15, 13, MIXTURE, **kw)
    rest = nm.run(p, 25, 13, MIXTURE, step0=15, lnp=first.lnp[-1].copy(), acc=first.acc, state=first.state, **kw)
    for f in ("chain", "lnp", "drawn", "accepted", "sigma"):
        assert np.array_equal(np.concatenate([getattr(first, f), getattr(rest, f)]), getattr(whole, f)), f
    assert np.array_equal(rest.acc, whole.acc) and np.array_equal(first.swaps + rest.swaps, whole.swaps)
    assert set(whole.drawn) == {0, 1, 2, 3} and np.array_equal(whole.accepted.sum(axis=0), whole.acc)
    n_gauss = int(np.sum(whole.drawn == 0))
    assert np.all(whole.state.n_tuned == min(n_gauss, 10)) and np.all(whole.state.n_proposed == 16 * n_gauss)
    changed = np.any(np.diff(np.concatenate([[[0.7] * 3], whole.sigma]), axis=0) != 0.0, axis=1)
    assert not np.any(changed & (whole.drawn != 0))                      # steps of another move change nothing of the state
    assert (whole.swaps.sum() > 0) == tempered
    if tempered:
        assert whole.state.sigma[2] > whole.state.sigma[0]               # the hot ensemble accepts more and widens its scale
