"""GPU tests of the Gaussian (Metropolis) and walk moves of the device-resident sampler (include/magprop_amd.h MP_MOVE_GAUSSIAN,
MP_MOVE_WALK; magprop_amd/csrc/mp_normal.hip): device chains against the numpy restatement (tests/normal_moves_restated.py) on
the unit Gaussian -- decisions and acceptance counts exactly, the Gaussian move's rational tune state exactly, positions and
lnprob to the accuracy of the device's log / sqrt / cos / sin --, split runs, the real posterior on every kernel build against
mp_lnprob_batch calls of the launch's size, tempering, mixtures, the moves' statistics, Humped from the reference's starting
ball, the monitors, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import normal_moves_restated as nm
from conftest import TRUTHS, TYPES
from moves_restated import DE, STRETCH
from raw_abi import RawSampler, dp, lp
from slice_move_restated import autocorr_time
from test_gpu_moves_kde import ATOL, RTOL
from test_gpu_nested import (LONG_MIXED_LENGTHS, assert_long_reference_is_not_vacuous, launch_class, long_cases,  # noqa: F401
                             long_mixed_sets, long_sets, posterior_cases, synth_sets)  # (the three handles are fixtures)
from test_moves_normal_cpu import ACCEPT_BRACKET, TUNE_CASE, tune_case

pytestmark = pytest.mark.gpu

MEAN_TOL, VAR_TOL = 0.05, 0.06       # tests/test_gpu_moves.py: 256 walkers x 6 dims on the unit Gaussian
STATS = ("sigma", "n_proposed", "n_accepted", "n_tuned")
FULL_L = np.linalg.cholesky(np.array([[1.0, 0.3, 0.0], [0.3, 0.8, 0.2], [0.0, 0.2, 1.2]]))


def pack(L):
    """The lower triangle by rows, as mp_sampler_set_gaussian takes it."""
    L = np.asarray(L, dtype=np.float64)
    return np.ascontiguousarray(L[np.tril_indices(L.shape[0])])


class RawNormal(RawSampler):
    """RawSampler with the entry points of the Gaussian move."""

    def set_gaussian(self, gauss, check=True):
        rc = self.L.mp_sampler_set_gaussian(self.sp, dp(pack(gauss.L)), int(gauss.mode), C.c_double(gauss.target))
        if check:
            self._ok(rc)
        return rc

    def gauss_stats(self):
        out = {"sigma": np.empty(self.ne)}
        out.update({k: np.empty(self.ne, dtype=np.int64) for k in STATS[1:]})
        self._ok(self.L.mp_sampler_get_gaussian(self.sp, dp(out["sigma"]), *(lp(out[k]) for k in STATS[1:])))
        return out

    @property
    def waves(self):
        """Wavefronts of a workgroup of this sampler's half-step launches (mp_device.h launch_point_kernel)."""
        return launch_class((self.nw // 2) * self.ne, self.h.n_simd)[0]


def device_run(n_walkers, n_ens, ndim, seed, table, pos, runs, gauss=None, betas=None):
    """The unit-Gaussian target through the C ABI: consecutive mp_sampler_run calls of runs[i] steps.  Returns chain, lnprob,
    n_accepted, the Gaussian move's state behind every call (None without the move), the swap counts (None untempered) and the
    wavefronts of the launches' workgroups."""
    with RawNormal(n_walkers, n_ens, ndim, seed) as r:
        if betas is not None:
            r.set_temperatures(betas)
        if gauss is not None:
            r.set_gaussian(gauss)
        r.set_moves(table)
        r.set_positions(pos)
        parts, stats = [], []
        for n in runs:
            parts.append(r.run(n))
            stats.append(r.gauss_stats() if gauss is not None else None)
        swaps = r.swaps(n_ens // len(betas), len(betas)) if betas is not None else None
        return (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), r.accepted(), stats, swaps, r.waves)


def restated_run(n_ens, seed, table, pos, runs, gauss, betas, waves):
    """The restatement in the same calls: the concatenated Run fields and the Gaussian state behind every call."""
    p, lnp, acc, state, step0 = pos.copy(), None, None, None, 0
    outs, stats = [], []
    kw = {} if betas is None else dict(betas=[betas[e % len(betas)] for e in range(n_ens)], n_temps=len(betas))
    for n in runs:
        o = nm.run(p, n, seed, table, gauss=gauss, n_ensembles=n_ens, step0=step0, lnp=lnp, acc=acc, state=state, waves=waves, **kw)
        lnp, acc, state, step0 = o.lnp[-1].copy(), o.acc, o.state, step0 + n
        outs.append(o)
        stats.append(state.stats() if state is not None else None)
    cat = {f: np.concatenate([getattr(o, f) for o in outs]) for f in ("chain", "lnp", "drawn", "accepted", "sigma")}
    cat["acc"], cat["swaps"] = outs[-1].acc, sum(o.swaps for o in outs)
    return cat, stats


def compare(n_walkers, n_ens, ndim, seed, table, pos, runs, gauss=None, betas=None):
    """Device against restatement: acceptance counts and per-step decisions identical, positions and lnprob to RTOL / ATOL, the
    Gaussian state array_equal at every chunk end, the swap counts.  Returns (device tuple, restated fields)."""
    dev = device_run(n_walkers, n_ens, ndim, seed, table, pos, runs, gauss, betas)
    chain, lnp, acc, stats, swaps, waves = dev
    ref, ref_stats = restated_run(n_ens, seed, table, pos, runs, gauss, betas, waves)
    print(f"{n_walkers} x {n_ens} x {ndim}, {sum(runs)} steps, {waves} wavefronts: max |chain - restated| {np.abs(chain - ref['chain']).max():.3e}, "
          f"max |lnprob - restated| {np.abs(lnp - ref['lnp']).max():.3e}, accepted {int(acc.sum())} of {sum(runs) * n_walkers * n_ens}")
    assert np.array_equal(acc, ref["acc"])
    if betas is None:    # (a swap moves rows too: tempered runs are held by the counts and the values)
        prev = np.concatenate([pos[None], chain[:-1]])
        assert np.array_equal(np.any(chain != prev, axis=2), ref["accepted"])
    else:
        assert np.array_equal(swaps, ref["swaps"])
    assert np.allclose(chain, ref["chain"], rtol=RTOL, atol=ATOL) and np.allclose(lnp, ref["lnp"], rtol=RTOL, atol=ATOL)
    for got, want in zip(stats, ref_stats):
        if want is not None:
            for k in STATS:
                assert np.array_equal(got[k], want[k]), (k, got[k], want[k])
    return dev, ref


def start(n_total, ndim, seed, spread=1.5):
    return np.random.default_rng(seed).normal(size=(n_total, ndim)) * spread


# ---------------------------------------------------------------- the walk move against the restatement
@pytest.mark.parametrize("n_walkers,ndim,steps,s", [
    (4, 3, 60, 0),          # n_comp = s = 2: the smallest ensemble
    (10, 3, 40, 3),         # Floyd with collisions
    (130, 3, 8, 64),        # 64 of 65: the largest subset
    (130, 3, 8, 0),         # 65 members: one more than a wavefront
    (514, 2, 6, 0),         # 257 members: one more than a team workgroup's stride
    (2048, 2, 6, 0),        # the one-wavefront builds: 1 024 members over 64 lanes
])
def test_walk_chains_match_the_restatement(n_walkers, ndim, steps, s):
    seed = 20261210 + n_walkers + s
    pos = start(n_walkers, ndim, seed)
    dev, ref = compare(n_walkers, 1, ndim, seed, [(nm.WALK, 1.0, float(s), 0.0)], pos, (steps // 3, steps - steps // 3))
    assert 0 < dev[2].sum() < steps * n_walkers
    assert dev[5] == (1 if n_walkers == 2048 else 4)
    if s == 3:   # subsets of the first step did collide (a draw repeated a member, which took j instead)
        assert any(len(set(nm.floyd_draws(seed, 0, half, k, 5, 3))) < 3 for half in (0, 1) for k in range(10))


def test_an_explicit_s_of_the_whole_half_is_s_zero_and_split_runs_are_one_run():
    seed = 20261220
    pos = start(10, 3, seed)
    a = device_run(10, 1, 3, seed, [(nm.WALK, 1.0, 0.0, 0.0)], pos, (60,))
    b = device_run(10, 1, 3, seed, [(nm.WALK, 1.0, 5.0, 0.0)], pos, (25, 35))
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x, y)
    c = device_run(10, 1, 3, seed, [(nm.WALK, 1.0, 4.0, 0.0)], pos, (60,))
    assert not np.array_equal(a[0], c[0])


# ---------------------------------------------------------------- the Gaussian move against the restatement
def test_gaussian_chain_with_a_full_factor_across_the_tune_boundary():
    """8 walkers x 3 dims, a full L, tune 20 of 60 steps, as 25 + 35 and as one run."""
    seed, table, gauss = 20261221, [(nm.GAUSSIAN, 1.0, 2.0, 20.0)], nm.Gauss(FULL_L, nm.VECTOR, 0.25)
    pos = start(8, 3, seed)
    dev, ref = compare(8, 1, 3, seed, table, pos, (25, 35), gauss)
    stats = dev[3]
    assert stats[0]["n_tuned"][0] == 20 == stats[1]["n_tuned"][0] and stats[0]["sigma"][0] == stats[1]["sigma"][0] != 2.0
    assert ref["sigma"][18, 0] != ref["sigma"][19, 0] == ref["sigma"][59, 0]
    assert stats[1]["n_proposed"][0] == 60 * 8 and stats[1]["n_accepted"][0] == dev[2].sum()
    one = device_run(8, 1, 3, seed, table, pos, (60,), gauss)
    for x, y in zip(one[:3], dev[:3]):
        assert np.array_equal(x, y)
    for k in STATS:
        assert np.array_equal(one[3][-1][k], stats[-1][k]), k


def test_gaussian_move_runs_two_walkers():
    """The one move that reads nothing of the other half: 2 walkers x 1 ensemble."""
    seed = 20261222
    dev, _ = compare(2, 1, 3, seed, [(nm.GAUSSIAN, 1.0, 1.0, 10.0)], start(2, 3, seed), (12, 18), nm.Gauss(FULL_L, nm.VECTOR, 0.25))
    assert 0 < dev[2].sum() < 60


@pytest.mark.parametrize("mode", [nm.RANDOM, nm.SEQUENTIAL])
def test_single_axis_modes(mode):
    """A diagonal L, 8 walkers x 2 ensembles x 3 dims, 45 steps; every step moves one coordinate of a walker."""
    seed, gauss = 20261223 + mode, nm.Gauss(np.diag([0.5, 1.0, 2.0]), mode, 0.44)
    pos = start(16, 3, seed)
    dev, ref = compare(8, 2, 3, seed, [(nm.GAUSSIAN, 1.0, 1.5, 15.0)], pos, (20, 25), gauss)
    chain = dev[0]
    moved = np.concatenate([pos[None], chain[:-1]]) != chain                     # [steps, walkers, dims]
    assert np.all(moved.sum(axis=2) <= 1) and np.all(moved.any(axis=(0, 1)))
    if mode == nm.SEQUENTIAL:
        for s in range(45):
            assert not moved[s][:, np.arange(3) != s % 3].any()
    else:
        assert any(moved[s].any(axis=0).sum() > 1 for s in range(45))           # the axis is drawn per proposal


def test_ensembles_tune_scales_of_their_own():
    """3 ensembles that start 0.2, 1 and 5 wide: their acceptance differs, so their sigmas differ after tuning."""
    seed = 20261225
    pos = np.concatenate([start(16, 3, seed + e, w) for e, w in enumerate((0.2, 1.0, 5.0))])
    dev, _ = compare(16, 3, 3, seed, [(nm.GAUSSIAN, 1.0, 1.0, 25.0)], pos, (10, 30), nm.Gauss(np.eye(3), nm.VECTOR, 0.25))
    sigma = dev[3][-1]["sigma"]
    assert len(set(sigma.tolist())) == 3 and np.all(dev[3][-1]["n_tuned"] == 25)


def test_tempered_gaussian_keeps_a_scale_per_temperature():
    """Ladder (1, 0.5, 0.25), 24 walkers, tune 40 of 60 steps: the hot ensemble's sigma ends above the cold one's."""
    seed, ladder = 20261226, (1.0, 0.5, 0.25)
    dev, ref = compare(24, 3, 3, seed, [(nm.GAUSSIAN, 1.0, 1.0, 40.0)], start(72, 3, seed, 1.0), (25, 35), nm.Gauss(np.eye(3), nm.VECTOR, 0.25),
                       betas=ladder)
    assert ref["sigma"][-1, 2] > ref["sigma"][-1, 0] and np.array_equal(dev[3][-1]["sigma"], ref["sigma"][-1])
    assert ref["swaps"].shape == (1, 2) and np.all(ref["swaps"] > 0)


def test_tempered_walk_matches_the_restatement():
    seed = 20261227
    _, ref = compare(16, 4, 3, seed, [(nm.WALK, 1.0, 3.0, 0.0)], start(64, 3, seed), (12, 18), betas=(1.0, 0.3))
    assert ref["swaps"].shape == (2, 1) and np.all(ref["swaps"] > 0)


def test_mixture_of_both_moves_with_stretch_and_de():
    """16 walkers x 2 ensembles, 60 steps of [Gaussian 0.3, walk 0.3, stretch 0.2, DE 0.2]: every move is drawn, and the Gaussian
    steps alone count and tune."""
    seed = 20261228
    table = [(nm.GAUSSIAN, 0.3, 0.7, 10.0), (nm.WALK, 0.3, 3.0, 0.0), (STRETCH, 0.2, 2.0, 0.0), (DE, 0.2, 0.0, 1.0e-5)]
    dev, ref = compare(16, 2, 3, seed, table, start(32, 3, seed), (25, 35), nm.Gauss(FULL_L, nm.VECTOR, 0.25))
    assert set(ref["drawn"]) == {0, 1, 2, 3}
    n_gauss = int(np.sum(ref["drawn"] == 0))
    assert n_gauss > 10 and np.all(dev[3][-1]["n_proposed"] == 16 * n_gauss) and np.all(dev[3][-1]["n_tuned"] == 10)


# ---------------------------------------------------------------- the real posterior against mp_lnprob_batch, build by build
def gauss_near_truths():
    """The proposal of the posterior cases: isotropic, 2.38 / sqrt(6) times the 1e-2 ball the walkers start in."""
    return nm.Gauss(np.eye(6) * (1.0e-2 * 2.38 / np.sqrt(6.0)), nm.VECTOR, 0.25)


def drive_posterior(h, ens_ds, truths, n_half, steps, seed, build, move, betas=None):
    """A sampler of len(ens_ds) ensembles of 2 n_half walkers on h (target 0) under the walk or the Gaussian move: the lnprob
    stored with every row that a step changed (an accepted proposal; tempered: a swapped row too, which carries its lnprob along)
    equals mp_lnprob_batch at the stored position in a batch of the launch's n_half * n_ensembles rows, bit for bit -- or, where a
    swap brought in a walker that has not moved yet, the value it started with -- and every other row keeps its value.  Returns the accepted proposals per ensemble and the final lnprob."""
    n_ens, nw = len(ens_ds), 2 * n_half
    n = n_half * n_ens
    assert launch_class(n, h.n_simd) == build, (n, h.n_simd)
    ids = np.asarray(ens_ds, dtype=np.int32)
    rng = np.random.default_rng(seed)
    pos = np.concatenate([np.array(t) + 1.0e-2 * rng.standard_normal((nw, 6)) for t in truths])
    table = [(nm.WALK, 1.0, 0.0 if move == "walk" else 3.0, 0.0)] if move != "gauss" else [(nm.GAUSSIAN, 1.0, 1.0, 1.0)]
    with RawNormal(nw, n_ens, 6, seed, target=0, handle=h, ds=ids) as r:
        if betas is not None:
            r.set_temperatures(betas)
        if move == "gauss":
            r.set_gaussian(gauss_near_truths())
        r.set_moves(table)
        r.set_positions(pos)
        _, lnp0, _ = r.state()
        chain, lnp = r.run(steps)
        dpos, dlnp, dacc = r.state()
        n_bad, _ = r.bad()

    def evaluate(rows, walkers):
        k = len(rows)
        padded = np.concatenate([rows, np.repeat(rows[:1], n - k, axis=0)])
        ds = ids[np.concatenate([walkers, np.full(n - k, walkers[0])]).astype(int) // nw]
        return h.lnprob_batch(padded, ds_id=ds)[:k]

    started = {tuple(x): v for x, v in zip(pos, lnp0)}                            # (evaluated by mp_sampler_set_positions)
    cur, prev, checked = lnp0.copy(), pos, 0
    for s in range(steps):
        moved = np.flatnonzero(np.any(chain[s] != prev, axis=1))
        fresh = np.array([k for k in moved if tuple(chain[s][k]) not in started], dtype=int)
        assert betas is not None or len(fresh) == len(moved)
        for k in set(moved) - set(fresh):
            cur[k] = started[tuple(chain[s][k])]
        for part in (fresh[i:i + n] for i in range(0, len(fresh), n)):
            cur[part] = evaluate(chain[s][part], part)
        checked += len(fresh)
        assert np.array_equal(lnp[s], cur), (s, np.flatnonzero(lnp[s] != cur)[:4])
        prev = chain[s]
    assert np.array_equal(dpos, chain[-1]) and np.array_equal(dlnp, cur)
    acc = dacc.reshape(n_ens, nw).sum(axis=1)
    # the reference is not vacuous: every ensemble accepted and rejected proposals, and the stored values are finite
    assert np.all(acc > 0) and np.all(acc < steps * nw) and checked >= acc.sum() and np.all(np.isfinite(cur))
    print(f"{move} launch {n} {build}: {checked} changed rows of {steps * nw * n_ens} held to lnprob_batch, accepted {acc.tolist()}, bad {n_bad}")
    return acc, cur


@pytest.mark.parametrize("case,move", [(c, m) for m in ("walk", "gauss") for c in ("team-1", "team-2", "wave-4", "wave-2")]
                         + [("team-1", "walk3")])     # (Floyd's subsets on one build: the members do not change what is evaluated)
def test_posterior_lnprob_is_lnprob_batch_on_every_build(synth_sets, case, move):  # noqa: F811
    h = synth_sets
    c = posterior_cases(h.n_simd)[case]
    truths = [TRUTHS[TYPES[d]] for d in c["run_ds"]]
    drive_posterior(h, c["run_ds"], truths, c["nbatch"], 3 if case == "team-1" else 2, 20261230, c["build"], move)


@pytest.mark.parametrize("move", ["walk", "gauss"])
def test_posterior_lnprob_is_lnprob_batch_on_the_long_builds(long_sets, move):  # noqa: F811
    drive_posterior(long_sets, [0, 1], [TRUTHS["Humped"], TRUTHS["Humped"]], 8, 3, 20261231, (4, 1, 1), move)


@pytest.mark.parametrize("move", ["walk", "gauss"])
@pytest.mark.parametrize("case", ["team-2", "wave-4", "wave-2"])
def test_posterior_lnprob_is_lnprob_batch_on_the_long_builds_of_every_class(long_mixed_sets, case, move):  # noqa: F811
    """normal_half_kernel's LONG builds beyond (4, 1, 1): one ensemble on Humped next to one on a light curve of 410 or 1 944
    points (long_cases); the 50-point set comes first, so the launches start the ensembles in another order than they are
    numbered."""
    h = long_mixed_sets
    c = long_cases(h.n_simd)[case]
    ds, n_half = c["ds"], c["nbatch"]
    lens = [LONG_MIXED_LENGTHS[d] for d in ds]
    assert sorted(range(len(ds)), key=lambda e: -lens[e]) != list(range(len(ds)))
    steps = 2
    acc, cur = drive_posterior(h, ds, [TRUTHS["Humped"]] * len(ds), n_half, steps, 20261232, c["build"], move)
    assert_long_reference_is_not_vacuous(ds, acc, np.full(len(ds), steps * 2 * n_half), cur.reshape(len(ds), -1).max(axis=1))


def tempered_halves(ns):
    """Slots per ensemble of two groups x ladder (1, 0.3) (four ensembles) whose half-step launch runs each build: the moves of
    normal_half_kernel choose by their own launch size, so these are posterior_cases' fractions of ns over four ensembles."""
    return {"team-1": (8, (4, 1, 1)), "team-2": (3 * ns // 32, (4, 1, 2)), "wave-4": (3 * ns // 16, (1, 4, 1)), "wave-2": (5 * ns // 16, (1, 2, 2))}


@pytest.mark.parametrize("move", ["walk", "gauss"])
@pytest.mark.parametrize("case", ["team-1", "team-2", "wave-4", "wave-2"])
def test_tempered_posterior_lnprob_is_lnprob_batch_on_every_build(synth_sets, case, move):  # noqa: F811
    """Two groups x ladder (1, 0.3), both ensembles of a group on one light curve, two steps with their swap sweeps."""
    h = synth_sets
    n_half, build = tempered_halves(h.n_simd)[case]
    ens_ds = [2, 2, 0, 0]
    drive_posterior(h, ens_ds, [TRUTHS[TYPES[d]] for d in ens_ds], n_half, 2, 20261233, build, move, betas=(1.0, 0.3))


# ---------------------------------------------------------------- statistics
@pytest.mark.parametrize("name", ["walk", "walk-3", "gaussian"])
def test_moves_sample_the_unit_gaussian(name):
    """256 walkers x 6 dims x 3 000 steps, the first third discarded: mean within 0.05 and variance within 0.06 of the unit
    Gaussian's (the bounds of tests/test_gpu_moves.py), which at this length are at least 4 standard errors by the chain's own
    autocorrelation times of x and of x^2 (sqrt(tau / n) and sqrt(2 tau_2 / n) over n = 2 000 x 256 draws), asserted below."""
    from magprop_amd import EnsembleSampler, GaussianMove, WalkMove
    mv = {"walk": WalkMove(), "walk-3": WalkMove(s=3), "gaussian": GaussianMove(np.eye(6), tune=300)}[name]
    s = EnsembleSampler(256, 6, target="gaussian", seed=61, moves=mv)
    s.run_mcmc(np.random.default_rng(60).standard_normal((256, 6)), 3000)
    x = s.get_chain()[1000:]
    af = s.acceptance_fraction
    st = s.get_gaussian_stats() if name == "gaussian" else None
    s.close()
    n = x.shape[0] * x.shape[1]
    tau = max(autocorr_time(x[:, :, d]) for d in range(6))
    tau2 = max(autocorr_time(x[:, :, d] ** 2) for d in range(6))
    mean, var = x.reshape(-1, 6).mean(axis=0), x.reshape(-1, 6).var(axis=0)
    se_mean, se_var = np.sqrt(tau / n), np.sqrt(2.0 * tau2 / n)
    print(f"{name}: acceptance {af.mean():.3f}, tau {tau:.1f}, tau of x^2 {tau2:.1f}, 4 standard errors {4 * se_mean:.4f} / {4 * se_var:.4f}, "
          f"max |mean| {np.abs(mean).max():.4f}, max |var - 1| {np.abs(var - 1.0).max():.4f}" + (f", sigma {st['sigma'][0]:.4f}" if st else ""))
    assert 4.0 * se_mean <= MEAN_TOL and 4.0 * se_var <= VAR_TOL
    assert np.all(np.abs(mean) < MEAN_TOL) and np.all(np.abs(var - 1.0) < VAR_TOL)


def test_gaussian_stats_report_the_tuned_acceptance():
    """The tuning case of tests/test_moves_normal_cpu.py on the device, from both sides: get_gaussian_stats() equals the restated
    state, and the acceptance behind the tuning lies in the CPU test's bracket."""
    from magprop_amd import EnsembleSampler, GaussianMove
    c = TUNE_CASE
    sigmas = []
    for scale0 in (1.0e-3, 1.0e3):
        sigma_ref, acc_ref, ref = tune_case(scale0)
        s = EnsembleSampler(c["n_walkers"], c["ndim"], target="gaussian", seed=c["seed"],
                            moves=GaussianMove(np.eye(c["ndim"]), scale=scale0, tune=c["tune"], target_accept=c["target"]))
        s.run_mcmc(np.random.default_rng(c["seed"]).normal(size=(c["n_walkers"], c["ndim"])), c["tune"])
        mid = s.get_gaussian_stats()
        s.run_mcmc(None, c["after"])
        end = s.get_gaussian_stats()
        s.close()
        got = (end["n_accepted"][0] - mid["n_accepted"][0]) / (end["n_proposed"][0] - mid["n_proposed"][0])
        print(f"from {scale0:g}: sigma {end['sigma'][0]:.4f}, acceptance behind the tuning {got:.3f} (restated {acc_ref:.3f})")
        for k in STATS:
            assert np.array_equal(end[k], ref.state.stats()[k]), k
        assert end["sigma"][0] == mid["sigma"][0] == sigma_ref and end["n_tuned"][0] == c["tune"]
        assert got == acc_ref and ACCEPT_BRACKET[0] < got < ACCEPT_BRACKET[1]
        sigmas.append(end["sigma"][0])
    assert 0.5 < sigmas[0] / sigmas[1] < 2.0


# ---------------------------------------------------------------- Humped, the monitors
def humped_run(gsynth, moves, seed, steps=2000, discard=1000):
    """512 walkers from the reference's ball of 1e-4 around the truths; the chain behind `discard` steps, flattened."""
    from magprop_amd import EnsembleSampler
    truth = np.array(TRUTHS["Humped"])
    s = EnsembleSampler(512, 6, gsynth["Humped_x"], gsynth["Humped_y"], gsynth["Humped_yerr"], seed=seed, moves=moves)
    s.run_mcmc(truth + 1.0e-4 * np.random.default_rng(seed - 1).standard_normal((512, 6)), steps)
    chain, lnp, af = s.get_chain()[discard:], s.get_log_prob()[discard:], s.acceptance_fraction
    s.close()
    tau = max(autocorr_time(chain[:, :, d]) for d in range(6))
    q025, q975 = np.quantile(chain.reshape(-1, 6), [0.025, 0.975], axis=0)
    print(f"Humped, {moves}: acceptance {af.mean():.3f}, tau {tau:.1f} over {len(chain)} steps, central 95 % {np.round(q025, 3)} .. {np.round(q975, 3)}")
    assert np.all(np.isfinite(lnp))
    assert np.all((truth >= q025) & (truth <= q975)), (q025, q975)
    return chain


def test_humped_with_walk_and_de(gsynth):
    """[(WalkMove(), 0.5), (DEMove(), 0.5)], 2 000 steps of which the first 1 000 are burn-in from the ball: every truth inside
    the central 95 %, every stored lnprob finite."""
    from magprop_amd import DEMove, WalkMove
    humped_run(gsynth, [(WalkMove(), 0.5), (DEMove(), 0.5)], 71)


def test_humped_with_kde_and_a_gaussian_move_from_samples(gsynth):
    """[(KDEMove(), 0.8), (GaussianMove.from_samples(burn-in chain, tune=200), 0.2)]: the covariance from the last 100 steps of
    a 400-step KDE burn-in, then the same run and gates."""
    from magprop_amd import EnsembleSampler, GaussianMove, KDEMove
    truth = np.array(TRUTHS["Humped"])
    b = EnsembleSampler(512, 6, gsynth["Humped_x"], gsynth["Humped_y"], gsynth["Humped_yerr"], seed=72, moves=KDEMove())
    b.run_mcmc(truth + 1.0e-4 * np.random.default_rng(73).standard_normal((512, 6)), 400)
    burn = b.get_chain()[300:].reshape(-1, 6)
    b.close()
    humped_run(gsynth, [(KDEMove(), 0.8), (GaussianMove.from_samples(burn, tune=200), 0.2)], 75)


def test_unstored_run_until_converged_ends_with_a_tau_and_a_reservoir():
    from magprop_amd import EnsembleSampler, WalkMove
    s = EnsembleSampler(64, 6, target="gaussian", seed=81, moves=WalkMove())
    s.monitor_autocorr(max_lag=1024)
    s.monitor_samples(size=512)
    s.run_mcmc_until(np.random.default_rng(80).standard_normal((64, 6)), 4000, check_every=200, store=False)
    tau, _, n = s.get_autocorr_device()
    res = s.get_samples()
    print(f"walk move: converged {s.converged} after {s.iteration} steps, tau {tau}")
    assert s.converged and s.iteration < 4000 and n == s.iteration and np.all(np.isfinite(tau)) and np.all(tau > 1.0)
    assert res["x"].shape == (512, 6) and res["n_seen"] == s.iteration * 64 and np.all(np.isfinite(res["log_prob"]))
    s.close()


# ---------------------------------------------------------------- refusals
def test_refusals():
    from magprop_amd import _capi
    inf, nan = float("inf"), float("nan")
    with RawNormal(8, 1, 3, 1) as r:
        for p0, p1 in ((0.0, 0.0), (0.0, 10.0), (nan, 10.0), (inf, 10.0), (-1.0, 10.0), (1.0, 0.5), (1.0, -1.0), (1.0, nan), (1.0, 2.0 ** 31)):
            assert r.set_moves([(nm.GAUSSIAN, 1.0, p0, p1)], check=False) == _capi.MP_EINVAL, (p0, p1)      # (before any other check)
            assert "Gaussian" in _capi.last_error()
        assert r.set_moves([(nm.GAUSSIAN, 1.0, 1.0, 10.0)], check=False) == _capi.MP_ESTATE                  # no covariance yet
        assert "mp_sampler_set_gaussian" in _capi.last_error()
        assert r.L.mp_sampler_get_gaussian(r.sp, None, None, None, None) == _capi.MP_ESTATE                 # no table yet
        bad = FULL_L.copy()
        for i, j, v in ((1, 0, nan), (2, 2, inf), (1, 1, 0.0), (0, 0, -1.0)):
            bad[:] = FULL_L
            bad[i, j] = v
            assert r.set_gaussian(nm.Gauss(bad, nm.VECTOR, 0.25), check=False) == _capi.MP_EINVAL, (i, j, v)
        for mode in (nm.RANDOM, nm.SEQUENTIAL):
            assert r.set_gaussian(nm.Gauss(FULL_L, mode, 0.44), check=False) == _capi.MP_EINVAL
            assert "diagonal" in _capi.last_error()
        for target in (0.0, 1.0, -0.1, 1.5, nan):
            assert r.set_gaussian(nm.Gauss(FULL_L, nm.VECTOR, target), check=False) == _capi.MP_EINVAL, target
        for mode in (-1, 3):
            assert r.set_gaussian(nm.Gauss(FULL_L, mode, 0.25), check=False) == _capi.MP_EINVAL
        assert r.set_moves([(nm.GAUSSIAN, 1.0, 1.0, 10.0)], check=False) == _capi.MP_ESTATE                  # refused calls set nothing
        r.set_gaussian(nm.Gauss(np.diag([1.0, 2.0, 3.0]), nm.RANDOM, 0.44))
        r.set_gaussian(nm.Gauss(FULL_L, nm.VECTOR, 0.25))
        assert r.set_moves([(nm.GAUSSIAN, 0.5, 1.0, 10.0), (nm.GAUSSIAN, 0.5, 2.0, 10.0)], check=False) == _capi.MP_EINVAL
        assert "one Gaussian" in _capi.last_error()
        r.set_moves([(DE, 1.0, 0.0, 1.0e-5)])
        assert r.L.mp_sampler_get_gaussian(r.sp, None, None, None, None) == _capi.MP_ESTATE                 # a table without one
        assert "no Gaussian move" in _capi.last_error()
        # the walk move: n_comp = 4 here
        for p0, p1 in ((1.0, 0.0), (5.0, 0.0), (2.5, 0.0), (-2.0, 0.0), (nan, 0.0), (inf, 0.0), (3.0, 1.0), (0.0, nan)):
            assert r.set_moves([(nm.WALK, 1.0, p0, p1)], check=False) == _capi.MP_EINVAL, (p0, p1)
            assert "walk" in _capi.last_error()
        for s_ok in (0.0, 2.0, 4.0):
            r.set_moves([(nm.WALK, 1.0, s_ok, 0.0)])
        r.set_moves([(nm.GAUSSIAN, 0.5, 1.0, float(2 ** 31 - 1)), (nm.WALK, 0.5, 3.0, 0.0)])
        r.set_positions(np.random.default_rng(2).normal(size=(8, 3)))
        assert r.L.mp_sampler_halfstep_shard(r.sp, 0, 0, 4, None, None) == _capi.MP_ESTATE                 # a table is set
        assert "move table" in _capi.last_error()
        assert r.L.mp_sampler_step_shard(r.sp, 0, 12, None, None) == _capi.MP_ESTATE
        r.run(3)
        assert r.gauss_stats()["n_proposed"][0] in (0, 8, 16, 24)
    with RawNormal(200, 1, 3, 1) as r:                                                                      # n_comp = 100
        assert r.set_moves([(nm.WALK, 1.0, 65.0, 0.0)], check=False) == _capi.MP_EINVAL
        assert "MP_WALK_MAX_S" in _capi.last_error()
        for s_ok in (64.0, 100.0, 0.0):
            r.set_moves([(nm.WALK, 1.0, s_ok, 0.0)])
    with RawNormal(2, 1, 3, 1) as r:
        assert r.set_moves([(nm.WALK, 1.0, 0.0, 0.0)], check=False) == _capi.MP_EINVAL                      # 2 walkers: n_half < 2
        assert "n_walkers >= 4" in _capi.last_error()
