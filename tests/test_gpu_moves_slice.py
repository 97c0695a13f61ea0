"""GPU tests of the ensemble slice-sampling move of the device-resident sampler (include/magprop_amd.h MP_MOVE_SLICE): device
chains against the numpy restatement (tests/slice_move_restated.py) bit for bit on the unit Gaussian -- chain, lnprob,
n_accepted, the mu of every chunk end and the four counters -- split runs, the real posterior on every kernel build against
mp_lnprob_batch calls of the launch's size, tempering, a mixture, the monitors, Humped from the reference's starting ball, and
the refusals."""
import numpy as np
import pytest

import acf_restated as ar
import slice_move_restated as sm
from conftest import TRUTHS, TYPES
from moves_restated import DE
from raw_abi import RawSampler, dp, ip, lp, table_args
from test_autocorr_cpu import MEASURED_DISCREPANCY
from test_gpu_nested import (LONG_MIXED_LENGTHS, assert_long_reference_is_not_vacuous, launch_class, long_cases,  # noqa: F401
                             long_mixed_sets, long_sets, posterior_cases, synth_sets)  # (the three handles are fixtures)

pytestmark = pytest.mark.gpu

HOST_RTOL = 10.0 * MEASURED_DISCREPANCY      # tests/test_gpu_autocorr.py: the device monitor against the host's FFT estimator
COUNTERS = ("nexpand", "ncontract", "nfail", "neval", "n_tuned")
FAILS = np.array([1.8171068, 3.68147895, -2.61786801, 1.99840102, -0.33083576, 2.95613803])   # Humped-box point whose model flags


class RawSlice(RawSampler):
    """RawSampler with the entry points of the slice move."""

    def __init__(self, n_walkers, n_ens, ndim, seed, target=1, handle=None, ds=None):
        super().__init__(n_walkers, n_ens, ndim, seed, target=target, handle=handle, ds=ds)

    def set_limits(self, limits, check=True):
        rc = self.L.mp_sampler_set_slice_limits(self.sp, int(limits[0]), int(limits[1]))
        if check:
            self._ok(rc)
        return rc

    def slice_stats(self):
        out = {"mu": np.empty(self.ne)}
        out.update({k: np.empty(self.ne, dtype=np.int64) for k in COUNTERS})
        self._ok(self.L.mp_sampler_get_slice(self.sp, dp(out["mu"]), *(lp(out[k]) for k in COUNTERS)))
        return out


def device_run(n_walkers, n_ens, ndim, seed, table, limits, pos, runs, betas=None, autocorr=0):
    """The unit-Gaussian target through the C ABI: consecutive mp_sampler_run calls of runs[i] steps.  Returns chain, lnprob,
    n_accepted, the mu behind every call, the move's state and the swap counts (None untempered)."""
    with RawSlice(n_walkers, n_ens, ndim, seed) as r:
        if betas is not None:
            r.set_temperatures(betas)
        r.set_moves(table)
        r.set_limits(limits)
        if autocorr:
            r.set_autocorr(autocorr, 0)
        r.set_positions(pos)
        parts, mus = [], []
        for n in runs:
            parts.append(r.run(n))
            mus.append(r.slice_stats()["mu"])
        swaps = r.swaps(n_ens // len(betas), len(betas)) if betas is not None else None
        return (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), r.accepted(), np.array(mus),
                r.slice_stats(), swaps)


def assert_equal(dev, ref, runs):
    chain, lnp, acc, mus, stats, swaps = dev
    assert np.array_equal(chain, ref.chain) and np.array_equal(lnp, ref.lnp) and np.array_equal(acc, ref.acc)
    ends = np.cumsum(runs) - 1
    assert np.array_equal(mus, ref.mu[ends]), (mus, ref.mu[ends])
    want = ref.state.counters()
    for k in COUNTERS:
        assert np.array_equal(stats[k], want[k]), (k, stats[k], want[k])
    assert np.array_equal(stats["mu"], ref.state.mu)
    if swaps is not None:
        assert np.array_equal(swaps, ref.swaps)


def gaussian_case(n_walkers, n_ens, ndim, steps, mu0, tune, limits, seed, pos=None, runs=None):
    if pos is None:
        pos = np.random.default_rng(seed).normal(size=(n_walkers * n_ens, ndim)) * 1.5
    table = [(sm.SLICE, 1.0, mu0, float(tune))]
    runs = runs or (steps // 3, steps - steps // 3)
    ref = sm.run(pos.copy(), steps, seed, table, limits=limits, n_ensembles=n_ens)
    dev = device_run(n_walkers, n_ens, ndim, seed, table, limits, pos, runs)
    assert_equal(dev, ref, runs)
    return ref


def test_smallest_ensemble_matches_the_restatement_bit_for_bit():
    """4 walkers x 1 ensemble (two partners: n_comp = 2), 3 dims, 60 steps across the tuning boundary (tune 20), limits 4 / 8."""
    ref = gaussian_case(4, 1, 3, 60, 1.0, 20, (4, 8), 20261101)
    assert ref.state.n_tuned[0] == 60 and ref.mu[19, 0] == ref.mu[59, 0] and ref.mu[0, 0] != 1.0
    assert ref.state.nexpand[0] > 0 and ref.state.ncontract[0] > 0


def test_tight_limits_exhaust_budgets_and_fail_slices():
    """18 walkers x 3 ensembles (halves of 9), 3 dims, 40 steps, tune 10, mu0 = 0.05, limits 2 / 2: both budgets come out 0, and
    slices fail at the shrink cap."""
    ref = gaussian_case(18, 3, 3, 40, 0.05, 10, (2, 2), 20261102)
    budgets = [u.budgets for u in ref.state.updates if u.budgets is not None]
    assert any(j == 0 for j, _ in budgets) and any(k == 0 for _, k in budgets)
    assert np.all(ref.state.nfail > 0) and np.any(ref.acc < 40) and np.all(ref.acc > 0)


def test_a_huge_scale_is_shrunk_without_failures():
    """mu0 = 1e6 untuned (tune 0), limits 4 / 64: every slice contracts its way down from an interval of 1e6 directions."""
    ref = gaussian_case(8, 1, 3, 10, 1.0e6, 0, (4, 64), 20261103)
    assert ref.state.ncontract[0] > 10 * max(1, ref.state.nexpand[0]) and ref.state.nfail[0] == 0
    assert np.all(ref.mu == 1.0e6) and np.all(ref.acc == 10)


def test_coinciding_partners_fail_the_slice_where_it_starts():
    """6 walkers of which two start at the same position: a walker that draws the two as its partners has d = 0."""
    seed = 20261110      # (the first seed from 20261104 on at which the restatement takes the path)
    pos = np.random.default_rng(seed).normal(size=(6, 3))
    pos[4] = pos[1]
    ref = gaussian_case(6, 1, 3, 5, 1.0, 2, (4, 8), seed, pos=pos)
    assert any(u.budgets is None for u in ref.state.updates) and ref.state.nfail[0] > 0


def test_a_half_of_one_more_than_a_wavefront_of_slots():
    ref = gaussian_case(130, 1, 3, 5, 1.0, 3, (4, 8), 20261105, runs=(2, 3))
    assert np.all(ref.acc > 0)


@pytest.mark.parametrize("autocorr", [0, 64])
def test_runs_of_one_step_equal_one_run(autocorr):
    """mp_sampler_run(1) x 25 equals one mp_sampler_run(25) across the tuning boundary (tune 10); likewise with the
    autocorrelation monitor on, whose chunk cap differs."""
    seed, table, limits = 20261106, [(sm.SLICE, 1.0, 1.0, 10.0)], (4, 8)
    pos = np.random.default_rng(seed).normal(size=(2 * 16, 3)) * 1.5
    one = device_run(16, 2, 3, seed, table, limits, pos, (25,), autocorr=autocorr)
    many = device_run(16, 2, 3, seed, table, limits, pos, (1,) * 25, autocorr=autocorr)
    for a, b in zip(one[:3], many[:3]):
        assert np.array_equal(a, b)
    assert np.array_equal(one[3][-1], many[3][-1])
    for k in COUNTERS + ("mu",):
        assert np.array_equal(one[4][k], many[4][k]), k
    ref = sm.run(pos.copy(), 25, seed, table, limits=limits, n_ensembles=2)
    assert_equal(many, ref, (1,) * 25)


# ---------------------------------------------------------------- the real posterior against mp_lnprob_batch, build by build
def drive_posterior(h, ens_ds, truths, n_half, steps, seed, build, wide=False):
    """A slice sampler of len(ens_ds) ensembles of 2 n_half walkers on h (target 0) and the restatement in step, every round of
    the restatement ONE mp_lnprob_batch call of the launch's n_half * n_ensembles rows (padded with copies of the first)."""
    from magprop_amd import synth
    n_ens, nw = len(ens_ds), 2 * n_half
    n = n_half * n_ens
    assert launch_class(n, h.n_simd) == build, (n, h.n_simd)
    ids = np.asarray(ens_ds, dtype=np.int32)
    rng = np.random.default_rng(seed)
    pos = np.concatenate([np.array(t) + 1.0e-2 * rng.standard_normal((nw, 6)) for t in truths])
    if wide:   # half of every ensemble in a ball of 0.05 around a point whose model fails: walkers at -inf, failing slices
        for e in range(n_ens):
            pos[e * nw:e * nw + n_half] = np.clip(FAILS + 0.05 * rng.standard_normal((n_half, 6)), synth.PRIOR_LOWER, synth.PRIOR_UPPER)
    calls = [0]

    def evaluate(rows, walkers):
        k = len(rows)
        assert 1 <= k <= n
        padded = np.concatenate([rows, np.repeat(rows[:1], n - k, axis=0)])
        ds = ids[np.concatenate([walkers, np.full(n - k, walkers[0])]).astype(int) // nw]
        out, st = h.lnprob_batch(padded, ds_id=ds, want_status=True)
        calls[0] += 1
        return out[:k], st[:k]

    table, limits = [(sm.SLICE, 1.0, 1.0, 100.0)], (4, 16)
    with RawSlice(nw, n_ens, 6, seed, target=0, handle=h, ds=ids) as r:
        r.set_moves(table)
        r.set_limits(limits)
        r.set_positions(pos)
        _, lnp0, _ = r.state()
        chain, lnp = r.run(steps)
        dpos, dlnp, dacc = r.state()
        stats = r.slice_stats()
        n_bad, bad_rows = r.bad()
    ref = sm.run(pos.copy(), steps, seed, table, limits=limits, n_ensembles=n_ens, lnp=lnp0.copy(), evaluate=evaluate,
                 box=(synth.PRIOR_LOWER, synth.PRIOR_UPPER))
    assert np.array_equal(chain, ref.chain) and np.array_equal(lnp, ref.lnp)
    assert np.array_equal(dpos, ref.chain[-1]) and np.array_equal(dlnp, ref.lnp[-1]) and np.array_equal(dacc, ref.acc)
    want = ref.state.counters()
    for k in COUNTERS:
        assert np.array_equal(stats[k], want[k]), (k, stats[k], want[k])
    assert np.array_equal(stats["mu"], ref.state.mu)
    assert n_bad == len(ref.state.bad) == len(bad_rows)
    assert sorted(map(tuple, bad_rows)) == sorted(map(tuple, ref.state.bad))
    # conditions on the inputs, read off the restatement: a step out happened, a shrink point was rejected, every ensemble moved
    assert ref.state.nexpand.sum() > 0 and ref.state.ncontract.sum() > 0
    assert np.all(ref.acc.reshape(n_ens, nw).sum(axis=1) > 0)
    if wide:   # failed evaluations reached the log, and walkers that started at -inf escaped
        assert n_bad > 0 and np.any(~np.isfinite(lnp0) & np.isfinite(ref.lnp[-1]))
    print(f"launch {n} {build}: {calls[0]} batches, start lnprob -inf {int(np.sum(~np.isfinite(lnp0)))}, bad {n_bad}, "
          + ", ".join(f"{k} {want[k].tolist()}" for k in COUNTERS) + f", mu {ref.state.mu.tolist()}")
    return ref, pos, lnp0


@pytest.mark.parametrize("case", ["team-1", "team-2", "wave-4", "wave-2"])
def test_posterior_slices_match_lnprob_batch_on_every_build(synth_sets, case):  # noqa: F811
    h = synth_sets
    c = posterior_cases(h.n_simd)[case]
    truths = [TRUTHS[TYPES[d]] for d in c["run_ds"]]
    drive_posterior(h, c["run_ds"], truths, c["nbatch"], 2 if case == "team-1" else 1, 20261107, c["build"])


def test_failed_evaluations_reach_the_fbad_window_and_lost_walkers_escape(synth_sets):  # noqa: F811
    """The team-1 shape with half of every ensemble started around a point whose model fails, 3 steps: the models that fail
    inside slices are counted and logged as the restatement lists them, and walkers whose own lnprob is -inf move to a finite
    one.  (The serial oracle puts this start at 24 walkers at -inf, about 500 failed evaluations and 13 escapes.)"""
    c = posterior_cases(synth_sets.n_simd)["team-1"]
    truths = [TRUTHS[TYPES[d]] for d in c["run_ds"]]
    drive_posterior(synth_sets, c["run_ds"], truths, c["nbatch"], 3, 20261111, c["build"], wide=True)


def test_posterior_slices_match_lnprob_batch_on_the_long_builds(long_sets):  # noqa: F811
    drive_posterior(long_sets, [0, 1], [TRUTHS["Humped"], TRUTHS["Humped"]], 8, 1, 20261108, (4, 1, 1))


@pytest.mark.parametrize("case", ["team-2", "wave-4", "wave-2"])
def test_posterior_slices_match_lnprob_batch_on_the_long_builds_of_every_class(long_mixed_sets, case):  # noqa: F811
    """slice_half_kernel's LONG builds beyond (4, 1, 1): one ensemble on Humped next to one on a light curve of 410 or 1 944
    points (long_cases); the 50-point set comes first, so the launches start the ensembles in another order than they are
    numbered.  Conditions on the inputs, from the restatement: the ensemble on the long set moved a walker and turned a shrink
    point down, and its best lnprob is finite."""
    h = long_mixed_sets
    c = long_cases(h.n_simd)[case]
    ds, n_half = c["ds"], c["nbatch"]
    lens = [LONG_MIXED_LENGTHS[d] for d in ds]
    assert sorted(range(len(ds)), key=lambda e: -lens[e]) != list(range(len(ds)))
    ref, pos, lnp0 = drive_posterior(h, ds, [TRUTHS["Humped"]] * len(ds), n_half, c["iters"], 20261304, c["build"])
    acc = ref.acc.reshape(len(ds), -1).sum(axis=1)
    assert_long_reference_is_not_vacuous(ds, acc, acc + ref.state.ncontract, ref.lnp[-1].reshape(len(ds), -1).max(axis=1))
    if case == "wave-4":   # a kernel that read the other ensemble's light curve would start from these values instead
        ens = np.arange(len(pos)) // (2 * n_half)
        first, other = (h.lnprob_batch(pos, ds_id=np.asarray(d, dtype=np.int32)[ens]) for d in (ds, ds[::-1]))
        assert np.array_equal(first, lnp0)
        assert np.all(np.any((first != other).reshape(len(ds), -1), axis=1))


# ---------------------------------------------------------------- tempering, mixtures, monitors
def test_tempered_slices_match_the_restatement_and_keep_a_scale_per_temperature():
    """2 groups x ladder (1, 0.3), 16 walkers each, 30 steps: equal to the restatement, swap counts included."""
    seed, table, limits, ladder = 20261109, [(sm.SLICE, 1.0, 1.0, 20.0)], (8, 16), (1.0, 0.3)
    pos = np.random.default_rng(seed).normal(size=(4 * 16, 3)) * 1.5
    ref = sm.run(pos.copy(), 30, seed, table, limits=limits, n_ensembles=4, betas=[ladder[e % 2] for e in range(4)], n_temps=2)
    dev = device_run(16, 4, 3, seed, table, limits, pos, (12, 18), betas=ladder)
    assert_equal(dev, ref, (12, 18))
    assert ref.swaps.shape == (2, 1) and np.all(ref.swaps > 0)
    assert ref.state.mu[0] != ref.state.mu[1] and ref.state.mu[2] != ref.state.mu[3]


def test_mixture_with_de_matches_the_restatement():
    """[(SliceMove(), 0.5), (DEMove(), 0.5)], 32 walkers, 40 steps: equal to the restatement, and only slice steps count."""
    seed, limits = 20261110, (32, 64)
    table = [(sm.SLICE, 0.5, 1.0, 100.0), (DE, 0.5, 0.0, 1.0e-5)]
    pos = np.random.default_rng(seed).normal(size=(32, 3)) * 1.5
    ref = sm.run(pos.copy(), 40, seed, table, limits=limits)
    dev = device_run(32, 1, 3, seed, table, limits, pos, (15, 25))
    assert_equal(dev, ref, (15, 25))
    n_slice = int(np.sum(ref.drawn == 0))
    assert 5 < n_slice < 35 and dev[4]["n_tuned"][0] == n_slice


def test_monitors_and_run_until_converged():
    """64 walkers x 6-d Gaussian x 1 200 steps behind 100 tuning steps: the device autocorrelation time against the host
    estimate on the stored chain, below the same measurement of a stretch run; run_mcmc_until converges; the posterior monitor
    counts the run's samples."""
    from magprop_amd import EnsembleSampler, SliceMove
    pos = np.random.default_rng(41).standard_normal((64, 6))
    taus = {}
    for name, mv in (("slice", SliceMove()), ("stretch", None)):
        s = EnsembleSampler(64, 6, target="gaussian", seed=42, moves=mv)
        s.run_mcmc(pos, 100)
        s.monitor_autocorr(max_lag=1024)
        s.monitor_posterior(bins=64, bins2=0, range=np.array([[-6.0, 6.0]] * 6))
        s.run_mcmc(None, 1200)
        tau, win, n = s.get_autocorr_device()
        ht, hw = ar.host_tau_window(s.get_chain()[100:], 5.0)
        assert n == 1200 and np.array_equal(win, hw) and np.max(np.abs(tau / ht - 1.0)) <= HOST_RTOL
        assert s.get_posterior()["n"] == 1200 * 64
        if mv is not None:
            st = s.get_slice_stats()
            assert st["n_tuned"][0] == 1300 and st["nfail"][0] == 0 and np.all(s.acceptance_fraction == 1.0)
            print(f"slice: mu {st['mu'][0]:.3f}, {st['neval'][0] / (1300 * 64):.2f} evaluations per walker and step")
        taus[name] = tau
        s.close()
    print(f"tau: slice {taus['slice']}, stretch {taus['stretch']}")
    assert np.max(taus["slice"]) < np.max(taus["stretch"])
    u = EnsembleSampler(64, 6, target="gaussian", seed=43, moves=SliceMove())
    u.run_mcmc_until(pos, 3000, check_every=100, store=False)
    assert u.converged and u.iteration < 3000
    u.close()


def test_humped_from_the_reference_ball(gsynth):
    """Humped as it is, 128 walkers from the reference's ball of 1e-4 around the truths, 200 tuning steps dropped, 1 000 kept,
    against a stretch chain of 512 walkers x 3 000 steps (first 1 000 discarded), with the gates of
    tests/test_gpu_nested.py::test_humped_posterior_samples: truths inside the central 95 %, means within 0.3 chain sigma,
    standard deviations within a factor 1.35.  Additionally at most 1 % of the slices fail and every walker moves in at least
    99 % of its steps; a band over the slice chain brackets its median."""
    from magprop_amd import EnsembleSampler, SliceMove
    x, y, yerr = gsynth["Humped_x"], gsynth["Humped_y"], gsynth["Humped_yerr"]
    truth = np.array(TRUTHS["Humped"])
    s = EnsembleSampler(128, 6, x, y, yerr, seed=51, moves=SliceMove(tune=200))
    s.run_mcmc(truth + 1.0e-4 * np.random.default_rng(50).standard_normal((128, 6)), 1200)
    eq = s.get_chain()[200:].reshape(-1, 6)
    st = s.get_slice_stats()
    af = s.acceptance_fraction
    band = s.get_model_band(q=(0.025, 0.5, 0.975), discard=200, thin=100)
    n_bad, _ = s.get_bad()
    s.close()
    e = EnsembleSampler(512, 6, x, y, yerr, seed=31)
    e.run_mcmc(truth + 1.0e-4 * np.random.default_rng(30).standard_normal((512, 6)), 3000)
    ref = e.get_chain()[1000:].reshape(-1, 6)
    e.close()
    q025, q975 = np.quantile(eq, [0.025, 0.975], axis=0)
    dmean = np.abs(eq.mean(axis=0) - ref.mean(axis=0)) / ref.std(axis=0)
    sratio = eq.std(axis=0) / ref.std(axis=0)
    print(f"Humped, slice: mu {st['mu'][0]:.4f}, {st['neval'][0] / (1200 * 128):.2f} evaluations per walker and step, nexpand "
          f"{st['nexpand'][0]}, ncontract {st['ncontract'][0]}, nfail {st['nfail'][0]}, failed models {n_bad}, acceptance "
          f"{af.min():.4f} .. {af.max():.4f}; mean shift / sigma {np.round(dmean, 3)}, sd ratio {np.round(sratio, 3)}")
    assert np.all((truth >= q025) & (truth <= q975)), (q025, q975)
    assert np.all(dmean < 0.3), dmean
    assert np.all((sratio > 1 / 1.35) & (sratio < 1.35)), sratio
    assert st["nfail"][0] <= 0.01 * 1200 * 128
    assert np.all(af >= 0.99), af.min()
    lo_, mid, hi_ = band["Ltot"]
    ok = np.isfinite(mid)
    assert band["n_used"] > 0 and np.all(lo_[ok] <= mid[ok]) and np.all(mid[ok] <= hi_[ok])


def test_refusals():
    from magprop_amd import _capi
    with RawSlice(8, 1, 3, 1) as r:
        for p0, p1 in ((0.0, 10.0), (-1.0, 10.0), (float("nan"), 10.0), (float("inf"), 10.0), (1.0, -1.0), (1.0, 0.5),
                       (1.0, float("nan")), (1.0, 2.0 ** 31), (1.0, float("inf"))):
            assert r.set_moves([(sm.SLICE, 1.0, p0, p1)], check=False) == _capi.MP_EINVAL, (p0, p1)
            assert "slice" in _capi.last_error()
        assert r.set_moves([(sm.SLICE, 1.0, 1.0, 10.0), (sm.SLICE, 1.0, 2.0, 10.0)], check=False) == _capi.MP_EINVAL
        assert "one slice" in _capi.last_error()
        assert r.L.mp_sampler_get_slice(r.sp, None, None, None, None, None, None) == _capi.MP_ESTATE      # no table yet
        r.set_moves([(DE, 1.0, 0.0, 1.0e-5)])
        assert r.L.mp_sampler_get_slice(r.sp, None, None, None, None, None, None) == _capi.MP_ESTATE      # a table without one
        assert "no slice move" in _capi.last_error()
        r.set_moves([(sm.SLICE, 1.0, 1.0, float(2 ** 31 - 1))])
        for limits in ((0, 8), (4097, 8), (4, 0), (4, 253), (-1, -1)):
            assert r.set_limits(limits, check=False) == _capi.MP_EINVAL, limits
        r.set_limits((4096, 252))
        r.set_limits((1, 1))
        r.set_positions(np.random.default_rng(2).normal(size=(8, 3)))
        assert r.L.mp_sampler_halfstep_shard(r.sp, 0, 0, 4, None, None) == _capi.MP_ESTATE                 # a table is set
        assert "move table" in _capi.last_error()
        r.run(3)
        st = r.slice_stats()
        assert st["n_tuned"][0] == 3 and st["nexpand"][0] == 0                                             # (a budget of 1: no step out)
    with RawSlice(2, 1, 3, 1) as r:
        assert r.set_moves([(sm.SLICE, 1.0, 1.0, 10.0)], check=False) == _capi.MP_EINVAL                   # 2 walkers: n_half < 2
        assert "n_walkers >= 4" in _capi.last_error()
    kinds, weights, params = table_args([(sm.SLICE, 1.0, 1.0, 10.0)])
    assert _capi.lib().mp_sampler_set_moves(None, 1, ip(kinds), dp(weights), dp(params)) == _capi.MP_EINVAL
