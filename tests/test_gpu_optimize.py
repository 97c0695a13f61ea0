"""GPU tests of the differential-evolution optimizer (include/magprop_amd.h mp_optimizer_*, magprop_amd.optimize): the device
state against the numpy restatement (tests/de_restated.py) bit for bit, best fits on the synthetic sets and on long Swift light
curves, frozen populations and refused handles."""
import ctypes as C

import numpy as np
import pytest

import de_restated as de
from conftest import GOLDEN, TRUTHS, TYPES
from raw_abi import dp, ip, synth_handle
from test_gpu_nested import assert_long_reference_is_not_vacuous, launch_class, long_cases, long_mixed_sets  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu


class RawOptimizer:
    """mp_optimizer_* through ctypes on handle h."""

    def __init__(self, h, popsize, n_pops, ndim, lower, upper, seed, strategy, target, ds=None, f=(0.5, 1.0), cr=0.7, tol=0.01,
                 atol=0.0):
        from magprop_amd import _capi
        self.L, self.popsize, self.n_pops, self.ndim = _capi.lib(), popsize, n_pops, ndim
        self.lo, self.hi = np.ascontiguousarray(lower, dtype=np.float64), np.ascontiguousarray(upper, dtype=np.float64)
        ids = None if ds is None else np.ascontiguousarray(ds, dtype=np.int32)
        self.o = self.L.mp_optimizer_create(h._h, popsize, n_pops, ndim, ip(ids), C.c_uint64(seed), strategy, f[0], f[1], cr, tol,
                                            atol, dp(self.lo), dp(self.hi), target)
        assert self.o, _capi.last_error()

    def set_population(self, pop):
        p = np.ascontiguousarray(pop, dtype=np.float64)
        assert self.L.mp_optimizer_set_population(self.o, dp(p)) == 0

    def run(self, n):
        running = C.c_int32(-1)
        assert self.L.mp_optimizer_run(self.o, n, C.byref(running)) == 0
        return running.value

    def state(self):
        from magprop_amd import optimize
        return optimize.get_state(self.L, self.o, self.n_pops, self.popsize, self.ndim)

    def close(self):
        self.L.mp_optimizer_destroy(self.o)


def _assert_equal(st, s):
    assert np.array_equal(st["pop"], s.pop)
    assert np.array_equal(st["lnprob"], s.lnp)
    assert np.array_equal(st["status"], s.status)
    assert np.array_equal(st["best"], s.best)
    assert np.array_equal(st["nit"], s.nit)
    assert np.array_equal(st["converged"], s.converged)
    assert np.array_equal(st["nfev"], s.nfev)


@pytest.mark.parametrize("strategy", [de.BEST1BIN, de.RAND1BIN])
@pytest.mark.parametrize("n_pops", [1, 3])
def test_gaussian_state_matches_the_restatement_bit_for_bit(strategy, n_pops):
    """Unit Gaussian in a box whose corner (0.05, 0.1, -0.2) lies next to the optimum: 300 generations run as 120 + 180, every
    population, lnprob, status, best index, nit and nfev equal to the restatement."""
    ndim, popsize, seed = 3, 12, 20261015 + strategy
    lo, hi = np.array([0.05, 0.1, -3.0]), np.array([3.0, 2.5, -0.2])
    pop0 = lo + (hi - lo) * np.random.default_rng(7 + n_pops).random((n_pops, popsize, ndim))
    kw = dict(strategy=strategy, f_lo=0.5, f_hi=1.0, cr=0.7, tol=1e-12, atol=0.0, lower=lo, upper=hi)
    ref = de.run(pop0, 300, de.gaussian, seed, **kw)
    h = synth_handle()
    opt = RawOptimizer(h, popsize, n_pops, ndim, lo, hi, seed, strategy, 1, tol=1e-12)
    try:
        opt.set_population(pop0.reshape(-1, ndim))
        opt.run(120)
        opt.run(180)
        st = opt.state()
    finally:
        opt.close()
        h.close()
    _assert_equal(st, ref)
    assert ref.lnp.max() > -0.5 * (0.05 ** 2 + 0.1 ** 2 + 0.2 ** 2) - 1e-3


def test_humped_posterior_matches_the_restatement_with_lnprob_batch():
    """20 generations of two populations on Humped with the posterior: the restatement's evaluations are mp_lnprob_batch calls on
    batches of the launch's size (60 rows: the same kernel build), and the device state equals it bit for bit."""
    from magprop_amd import optimize, synth
    g = np.load(GOLDEN + "/golden_synth.npz")
    h = synth_handle()
    h.set_prior(synth.PRIOR_LOWER, synth.PRIOR_UPPER, synth.LOG_MASK)
    h.set_dataset(0, g["Humped_x"], g["Humped_y"], g["Humped_yerr"])
    lo, hi = synth.PRIOR_LOWER, synth.PRIOR_UPPER
    rng = np.random.default_rng(5)
    pop0 = np.stack([optimize.latin_hypercube(rng, 30, lo, hi) for _ in range(2)])

    def evaluate(rows):
        assert rows.shape == (60, 6)
        return h.lnprob_batch(rows, ds_id=0, want_status=True)

    ref = de.run(pop0, 20, evaluate, 99, de.BEST1BIN, 0.5, 1.0, 0.7, 0.01, 0.0, lo, hi)
    opt = RawOptimizer(h, 30, 2, 6, lo, hi, 99, de.BEST1BIN, 0, ds=[0, 0])
    try:
        opt.set_population(pop0.reshape(-1, 6))
        opt.run(20)
        st = opt.state()
    finally:
        opt.close()
        h.close()
    _assert_equal(st, ref)
    assert np.all(np.isfinite(ref.lnp.max(axis=1)))


def _humped_and_classic():
    """A handle with the synthetic prior, Humped (ds 0) and Classic (ds 1)."""
    from magprop_amd import synth
    g = np.load(GOLDEN + "/golden_synth.npz")
    h = synth_handle()
    h.set_prior(synth.PRIOR_LOWER, synth.PRIOR_UPPER, synth.LOG_MASK)
    h.set_dataset(0, g["Humped_x"], g["Humped_y"], g["Humped_yerr"])
    h.set_dataset(1, g["Classic_x"], g["Classic_y"], g["Classic_yerr"])
    return h


@pytest.mark.parametrize("case, strategy", [("team-2", de.BEST1BIN), ("team-2", de.RAND1BIN), ("wave-4", de.BEST1BIN),
                                            ("wave-2", de.BEST1BIN)])
def test_posterior_matches_the_restatement_with_lnprob_batch_on_the_other_builds(case, strategy):
    """Two populations on different datasets (population 0 on ds 1, population 1 on ds 0) at the smallest launch of each build
    the 60-member test does not run -- a team with two wavefronts per SIMD (3/8 of the SIMDs), one wavefront per walker with 4
    steps per lane (3/4) and with 2 (5/4): 5 generations (20 at the smaller launch) equal the restatement whose evaluations are
    mp_lnprob_batch calls of the launch's size with every row's dataset.  (The LONG builds: below.)"""
    from magprop_amd import optimize, synth
    h = _humped_and_classic()
    try:
        ns = h.n_simd
        n, build, gens = {"team-2": (3 * ns // 8, (4, 1, 2), 20), "wave-4": (3 * ns // 4, (1, 4, 1), 5),
                          "wave-2": (5 * ns // 4, (1, 2, 2), 5)}[case]
        popsize, ds = n // 2, [1, 0]
        assert launch_class(2 * popsize, ns) == build and 5 <= popsize <= 1024
        lo, hi = synth.PRIOR_LOWER, synth.PRIOR_UPPER
        rng = np.random.default_rng(6)
        pop0 = np.stack([optimize.latin_hypercube(rng, popsize, lo, hi) for _ in range(2)])
        ids = np.repeat(np.array(ds, dtype=np.int32), popsize)

        def evaluate(rows):
            assert rows.shape == (2 * popsize, 6)
            return h.lnprob_batch(rows, ds_id=ids, want_status=True)

        ref = de.run(pop0, gens, evaluate, 101, strategy, 0.5, 1.0, 0.7, 0.01, 0.0, lo, hi)
        opt = RawOptimizer(h, popsize, 2, 6, lo, hi, 101, strategy, 0, ds=ds)
        try:
            opt.set_population(pop0.reshape(-1, 6))
            opt.run(gens)
            st = opt.state()
        finally:
            opt.close()
    finally:
        h.close()
    _assert_equal(st, ref)
    # conditions on the inputs, from the restatement: both populations ran every generation and replaced members
    assert np.all(ref.nit == gens) and np.all(np.isfinite(ref.lnp.max(axis=1)))
    assert np.all(np.any(ref.pop != pop0, axis=(1, 2)))
    print(f"{case}: launch {2 * popsize} {build}, flagged members at the end {int(np.sum(ref.status != 0))}")


@pytest.mark.parametrize("case", ["team-1", "team-2", "wave-4", "wave-2"])
def test_posterior_matches_the_restatement_with_lnprob_batch_on_the_long_builds(long_mixed_sets, case):
    """opt_trial_kernel's LONG builds on every class: a handle that holds light curves of 50, 112, 410 and 1 944 points, one
    population on Humped and the others on long sets (long_cases), 20 generations on the 60-member team, 10 on the larger
    team, 3 and 2 on the one-wavefront launches.  The restatement goes generation by generation, so that the members every
    population replaced and kept are counted."""
    from magprop_amd import optimize, synth
    h = long_mixed_sets
    c = long_cases(h.n_simd)[case]
    ds, gens = c["ds"], {"team-1": 20, "team-2": 10, "wave-4": 3, "wave-2": 2}[case]
    n_pops, popsize = len(ds), c["pop"] // len(ds)
    assert launch_class(n_pops * popsize, h.n_simd) == c["build"] and 5 <= popsize <= 1024
    lo, hi = synth.PRIOR_LOWER, synth.PRIOR_UPPER
    rng = np.random.default_rng(7)
    pop0 = np.stack([optimize.latin_hypercube(rng, popsize, lo, hi) for _ in range(n_pops)])

    def evaluator(pop_ds):
        ids = np.repeat(np.array(pop_ds, dtype=np.int32), popsize)

        def evaluate(rows):
            assert rows.shape == (n_pops * popsize, 6)
            return h.lnprob_batch(rows, ds_id=ids, want_status=True)
        return evaluate

    ref = de.start(pop0, evaluator(ds))
    lnp0 = ref.lnp.copy()
    replaced = np.zeros(n_pops, dtype=np.int64)
    for g in range(1, gens + 1):
        before = ref.pop.copy()
        de.generation(ref, g, evaluator(ds), 102, de.BEST1BIN, 0.5, 1.0, 0.7, 0.01, 0.0, lo, hi)
        replaced += np.any(ref.pop != before, axis=2).sum(axis=1)
    opt = RawOptimizer(h, popsize, n_pops, 6, lo, hi, 102, de.BEST1BIN, 0, ds=ds)
    try:
        opt.set_population(pop0.reshape(-1, 6))
        opt.run(gens)
        st = opt.state()
    finally:
        opt.close()
    _assert_equal(st, ref)
    assert np.all(ref.nit == gens)
    assert_long_reference_is_not_vacuous(ds, replaced, gens * np.full(n_pops, popsize), ref.lnp.max(axis=1))
    if case == "team-1":   # a kernel that read another population's light curve would start from these values instead
        lnp1 = de.start(pop0, evaluator([ds[1], ds[0]] + ds[2:])).lnp
        assert not np.array_equal(lnp1[0], lnp0[0]) and not np.array_equal(lnp1[1], lnp0[1]) and np.array_equal(lnp1[2], lnp0[2])
    print(f"long {case}: launch {n_pops * popsize} {c['build']}, replaced {replaced.tolist()} of {gens * popsize}, flagged members "
          f"at the end {int(np.sum(ref.status != 0))}")


@pytest.fixture(scope="module")
def synth_fit():
    """Four populations per synthetic dataset from Latin hypercubes over the prior box, all in one call."""
    from magprop_amd import optimize
    g = np.load(GOLDEN + "/golden_synth.npz")
    ds = [(g[f"{t}_x"], g[f"{t}_y"], g[f"{t}_yerr"]) for t in TYPES]
    res = optimize.differential_evolution(datasets=ds, n_starts=4, seed=3, maxiter=1000)
    return ds, res


def test_best_fits_on_the_four_synthetic_sets_reach_the_truth(synth_fit):
    from magprop_amd import LogProb
    ds, res = synth_fit
    assert len(res) == 16
    for k, t in enumerate(TYPES):
        lp_truth = LogProb(*ds[k])(np.array(TRUTHS[t], dtype=float))
        best = max(r.lnprob for r in res[4 * k:4 * k + 4])
        assert best >= lp_truth - 1.0, (t, best, lp_truth)
        for r in res[4 * k:4 * k + 4]:
            assert r.fun == -r.lnprob and r.nfev == r.population.shape[0] * (r.nit + 1)
            assert r.success == (r.nit < 1000)


def test_population_lnprob_equals_logprob_in_a_batch_of_the_same_size(synth_fit):
    from magprop_amd import LogProb
    ds, res = synth_fit
    lp = LogProb(*ds[0])
    for d in ds[1:]:
        lp.add_dataset(*d)
    P = np.concatenate([r.population for r in res])
    ids = np.repeat(np.arange(4, dtype=np.int32), 4 * res[0].population.shape[0])
    out, st = lp.handle.lnprob_batch(P, ds_id=ids, want_status=True)
    assert P.shape[0] == 16 * 90
    assert np.array_equal(out, np.concatenate([r.population_lnprob for r in res]))
    assert np.array_equal(st, np.concatenate([r.population_status for r in res]))


def test_converged_populations_stay_frozen():
    """Population 0 starts collapsed (converges at once), population 1 spread over the box: after the first converges, its
    members, lnprob, nit and nfev no longer change while the other goes on; the whole run equals the restatement."""
    ndim, popsize, seed = 2, 10, 4
    lo, hi = np.array([-5.0, -5.0]), np.array([5.0, 5.0])
    rng = np.random.default_rng(0)
    pop0 = np.stack([1.0 + 1e-9 * rng.random((popsize, ndim)), lo + (hi - lo) * rng.random((popsize, ndim))])
    h = synth_handle()
    opt = RawOptimizer(h, popsize, 2, ndim, lo, hi, seed, de.BEST1BIN, 1, tol=1e-3, atol=1e-9)
    try:
        opt.set_population(pop0.reshape(-1, ndim))
        assert opt.run(3) == 1
        a = opt.state()
        assert a["converged"].tolist() == [1, 0]
        assert opt.run(40) in (0, 1)
        b = opt.state()
    finally:
        opt.close()
        h.close()
    assert np.array_equal(a["pop"][0], b["pop"][0]) and np.array_equal(a["lnprob"][0], b["lnprob"][0])
    assert a["nit"][0] == b["nit"][0] and a["nfev"][0] == b["nfev"][0] == popsize * (a["nit"][0] + 1)
    assert b["nit"][1] > a["nit"][1] and b["nfev"][1] == popsize * (b["nit"][1] + 1)
    _assert_equal(b, de.run(pop0, 43, de.gaussian, seed, de.BEST1BIN, 0.5, 1.0, 0.7, 1e-3, 1e-9, lo, hi))


def test_long_swift_light_curve_synth_reaches_the_truth(gswift):
    """LONG builds: the synth variant on the 1 921 points of GRB 060614 (swift_060614_pars[0] is its truth)."""
    from magprop_amd import LogProb, optimize
    x, y, yerr = gswift["swift_060614_ds"]
    truth = gswift["swift_060614_pars"][0]
    res = optimize.differential_evolution(x, y, yerr, seed=1, maxiter=1000)
    lp_truth = LogProb(x, y, yerr)(truth)
    assert res.lnprob >= lp_truth - 1.0, (res.lnprob, lp_truth)


def test_long_swift_light_curve_lib(gswift):
    """The lib variant on GRB 051016B (79 points, GRBtype "S"): 6 dimensions reach the best finite lnlike of the fixture's
    parameter sets; 9 dimensions finish with a finite best inside the box."""
    from magprop_amd import mcmc_eqns, optimize
    x, y, yerr = gswift["swift_051016B_libS_ds"]
    ref = gswift["swift_051016B_libS_lnlike"]
    res = optimize.differential_evolution(x, y, yerr, variant="lib", GRBtype="S", seed=2, maxiter=1000)
    assert res.lnprob >= np.max(ref[np.isfinite(ref)]), (res.lnprob, ref)
    lo, hi = mcmc_eqns._bounds(9)
    res9 = optimize.differential_evolution(x, y, yerr, variant="lib", GRBtype="S", bounds=np.stack([lo, hi], axis=1), popsize=10,
                                           seed=2, maxiter=300)
    assert np.isfinite(res9.lnprob) and np.all((res9.x >= lo) & (res9.x <= hi))


def test_multi_device_and_alternative_torque_handles_are_refused():
    from magprop_amd import _capi
    L = _capi.lib()
    lo, hi = np.zeros(6), np.ones(6)
    x = np.logspace(0.5, 3.0, 20)
    hm = synth_handle(device=[0])
    ha = synth_handle(dipole_torque=1)
    try:
        for h, what in ((hm, "ONE device"), (ha, "dipole torque")):
            h.set_dataset(0, x, np.ones_like(x), np.ones_like(x))
            o = L.mp_optimizer_create(h._h, 10, 1, 6, None, C.c_uint64(0), 0, 0.5, 1.0, 0.7, 0.01, 0.0, dp(lo), dp(hi), 0)
            assert not o and what in _capi.last_error()
        # argument codes on a plain handle
        h = synth_handle()
        for bad in (dict(popsize=4), dict(cr=1.5), dict(f=(1.0, 0.5)), dict(upper=np.zeros(6))):
            kw = dict(popsize=10, cr=0.7, f=(0.5, 1.0), upper=hi)
            kw.update(bad)
            o = L.mp_optimizer_create(h._h, kw["popsize"], 1, 6, None, C.c_uint64(0), 0, kw["f"][0], kw["f"][1], kw["cr"], 0.01,
                                      0.0, dp(lo), dp(np.ascontiguousarray(kw["upper"])), 1)
            assert not o, bad
        h.close()
    finally:
        hm.close()
        ha.close()
