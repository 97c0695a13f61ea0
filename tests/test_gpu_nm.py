"""GPU tests of the Nelder-Mead simplex search (include/magprop_amd.h mp_simplex_*, magprop_amd.optimize.nelder_mead and
differential_evolution(polish=True)): the device state against the numpy restatement (tests/nm_restated.py, which the CPU tests
hold against scipy) bit for bit on the test targets and on the posterior on every kernel build, frozen simplexes, split runs,
break-up corners, the polish and refused handles."""
import ctypes as C

import numpy as np
import pytest

import nm_restated as nm
from conftest import GOLDEN, TRUTHS, TYPES
from raw_abi import dp, ip, synth_handle
from test_gpu_nested import assert_long_reference_is_not_vacuous, launch_class, long_cases, long_mixed_sets  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu


class RawSimplex:
    """mp_simplex_* through ctypes on handle h."""

    def __init__(self, h, n, ndim, lower, upper, target, ds=None, co=(1.0, 2.0, 0.5, 0.5), xatol=1e-4, fatol=1e-4):
        from magprop_amd import _capi
        self.L, self.n, self.ndim = _capi.lib(), n, ndim
        self.lo, self.hi = np.ascontiguousarray(lower, dtype=np.float64), np.ascontiguousarray(upper, dtype=np.float64)
        ids = None if ds is None else np.ascontiguousarray(ds, dtype=np.int32)
        self.s = self.L.mp_simplex_create(h._h, n, ndim, ip(ids), *co, xatol, fatol, dp(self.lo), dp(self.hi), target)
        assert self.s, _capi.last_error()

    def set_vertices(self, sim):
        v = np.ascontiguousarray(sim, dtype=np.float64)
        assert v.shape == (self.n, self.ndim + 1, self.ndim)
        assert self.L.mp_simplex_set_vertices(self.s, dp(v)) == 0

    def run(self, n):
        running = C.c_int32(-1)
        assert self.L.mp_simplex_run(self.s, n, C.byref(running)) == 0
        return running.value

    def state(self):
        from magprop_amd import optimize
        return optimize.get_simplex_state(self.L, self.s, self.n, self.ndim)

    def close(self):
        self.L.mp_simplex_destroy(self.s)


def _assert_equal(st, s):
    assert np.array_equal(st["sim"], s.sim)
    assert np.array_equal(st["lnprob"], s.lnp)
    assert np.array_equal(st["status"], s.status)
    assert np.array_equal(st["nit"], s.nit)
    assert np.array_equal(st["nfev"], s.nfev)
    assert np.array_equal(st["stopped"], s.stopped)
    assert np.array_equal(st["outcomes"], s.outcomes)
    assert not np.any(np.isnan(st["lnprob"])) and not np.any(np.isnan(st["sim"]))


def _test_box(ndim):
    """Binds in the even coordinates (the targets' optimum 0 lies above [-0.9, -0.01]), free in the odd ones.  Below x_0 = 0 the
    terraces of target 2 rise against the Gaussian, and next to the bound they outweigh it: ridges a simplex has to shrink on."""
    even = np.arange(ndim) % 2 == 0
    return np.where(even, -0.9, -2.0), np.where(even, -0.01, 2.0)


def _test_simplexes(n, ndim, seed):
    """Even simplexes: random over the box and partly beyond it (the reflect-then-clip rule); odd ones: of the terraces' size
    (0.03) next to the binding bounds, where the shrinks happen within the 60 iterations.  Simplex 0 starts with a tie between
    different rows: its vertex 1 is vertex 0 with x_1 mirrored, which both test targets value alike."""
    lo, hi = _test_box(ndim)
    rng = np.random.default_rng(seed)
    sim = rng.uniform(lo - 0.05, hi + 0.05, (n, ndim + 1, ndim))
    small = np.arange(n) % 2 == 1
    centre = rng.uniform(np.where(lo < -1, -0.2, -0.12), np.where(lo < -1, 0.2, -0.01), (n, 1, ndim))
    sim[small] = (centre + 0.03 * rng.uniform(-1, 1, sim.shape))[small]
    sim[0, 0, 1] = 0.7
    sim[0, 1] = sim[0, 0]
    sim[0, 1, 1] = -0.7
    return lo, hi, sim


def _ties(s):
    return sum(len(set(row)) < len(row) for row in s.lnp)


@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("ndim", [2, 6, 9])
@pytest.mark.parametrize("target", [1, 2])
def test_test_targets_match_the_restatement_bit_for_bit(target, ndim, adaptive):
    """The unit Gaussian and the terraced Gaussian in a binding box, 1, 3 and 70 simplexes, 60 iterations run as 25 + 35: the
    sorted simplexes, lnprob, status, nit, nfev, stopped and the outcome counters equal the restatement.  On the terraces shrinks
    and ties have to occur (conditions on the inputs, judged on the restatement)."""
    co = nm.coefficients(ndim, adaptive)
    fn = nm.gaussian if target == 1 else nm.terraced
    h = synth_handle()
    try:
        for n in (1, 3, 70):
            lo, hi, sim0 = _test_simplexes(n, ndim, 1000 * target + 10 * ndim + n)
            kw = dict(lower=lo, upper=hi, xatol=1e-3, fatol=1e-3)
            ref = nm.start(sim0, fn, lo, hi, 1e-3, 1e-3)
            ties = _ties(ref)
            assert ties >= 1
            for _ in range(60):
                nm.iterate(ref, fn, *co, **kw)
                ties += _ties(ref)
            r = RawSimplex(h, n, ndim, lo, hi, target, co=co, xatol=1e-3, fatol=1e-3)
            try:
                r.set_vertices(sim0)
                r.run(25)
                r.run(35)
                st = r.state()
            finally:
                r.close()
            _assert_equal(st, ref)
            assert np.all((st["sim"] >= lo) & (st["sim"] <= hi))
            if target == 2 and n == 70:
                assert ref.outcomes[:, nm.SHRINK].sum() > 0, ref.outcomes.sum(axis=0)
            if n == 70:
                assert np.all(ref.outcomes.sum(axis=0)[:4] > 0)          # every non-shrink branch of the tree was taken
    finally:
        h.close()


def _posterior_handle(second=None):
    """Humped (ds 0) and Classic (ds 1), or Humped and `second`, under the synthetic prior."""
    from magprop_amd import synth
    g = np.load(GOLDEN + "/golden_synth.npz")
    h = synth_handle()
    h.set_prior(synth.PRIOR_LOWER, synth.PRIOR_UPPER, synth.LOG_MASK)
    h.set_dataset(0, g["Humped_x"], g["Humped_y"], g["Humped_yerr"])
    h.set_dataset(1, *(second if second is not None else (g["Classic_x"], g["Classic_y"], g["Classic_yerr"])))
    return h


def _posterior_run(h, sim0, ds, iterations, pieces=None):
    """(device state, restatement) of sim0 with simplex k on dataset ds[k]: the restatement evaluates through mp_lnprob_batch on
    batches of exactly n_simplex (N + 4) rows in candidate order, every row with its simplex's dataset."""
    from magprop_amd import synth
    n, nv, N = sim0.shape
    lo, hi = synth.PRIOR_LOWER, synth.PRIOR_UPPER
    ids = np.repeat(np.asarray(ds, dtype=np.int32), N + 4)

    def evaluate(rows):
        assert rows.shape == (n * (N + 4), N)
        return h.lnprob_batch(rows, ds_id=ids, want_status=True)

    ref = nm.run(sim0, iterations, evaluate, lower=lo, upper=hi, xatol=1e-4, fatol=1e-4)
    r = RawSimplex(h, n, N, lo, hi, 0, ds=ds)
    try:
        r.set_vertices(sim0)
        for k in pieces or (iterations,):
            r.run(k)
        st = r.state()
    finally:
        r.close()
    return st, ref


def _start_simplexes(ds, seed, scale=0.05):
    """scipy's default simplex around a point near the truth of every simplex's dataset (TYPES order)."""
    rng = np.random.default_rng(seed)
    return np.stack([nm.default_simplex(np.array(TRUTHS[TYPES[d]]) + scale * rng.standard_normal(6)) for d in ds])


@pytest.mark.parametrize("n_simplex, build", [(20, (4, 1, 1)), (40, (4, 1, 2)), (80, (1, 4, 1)), (128, (1, 2, 2))])
def test_posterior_matches_the_restatement_with_lnprob_batch_on_every_build(n_simplex, build):
    """Humped (even simplexes) and Classic (odd ones) at ndim 6: 200, 400, 800 and 1 280 workgroups per launch reach the team
    builds with one and two wavefronts per SIMD and the one-wavefront builds with 4 and 2 steps per lane.  12 iterations equal
    the restatement whose evaluations are mp_lnprob_batch calls of the launch's size."""
    ds = [k % 2 for k in range(n_simplex)]
    h = _posterior_handle()
    try:
        assert launch_class(10 * n_simplex, h.n_simd) == build
        sim0 = _start_simplexes(ds, 40 + n_simplex)
        st, ref = _posterior_run(h, sim0, ds, 12)
    finally:
        h.close()
    _assert_equal(st, ref)
    assert np.all(ref.nit == 13) and np.all(np.isfinite(ref.lnp[:, 0]))
    assert np.all(ref.outcomes.sum(axis=1) == 12)
    print(f"launch {10 * n_simplex} {build}: outcomes {ref.outcomes.sum(axis=0).tolist()}")


def test_posterior_matches_the_restatement_on_a_long_light_curve(glonglc):
    """The LONG builds: a handle that holds a light curve of 112 points (ds 1), six simplexes over both datasets."""
    long_set = tuple(glonglc["synth112_ds"])
    assert len(long_set[0]) > 64
    ds = [1, 0, 1, 1, 0, 1]
    h = _posterior_handle(long_set)
    try:
        sim0 = np.stack([nm.default_simplex(np.array(TRUTHS["Humped"]) + 0.05 * r) for r in np.random.default_rng(8).standard_normal((6, 6))])
        st, ref = _posterior_run(h, sim0, ds, 12, pieces=(5, 7))
    finally:
        h.close()
    _assert_equal(st, ref)
    assert np.all(ref.nit == 13) and np.all(np.isfinite(ref.lnp[:, 0]))


@pytest.mark.parametrize("case", ["team-1", "team-2", "wave-4", "wave-2"])
def test_posterior_matches_the_restatement_on_the_long_builds_of_every_class(long_mixed_sets, case):
    """nm_eval_kernel's LONG builds on every class: the four launch shapes of the test on every build on a handle that holds
    light curves of 50, 112, 410 and 1 944 points, the simplexes alternating between Humped and the long sets of the case
    (long_cases), 12 iterations as there.  Conditions on the inputs, from the restatement: every simplex on a long set took a
    candidate and turned one down (an iteration of two or more evaluations), and its best vertex is finite.  (With 3 iterations
    on the one-wavefront launches some simplexes only ever reflected, at 1 evaluation each -- of the 40 and the 64
    simplexes on 1 944 points number 3 and number 9 were the first --, which a seed does not cure at that many simplexes; 12
    iterations take 0.01 s.)"""
    h = long_mixed_sets
    c = long_cases(h.n_simd)[case]
    n_simplex, iterations = c["n_simplex"], 12
    assert launch_class(10 * n_simplex, h.n_simd) == c["build"] and 1 <= n_simplex <= 1024
    ds = [c["ds"][k % len(c["ds"])] for k in range(n_simplex)]
    seed = 60 + n_simplex
    sim0 = np.stack([nm.default_simplex(np.array(TRUTHS["Humped"]) + 0.05 * r)
                     for r in np.random.default_rng(seed).standard_normal((n_simplex, 6))])
    st, ref = _posterior_run(h, sim0, ds, iterations)
    _assert_equal(st, ref)
    assert np.all(ref.nit == iterations + 1) and np.all(ref.outcomes.sum(axis=1) == iterations)
    taken = ref.outcomes[:, :nm.SHRINK].sum(axis=1)
    assert_long_reference_is_not_vacuous(ds, taken, ref.nfev - 7, ref.lnp[:, 0])
    if case == "team-1":   # a kernel that read another simplex's light curve would start from these values instead
        swapped = [ds[1], ds[0]] + ds[2:]
        first, other = (_posterior_run(h, sim0, d, 0)[1] for d in (ds, swapped))
        differ = np.any(np.sort(first.lnp, axis=1) != np.sort(other.lnp, axis=1), axis=1)
        assert differ.tolist() == [True, True] + [False] * (n_simplex - 2)
    print(f"long launch {10 * n_simplex} {c['build']}: outcomes {ref.outcomes.sum(axis=0).tolist()}")


def test_break_up_corners_keep_their_status_and_store_no_nan(gcorners):
    """Two simplexes whose vertices are corners of the prior box, flagged ones (the model breaks up: lnprob -inf, status flag)
    among them: after the initial evaluation the flagged vertices sit last with lnprob -inf and their status, and after 1 and
    after 10 iterations, which replace them one by one, the device still follows the restatement, with the statuses
    mp_lnprob_batch gives."""
    pars, status = gcorners["pars"], gcorners["status"]
    flagged, fine = pars[status == 1], pars[status == 0]
    assert len(flagged) >= 4 and len(fine) >= 10
    sim0 = np.stack([np.concatenate([fine[:4], flagged[:3]]), np.concatenate([flagged[3:4], fine[4:10]])])
    h = _posterior_handle()
    try:
        runs = [_posterior_run(h, sim0, [0, 0], k) for k in (0, 1, 10)]
    finally:
        h.close()
    for st, ref in runs:
        _assert_equal(st, ref)
        assert np.all(ref.status[np.isneginf(ref.lnp)] != 0) and np.all(np.isfinite(ref.lnp[:, 0]))
    first = runs[0][1]
    assert np.all(first.nit == 1) and np.all(first.stopped == 0)
    assert np.all(first.status[0, 4:] == 1) and np.all(np.isneginf(first.lnp[0, 4:])) and first.status[1, 6] == 1
    assert np.all(runs[1][1].nit == 2) and np.all(runs[2][1].nit == 11)


def test_final_simplex_lnprob_equals_logprob_in_a_batch_of_the_same_size(gsynth):
    """nelder_mead on the four synthetic sets, two starts each (80 workgroups per launch): the stored lnprob and status of the
    final simplexes are what LogProb's handle returns for those rows in a batch of 80 (the rest filled with vertex 0)."""
    from magprop_amd import LogProb, optimize
    ds = [(gsynth[f"{t}_x"], gsynth[f"{t}_y"], gsynth[f"{t}_yerr"]) for t in TYPES]
    x0 = _start_simplexes(np.repeat(np.arange(4), 2), 3)[:, 0]
    res = optimize.nelder_mead(x0, datasets=ds, n_starts=2, maxiter=25)
    assert len(res) == 8 and all(r.nit == 25 and not r.success and r.status == 2 for r in res)
    lp = LogProb(*ds[0])
    for d in ds[1:]:
        lp.add_dataset(*d)
    P = np.concatenate([np.concatenate([r.final_simplex[0], np.repeat(r.final_simplex[0][:1], 3, axis=0)]) for r in res])
    assert P.shape == (80, 6)
    out, st = lp.handle.lnprob_batch(P, ds_id=np.repeat(np.arange(4, dtype=np.int32), 20), want_status=True)
    keep = np.tile(np.arange(10) < 7, 8)
    assert np.array_equal(out[keep], -np.concatenate([r.final_simplex[1] for r in res]))
    assert np.array_equal(st[keep], np.concatenate([r.simplex_status for r in res]))
    for r in res:
        assert r.fun == -r.lnprob == r.final_simplex[1][0] and np.array_equal(r.x, r.final_simplex[0][0])
        assert sum(r.outcomes.values()) == r.nit - 1 and np.all(np.diff(r.final_simplex[1]) >= 0)


def test_stopped_simplexes_stay_frozen_and_a_split_run_equals_one_run():
    """Simplex 0 starts collapsed (stops at once), 1 and 2 spread over the box: the first never changes while the others go on,
    run(5) then run(7) equals run(12), and both equal the restatement."""
    ndim = 3
    lo, hi = np.full(ndim, -5.0), np.full(ndim, 5.0)
    rng = np.random.default_rng(0)
    sim0 = rng.uniform(-3.0, 3.0, (3, ndim + 1, ndim))
    sim0[0] = 1.0 + 1e-9 * rng.random((ndim + 1, ndim))
    h = synth_handle()
    a = RawSimplex(h, 3, ndim, lo, hi, 2, xatol=1e-6, fatol=1e-6)
    b = RawSimplex(h, 3, ndim, lo, hi, 2, xatol=1e-6, fatol=1e-6)
    try:
        a.set_vertices(sim0)
        first = a.state()
        assert first["stopped"].tolist() == [1, 0, 0] and first["nit"].tolist() == [1, 1, 1] and first["nfev"].tolist() == [4, 4, 4]
        assert a.run(5) == 2
        assert a.run(7) == 2
        split = a.state()
        b.set_vertices(sim0)
        assert b.run(12) == 2
        whole = b.state()
        assert b.run(0) == 2
    finally:
        a.close()
        b.close()
        h.close()
    for key in first:
        assert np.array_equal(first[key][0], split[key][0]), key
        assert np.array_equal(split[key], whole[key]), key
    assert split["nit"].tolist() == [1, 13, 13]
    _assert_equal(whole, nm.run(sim0, 12, nm.terraced, lower=lo, upper=hi, xatol=1e-6, fatol=1e-6))


def test_polish_never_loses(gsynth):
    """differential_evolution stopped early (maxiter = 20) on the four synthetic sets, with and without the polish: the DE part
    is the same run, and scipy's rule keeps the better point, so lnprob with the polish >= lnprob without, exactly.  The polish
    either ends on the stop rule (recomputed here from its final simplex) or at its iteration budget."""
    from magprop_amd import optimize
    ds = [(gsynth[f"{t}_x"], gsynth[f"{t}_y"], gsynth[f"{t}_yerr"]) for t in TYPES]
    plain = optimize.differential_evolution(datasets=ds, seed=3, maxiter=20)
    res = optimize.differential_evolution(datasets=ds, seed=3, maxiter=20, polish=True)
    for t, r0, r in zip(TYPES, plain, res):
        assert "polish" not in r0 and np.array_equal(r0.population, r.population) and r.nit == r0.nit
        assert r.lnprob >= r0.lnprob and r.lnprob == max(r0.lnprob, r.polish.lnprob) and r.fun == -r.lnprob
        assert r.nfev == r0.nfev + r.polish.nfev
        sim, fsim = r.polish.final_simplex
        # the simplex started from the population's 7 best members, so it never ends worse than the best of them
        assert r.polish.lnprob >= r0.lnprob
        stopped = nm.stop_rule(sim, -fsim, 1e-4, 1e-4)
        assert (stopped and r.polish.success) or (r.polish.nit == 200 * 6 and not r.polish.success)
        print(f"{t}: lnprob {r0.lnprob:.6f} -> {r.lnprob:.6f} (gain {r.lnprob - r0.lnprob:.3e}), polish nit {r.polish.nit} nfev "
              f"{r.polish.nfev} {r.polish.outcomes}, |x - truth| {np.abs(r0.x - TRUTHS[t]).max():.3e} -> {np.abs(r.x - TRUTHS[t]).max():.3e}")


def test_multi_device_and_alternative_torque_handles_are_refused():
    from magprop_amd import _capi
    L = _capi.lib()
    lo, hi = np.zeros(6), np.ones(6)
    x = np.logspace(0.5, 3.0, 20)
    hm = synth_handle(device=[0])
    ha = synth_handle(dipole_torque=1)
    h = synth_handle()
    try:
        def create(handle, n=1, ndim=6, co=(1.0, 2.0, 0.5, 0.5), xatol=1e-4, fatol=1e-4, upper=hi, target=0, ds=None):
            return L.mp_simplex_create(handle._h, n, ndim, ds, *co, xatol, fatol, dp(lo), dp(np.ascontiguousarray(upper)), target)

        for bad, what in ((hm, "ONE device"), (ha, "dipole torque")):
            bad.set_dataset(0, x, np.ones_like(x), np.ones_like(x))
            assert not create(bad) and what in _capi.last_error()
        s = create(ha, target=1)                               # the test targets never reach the torque
        assert s and L.mp_simplex_destroy(s) == 0
        # argument codes on a plain handle (no dataset set: target 0 is refused, the test targets are not)
        assert not create(h) and "unset dataset" in _capi.last_error()
        for kw in (dict(n=0), dict(n=1025), dict(ndim=0), dict(ndim=10), dict(ndim=5, target=0), dict(co=(0.0, 2.0, 0.5, 0.5)),
                   dict(co=(1.0, np.inf, 0.5, 0.5)), dict(co=(1.0, 2.0, 1.0, 0.5)), dict(co=(1.0, 2.0, 0.5, 1.5)),
                   dict(xatol=-1.0), dict(fatol=np.nan), dict(upper=np.zeros(6)), dict(target=3)):
            assert not create(h, **dict(dict(target=1), **kw)), kw
        s = create(h, target=2)
        assert s
        assert L.mp_simplex_run(s, 1, None) == _capi.MP_ESTATE            # before mp_simplex_set_vertices
        assert L.mp_simplex_get_state(s, None, None, None, None, None, None, None) == _capi.MP_ESTATE
        v = np.zeros((7, 6))
        v[3, 2] = np.nan
        assert L.mp_simplex_set_vertices(s, dp(v)) == _capi.MP_EINVAL
        assert L.mp_simplex_run(s, -1, None) == _capi.MP_EINVAL
        assert L.mp_simplex_destroy(s) == 0
    finally:
        hm.close()
        ha.close()
        h.close()
