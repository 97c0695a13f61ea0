"""GPU tests of the nested sampler's slice mode (include/magprop_amd.h mp_nested_set_slice, NestedSampler(sample="slice")): the
device state against the numpy restatement (tests/nest_slice_restated.py) bit for bit, also under tight limits (zero budgets, the
shrink cap) and with coinciding survivors, chunk independence, slices = 0 as the
random walk, evidence against closed forms and brute force, posterior samples on Humped as it is (the case the random walk
mixes poorly), a long Swift light curve through the LONG builds, and refused arguments."""
import ctypes as C
import math
import warnings

import numpy as np
import pytest

import nest_restated as nr
import nest_slice_restated as sr
import test_nested_slice_cpu as edge
from conftest import TRUTHS, TYPES
from raw_abi import lp, synth_handle
from test_gpu_nested import (EVIDENCE_INFLATION, BatchEvaluator, RawNested, _assert_equal, _gaussian_lnz,  # noqa: F401
                             assert_long_reference_is_not_vacuous, drive_posterior, long_cases, long_mixed_sets, long_sets,
                             posterior_cases, synth_sets)

pytestmark = pytest.mark.gpu


def _set_slice(ns, slices, mu=1.0, steps_out=8, shrink=64):
    return ns.L.mp_nested_set_slice(ns.ns, slices, mu, steps_out, shrink)


def _state(ns):
    from magprop_amd import nested
    st = ns.state()
    st.update(nested.get_slice_stats(ns.L, ns.ns, ns.n_runs))
    return st


def _assert_slice_equal(st, s):
    _assert_equal(st, s)
    for k in ("nexpand", "ncontract", "nfail"):
        assert np.array_equal(st[k], getattr(s, k)), k


@pytest.mark.parametrize("n_runs", [1, 3])
def test_slice_state_matches_the_restatement_bit_for_bit(n_runs):
    """Unit Gaussian in an asymmetric 3-d box, N = 32, K = 8, 3 slices per walk (m = 4, 32 shrink points at most), dlogz = 0.05:
    6 iterations, then on to the stop rule; live set, lnL, status, moved-slice counts, the dead sequence, the stop iteration
    and every counter equal the restatement, ln X and ln Z to 1e-14 relative."""
    ndim, nlive, nbatch, slices, seed = 3, 32, 8, 3, 20261016 + n_runs
    lo, hi = np.array([-2.0, -1.0, -4.0]), np.array([3.0, 2.5, 1.5])
    live0 = lo + (hi - lo) * np.random.default_rng(17 + n_runs).random((n_runs, nlive, ndim))
    kw = dict(mu=1.0, max_steps_out=4, max_shrink=32, dlogz=0.05, lower=lo, upper=hi, evaluate_one=nr.gaussian_one)
    s = sr.start(live0, nr.gaussian)
    h = synth_handle()
    ns = RawNested(h, nlive, nbatch, n_runs, ndim, lo, hi, seed, 25, 1, dlogz=0.05)
    try:
        assert _set_slice(ns, slices, 1.0, 4, 32) == 0
        ns.set_live(live0.reshape(-1, ndim))
        ns.run(6)
        sr.run(s, 6, nbatch, seed, slices, **kw)
        _assert_slice_equal(_state(ns), s)
        assert ns.run(1000) == 0
        sr.run(s, 1000, nbatch, seed, slices, **kw)
        st = _state(ns)
    finally:
        ns.close()
        h.close()
    _assert_slice_equal(st, s)
    assert np.all(st["stopped"] == 1) and np.all(st["nit"] > 6) and np.all(st["nexpand"] > 0) and np.all(st["ncontract"] > 0)
    print(f"stop iterations {st['nit'].tolist()}, ln Z {st['lnz'].tolist()}, nfail {st['nfail'].tolist()}")


def _device_edge_run(live0, nlive, iterations, slices, mu, steps_out, shrink, dlogz):
    """One run on the unit Gaussian in the box of the edge cases of tests/test_nested_slice_cpu.py: the device state behind
    `iterations` iterations of slice mode."""
    h = synth_handle()
    ns = RawNested(h, nlive, 8, 1, 3, edge.EDGE_LO, edge.EDGE_HI, edge.EDGE_SEED, 25, 1, dlogz=dlogz)
    try:
        assert _set_slice(ns, slices, mu, steps_out, shrink) == 0
        ns.set_live(live0.reshape(-1, 3))
        ns.run(iterations)
        return _state(ns)
    finally:
        ns.close()
        h.close()


@pytest.mark.parametrize("limits", sorted(edge.TIGHT))
def test_tight_limits_match_the_restatement_bit_for_bit(limits):
    """N = 32, K = 8, 3 slices, 6 iterations under max_steps_out = 1 (both budgets 0) and a shrink cap of 2 (mu = 0.05) or 1
    (mu = 5): slices that fail at the cap and shrink points outside the box, the paths the CPU twin
    (test_nested_slice_cpu.py::test_tight_limits_take_the_slices_to_zero_budgets_and_the_shrink_cap) asserts on the restated run."""
    live0, s = edge.tight_run(limits)
    st = _device_edge_run(live0, 32, 6, 3, limits[2], limits[0], limits[1], 0.05)
    _assert_slice_equal(st, s)
    assert (int(st["nexpand"][0]), int(st["ncontract"][0]), int(st["nfail"][0])) == edge.TIGHT[limits]


def test_coinciding_survivors_match_the_restatement_bit_for_bit():
    """N = 16 (MP_NEST_MIN_LIVE), K = 8, 3 slices, limits 4 / 8, 2 iterations, the eight highest-lnL points of the start set at
    one position: every direction is zero, no point is evaluated and all 48 slices fail where they start."""
    live0, s = edge.coinciding_run()
    st = _device_edge_run(live0, 16, 2, 3, 1.0, 4, 8, 1e-9)
    _assert_slice_equal(st, s)
    assert st["nfail"][0] == 48 and st["ncall"][0] == 0 and st["nzero"][0] == 16 and st["stopped"][0] == 0


def test_slice_chunks_of_one_iteration_equal_one_unsplit_run():
    """Two runs of N = 64 (K = 8, 4 slices) on the unit Gaussian: mp_nested_run(1) called until both stopped equals one
    mp_nested_run(10 000)."""
    ndim, nlive, nbatch = 4, 64, 8
    lo, hi = np.full(ndim, -3.0), np.array([2.0, 3.0, 4.0, 5.0])
    live0 = lo + (hi - lo) * np.random.default_rng(3).random((2 * nlive, ndim))
    h = synth_handle()
    states = []
    try:
        for split in (True, False):
            ns = RawNested(h, nlive, nbatch, 2, ndim, lo, hi, 11, 25, 1)
            try:
                assert _set_slice(ns, 4) == 0
                ns.set_live(live0)
                if split:
                    for _ in range(10000):
                        if ns.run(1) == 0:
                            break
                else:
                    assert ns.run(10000) == 0
                states.append(_state(ns))
            finally:
                ns.close()
    finally:
        h.close()
    a, b = states
    for k in ("live", "lnl", "status", "acc", "nit", "stopped", "lnx", "lnz", "ncall", "nacc", "nzero", "nexpand", "ncontract",
              "nfail"):
        assert np.array_equal(a[k], b[k]), k
    for (pa, la, na), (pb, lb, nb) in zip(a["dead"], b["dead"]):
        assert np.array_equal(pa, pb) and np.array_equal(la, lb) and np.array_equal(na, nb)
    assert np.all(a["nit"] > 33)                # (more than one of the library's chunks of 32)


def test_zero_slices_is_the_random_walk():
    """A sampler switched to slice mode and back (slices = 0) before its run equals one never switched, bit for bit, and its
    slice counters stay 0."""
    ndim, nlive, nbatch = 3, 64, 16
    lo, hi = np.array([-2.0, -1.0, -4.0]), np.array([3.0, 2.5, 1.5])
    live0 = lo + (hi - lo) * np.random.default_rng(8).random((2 * nlive, ndim))
    h = synth_handle()
    states = []
    try:
        for switch in (True, False):
            ns = RawNested(h, nlive, nbatch, 2, ndim, lo, hi, 5, 10, 1)
            try:
                if switch:
                    assert _set_slice(ns, 3) == 0 and _set_slice(ns, 0) == 0
                ns.set_live(live0)
                assert ns.run(10000) == 0
                states.append(_state(ns))
            finally:
                ns.close()
    finally:
        h.close()
    a, b = states
    for k in ("live", "lnl", "status", "acc", "nit", "stopped", "lnx", "lnz", "ncall", "nacc", "nzero"):
        assert np.array_equal(a[k], b[k]), k
    for k in ("nexpand", "ncontract", "nfail"):
        assert np.all(a[k] == 0) and np.all(b[k] == 0), k


def _assert_slices_are_not_vacuous(s, status0):
    """Conditions on the inputs, read off the restatement alone: a live point started flagged, a slice stepped out, a shrink
    point was rejected, and every run moved a slice."""
    assert np.any(status0 != 0)
    assert s.nexpand.sum() > 0 and s.ncontract.sum() > 0 and np.all(s.nacc > 0)


@pytest.mark.parametrize("case", ["team-1", "team-2", "wave-4", "wave-2"])
def test_posterior_slices_match_lnprob_batch_on_every_build(synth_sets, case):
    """Slice mode on the real posterior at the shapes of test_gpu_nested.py's random-walk cases (runs on different datasets, the
    smallest shape of each build): the device state and the slice counters equal the restatement bit for bit where every
    likelihood of the restatement is an mp_lnprob_batch call of the launch's size on the row's dataset.  Small budgets bound
    the rounds: 2 slices, 4 steps out, 16 shrink points over 1 + 3 iterations on the first case; 1 slice and 1 iteration on the
    larger ones."""
    h = synth_sets
    c = posterior_cases(h.n_simd)[case]
    truths = [TRUTHS[TYPES[d]] for d in c["run_ds"]]
    chunks = ((1, (2, 1.0, 4, 16)), 3) if case == "team-1" else ((1, (1, 1.0, 4, 16)),)
    s, (_, _, status0), ev = drive_posterior(h, c["run_ds"], truths, c["nbatch"], chunks, c["walks"], 20261061, c["build"])
    _assert_slices_are_not_vacuous(s, status0)


def test_posterior_slices_match_lnprob_batch_on_the_long_builds(long_sets):
    """The LONG builds in slice mode: one run on Humped and one on a light curve of 112 points."""
    truths = [TRUTHS["Humped"], TRUTHS["Humped"]]
    s, (_, _, status0), ev = drive_posterior(long_sets, [0, 1], truths, 8, ((1, (2, 1.0, 4, 16)), 3), 10, 20261192, (4, 1, 1))
    _assert_slices_are_not_vacuous(s, status0)


@pytest.mark.parametrize("case", ["team-2", "wave-4", "wave-2"])
def test_posterior_slices_match_lnprob_batch_on_the_long_builds_of_every_class(long_mixed_sets, case):
    """nest_slice_kernel's LONG builds beyond (4, 1, 1): one run on Humped next to one on a light curve of 410 or 1 944
    points (long_cases), 1 slice per walk with 4 steps out and 16 shrink points (2 slices on the team)."""
    h = long_mixed_sets
    c = long_cases(h.n_simd)[case]
    truths = [TRUTHS["Humped"]] * len(c["ds"])
    chunks = ((c["iters"], (2 if case == "team-2" else 1, 1.0, 4, 16)),)
    s, (live0, lnl0, status0), ev = drive_posterior(h, c["ds"], truths, c["nbatch"], chunks, 3, 20261302, c["build"])
    _assert_slices_are_not_vacuous(s, status0)
    # a slice that moved accepted its last point; a shrink point that was rejected was evaluated
    assert_long_reference_is_not_vacuous(c["ds"], s.nacc, s.nacc + s.ncontract, s.lnl.max(axis=1))
    assert np.all(s.ncall >= s.nacc + s.ncontract)
    if case == "team-2":   # a kernel that read the other run's light curve would start from these values instead
        swap = BatchEvaluator(h, c["ds"][::-1]).at(lnl0.size)
        lnl1 = nr.start(live0, swap, with_runs=True).lnl
        assert not np.array_equal(lnl1[0], lnl0[0]) and not np.array_equal(lnl1[1], lnl0[1])


def test_switching_walks_between_iterations_on_the_posterior(synth_sets):
    """A random-walk iteration, two slice iterations after mp_nested_set_slice, and a random-walk iteration again after
    mp_nested_set_slice(0, ...), on the real posterior with three runs on different datasets: equal to the restatement behind
    every call, the slice counters standing still while the random walk runs."""
    c = posterior_cases(synth_sets.n_simd)["team-1"]
    truths = [TRUTHS[TYPES[d]] for d in c["run_ds"]]
    chunks = (1, (2, (2, 1.0, 4, 16)), (1, (0, 1.0, 4, 16)))
    s, (_, _, status0), ev = drive_posterior(synth_sets, c["run_ds"], truths, c["nbatch"], chunks, c["walks"], 20261073, c["build"])
    _assert_slices_are_not_vacuous(s, status0)
    assert np.all(s.ncall > s.nacc)


def test_slice_gaussian_evidence_and_scatter_in_an_asymmetric_6d_box():
    """6 slices per walk, N = 512, K = 128.  Four runs in one launch: ln Z of each within 3 logzerr of the closed form.  Eight
    runs of another seed in one launch: std / mean logzerr of ln Z in [0.3, 2.0].  Calibrated once on an MI355X: the four runs
    lie within 2.1 logzerr; std / mean logzerr 1.77 over the 8 runs of seed 6 (one of them 4.0 logzerr high), 1.75 over 16 runs
    of seeds 200 and 201 (1.42 with 12 slices, 1.11 for the random walk; profiles/r11_nest_slice_sweep.json).  With ndim slices
    per walk the scatter on this case exceeds logzerr by about 1.7x; the bound holds that figure, it does
    not claim that logzerr covers it."""
    from magprop_amd import NestedSampler
    lo = np.array([-2.0, -1.0, -4.0, -0.5, -3.0, -1.5])
    hi = np.array([3.0, 2.5, 1.5, 4.0, 0.5, 1.0])
    truth = _gaussian_lnz(lo, hi)
    out = []
    for n_runs, seed in ((4, 5), (8, 6)):
        s = NestedSampler(nlive=512, nbatch=128, target="gaussian", bounds=np.stack([lo, hi], axis=1), n_runs=n_runs, seed=seed,
                          sample="slice")
        res = s.run_nested()
        s.close()
        lnz = np.array([r.logz for r in res])
        err = np.array([r.logzerr for r in res])
        print(f"6-d Gaussian, slice, seed {seed}: ln Z {np.round(lnz, 4).tolist()} (truth {truth:.4f}), (ln Z - truth) / logzerr "
              f"{np.round((lnz - truth) / err, 2).tolist()}, std / mean logzerr {lnz.std(ddof=1) / err.mean():.3f}, iterations "
              f"{[r.niter for r in res]}, ncall {[r.ncall for r in res]}, nfail {[r.nfail for r in res]}")
        for r in res:
            assert r.stopped and abs(r.device_logz - r.logz) < 0.05
            assert r.nacc + r.nfail == 6 * 128 * r.niter
        out.append((res, lnz, err))
    res, lnz, err = out[0]
    for r in res:
        assert abs(r.logz - truth) < 3.0 * r.logzerr, (r.logz, r.logzerr, truth)
    res, lnz, err = out[1]
    assert 0.3 < lnz.std(ddof=1) / err.mean() < 2.0


def test_slice_humped_evidence_against_brute_force(gsynth):
    """Humped with yerr x 10: the brute-force evidence over 4 x 2^20 uniform box draws against a slice-mode run of N = 1024,
    K = 256; within max(3 logzerr, 0.05)."""
    from magprop_amd import LogProb, NestedSampler, synth
    x, y, yerr = gsynth["Humped_x"], gsynth["Humped_y"], gsynth["Humped_yerr"] * EVIDENCE_INFLATION
    lo, hi = synth.PRIOR_LOWER, synth.PRIOR_UPPER
    lp = LogProb(x, y, yerr)
    rng = np.random.default_rng(2026)
    n_bf, chunk = 4 << 20, 1 << 18
    vals = np.concatenate([lp(lo + (hi - lo) * rng.random((chunk, 6))) for _ in range(n_bf // chunk)])
    w = np.exp(vals - vals.max())
    lnz_bf = vals.max() + np.log(w.sum()) - np.log(n_bf)
    s = NestedSampler(x, y, yerr, nlive=1024, nbatch=256, seed=9, sample="slice")
    r = s.run_nested()
    s.close()
    print(f"Humped yerr x 10, slice: brute force {lnz_bf:.4f}, nested {r.logz:.4f} +- {r.logzerr:.4f}, {r.niter} iterations, "
          f"ncall {r.ncall}, walks without a move {r.nzero}, failed slices {r.nfail}")
    assert r.stopped
    assert abs(r.logz - lnz_bf) < max(3.0 * r.logzerr, 0.05), (r.logz, r.logzerr, lnz_bf)


def test_slice_humped_posterior_samples_without_a_warning(gsynth):
    """Humped as it is, N = 1024, K = 256, slice mode: the gates of test_gpu_nested.py::test_humped_posterior_samples (truths
    inside the central 95 %, means within 0.3 chain sigma of a stretch chain, standard deviations within a factor 1.35), no
    RuntimeWarning, at most 1 % failed slices and at most 0.1 % walks in which no slice moved (the random walk: 9 %)."""
    from magprop_amd import EnsembleSampler, NestedSampler
    x, y, yerr = gsynth["Humped_x"], gsynth["Humped_y"], gsynth["Humped_yerr"]
    s = NestedSampler(x, y, yerr, nlive=1024, nbatch=256, seed=4, sample="slice")
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        r = s.run_nested()
    eq = s.resample_equal()
    s.close()
    truth = np.array(TRUTHS["Humped"])
    q025, q975 = np.quantile(eq, [0.025, 0.975], axis=0)
    rng = np.random.default_rng(30)
    e = EnsembleSampler(512, 6, x, y, yerr, seed=31)
    e.run_mcmc(truth + 1.0e-4 * rng.standard_normal((512, 6)), 3000)
    ref = e.get_chain()[1000:].reshape(-1, 6)
    e.close()
    dmean = np.abs(eq.mean(axis=0) - ref.mean(axis=0)) / ref.std(axis=0)
    sratio = eq.std(axis=0) / ref.std(axis=0)
    walks = r.niter * 256
    print(f"Humped, slice: ln Z {r.logz:.3f} +- {r.logzerr:.3f}, {r.niter} iterations, ncall {r.ncall}; mean shift / sigma "
          f"{np.round(dmean, 3)}, sd ratio {np.round(sratio, 3)}; walks without a move {r.nzero} of {walks}, failed slices "
          f"{r.nfail} of {6 * walks}, nexpand {r.nexpand}, ncontract {r.ncontract}")
    assert np.all((truth >= q025) & (truth <= q975)), (q025, q975)
    assert np.all(dmean < 0.3), dmean
    assert np.all((sratio > 1 / 1.35) & (sratio < 1.35)), sratio
    assert r.nfail <= 0.01 * 6 * walks
    assert r.nzero <= 0.001 * walks


def test_slice_long_swift_light_curve_lib_reaches_the_best_fit(gswift):
    """LONG builds, lib variant, slice mode: GRB 051016B (GRBtype "S") runs to the stop rule; its best dead lnL lies within 1
    of the DE optimizer's best fit."""
    from magprop_amd import NestedSampler, optimize
    x, y, yerr = gswift["swift_051016B_libS_ds"]
    best = optimize.differential_evolution(x, y, yerr, variant="lib", GRBtype="S", seed=2, maxiter=1000)
    s = NestedSampler(x, y, yerr, nlive=256, nbatch=64, variant="lib", GRBtype="S", seed=6, sample="slice")
    r = s.run_nested()
    s.close()
    print(f"GRB 051016B, slice: ln Z {r.logz:.3f} +- {r.logzerr:.3f}, best dead lnL {np.max(r.logl):.3f} (DE "
          f"{best.lnprob:.3f}), {r.niter} iterations, ncall {r.ncall}, failed slices {r.nfail}")
    assert r.stopped
    assert np.max(r.logl) >= best.lnprob - 1.0, (np.max(r.logl), best.lnprob)


def test_set_slice_refuses_bad_arguments():
    from magprop_amd import _capi
    lo, hi = np.zeros(3), np.ones(3)
    h = synth_handle()
    ns = RawNested(h, 32, 8, 1, 3, lo, hi, 0, 25, 1)
    try:
        for bad in ((-1, 1.0, 8, 64), (_capi.NEST_MAX_SLICES + 1, 1.0, 8, 64), (3, 0.0, 8, 64), (3, -1.0, 8, 64),
                    (3, math.inf, 8, 64), (3, math.nan, 8, 64), (3, 1.0, 0, 64), (3, 1.0, _capi.NEST_MAX_STEPS_OUT + 1, 64),
                    (3, 1.0, 8, 0), (3, 1.0, 8, _capi.NEST_MAX_SHRINK + 1)):
            assert _set_slice(ns, *bad) == _capi.MP_EINVAL, bad
        assert ns.L.mp_nested_set_slice(None, 3, 1.0, 8, 64) == _capi.MP_EINVAL
        out = np.zeros(1, dtype=np.int64)
        assert ns.L.mp_nested_get_slice_stats(ns.ns, lp(out), None, None) == _capi.MP_ESTATE
        assert _set_slice(ns, _capi.NEST_MAX_SLICES, 0.5, _capi.NEST_MAX_STEPS_OUT, _capi.NEST_MAX_SHRINK) == 0
        assert _set_slice(ns, 0) == 0
        ns.set_live(lo + (hi - lo) * np.random.default_rng(0).random((32, 3)))
        assert ns.L.mp_nested_get_slice_stats(ns.ns, None, None, None) == 0
    finally:
        ns.close()
        h.close()
