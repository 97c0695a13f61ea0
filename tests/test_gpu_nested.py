"""GPU tests of the nested sampler (include/magprop_amd.h mp_nested_*, magprop_amd.nested): the device state against the numpy
restatement (tests/nest_restated.py) bit for bit, chunk independence, evidence against closed forms and brute force, posterior
samples against a long ensemble chain, a long Swift light curve, and refused handles.  On the real posterior the restatement's
evaluations are mp_lnprob_batch calls of the launch's own size, on every kernel build."""
import ctypes as C
import math

import numpy as np
import pytest
from scipy.special import erf

import nest_restated as nr
import nest_slice_restated as sr
from conftest import TRUTHS, TYPES
from raw_abi import dp, ip, synth_handle

pytestmark = pytest.mark.gpu

EVIDENCE_INFLATION = 10.0       # tests/test_gpu_tempering.py: Humped with yerr x 10


class RawNested:
    """mp_nested_* through ctypes on handle h."""

    def __init__(self, h, nlive, nbatch, n_runs, ndim, lower, upper, seed, walks, target, ds=None, g0=0.0, sigma=0.1, dlogz=0.01):
        from magprop_amd import _capi
        self.L, self.nlive, self.n_runs, self.ndim = _capi.lib(), nlive, n_runs, ndim
        self.lo, self.hi = np.ascontiguousarray(lower, dtype=np.float64), np.ascontiguousarray(upper, dtype=np.float64)
        ids = None if ds is None else np.ascontiguousarray(ds, dtype=np.int32)
        self.ns = self.L.mp_nested_create(h._h, nlive, nbatch, n_runs, ndim, ip(ids), C.c_uint64(seed), walks, g0, sigma, dlogz,
                                          dp(self.lo), dp(self.hi), target)
        assert self.ns, _capi.last_error()

    def set_live(self, live):
        p = np.ascontiguousarray(live, dtype=np.float64)
        assert self.L.mp_nested_set_live(self.ns, dp(p)) == 0

    def run(self, n):
        running = C.c_int32(-1)
        assert self.L.mp_nested_run(self.ns, n, C.byref(running)) == 0
        return running.value

    def state(self):
        from magprop_amd import nested
        st = nested.get_state(self.L, self.ns, self.n_runs, self.nlive, self.ndim)
        st["dead"] = [nested.get_dead(self.L, self.ns, r, self.ndim) for r in range(self.n_runs)]
        return st

    def close(self):
        self.L.mp_nested_destroy(self.ns)


def _assert_equal(st, s):
    assert np.array_equal(st["live"], s.live)
    assert np.array_equal(st["lnl"], s.lnl)
    assert np.array_equal(st["status"], s.status)
    assert np.array_equal(st["acc"], s.acc)
    assert np.array_equal(st["nit"], s.nit)
    assert np.array_equal(st["stopped"], s.stopped)
    assert np.array_equal(st["ncall"], s.ncall)
    assert np.array_equal(st["nacc"], s.nacc)
    assert np.array_equal(st["nzero"], s.nzero)
    for r, (pars, lnl, n) in enumerate(st["dead"]):
        assert np.array_equal(pars, np.array(s.dead_pars[r]).reshape(-1, s.live.shape[2]))
        assert np.array_equal(lnl, np.array(s.dead_lnl[r]))
        assert np.array_equal(n, np.array(s.dead_n[r], dtype=np.int32))
    assert np.allclose(st["lnx"], s.lnx, rtol=1e-14, atol=0.0)
    assert np.allclose(st["lnz"], s.lnz, rtol=1e-14, atol=0.0)


def _gaussian_lnz(lo, hi):
    """ln Z of exp(-0.5 |x|^2) under the uniform prior on the box: a product of erf differences over the box volume."""
    return sum(math.log(math.sqrt(math.pi / 2.0) * (erf(h / math.sqrt(2.0)) - erf(l / math.sqrt(2.0))) / (h - l))
               for l, h in zip(lo, hi))


@pytest.mark.parametrize("n_runs", [1, 3])
def test_gaussian_state_matches_the_restatement_bit_for_bit(n_runs):
    """Unit Gaussian in an asymmetric 3-d box, N = 32, K = 8, 10 steps per walk, dlogz = 0.05: 6 iterations, then on to the stop
    rule; live set, lnL, status, accepted counts, the dead sequence, the stop iteration and the counters equal the restatement,
    ln X and ln Z to 1e-14 relative."""
    ndim, nlive, nbatch, walks, seed = 3, 32, 8, 10, 20261015 + n_runs
    lo, hi = np.array([-2.0, -1.0, -4.0]), np.array([3.0, 2.5, 1.5])
    live0 = lo + (hi - lo) * np.random.default_rng(7 + n_runs).random((n_runs, nlive, ndim))
    kw = dict(walks=walks, g0=0.0, sigma=0.1, dlogz=0.05, lower=lo, upper=hi, evaluate_one=nr.gaussian_one)
    s = nr.start(live0, nr.gaussian)
    h = synth_handle()
    ns = RawNested(h, nlive, nbatch, n_runs, ndim, lo, hi, seed, walks, 1, dlogz=0.05)
    try:
        ns.set_live(live0.reshape(-1, ndim))
        ns.run(6)
        nr.run(s, 6, nbatch, seed, **kw)
        _assert_equal(ns.state(), s)
        assert ns.run(1000) == 0
        nr.run(s, 1000, nbatch, seed, **kw)
        st = ns.state()
    finally:
        ns.close()
        h.close()
    _assert_equal(st, s)
    assert np.all(st["stopped"] == 1) and np.all(st["nit"] > 6)
    print(f"stop iterations {st['nit'].tolist()}, ln Z {st['lnz'].tolist()}")


# ---------------------------------------------------------------- the real posterior against mp_lnprob_batch, build by build
def launch_class(n, ns):
    """(wavefronts per walker, steps per lane, wavefronts per SIMD) of a walker launch of n workgroups on a device of ns SIMDs
    (mp_device.h kernel_waves / walker_variant): a team of four up to ns / 2 (a SIMD per wavefront up to ns / 4), one wavefront
    with four steps per lane up to ns, two beyond."""
    return (4, 1, 1) if 4 * n <= ns else ((4, 1, 2) if 2 * n <= ns else ((1, 4, 1) if n <= ns else (1, 2, 2)))


def posterior_cases(ns):
    """The smallest shapes whose walk launch (n_runs * nbatch workgroups) runs each build; nlive = 2 nbatch, so that the live-set
    launch lies a class further on.  run_ds: the dataset of every run (TYPES); chunks: the iterations of every mp_nested_run."""
    return {"team-1": dict(run_ds=[2, 0, 1], nbatch=8, chunks=(1, 3), walks=10, build=(4, 1, 1)),
            "team-2": dict(run_ds=[3, 1], nbatch=3 * ns // 16, chunks=(2,), walks=3, build=(4, 1, 2)),
            "wave-4": dict(run_ds=[1, 2], nbatch=3 * ns // 8, chunks=(2,), walks=3, build=(1, 4, 1)),
            "wave-2": dict(run_ds=[0, 3], nbatch=5 * ns // 8, chunks=(2,), walks=3, build=(1, 2, 2))}


def posterior_live(truths, nlive, seed):
    """Live points (n_runs, nlive, 6) in the synthetic prior box: the first half uniform in the box (flagged, out-of-range and
    -inf points among them), the other half truths[r] + 0.05 randn, clipped into the box."""
    from magprop_amd import synth
    lo, hi = synth.PRIOR_LOWER, synth.PRIOR_UPPER
    rng = np.random.default_rng(seed)
    live = lo + (hi - lo) * rng.random((len(truths), nlive, 6))
    for r, t in enumerate(truths):
        live[r, nlive // 2:] = np.clip(np.array(t) + 0.05 * rng.standard_normal((nlive - nlive // 2, 6)), lo, hi)
    return live


class BatchEvaluator:
    """The restatement's evaluate(rows, runs) as ONE mp_lnprob_batch call of exactly n rows, the size of the device launch (and
    so its kernel build): the pending rows, padded with copies of the first (on that row's dataset); row i runs on the dataset
    of its run."""

    def __init__(self, h, run_ds):
        self.h, self.run_ds, self.calls = h, np.asarray(run_ds, dtype=np.int32), 0

    def at(self, n):
        def evaluate(rows, runs):
            k = len(rows)
            assert 1 <= k <= n and len(runs) == k
            padded = np.concatenate([rows, np.repeat(rows[:1], n - k, axis=0)])
            ids = self.run_ds[np.concatenate([runs, np.full(n - k, runs[0])]).astype(int)]
            assert padded.shape == (n, 6) and ids.shape == (n,)
            out, st = self.h.lnprob_batch(padded, ds_id=ids, want_status=True)
            self.calls += 1
            return out[:k], st[:k]
        return evaluate


def assert_reference_is_not_vacuous(s, status0, walks):
    """Conditions on the inputs, read off the restatement alone: a live point started flagged; a proposal fell outside the box
    (a step without an evaluation); evaluated steps were accepted and rejected; every run moved."""
    steps = walks * int(np.sum(s.nit)) * (s.lnl.shape[1] // 2)
    assert np.any(status0 != 0)
    assert s.ncall.sum() < steps
    assert np.all(s.nacc > 0) and s.nacc.sum() < s.ncall.sum()


@pytest.fixture(scope="module")
def synth_sets(gsynth):
    """One handle with the synthetic prior and the four synthetic datasets (ds k = TYPES[k])."""
    from magprop_amd import synth
    h = synth_handle()
    h.set_prior(synth.PRIOR_LOWER, synth.PRIOR_UPPER, synth.LOG_MASK)
    for k, t in enumerate(TYPES):
        h.set_dataset(k, gsynth[t + "_x"], gsynth[t + "_y"], gsynth[t + "_yerr"])
    yield h
    h.close()


@pytest.fixture(scope="module")
def long_sets(gsynth, glonglc):
    """One handle with Humped (ds 0) and a Humped-type light curve of 112 points (ds 1: every launch runs the LONG builds)."""
    from magprop_amd import synth
    h = synth_handle()
    h.set_prior(synth.PRIOR_LOWER, synth.PRIOR_UPPER, synth.LOG_MASK)
    h.set_dataset(0, gsynth["Humped_x"], gsynth["Humped_y"], gsynth["Humped_yerr"])
    x, y, yerr = glonglc["synth112_ds"]
    assert len(x) > 64
    h.set_dataset(1, x, y, yerr)
    yield h
    h.close()


LONG_MIXED_LENGTHS = (50, 112, 410, 1944)      # ds k of long_mixed_sets


@pytest.fixture(scope="module")
def long_mixed_sets(gsynth, glonglc):
    """One handle with Humped (ds 0, 50 points) and the Humped-type light curves of 112, 410 and 1 944 points (ds 1, 2, 3):
    every launch runs the LONG builds, a short light curve next to ones of one and of many chunks behind the 64 captured
    observations."""
    from magprop_amd import synth
    h = synth_handle()
    h.set_prior(synth.PRIOR_LOWER, synth.PRIOR_UPPER, synth.LOG_MASK)
    sets = [(gsynth["Humped_x"], gsynth["Humped_y"], gsynth["Humped_yerr"])]
    sets += [tuple(glonglc[f"synth{n}_ds"]) for n in LONG_MIXED_LENGTHS[1:]]
    assert tuple(len(s[0]) for s in sets) == LONG_MIXED_LENGTHS
    for k, s in enumerate(sets):
        h.set_dataset(k, *s)
    yield h
    h.close()


def long_cases(ns):
    """The LONG cases of every resident driver on long_mixed_sets, one per build, at the smallest shapes that reach it (the
    formulas of posterior_cases here, of smc_cases, of the optimizer's and the simplex search's tables and of family_cases):
    ds: the datasets of the runs, ensembles or populations, the 50-point set first, so that every case scores a short light
    curve on a LONG build and the lengths are not in descending order as numbered (the sampler's ens_order is then not the
    identity); over the four cases every long set appears.  nbatch: workgroups per run of a nested walk launch and slots per
    ensemble of a slice-move launch; n: particles per SMC run; pop: members of a launch of the optimizer, over all populations;
    n_simplex: simplexes (10 workgroups each at ndim 6), cycling through ds; whole / half: walkers per ensemble of a sampler by
    whole steps and by half-step launches (half has no two-per-SIMD team).  iters: iterations, stages, generations or steps."""
    return {"team-1": dict(ds=[0, 3, 1], build=(4, 1, 1), nbatch=8, n=ns // 16, pop=60, n_simplex=ns // 50, whole=16, half=16,
                           iters=4),
            "team-2": dict(ds=[0, 2], build=(4, 1, 2), nbatch=3 * ns // 16, n=3 * ns // 16, pop=3 * ns // 8, n_simplex=ns // 25,
                           whole=3 * ns // 32, half=None, iters=3),
            "wave-4": dict(ds=[0, 3], build=(1, 4, 1), nbatch=3 * ns // 8, n=3 * ns // 8, pop=3 * ns // 4,
                           n_simplex=5 * ns // 64, whole=ns // 4, half=ns // 4, iters=2),
            "wave-2": dict(ds=[0, 3], build=(1, 2, 2), nbatch=5 * ns // 8, n=5 * ns // 8, pop=5 * ns // 4, n_simplex=ns // 8,
                           whole=3 * ns // 8, half=5 * ns // 4, iters=1)}


def assert_long_reference_is_not_vacuous(ds, accepted, evaluated, best):
    """Conditions on the inputs of a long_cases run, read off the restatement alone: every run (ensemble, population) on a
    light curve of more than 64 points accepted and rejected at least one evaluated point, and its best lnprob is finite."""
    accepted, evaluated, best = np.asarray(accepted), np.asarray(evaluated), np.asarray(best)
    long_runs = [r for r, d in enumerate(ds) if LONG_MIXED_LENGTHS[d] > 64]
    assert long_runs and len(long_runs) < len(ds)
    for r in long_runs:
        assert 0 < accepted[r] < evaluated[r], (r, accepted[r], evaluated[r])
        assert np.isfinite(best[r]), (r, best[r])


def drive_posterior(h, run_ds, truths, nbatch, chunks, walks, seed, build=None):
    """RawNested(target=0, ds=run_ds) on h and the restatement in step, nlive = 2 nbatch: equal after the live-set evaluation
    and behind every mp_nested_run of `chunks` -- n iterations each, or (n, (slices, mu, max_steps_out, max_shrink)) after an
    mp_nested_set_slice of those (slices = 0: back to the random walk); the slice counters are compared throughout.  Returns the
    restatement's state, its first (live, lnL, status), and the evaluator."""
    from magprop_amd import nested, synth
    lo, hi = synth.PRIOR_LOWER, synth.PRIOR_UPPER
    n_runs, nlive, ns_ = len(run_ds), 2 * nbatch, h.n_simd
    if build is not None:
        assert launch_class(n_runs * nbatch, ns_) == build, (n_runs * nbatch, ns_)
    assert len(set(run_ds)) == n_runs
    live0 = posterior_live(truths, nlive, seed)
    ev = BatchEvaluator(h, run_ds)
    kw = dict(dlogz=1e-9, lower=lo, upper=hi, evaluate=ev.at(n_runs * nbatch))
    s = sr.start(live0, ev.at(n_runs * nlive), with_runs=True)
    first = live0, s.lnl.copy(), s.status.copy()
    ns = RawNested(h, nlive, nbatch, n_runs, 6, lo, hi, seed, walks, 0, ds=run_ds, dlogz=1e-9)

    def check():
        st = ns.state()
        st.update(nested.get_slice_stats(ns.L, ns.ns, n_runs))
        _assert_equal(st, s)
        for k in ("nexpand", "ncontract", "nfail"):
            assert np.array_equal(st[k], getattr(s, k)), k

    try:
        ns.set_live(live0.reshape(-1, 6))
        check()
        sl = (0, 1.0, 1, 1)
        for c in chunks:
            n, new = c if isinstance(c, tuple) else (c, None)
            if new is not None:
                sl = new
                assert ns.L.mp_nested_set_slice(ns.ns, *sl) == 0
            assert ns.run(n) == n_runs
            if sl[0]:
                sr.run(s, n, nbatch, seed, sl[0], mu=sl[1], max_steps_out=sl[2], max_shrink=sl[3], **kw)
            else:
                nr.run(s, n, nbatch, seed, walks=walks, g0=0.0, sigma=0.1, **kw)
            check()
    finally:
        ns.close()
    total = sum(c[0] if isinstance(c, tuple) else c for c in chunks)
    assert np.all(s.nit == total) and not np.any(s.stopped)
    print(f"walk launch {n_runs * nbatch} {launch_class(n_runs * nbatch, ns_)}, live-set launch {n_runs * nlive} "
          f"{launch_class(n_runs * nlive, ns_)}: {ev.calls} batches, flagged at the start {int(np.sum(first[2] != 0))}, ncall "
          f"{s.ncall.tolist()}, nacc {s.nacc.tolist()}, nzero {s.nzero.tolist()}, nexpand {s.nexpand.tolist()}, ncontract "
          f"{s.ncontract.tolist()}, nfail {s.nfail.tolist()}")
    return s, first, ev


@pytest.mark.parametrize("case", ["team-1", "team-2", "wave-4", "wave-2"])
def test_posterior_walks_match_lnprob_batch_on_every_build(synth_sets, case):
    """The random walk on the real posterior, runs on different datasets, at the smallest shape of each of the four builds:
    the device state equals the restatement bit for bit where every likelihood of the restatement -- the live set and every
    round of the walks -- is an mp_lnprob_batch call of the launch's size on the row's dataset (ln X, ln Z to 1e-14)."""
    h = synth_sets
    c = posterior_cases(h.n_simd)[case]
    truths = [TRUTHS[TYPES[d]] for d in c["run_ds"]]
    s, (live0, lnl0, status0), ev = drive_posterior(h, c["run_ds"], truths, c["nbatch"], c["chunks"], c["walks"], 20261019,
                                                    c["build"])
    assert_reference_is_not_vacuous(s, status0, c["walks"])
    if case == "team-1":   # the runs' datasets matter: the reference with two of them swapped starts from another live lnL
        swap = BatchEvaluator(h, [c["run_ds"][1], c["run_ds"][0]] + c["run_ds"][2:]).at(lnl0.size)
        lnl1 = nr.start(live0, swap, with_runs=True).lnl
        assert not np.array_equal(lnl1[0], lnl0[0]) and not np.array_equal(lnl1[1], lnl0[1]) and np.array_equal(lnl1[2], lnl0[2])


def test_posterior_walks_match_lnprob_batch_on_the_long_builds(long_sets):
    """The LONG builds: a handle that also holds a light curve of 112 points, one run on Humped and one on the long set."""
    truths = [TRUTHS["Humped"], TRUTHS["Humped"]]
    s, (_, _, status0), ev = drive_posterior(long_sets, [0, 1], truths, 8, (1, 3), 10, 20261220, (4, 1, 1))
    assert_reference_is_not_vacuous(s, status0, 10)


@pytest.mark.parametrize("case", ["team-2", "wave-4", "wave-2"])
def test_posterior_walks_match_lnprob_batch_on_the_long_builds_of_every_class(long_mixed_sets, case):
    """nest_walk_kernel's LONG builds beyond (4, 1, 1): one run on Humped next to one on a light curve of 410 or 1 944 points
    (long_cases).  At wave-2 the live-set evaluation of the restatement is a batch of more than 2 n_simd rows on light curves
    of different lengths, which mp_lnprob_batch evaluates longest first (launch_lnprob_ordered) without changing a row's
    bits (test_gpu_batched.py::test_longest_light_curves_first_launch_order)."""
    h = long_mixed_sets
    c = long_cases(h.n_simd)[case]
    truths = [TRUTHS["Humped"]] * len(c["ds"])
    s, (live0, lnl0, status0), ev = drive_posterior(h, c["ds"], truths, c["nbatch"], (c["iters"],), 3, 20261301, c["build"])
    assert_reference_is_not_vacuous(s, status0, 3)
    assert_long_reference_is_not_vacuous(c["ds"], s.nacc, s.ncall, s.lnl.max(axis=1))
    assert (lnl0.size > 2 * h.n_simd) == (case == "wave-2")
    if case == "team-2":   # a kernel that read the other run's light curve would start from these values instead
        swap = BatchEvaluator(h, c["ds"][::-1]).at(lnl0.size)
        lnl1 = nr.start(live0, swap, with_runs=True).lnl
        assert not np.array_equal(lnl1[0], lnl0[0]) and not np.array_equal(lnl1[1], lnl0[1])


def test_chunks_of_one_iteration_equal_one_unsplit_run():
    """Two runs of N = 64 (K = 8, 25 steps) on the unit Gaussian: mp_nested_run(1) called until both stopped equals one
    mp_nested_run(10 000), whose chunks are the library's own."""
    ndim, nlive, nbatch = 4, 64, 8
    lo, hi = np.full(ndim, -3.0), np.array([2.0, 3.0, 4.0, 5.0])
    live0 = lo + (hi - lo) * np.random.default_rng(3).random((2 * nlive, ndim))
    h = synth_handle()
    states = []
    try:
        for split in (True, False):
            ns = RawNested(h, nlive, nbatch, 2, ndim, lo, hi, 11, 25, 1)
            try:
                ns.set_live(live0)
                if split:
                    for _ in range(10000):
                        if ns.run(1) == 0:
                            break
                else:
                    assert ns.run(10000) == 0
                states.append(ns.state())
            finally:
                ns.close()
    finally:
        h.close()
    a, b = states
    for k in ("live", "lnl", "status", "acc", "nit", "stopped", "lnx", "lnz", "ncall", "nacc", "nzero"):
        assert np.array_equal(a[k], b[k]), k
    for (pa, la, na), (pb, lb, nb) in zip(a["dead"], b["dead"]):
        assert np.array_equal(pa, pb) and np.array_equal(la, lb) and np.array_equal(na, nb)
    assert np.all(a["nit"] > 33)                # (more than one of the library's chunks of 32)


def test_gaussian_evidence_in_an_asymmetric_6d_box():
    """Four runs in one launch, N = 512, K = 128: ln Z of each within 3 logzerr of the closed form."""
    from magprop_amd import NestedSampler
    lo = np.array([-2.0, -1.0, -4.0, -0.5, -3.0, -1.5])
    hi = np.array([3.0, 2.5, 1.5, 4.0, 0.5, 1.0])
    truth = _gaussian_lnz(lo, hi)
    s = NestedSampler(nlive=512, nbatch=128, target="gaussian", bounds=np.stack([lo, hi], axis=1), n_runs=4, seed=5)
    res = s.run_nested()
    s.close()
    for r in res:
        print(f"6-d Gaussian: ln Z {r.logz:.4f} +- {r.logzerr:.4f} (truth {truth:.4f}), {r.niter} iterations, ncall {r.ncall}, "
              f"eff {r.eff:.2f} %, walks without a step {r.nzero}")
        assert r.stopped and abs(r.logz - truth) < 3.0 * r.logzerr, (r.logz, r.logzerr, truth)
        assert abs(r.device_logz - r.logz) < 0.05


def test_humped_evidence_against_brute_force(gsynth):
    """Humped with yerr x 10 (the brute-force case of tests/test_gpu_tempering.py, -5.5046 measured there): the brute-force
    evidence over 4 x 2^20 uniform box draws against a nested run of N = 1024, K = 256; within max(3 logzerr, 0.05)."""
    from magprop_amd import LogProb, NestedSampler, synth
    x, y, yerr = gsynth["Humped_x"], gsynth["Humped_y"], gsynth["Humped_yerr"] * EVIDENCE_INFLATION
    lo, hi = synth.PRIOR_LOWER, synth.PRIOR_UPPER
    lp = LogProb(x, y, yerr)
    rng = np.random.default_rng(2026)
    n_bf, chunk = 4 << 20, 1 << 18
    vals = np.concatenate([lp(lo + (hi - lo) * rng.random((chunk, 6))) for _ in range(n_bf // chunk)])
    w = np.exp(vals - vals.max())
    lnz_bf = vals.max() + np.log(w.sum()) - np.log(n_bf)
    s = NestedSampler(x, y, yerr, nlive=1024, nbatch=256, seed=9)
    r = s.run_nested()
    s.close()
    print(f"Humped yerr x 10: brute force {lnz_bf:.4f}, nested {r.logz:.4f} +- {r.logzerr:.4f} (H {r.information:.2f}, "
          f"ln f_valid {r.ln_f_valid:.4f}), {r.niter} iterations, ncall {r.ncall}, walks without a step {r.nzero}")
    assert r.stopped
    assert abs(r.logz - lnz_bf) < max(3.0 * r.logzerr, 0.05), (r.logz, r.logzerr, lnz_bf)


def test_humped_posterior_samples(gsynth):
    """Humped as it is, N = 1024, K = 256: every truth inside the central 95 % of the equal-weight samples; posterior means and
    standard deviations against a stretch chain of 512 walkers x 3 000 steps from the truths (first 1 000 discarded): means within
    0.3 chain sigma, standard deviations within a factor 1.35.  A band of the equal-weight samples brackets its median.
    Calibrated once on an MI355X: mean shifts 0.005 .. 0.025 sigma, standard-deviation ratios 0.98 .. 1.21 (log10 M_disc: 1.21);
    ln Z = -46.20 +- 0.12 in 77 iterations."""
    from magprop_amd import EnsembleSampler, NestedSampler
    x, y, yerr = gsynth["Humped_x"], gsynth["Humped_y"], gsynth["Humped_yerr"]
    s = NestedSampler(x, y, yerr, nlive=1024, nbatch=256, seed=4)
    r = s.run_nested()
    eq = s.resample_equal()
    band = s.get_model_band(q=(0.025, 0.5, 0.975))
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
    print(f"Humped: ln Z {r.logz:.3f} +- {r.logzerr:.3f}, {r.niter} iterations, ncall {r.ncall}, {eq.shape[0]} samples; mean "
          f"shift / sigma {np.round(dmean, 3)}, sd ratio {np.round(sratio, 3)}, walks without a step {r.nzero}")
    assert np.all((truth >= q025) & (truth <= q975)), (q025, q975)
    assert np.all(dmean < 0.3), dmean
    assert np.all((sratio > 1 / 1.35) & (sratio < 1.35)), sratio
    lo_, mid, hi_ = band["Ltot"]
    ok = np.isfinite(mid)
    assert band["n_used"] > 0 and np.all(lo_[ok] <= mid[ok]) and np.all(mid[ok] <= hi_[ok])


def test_long_swift_light_curve_lib_reaches_the_best_fit(gswift):
    """LONG builds, lib variant: GRB 051016B (79 points, GRBtype "S") runs to the stop rule; its best dead lnL lies within 1 of
    the DE optimizer's best fit."""
    from magprop_amd import NestedSampler, optimize
    x, y, yerr = gswift["swift_051016B_libS_ds"]
    best = optimize.differential_evolution(x, y, yerr, variant="lib", GRBtype="S", seed=2, maxiter=1000)
    s = NestedSampler(x, y, yerr, nlive=256, nbatch=64, variant="lib", GRBtype="S", seed=6)
    r = s.run_nested()
    s.close()
    print(f"GRB 051016B: ln Z {r.logz:.3f} +- {r.logzerr:.3f}, best dead lnL {np.max(r.logl):.3f} (DE {best.lnprob:.3f}), "
          f"{r.niter} iterations, ncall {r.ncall}")
    assert r.stopped
    assert np.max(r.logl) >= best.lnprob - 1.0, (np.max(r.logl), best.lnprob)


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
            ns = L.mp_nested_create(h._h, 64, 16, 1, 6, None, C.c_uint64(0), 25, 0.0, 0.1, 0.01, dp(lo), dp(hi), 0)
            assert not ns and what in _capi.last_error()
        # argument codes on a plain handle
        h = synth_handle()
        for bad in (dict(nlive=8), dict(nbatch=33), dict(nbatch=0), dict(walks=0), dict(sigma=0.6), dict(dlogz=0.0),
                    dict(upper=np.zeros(6)), dict(n_runs=65)):
            kw = dict(nlive=64, nbatch=16, walks=25, sigma=0.1, dlogz=0.01, upper=hi, n_runs=1)
            kw.update(bad)
            ns = L.mp_nested_create(h._h, kw["nlive"], kw["nbatch"], kw["n_runs"], 6, None, C.c_uint64(0), kw["walks"], 0.0,
                                    kw["sigma"], kw["dlogz"], dp(lo), dp(np.ascontiguousarray(kw["upper"])), 1)
            assert not ns, bad
        ns = L.mp_nested_create(h._h, 64, 16, 1, 6, None, C.c_uint64(0), 25, 0.0, 0.1, 0.01, dp(lo), dp(hi), 1)
        assert ns
        assert L.mp_nested_run(ns, 1, None) == _capi.MP_ESTATE                   # before set_live
        out = np.full((64, 6), 2.0)
        assert L.mp_nested_set_live(ns, dp(out)) == _capi.MP_EINVAL   # outside the box
        L.mp_nested_destroy(ns)
        h.close()
    finally:
        hm.close()
        ha.close()
