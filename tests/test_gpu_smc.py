"""GPU tests of the tempered SMC sampler (include/magprop_amd.h mp_smc_*, magprop_amd.smc): the device state against the numpy
restatement (tests/smc_restated.py) stage by stage and bit for bit -- on the unit Gaussian, and on the real posterior on every
build of the move kernel with every likelihood of the restatement an mp_lnprob_batch call of the launch's own size --, split
runs, independence of the runs, failed models, the evidence against a closed form and against brute force, and the summaries.
The restatement takes the device's exp and log (libmp_probe_smc.so mpz_exp, libmp_probe_libm.so mpl_libm), which numpy's miss
by an ulp now and then."""
import ctypes as C
import math

import numpy as np
import pytest

import smc_restated as sm
from conftest import TRUTHS, TYPES
from raw_abi import dp, ip, synth_handle
from test_gpu_nested import (BatchEvaluator, assert_long_reference_is_not_vacuous, launch_class, long_cases,  # noqa: F401
                             long_mixed_sets, long_sets, posterior_live, synth_sets)  # (three are fixtures)
from test_gpu_smc_kernels import device_exp, device_log

pytestmark = pytest.mark.gpu

EVIDENCE_INFLATION = 10.0                 # tests/test_gpu_tempering.py: Humped with yerr x 10 ...
BRUTE_FORCE, BRUTE_ESS = -5.5046, 160641  # ... its brute-force ln Z and the effective sample size behind it
FLAGGED = [1.8171068, 3.68147895, -2.61786801, 1.99840102, -0.33083576, 2.95613803]   # a point where the model fails (flag)
DEVICE = dict(exp=device_exp, log=device_log, log_u=device_log)


class RawSMC:
    """mp_smc_* through ctypes on handle h."""

    def __init__(self, h, n, n_runs, ndim, lower, upper, seed, walks, target, ds=None, ess=0.5, g0=0.0, sigma=0.1):
        from magprop_amd import _capi
        self.L, self.n, self.n_runs, self.ndim, self.walks = _capi.lib(), n, n_runs, ndim, walks
        self.lo, self.hi = np.ascontiguousarray(lower, dtype=np.float64), np.ascontiguousarray(upper, dtype=np.float64)
        ids = None if ds is None else np.ascontiguousarray(ds, dtype=np.int32)
        self.s = self.L.mp_smc_create(h._h, n, n_runs, ndim, ip(ids), C.c_uint64(seed), dp(self.lo), dp(self.hi), ess, walks, g0,
                                      sigma, target)
        assert self.s, _capi.last_error()

    def set_particles(self, x):
        from magprop_amd import _capi
        p = np.ascontiguousarray(x, dtype=np.float64)
        assert self.L.mp_smc_set_particles(self.s, dp(p)) == 0, _capi.last_error()

    def run(self, n):
        running = C.c_int32(-1)
        assert self.L.mp_smc_run(self.s, n, C.byref(running)) == 0
        return running.value

    def state(self):
        from magprop_amd import smc
        st = smc.get_state(self.L, self.s, self.n_runs, self.n, self.ndim)
        st["anc"] = smc.get_ancestors(self.L, self.s, self.n_runs, self.n)
        st["stages"] = [smc.get_stages(self.L, self.s, r) for r in range(self.n_runs)]
        return st

    def close(self):
        self.L.mp_smc_destroy(self.s)


def _assert_equal(st, s, walks):
    for k, v in (("x", s.x), ("lnl", s.lnl), ("status", s.status), ("acc", s.acc), ("beta", s.beta), ("lnz", s.lnz),
                 ("nstage", s.nstage), ("run_status", s.run_status), ("ncall", s.ncall), ("nacc", s.nacc), ("nfail", s.nfail)):
        assert np.array_equal(st[k], v), (k, st[k], v)
    for r in range(s.lnl.shape[0]):
        if s.nstage[r]:
            assert np.array_equal(st["anc"][r], s.anc[r]), r
        beta, d, ess, lnz, accept, ncall = sm.stages_of(s, r, s.lnl.shape[1], walks)
        got = st["stages"][r]
        for k, v in (("beta", beta), ("d", d), ("ess", ess), ("lnz", lnz), ("accept", accept), ("ncall", ncall)):
            assert np.array_equal(got[k], v), (r, k, got[k], v)


@pytest.mark.parametrize("n, ndim", [(64, 2), (64, 6), (256, 2), (256, 6)])
def test_gaussian_stages_match_the_restatement_bit_for_bit(n, ndim):
    """Two runs on the unit Gaussian in an asymmetric box, 3 steps per move: behind every mp_smc_run(s, 1) the particles, lnl,
    status, accepted counts, ancestors, beta, ln Z, the log and the counters equal the restatement advanced by one stage."""
    n_runs, walks, seed = 2, 3, 20261020 + n + ndim
    lo, hi = np.full(ndim, -4.0), np.linspace(3.0, 5.0, ndim)
    x0 = lo + (hi - lo) * np.random.default_rng(n + ndim).random((n_runs, n, ndim))
    s = sm.start(x0, sm.gaussian)
    h = synth_handle()
    dev = RawSMC(h, n, n_runs, ndim, lo, hi, seed, walks, 1)
    try:
        dev.set_particles(x0.reshape(-1, ndim))
        _assert_equal(dev.state(), s, walks)
        for k in range(60):
            running = dev.run(1)
            sm.run(s, 1, seed, walks, 0.5, 0.0, 0.1, lo, hi, sm.gaussian, **DEVICE)
            _assert_equal(dev.state(), s, walks)
            assert running == int(np.sum(s.run_status == sm.RUNNING))
            if running == 0:
                break
    finally:
        dev.close()
        h.close()
    assert np.all(s.run_status == sm.DONE) and np.all(s.beta == 1.0) and np.all(s.nstage >= 2)
    assert 0 < s.nacc.sum() < s.ncall.sum() - n_runs * n < n_runs * n * walks * s.nstage.max()   # accepted, rejected, outside the box
    print(f"N {n}, ndim {ndim}: stages {s.nstage.tolist()}, ln Z {s.lnz.tolist()} (closed form "
          f"{sum(math.log(math.sqrt(math.pi / 2) * (math.erf(b / math.sqrt(2)) + math.erf(4 / math.sqrt(2))) / (b + 4)) for b in hi):.3f})")


def smc_cases(ns):
    """The smallest shapes whose move launch (n_runs * N workgroups) runs each build."""
    return {"team-1": dict(run_ds=[2, 0, 1], n=64, build=(4, 1, 1)),
            "team-2": dict(run_ds=[3, 1], n=3 * ns // 16, build=(4, 1, 2)),
            "wave-4": dict(run_ds=[1, 2], n=3 * ns // 8, build=(1, 4, 1)),
            "wave-2": dict(run_ds=[0, 3], n=5 * ns // 8, build=(1, 2, 2))}


def drive_posterior(h, run_ds, truths, n, stages, walks, seed, build):
    """RawSMC(target=0, ds=run_ds) on h and the restatement in step: equal after the first evaluation and behind every one of
    `stages` single stages; every evaluation of the restatement is one mp_lnprob_batch call of n_runs * n rows."""
    from magprop_amd import synth
    lo, hi = synth.PRIOR_LOWER, synth.PRIOR_UPPER
    n_runs = len(run_ds)
    assert launch_class(n_runs * n, h.n_simd) == build, (n_runs * n, h.n_simd)
    x0 = posterior_live(truths, n, seed)
    ev = BatchEvaluator(h, run_ds)
    s = sm.start(x0, ev.at(n_runs * n))
    status0 = s.status.copy()
    dev = RawSMC(h, n, n_runs, 6, lo, hi, seed, walks, 0, ds=run_ds)
    try:
        dev.set_particles(x0.reshape(-1, 6))
        _assert_equal(dev.state(), s, walks)
        for _ in range(stages):
            assert dev.run(1) == n_runs
            sm.run(s, 1, seed, walks, 0.5, 0.0, 0.1, lo, hi, ev.at(n_runs * n), **DEVICE)
            _assert_equal(dev.state(), s, walks)
    finally:
        dev.close()
    # not vacuous: particles started flagged and were counted; steps were accepted, rejected and fell outside the box
    assert np.any(status0 != 0) and np.all(s.nfail >= np.sum(status0 != 0, axis=1))
    assert np.all(s.nacc > 0) and np.all(s.nacc < s.ncall - n) and np.all(s.ncall - n <= stages * n * walks)
    assert np.all(s.nstage == stages) and np.all(s.beta < 1.0)
    print(f"move launch {n_runs * n} {build}: {ev.calls} batches, flagged at the start {int(np.sum(status0 != 0))}, beta "
          f"{s.beta.tolist()}, ncall {s.ncall.tolist()}, nacc {s.nacc.tolist()}, nfail {s.nfail.tolist()}")
    return s


@pytest.mark.parametrize("case", ["team-1", "team-2", "wave-4", "wave-2"])
def test_posterior_stages_match_lnprob_batch_on_every_build(synth_sets, case):
    """The real posterior, runs on different datasets, at the smallest shape of each of the four builds, two stages of 3 steps."""
    h = synth_sets
    c = smc_cases(h.n_simd)[case]
    drive_posterior(h, c["run_ds"], [TRUTHS[TYPES[d]] for d in c["run_ds"]], c["n"], 2, 3, 20261020, c["build"])


def test_posterior_stages_match_lnprob_batch_on_the_long_builds(long_sets):
    """The LONG builds: a handle that also holds a light curve of 112 points, one run on Humped and one on the long set."""
    drive_posterior(long_sets, [0, 1], [TRUTHS["Humped"], TRUTHS["Humped"]], 64, 2, 3, 20261221, (4, 1, 1))


@pytest.mark.parametrize("case", ["team-2", "wave-4", "wave-2"])
def test_posterior_stages_match_lnprob_batch_on_the_long_builds_of_every_class(long_mixed_sets, case):
    """smc_move_kernel's LONG builds beyond (4, 1, 1): one run on Humped next to one on a light curve of 410 or 1 944 points
    (long_cases), stages of 3 steps."""
    h = long_mixed_sets
    c = long_cases(h.n_simd)[case]
    ds, n, seed = c["ds"], c["n"], 20261303
    truths = [TRUTHS["Humped"]] * len(ds)
    s = drive_posterior(h, ds, truths, n, c["iters"], 3, seed, c["build"])
    assert_long_reference_is_not_vacuous(ds, s.nacc, s.ncall - n, s.lnl.max(axis=1))
    if case == "team-2":   # a kernel that read the other run's light curve would start from these values instead
        x0 = posterior_live(truths, n, seed)
        lnl0 = sm.start(x0, BatchEvaluator(h, ds).at(len(ds) * n)).lnl
        lnl1 = sm.start(x0, BatchEvaluator(h, ds[::-1]).at(len(ds) * n)).lnl
        assert not np.array_equal(lnl1[0], lnl0[0]) and not np.array_equal(lnl1[1], lnl0[1])


def _gaussian_runs(n, n_runs, ndim, seed, x0, calls, lo=None, hi=None, walks=4):
    """The unit Gaussian through the C ABI: mp_smc_run once per entry of calls; the state behind every call."""
    lo = np.full(ndim, -6.0) if lo is None else lo
    hi = np.full(ndim, 6.0) if hi is None else hi
    h = synth_handle()
    dev = RawSMC(h, n, n_runs, ndim, lo, hi, seed, walks, 1)
    out = []
    try:
        dev.set_particles(x0.reshape(-1, ndim))
        for c in calls:
            dev.run(c)
            out.append(dev.state())
    finally:
        dev.close()
        h.close()
    return out


def _same(a, b, runs_a=slice(None), runs_b=slice(None)):
    for k in ("x", "lnl", "status", "acc", "anc", "beta", "lnz", "nstage", "run_status", "ncall", "nacc", "nfail"):
        assert np.array_equal(a[k][runs_a], b[k][runs_b]), k
    for sa, sb in zip(a["stages"][runs_a], b["stages"][runs_b]):
        for k in sa:
            assert np.array_equal(sa[k], sb[k]), k


def test_split_runs_equal_one_run():
    """mp_smc_run(s, 1) until every run is done equals one mp_smc_run(s, 1000), whose chunks are the library's own; so does a
    run cut in the middle of a chunk."""
    n, n_runs, ndim, seed = 128, 3, 3, 77
    x0 = -6.0 + 12.0 * np.random.default_rng(2).random((n_runs, n, ndim))
    whole = _gaussian_runs(n, n_runs, ndim, seed, x0, [1000])[0]
    total = int(whole["nstage"].max())
    assert np.all(whole["run_status"] == sm.DONE) and total > 3
    _same(_gaussian_runs(n, n_runs, ndim, seed, x0, [1] * total)[-1], whole)
    _same(_gaussian_runs(n, n_runs, ndim, seed, x0, [3, 0, total])[-1], whole)


def test_runs_do_not_interact_and_a_stopped_run_stays():
    """Run 0 alone equals run 0 among three; a run that is done does not change while the others go on."""
    n, ndim, seed = 64, 2, 5
    rng = np.random.default_rng(3)
    lo, hi = np.full(ndim, -8.0), np.full(ndim, 8.0)
    x0 = lo + (hi - lo) * rng.random((3, n, ndim))
    x0[1] = 0.02 * rng.standard_normal((n, ndim))            # flat lnl over these: done at its first stage
    states = _gaussian_runs(n, 3, ndim, seed, x0, [1, 1, 1000], lo, hi)
    first, last = states[0], states[-1]
    assert first["run_status"].tolist() == [sm.RUNNING, sm.DONE, sm.RUNNING] and np.all(last["run_status"] == sm.DONE)
    assert last["nstage"][1] == 1 and last["nstage"][0] > 2
    _same(first, last, slice(1, 2), slice(1, 2))
    _same(states[1], last, slice(1, 2), slice(1, 2))
    alone = _gaussian_runs(n, 1, ndim, seed, x0[:1], [1000], lo, hi)[0]
    _same(alone, last, slice(0, 1), slice(0, 1))


def test_failed_models_die_at_the_first_stage_and_are_counted(synth_sets):
    """Particles set where the model fails (status flag, lnl = -inf) are counted, are nobody's ancestor at the first stage and are
    gone behind it; a run of nothing else ends with status FAILED and keeps its particles."""
    from magprop_amd import _capi, synth
    h = synth_sets
    lo, hi = synth.PRIOR_LOWER, synth.PRIOR_UPPER
    n, bad = 32, [0, 5, 31]
    rng = np.random.default_rng(6)
    x0 = np.clip(np.array(TRUTHS["Humped"]) + 0.05 * rng.standard_normal((2, n, 6)), lo, hi)
    x0[0, bad] = FLAGGED
    x0[1, :] = FLAGGED
    dev = RawSMC(h, n, 2, 6, lo, hi, 9, 2, 0, ds=[0, 0])
    try:
        dev.set_particles(x0.reshape(-1, 6))
        st0 = dev.state()
        assert dev.run(1) == 1
        st = dev.state()
        dev.run(5)
        st5 = dev.state()
    finally:
        dev.close()
    assert np.all(st0["status"][0, bad] != _capi.STATUS_OK) and np.all(st0["lnl"][0, bad] == -np.inf)
    assert np.all(st0["status"][1] != _capi.STATUS_OK) and st0["nfail"].tolist() == [len(bad), n] and st0["ncall"].tolist() == [n, n]
    assert st["run_status"].tolist() == [sm.RUNNING, sm.FAILED] and st["nstage"].tolist() == [1, 0]
    assert not np.any(np.isin(st["anc"][0], bad)) and np.all(np.isfinite(st["lnl"][0]))
    assert st["nfail"][0] >= len(bad) and st["nfail"][1] == n and st["ncall"][1] == n
    assert np.array_equal(st["x"][1], x0[1]) and np.array_equal(st5["x"][1], x0[1])
    assert st5["nstage"][1] == 0 and 2 <= st5["nstage"][0] <= 6 and st5["run_status"][1] == sm.FAILED
    assert len(st5["stages"][1]["beta"]) == 0 and len(st5["stages"][0]["beta"]) == st5["nstage"][0]


def test_gaussian_evidence_and_posterior_on_the_device():
    """The CPU test's case (tests/test_smc_cpu.py: 8 runs, N = 1 024, d = 6, [-10, 10]^6, 10 steps, the same seed and particles)
    through SMCSampler: the mean ln Z within 4 standard errors of the closed form, every pooled variance within 5 % of 1."""
    from magprop_amd import SMCSampler
    from test_smc_cpu import HALF, NDIM, NPART, NRUNS, SEED, WALKS, passes
    s = SMCSampler(target="gaussian", bounds=[(-HALF, HALF)] * NDIM, nparticles=NPART, walks=WALKS, n_runs=NRUNS, seed=SEED)
    res = s.run()
    s.close()
    lnz = np.array([r.logz for r in res])
    se = np.std(lnz, ddof=1) / math.sqrt(NRUNS)
    z = (lnz.mean() - sm.box_lnz(HALF, NDIM)) / se
    var = np.var(np.concatenate([r.samples for r in res]), axis=0)
    print(f"device: z = {z:.2f} standard errors (se {se:.4f}), variances {np.round(var, 3).tolist()}, stages "
          f"{[r.nstages for r in res]}, accept {np.round(res[0].accept, 3).tolist()}")
    assert all(r.status == "done" and r.betas[-1] == 1.0 for r in res)
    assert all(r.logzerr == se for r in res) and all(r.ncall == NPART + r.ncall_stage.sum() for r in res)
    assert passes(z, var)


def test_humped_evidence_against_brute_force(gsynth):
    """Humped with yerr x 10, the brute-force case of tests/test_gpu_tempering.py (-5.5046 from an effective sample size of
    160 641): 8 runs of N = 1 024, 10 steps; the mean ln Z within 4 sigma, sigma^2 = (sd / sqrt 8)^2 + 1 / 160 641.  The log-bias
    sd^2 / 2 of a single run is printed."""
    from magprop_amd import SMCSampler
    x, y, yerr = gsynth["Humped_x"], gsynth["Humped_y"], gsynth["Humped_yerr"] * EVIDENCE_INFLATION
    s = SMCSampler(x, y, yerr, nparticles=1024, walks=10, n_runs=8, seed=20261020)
    res = s.run()
    s.close()
    lnz = np.array([r.logz for r in res])
    sd = np.std(lnz, ddof=1)
    sigma = math.sqrt(sd ** 2 / 8.0 + 1.0 / BRUTE_ESS)
    print(f"Humped yerr x 10: brute force {BRUTE_FORCE}, SMC mean {lnz.mean():.4f}, sd over runs {sd:.4f} (log-bias sd^2 / 2 = "
          f"{sd ** 2 / 2:.4f}), sigma {sigma:.4f}, difference {lnz.mean() - BRUTE_FORCE:+.4f} = "
          f"{(lnz.mean() - BRUTE_FORCE) / sigma:+.2f} sigma; stages {[r.nstages for r in res]}, ncall {[r.ncall for r in res]}, "
          f"nfail {[r.nfail for r in res]}, accept of the last stage {[round(float(r.accept[-1]), 3) for r in res]}")
    assert all(r.status == "done" for r in res)
    assert abs(lnz.mean() - BRUTE_FORCE) < 4.0 * sigma


def test_summaries_go_through_the_one_path(gsynth):
    """get_derived and get_model_band of a finished run equal the summaries path called on its samples, without weights."""
    from magprop_amd import SMCSampler, summaries
    x, y, yerr = gsynth["Humped_x"], gsynth["Humped_y"], gsynth["Humped_yerr"]
    s = SMCSampler(x, y, yerr, nparticles=64, walks=5, seed=4)
    res = s.run()
    try:
        assert res.status == "done" and res.samples.shape == (64, 6) and math.isnan(res.logzerr)
        assert np.array_equal(res.logl, s.handle.lnprob_batch(res.samples))          # the samples' lnl is the library's own
        got, want = s.get_derived(), summaries.derived(summaries.on(s.handle), res.samples, (0.16, 0.5, 0.84))
        assert np.array_equal(got["values"], want["values"], equal_nan=True) and got["n_used"] == want["n_used"]
        for k in want["summary"]:
            assert np.array_equal(np.asarray(got["summary"][k]), np.asarray(want["summary"][k]), equal_nan=True), k
        got = s.get_model_band(components=("Ltot", "Ldip"))
        want = summaries.band(summaries.on(s.handle), res.samples, (0.025, 0.5, 0.975), ("Ltot", "Ldip"))
        assert got["n_used"] == want["n_used"] > 0
        for k in ("t", "Ltot", "Ldip"):
            assert np.array_equal(got[k], want[k], equal_nan=True), k
        assert s.get_pointwise()["n_used"] == got["n_used"]
    finally:
        s.close()
