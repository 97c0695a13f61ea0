"""GPU tests of the adaptive moves of the tempered SMC sampler (include/magprop_amd.h mp_smc_set_adaptive, mp_smc_get_tuning):
the tune kernel on crafted inputs through the probe library (mpz_tune), the device against the restatement
(tests/smc_adapt_restated.py) stage by stage and bit for bit on the unit Gaussian and on the real posterior, the round loop
against the fixed-length path on every build of the move kernel, run control, and the evidence of Humped against the nested
sampler.  The restatement takes the device's exp and log, as tests/test_gpu_smc.py does."""
import ctypes as C
import math

import numpy as np
import pytest

import smc_adapt_cases as cases
import smc_adapt_restated as ad
import smc_restated as sm
from conftest import TRUTHS, TYPES
from raw_abi import dp, ip, synth_handle
from test_gpu_nested import BatchEvaluator, launch_class, long_sets, posterior_live, synth_sets  # noqa: F401  (two are fixtures)
from test_gpu_smc import DEVICE, RawSMC, _same, smc_cases
from test_gpu_smc_kernels import device_exp, probe

pytestmark = pytest.mark.gpu

CANARY = -7


class RawAdaptive(RawSMC):
    """RawSMC with mp_smc_set_adaptive and the tuning log in its state."""

    def set_adaptive(self, min_rounds, max_rounds, corr, gain, accept_target=0.234, g_min=0.0, g_max=0.0):
        return self.L.mp_smc_set_adaptive(self.s, min_rounds, max_rounds, corr, gain, accept_target, g_min, g_max)

    def state(self):
        from magprop_amd import smc
        st = super().state()
        st["tuning"] = [smc.get_tuning(self.L, self.s, r) for r in range(self.n_runs)]
        return st


def _assert_equal(st, s, walks):
    """The device state st against the adaptive restatement s: state, log (accept over the steps made) and tuning log."""
    for k, v in (("x", s.x), ("lnl", s.lnl), ("status", s.status), ("acc", s.acc), ("beta", s.beta), ("lnz", s.lnz),
                 ("nstage", s.nstage), ("run_status", s.run_status), ("ncall", s.ncall), ("nacc", s.nacc), ("nfail", s.nfail)):
        assert np.array_equal(st[k], v), (k, st[k], v)
    for r in range(s.lnl.shape[0]):
        if s.nstage[r]:
            assert np.array_equal(st["anc"][r], s.anc[r]), r
        got = st["stages"][r]
        for k, v in zip(("beta", "d", "ess", "lnz", "accept", "ncall"), ad.stages_of(s, r, s.lnl.shape[1], walks)):
            assert np.array_equal(got[k], v), (r, k, got[k], v)
        for k, v in zip(("rounds", "g", "rho"), ad.tuning_of(s, r)):
            assert np.array_equal(st["tuning"][r][k], v), (r, k, st["tuning"][r][k], v)


def _same_with_tuning(a, b, runs_a=slice(None), runs_b=slice(None)):
    _same(a, b, runs_a, runs_b)
    for ta, tb in zip(a["tuning"][runs_a], b["tuning"][runs_b]):
        for k in ta:
            assert np.array_equal(ta[k], tb[k], equal_nan=True), k


# ---------------------------------------------------------------- 1. the tune kernel
def tune_launch(runs, n, ndim, made, cfg, moving=None, rounds=None):
    """One mpz_tune call behind the round that makes the stage's rounds `made` over the runs (name, start, now, acc, g)."""
    n_runs = len(runs)
    o = dict(g=np.array([c[4] for c in runs], dtype=np.float64),
             rounds=np.full(n_runs, made - 1, dtype=np.int32) if rounds is None else np.array(rounds, dtype=np.int32),
             moving=np.ones(n_runs, dtype=np.int32) if moving is None else np.array(moving, dtype=np.int32),
             rho_d=np.full((n_runs, ndim), -123.0), tune_rounds=np.full(n_runs, CANARY, dtype=np.int32),
             tune_log=np.full((n_runs, 2), -123.0))
    settings = np.array([cfg.corr, cfg.gain, cfg.accept_target, cfg.g_min, cfg.g_max, cfg.min_rounds, cfg.max_rounds], dtype=np.float64)
    start = np.ascontiguousarray(np.stack([c[1] for c in runs]))
    now = np.ascontiguousarray(np.stack([c[2] for c in runs]))
    acc = np.ascontiguousarray(np.stack([c[3] for c in runs]).astype(np.int32))
    rc = probe("smc").mpz_tune(C.c_int(n), C.c_int(n_runs), C.c_int(ndim), C.c_int(cases.WALKS), C.c_int(made - 1), dp(settings),
                               dp(start), dp(now), ip(acc), dp(o["g"]), ip(o["rounds"]), ip(o["moving"]), dp(o["rho_d"]),
                               ip(o["tune_rounds"]), dp(o["tune_log"]))
    assert rc == 0, rc
    return o


def assert_tuned(o, r, run, made, cfg):
    """Run r of the launch against the restatement with the device's exp: rho_d, rho, the decision, the next g."""
    name, start, now, acc, g = run
    rho_d, rho, go_on, g_next = ad.tune(start, now, acc, cases.WALKS, made, g, cfg, exp=device_exp)
    assert np.array_equal(o["rho_d"][r], rho_d), (name, o["rho_d"][r], rho_d)
    assert o["rounds"][r] == made and o["moving"][r] == int(go_on) and o["g"][r] == g_next, (name, o["g"][r], g_next)
    if go_on:
        assert o["tune_rounds"][r] == CANARY and np.all(o["tune_log"][r] == -123.0), name
    else:
        assert o["tune_rounds"][r] == made and o["tune_log"][r].tolist() == [g, rho], (name, o["tune_log"][r], rho)
    return rho_d, rho, go_on, g_next


@pytest.mark.parametrize("ndim", cases.NDIMS)
@pytest.mark.parametrize("n", cases.SIZES)
def test_tune_kernel_equals_the_restatement_bit_for_bit(n, ndim):
    """Every crafted case behind the first round (the rule decides) and behind the last (the cap does)."""
    rng = np.random.default_rng(7000 + n + ndim)
    cfg = ad.Adapt(cases.G0, min_rounds=1, max_rounds=4, corr=0.3, gain=1.0)
    went_on = stopped = 0
    for made in (1, 4):
        runs = cases.runs(n, ndim, made, rng, cfg.g_min, cfg.g_max)
        o = tune_launch(runs, n, ndim, made, cfg)
        for r, run in enumerate(runs):
            rho_d, rho, go_on, g_next = assert_tuned(o, r, run, made, cfg)
            exact = cases.exact_rho(run[0], ndim)
            assert exact is None or np.array_equal(rho_d, exact), run[0]
            assert go_on == (made < 4 and not rho <= 0.3), run[0]
            went_on, stopped = went_on + go_on, stopped + (not go_on)
            if run[0].startswith("g at") and not go_on:
                assert g_next == run[4]
    assert went_on >= 4 and stopped > len(runs)


def test_tune_kernel_at_one_ulp_of_corr_and_runs_that_take_no_part():
    n, ndim, made = 257, 6, 2
    rng = np.random.default_rng(5)
    runs = cases.runs(n, ndim, made, rng, 0.1, 2.0)
    mixed = runs[5]
    assert mixed[0] == "mixed"
    rho = ad.tune(*mixed[1:4], cases.WALKS, made, mixed[4], ad.Adapt(cases.G0, max_rounds=4), exp=device_exp)[1]
    for corr, want in ((rho, False), (float(np.nextafter(rho, 2.0)), False), (float(np.nextafter(rho, -1.0)), True)):
        cfg = ad.Adapt(cases.G0, min_rounds=1, max_rounds=4, corr=corr)
        o = tune_launch([mixed], n, ndim, made, cfg)
        assert assert_tuned(o, 0, mixed, made, cfg)[2] == want
    held = ad.Adapt(cases.G0, min_rounds=3, max_rounds=4, corr=rho)
    assert assert_tuned(tune_launch([mixed], n, ndim, 2, held), 0, mixed, 2, held)[2]
    assert not assert_tuned(tune_launch([mixed], n, ndim, 3, held), 0, mixed, 3, held)[2]
    # a run that has stopped, and one whose rounds are not the launch's: untouched, next to one that takes part
    cfg = ad.Adapt(cases.G0, min_rounds=1, max_rounds=4, corr=0.3)
    o = tune_launch([mixed, mixed, mixed], n, ndim, made, cfg, moving=[0, 1, 1], rounds=[1, 0, 1])
    for r in (0, 1):
        assert np.all(o["rho_d"][r] == -123.0) and o["tune_rounds"][r] == CANARY and o["g"][r] == mixed[4]
        assert (o["moving"][r], o["rounds"][r]) == ((0, 1), (1, 0))[r]
    assert_tuned(o, 2, mixed, made, cfg)
    L = probe("smc")
    z = np.zeros(8)
    assert L.mpz_tune(C.c_int(3), C.c_int(1), C.c_int(2), C.c_int(1), C.c_int(0), dp(z), dp(z), dp(z), None, dp(z), None, None,
                      dp(z), None, dp(z)) == -1


# ---------------------------------------------------------------- 2. the unit Gaussian against the restatement
@pytest.mark.parametrize("n, ndim", [(64, 2), (256, 6)])
def test_gaussian_stages_match_the_restatement_bit_for_bit(n, ndim):
    """Two runs, rounds of 2 steps, corr 0.2, at most 16 rounds, gain 1: behind every mp_smc_run(s, 1) the state, the log and the
    tuning log equal the restatement advanced by one stage.  The rounds made differ and none hits the cap."""
    n_runs, walks, seed = 2, 2, 20261020 + n + ndim
    lo, hi = np.full(ndim, -4.0), np.linspace(3.0, 5.0, ndim)
    x0 = lo + (hi - lo) * np.random.default_rng(n + ndim).random((n_runs, n, ndim))
    s = ad.begin(sm.start(x0, sm.gaussian), 0.0, 0.1)
    cfg = ad.Adapt(s.g[0], min_rounds=1, max_rounds=16, corr=0.2, gain=1.0)
    h = synth_handle()
    dev = RawAdaptive(h, n, n_runs, ndim, lo, hi, seed, walks, 1)
    try:
        assert dev.set_adaptive(1, 16, 0.2, 1.0) == 0
        dev.set_particles(x0.reshape(-1, ndim))
        _assert_equal(dev.state(), s, walks)
        for k in range(60):
            running = dev.run(1)
            ad.run(s, 1, seed, walks, 0.5, 0.0, 0.1, lo, hi, sm.gaussian, cfg, **DEVICE)
            _assert_equal(dev.state(), s, walks)
            assert running == int(np.sum(s.run_status == sm.RUNNING))
            if running == 0:
                break
    finally:
        dev.close()
        h.close()
    rounds = np.concatenate([ad.tuning_of(s, r)[0] for r in range(n_runs)])
    print(f"N {n}, ndim {ndim}: stages {s.nstage.tolist()}, rounds {rounds.tolist()}, g {np.round(s.g, 4).tolist()}, ln Z {s.lnz.tolist()}")
    assert np.all(s.run_status == sm.DONE) and np.all(s.nstage >= 2)
    assert rounds.min() < rounds.max() < 16 and np.all(s.g != cfg.g_min) and np.all(s.g != cfg.g_max)


# ---------------------------------------------------------------- 3. the round loop against the fixed-length path
def drive_fixed_rounds(h, run_ds, truths, n, stages, seed, build):
    """min_rounds = max_rounds = 3, gain = 0, rounds of 2 steps against a sampler without adaptation of 6 steps per move, on the
    real posterior: the same x, lnl, status, acc, ln Z, betas, counters and ancestors behind every stage."""
    from magprop_amd import synth
    lo, hi = synth.PRIOR_LOWER, synth.PRIOR_UPPER
    n_runs = len(run_ds)
    assert launch_class(n_runs * n, h.n_simd) == build, (n_runs * n, h.n_simd)
    x0 = posterior_live(truths, n, seed)
    fixed = RawAdaptive(h, n, n_runs, 6, lo, hi, seed, 6, 0, ds=run_ds)     # (mp_smc_set_adaptive is never called on it)
    dev = RawAdaptive(h, n, n_runs, 6, lo, hi, seed, 2, 0, ds=run_ds)
    try:
        assert dev.set_adaptive(3, 3, 0.0, 0.0) == 0
        for d in (fixed, dev):
            d.set_particles(x0.reshape(-1, 6))
        for _ in range(stages):
            assert fixed.run(1) == n_runs and dev.run(1) == n_runs
            a, b = fixed.state(), dev.state()
            _same(a, b)
        g0 = sm.resolve(0.0, 0.1, 6)[0]
        for t in b["tuning"]:
            assert t["rounds"].tolist() == [3] * stages and np.all(t["g"] == g0) and np.all(np.abs(t["rho"]) <= 1.0)
        for t in a["tuning"]:        # without adaptation: one round at g0, no rho
            assert t["rounds"].tolist() == [1] * stages and np.all(t["g"] == g0) and np.all(np.isnan(t["rho"]))
    finally:
        fixed.close()
        dev.close()
    assert np.all(b["nacc"] > 0) and np.all(b["nacc"] < b["ncall"] - n) and np.all(b["nstage"] == stages)


@pytest.mark.parametrize("case", ["team-1", "team-2", "wave-4", "wave-2"])
def test_fixed_rounds_equal_the_fixed_length_path_on_every_build(synth_sets, case):
    h = synth_sets
    c = smc_cases(h.n_simd)[case]
    drive_fixed_rounds(h, c["run_ds"], [TRUTHS[TYPES[d]] for d in c["run_ds"]], c["n"], 2, 20261020, c["build"])


def test_fixed_rounds_equal_the_fixed_length_path_on_the_long_builds(long_sets):
    drive_fixed_rounds(long_sets, [0, 1], [TRUTHS["Humped"], TRUTHS["Humped"]], 64, 2, 20261221, (4, 1, 1))


# ---------------------------------------------------------------- 4. the real posterior with adaptation live
@pytest.mark.parametrize("case", ["team-1", "wave-4"])
def test_posterior_stages_match_lnprob_batch_with_adaptation_live(synth_sets, case):
    """corr 0.3, at most 8 rounds of 2 steps, gain 1, runs on different datasets: the device equals the restatement behind every
    stage; every step of the restatement is one mp_lnprob_batch call of the launch's size."""
    from magprop_amd import synth
    h = synth_sets
    c = smc_cases(h.n_simd)[case]
    run_ds, n, walks, seed, stages = c["run_ds"], c["n"], 2, 20261020, 2
    lo, hi = synth.PRIOR_LOWER, synth.PRIOR_UPPER
    n_runs = len(run_ds)
    assert launch_class(n_runs * n, h.n_simd) == c["build"]
    x0 = posterior_live([TRUTHS[TYPES[d]] for d in run_ds], n, seed)
    ev = BatchEvaluator(h, run_ds)
    s = ad.begin(sm.start(x0, ev.at(n_runs * n)), 0.0, 0.1)
    cfg = ad.Adapt(s.g[0], min_rounds=1, max_rounds=8, corr=0.3, gain=1.0)
    dev = RawAdaptive(h, n, n_runs, 6, lo, hi, seed, walks, 0, ds=run_ds)
    try:
        assert dev.set_adaptive(1, 8, 0.3, 1.0) == 0
        dev.set_particles(x0.reshape(-1, 6))
        _assert_equal(dev.state(), s, walks)
        for _ in range(stages):
            assert dev.run(1) == n_runs
            ad.run(s, 1, seed, walks, 0.5, 0.0, 0.1, lo, hi, ev.at(n_runs * n), cfg, **DEVICE)
            _assert_equal(dev.state(), s, walks)
    finally:
        dev.close()
    rounds = [ad.tuning_of(s, r)[0].tolist() for r in range(n_runs)]
    print(f"move launch {n_runs * n} {c['build']}: {ev.calls} batches, rounds {rounds}, g {s.g.tolist()}, nacc {s.nacc.tolist()}")
    assert np.all(s.nacc > 0) and np.all(s.nstage == stages) and max(max(row) for row in rounds) > 1 and np.all(s.g < cfg.g_max)


# ---------------------------------------------------------------- 5. run control
def _adaptive_runs(n, n_runs, ndim, seed, x0, calls, lo, hi, walks=2, settings=(1, 16, 0.2, 1.0)):
    """The unit Gaussian, adaptively, through the C ABI: mp_smc_run once per entry of calls; the state behind every call."""
    h = synth_handle()
    dev = RawAdaptive(h, n, n_runs, ndim, lo, hi, seed, walks, 1)
    out = []
    try:
        assert dev.set_adaptive(*settings) == 0
        dev.set_particles(x0.reshape(-1, ndim))
        for c in calls:
            dev.run(c)
            out.append(dev.state())
    finally:
        dev.close()
        h.close()
    return out


def test_split_runs_equal_one_run():
    n, n_runs, ndim, seed = 128, 3, 3, 77
    lo, hi = np.full(ndim, -6.0), np.full(ndim, 6.0)
    x0 = -6.0 + 12.0 * np.random.default_rng(2).random((n_runs, n, ndim))
    whole = _adaptive_runs(n, n_runs, ndim, seed, x0, [1000], lo, hi)[0]
    total = int(whole["nstage"].max())
    assert np.all(whole["run_status"] == sm.DONE) and total > 3
    assert len({int(k) for t in whole["tuning"] for k in t["rounds"]}) > 1
    _same_with_tuning(_adaptive_runs(n, n_runs, ndim, seed, x0, [1] * total, lo, hi)[-1], whole)
    _same_with_tuning(_adaptive_runs(n, n_runs, ndim, seed, x0, [3, 0, total], lo, hi)[-1], whole)


def test_runs_stop_at_their_own_rounds_and_a_done_run_tunes_its_last_stage():
    """Three runs in one launch, the second done at its first stage: every run equals what it is alone (so the rounds one run
    makes do not reach another), the runs' rounds differ within a stage, and the done run has the tuning row of its only stage
    and stays as it is while the others go on."""
    n, ndim, seed = 64, 2, 5
    rng = np.random.default_rng(3)
    lo, hi = np.full(ndim, -8.0), np.full(ndim, 8.0)
    x0 = lo + (hi - lo) * rng.random((3, n, ndim))
    x0[1] = 0.02 * rng.standard_normal((n, ndim))            # flat lnl over these: done at its first stage
    states = _adaptive_runs(n, 3, ndim, seed, x0, [1, 1, 1000], lo, hi)
    first, last = states[0], states[-1]
    assert first["run_status"].tolist() == [sm.RUNNING, sm.DONE, sm.RUNNING] and np.all(last["run_status"] == sm.DONE)
    assert last["nstage"][1] == 1 and last["nstage"][0] > 2
    t = first["tuning"][1]
    assert len(t["rounds"]) == 1 and 1 <= t["rounds"][0] <= 16 and -1.0 <= t["rho"][0] <= 1.0 and first["nacc"][1] > 0
    _same_with_tuning(first, last, slice(1, 2), slice(1, 2))
    _same_with_tuning(states[1], last, slice(1, 2), slice(1, 2))
    stages = min(len(t["rounds"]) for t in last["tuning"][0:3:2])
    assert any(last["tuning"][0]["rounds"][k] != last["tuning"][2]["rounds"][k] for k in range(stages))
    alone = _adaptive_runs(n, 1, ndim, seed, x0[:1], [1000], lo, hi)[0]
    _same_with_tuning(alone, last, slice(0, 1), slice(0, 1))
    # run 2 carries its index in its Philox key: alone means in its own place among copies of itself
    alone = _adaptive_runs(n, 3, ndim, seed, np.stack([x0[2]] * 3), [1000], lo, hi)[0]
    _same_with_tuning(alone, last, slice(2, 3), slice(2, 3))


def test_set_adaptive_refusals():
    from magprop_amd import _capi
    ndim = 2
    lo, hi = np.full(ndim, -6.0), np.full(ndim, 6.0)
    h = synth_handle()
    dev = RawAdaptive(h, 16, 1, ndim, lo, hi, 1, 10, 1, g0=0.5)
    try:
        inf, nan = float("inf"), float("nan")
        for bad in ((0, 4, 0.3, 1.0), (5, 4, 0.3, 1.0), (1, -1, 0.3, 1.0), (1, 410, 0.3, 1.0), (1, 4, -0.1, 1.0), (1, 4, 1.0, 1.0),
                    (1, 4, nan, 1.0), (1, 4, 0.3, -1.0), (1, 4, 0.3, inf), (1, 4, 0.3, nan), (1, 4, 0.3, 1.0, 0.0), (1, 4, 0.3, 1.0, 1.0),
                    (1, 4, 0.3, 1.0, nan), (1, 4, 0.3, 1.0, 0.234, 0.6), (1, 4, 0.3, 1.0, 0.234, 0.0, 0.4), (1, 4, 0.3, 1.0, 0.234, inf),
                    (1, 4, 0.3, 1.0, 0.234, 0.0, inf), (1, 4, 0.3, 1.0, 0.234, nan)):
            assert dev.set_adaptive(*bad) == _capi.MP_EINVAL, bad
        assert dev.set_adaptive(1, 409, 0.0, 0.0, 0.5, 0.5, 0.5) == 0           # walks * max_rounds = 4 090; g_min = g0 = g_max
        assert dev.set_adaptive(0, 0, nan, nan, nan, nan, nan) == 0              # max_rounds = 0: off, nothing else is read
        assert dev.L.mp_smc_get_tuning(dev.s, 0, 0, None, None, None, None) == _capi.MP_ESTATE
        dev.set_particles(np.zeros((16, ndim)))
        assert dev.set_adaptive(1, 4, 0.3, 1.0) == _capi.MP_ESTATE
        assert dev.L.mp_smc_get_tuning(dev.s, 1, 0, None, None, None, None) == _capi.MP_EINVAL
        dev.run(1)
        t = dev.state()["tuning"][0]
        assert t["rounds"].tolist() == [1] and t["g"].tolist() == [0.5] and np.isnan(t["rho"][0])
    finally:
        dev.close()
        h.close()


# ---------------------------------------------------------------- 6. the evidence of Humped as it is
def test_humped_evidence_against_the_nested_sampler(gsynth):
    """8 adaptive runs of N = 1 024 at the shipped defaults and 8 nested runs (nlive 1 024, nbatch 256, 25 steps, dlogz 0.01: the
    settings of DESIGN.md section 8), the nested sampler the reference with its scatter measured here:
    |mean_smc - mean_nested| <= 4 sqrt(sd_smc^2 / 8 + sd_nested^2 / 8), and the adaptive runs scatter less than 8 runs of 10
    steps per move without adaptation from the same seed."""
    from magprop_amd import NestedSampler, SMCSampler
    x, y, yerr = gsynth["Humped_x"], gsynth["Humped_y"], gsynth["Humped_yerr"]

    def lnz_of(**kw):
        s = SMCSampler(x, y, yerr, nparticles=1024, n_runs=8, seed=20261020, **kw)
        res = s.run()
        s.close()
        assert all(r.status == "done" for r in res)
        return np.array([r.logz for r in res]), res

    adaptive, res = lnz_of(adapt=True)
    fixed, _ = lnz_of(walks=10)
    ns = NestedSampler(x, y, yerr, nlive=1024, nbatch=256, walks=25, n_runs=8, seed=20261020)
    nested = np.array([r.logz for r in ns.run_nested(dlogz=0.01)])
    ns.close()
    sd_a, sd_f, sd_n = (float(np.std(v, ddof=1)) for v in (adaptive, fixed, nested))
    bound = 4.0 * math.sqrt(sd_a ** 2 / 8.0 + sd_n ** 2 / 8.0)
    print(f"Humped: adaptive {adaptive.mean():.4f} sd {sd_a:.4f}, walks = 10 {fixed.mean():.4f} sd {sd_f:.4f}, nested "
          f"{nested.mean():.4f} sd {sd_n:.4f}; difference {adaptive.mean() - nested.mean():+.4f}, bound {bound:.4f}; rounds of run 0 "
          f"{res[0].rounds.tolist()}, scale {np.round(res[0].scale, 3).tolist()}, ncall {[r.ncall for r in res]}")
    assert all(len(r.rounds) == r.nstages and np.all(r.rounds >= 1) for r in res)
    assert abs(adaptive.mean() - nested.mean()) <= bound
    assert sd_a < sd_f
