"""The sample reservoir behind the sampler (mp_sampler_set_reservoir / mp_sampler_get_reservoir; EnsembleSampler.monitor_samples,
get_samples and source="reservoir"): on the unit-Gaussian target every held row against the stored chain and the held set against
the restatement of the rule (tests/reservoir_restated.py), bit for bit, however the run is driven; the chains untouched; a
tempered run; and on the Humped posterior an unstored run whose summaries equal the module functions on the reservoir's rows."""
import ctypes as C

import numpy as np
import pytest

import reservoir_restated as rr
from conftest import TRUTHS
from raw_abi import RawSampler, dp, ip, lp

pytestmark = pytest.mark.gpu

NW, NE, ND, K, SEED, RSEED = 32, 2, 3, 64, 11, 0xABCDEF0123456789


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def set_reservoir(r, size, seed=RSEED, discard=0):
    return r.L.mp_sampler_set_reservoir(r.sp, size, C.c_uint64(seed), C.c_int64(discard))


def get_reservoir(r, e, size=K, check=True):
    x, lnp, step = np.full((size, r.ndim), -7.0), np.full(size, -7.0), np.full(size, -7, dtype=np.int64)
    walker, key = np.full(size, -7, dtype=np.int32), np.zeros(size, dtype=np.uint64)
    n_rows, n_seen = C.c_int(-7), C.c_int64(-7)
    rc = r.L.mp_sampler_get_reservoir(r.sp, e, size, dp(x), dp(lnp), lp(step), ip(walker), key.ctypes.data_as(C.POINTER(C.c_uint64)),
                                      C.byref(n_rows), C.byref(n_seen))
    if not check:
        return rc
    assert rc == 0, r.cap.last_error()
    n = n_rows.value
    return {"x": x[:n], "log_prob": lnp[:n], "step": step[:n], "walker": walker[:n], "key": key[:n], "n_seen": n_seen.value}


def start(whole=None, size=K, discard=0, betas=None, n_ens=NE):
    r = RawSampler(NW, n_ens, ND, SEED)
    if betas is not None:
        r.set_temperatures(betas)
    if whole is not None:
        r.set_whole_step(whole)
    if size:
        assert set_reservoir(r, size, discard=discard) == 0, r.cap.last_error()
    r.set_positions(np.random.default_rng(3).standard_normal((NW * n_ens, ND)))
    return r


@pytest.fixture(scope="module")
def one_run():
    """200 stored steps with the monitor on: chain, lnprob and the two ensembles' reservoirs."""
    with start() as r:
        chain, lnp = r.run(200)
        return chain, lnp, [get_reservoir(r, e) for e in range(NE)]


def test_rows_are_the_chains_and_the_set_is_the_restatements(one_run):
    chain, lnp, res = one_run
    for e in range(NE):
        t, w, k = rr.as_arrays(rr.brute(RSEED, range(200), NW, e, K))
        got = res[e]
        assert got["n_seen"] == 200 * NW and len(got["step"]) == K
        assert np.array_equal(got["step"], t) and np.array_equal(got["walker"], w) and np.array_equal(got["key"], k), e
        assert same(got["x"], chain[t, e * NW + w]) and same(got["log_prob"], lnp[t, e * NW + w]), e
    assert not np.array_equal(res[0]["step"], res[1]["step"])


def test_the_reservoir_does_not_depend_on_how_the_run_is_driven(one_run):
    _, _, res = one_run
    for whole, runs in ((None, (70, 130)), (0, (200,)), (0, (1, 199)), (1, (200,))):
        with start(whole) as r:
            for n in runs:
                r.run(n, store=False)
            for e in range(NE):
                got = get_reservoir(r, e)
                assert got["n_seen"] == res[e]["n_seen"] and all(same(got[k], res[e][k]) for k in ("x", "log_prob", "step", "walker", "key")), (whole, runs, e)


def test_chains_are_unchanged_by_the_monitor(one_run):
    chain, lnp, _ = one_run
    with start(size=0) as r:
        c0, l0 = r.run(200)
        assert get_reservoir(r, 0, check=False) == r.cap.MP_ESTATE
    assert same(c0, chain) and same(l0, lnp)


def test_discard_and_restart_at_set_positions():
    with start(discard=30) as r:
        chain, lnp = r.run(100)
        got = get_reservoir(r, 1)
        t, w, k = rr.as_arrays(rr.brute(RSEED, range(30, 100), NW, 1, K))
        assert got["n_seen"] == 70 * NW and np.array_equal(got["step"], t) and np.array_equal(got["walker"], w) and np.array_equal(got["key"], k)
        assert same(got["x"], chain[t, NW + w])
        # set_positions restarts it: nothing held, and the discard applies again, to the steps that follow
        r.set_positions(chain[-1])
        assert get_reservoir(r, 1)["n_seen"] == 0 and len(get_reservoir(r, 1)["step"]) == 0
        chain2, _ = r.run(40)
        got = get_reservoir(r, 0)
        t, w, k = rr.as_arrays(rr.brute(RSEED, range(130, 140), NW, 0, K))
        assert got["n_seen"] == 10 * NW and np.array_equal(got["step"], t) and np.array_equal(got["key"], k)
        assert same(got["x"], chain2[t - 100, w])
        # fewer rows asked for than held: the first of them in (step, walker) order
        few = get_reservoir(r, 0, size=5)
        assert np.array_equal(few["step"], t[:5]) and np.array_equal(few["walker"], w[:5]) and same(few["x"], got["x"][:5])


def test_argument_codes_in_order():
    with start(size=0) as r:
        L, cap = r.L, r.cap
        assert L.mp_sampler_set_reservoir(None, K, C.c_uint64(1), C.c_int64(0)) == cap.MP_EINVAL
        assert set_reservoir(r, -1, discard=-1) == cap.MP_EINVAL and "size" in cap.last_error()
        assert set_reservoir(r, cap.RESERVOIR_MAX_ROWS + 1) == cap.MP_EINVAL and "MP_RESERVOIR_MAX_ROWS" in cap.last_error()
        assert set_reservoir(r, K, discard=-1) == cap.MP_EINVAL and "discard" in cap.last_error()
        assert set_reservoir(r, 0, discard=-1) == cap.MP_OK                      # (size 0: off, the rest is ignored)
        assert L.mp_sampler_get_reservoir(None, 0, 1, None, None, None, None, None, None, None) == cap.MP_EINVAL
        assert get_reservoir(r, 0, check=False) == cap.MP_ESTATE and "mp_sampler_set_reservoir" in cap.last_error()
        assert get_reservoir(r, NE, check=False) == cap.MP_ESTATE                # (off comes before the ensemble)
        assert set_reservoir(r, cap.RESERVOIR_MAX_ROWS) == cap.MP_OK and set_reservoir(r, K) == cap.MP_OK
        assert get_reservoir(r, NE, check=False) == cap.MP_EINVAL and get_reservoir(r, -1, check=False) == cap.MP_EINVAL
        assert L.mp_sampler_get_reservoir(r.sp, 0, -1, None, None, None, None, None, None, None) == cap.MP_EINVAL
        assert L.mp_sampler_get_reservoir(r.sp, 0, K, None, None, None, None, None, None, None) == cap.MP_OK   # any output may be NULL
        # a failed set leaves the monitor off
        assert set_reservoir(r, K, discard=-1) == cap.MP_EINVAL and get_reservoir(r, 0, check=False) == cap.MP_ESTATE


def test_sharded_entry_points_refuse_while_the_monitor_is_on():
    """(The refusal comes before the row buffers are looked at, so the calls pass none.)"""
    with start() as r:
        L, junk = r.L, C.c_void_p(8)
        for name, call in (("mp_sampler_halfstep_shard", lambda: L.mp_sampler_halfstep_shard(r.sp, 0, 0, r.n_slots, None, None)),
                           ("mp_sampler_halfstep_apply", lambda: L.mp_sampler_halfstep_apply(r.sp, 0, junk, None, None, None)),
                           ("mp_sampler_step_shard", lambda: L.mp_sampler_step_shard(r.sp, 0, r.step_blocks, None, None)),
                           ("mp_sampler_step_apply", lambda: L.mp_sampler_step_apply(r.sp, junk, None, None, None))):
            assert call() == r.cap.MP_ESTATE
            assert r.cap.last_error() == name + ": the sample reservoir (mp_sampler_set_reservoir) is fed by mp_sampler_run only; turn it off first"
        assert set_reservoir(r, 0) == 0
        assert L.mp_sampler_halfstep_shard(r.sp, 0, 0, 0, None, None) == r.cap.MP_OK   # (an empty block of slots: no launch)


def test_tempered_run_reads_the_beta_1_ensemble_of_the_group():
    from magprop_amd import EnsembleSampler, reservoir
    betas = (1.0, 0.5, 0.1)
    s = EnsembleSampler(NW, ND, target="gaussian", seed=SEED, betas=betas)
    s.monitor_samples(size=K, seed=RSEED)
    s.run_mcmc(np.random.default_rng(3).standard_normal((NW * 3, ND)), 60)
    chain, lnp = s.get_chain(), s.get_log_prob()
    for temp, e in ((None, 0), (0, 0), (2, 2)):
        got = s.get_samples(0, temp=temp)
        assert got["n_seen"] == 60 * NW and got["key"].dtype == np.uint64 and got["walker"].dtype == np.int32
        assert np.array_equal(got["key"], reservoir.keys(RSEED, got["step"], got["walker"], e, NW))
        t, w, k = rr.as_arrays(rr.brute(RSEED, range(60), NW, e, K))
        assert np.array_equal(got["step"], t) and np.array_equal(got["walker"], w) and np.array_equal(got["key"], k)
        assert same(got["x"], chain[t, e * NW + w]) and same(got["log_prob"], lnp[t, e * NW + w])
    with pytest.raises(ValueError, match="ensemble must be in"):
        s.get_samples(1)
    s.monitor_samples(None)
    with pytest.raises(Exception, match="the sample reservoir is off"):
        s.get_samples()
    s.close()


def test_unstored_humped_run_ends_with_every_summary(gsynth):
    from magprop_amd import EnsembleSampler, synth
    x, y, yerr = gsynth["Humped_x"], gsynth["Humped_y"], gsynth["Humped_yerr"]
    rng = np.random.default_rng(4)
    p0 = np.array(TRUTHS["Humped"]) + 1e-3 * rng.standard_normal((64, 6))
    s = EnsembleSampler(64, 6, x, y, yerr, seed=5)
    s.monitor_samples(size=256)
    s.run_mcmc_until(p0, 300, check_every=100, store=False)
    assert s.get_chain() is None
    got = s.get_samples()
    rows = got["x"]
    assert rows.shape == (256, 6) and got["n_seen"] == s.iteration * 64 and np.all(np.diff(got["step"] * 64 + got["walker"]) > 0)
    assert np.all(np.isfinite(got["log_prob"])) and len(set(got["step"].tolist())) > 100
    q = (0.16, 0.5, 0.84)
    d, wd = s.get_derived(source="reservoir"), synth.model_derived(rows)
    assert d["n_used"] == wd["n_used"] > 0 and same(d["values"], wd["values"]) and np.array_equal(d["status"], wd["status"])
    b, wb = s.get_model_band(source="reservoir"), synth.model_band(rows)
    assert b["n_used"] == wb["n_used"] > 0 and same(b["Ltot"], wb["Ltot"])
    f, wf = s.get_flows(q=q, curves=("fastness",), source="reservoir"), synth.model_flows(rows, curves=("fastness",), q=q)
    assert f["n_used"] == wf["n_used"] > 0 and same(f["values"], wf["values"]) and same(f["fastness"], wf["fastness"])
    fb, wfb = s.get_flow_band(curves=("Rm",), source="reservoir"), synth.model_flow_band(rows, curves=("Rm",))
    assert fb["n_used"] == wfb["n_used"] > 0 and same(fb["Rm"], wfb["Rm"])
    p, wp = s.get_pointwise(source="reservoir"), synth.model_pointwise(rows, x, y, yerr)
    assert p["n_used"] == wp["n_used"] > 0 and same(p["obs"], wp["obs"]) and same(p["tail"], wp["tail"])
    # the default source is the stored chain, and there is none
    for call in (s.get_model_band, s.get_derived, s.get_flows, s.get_flow_band, s.get_pointwise):
        with pytest.raises(ValueError, match=r"the chain is empty: run_mcmc\(\.\.\., store=True\) first"):
            call()
        with pytest.raises(ValueError, match="discard and thin must be 0 and 1"):
            call(discard=10, source="reservoir")
        with pytest.raises(ValueError, match="source must be 'chain' or 'reservoir'"):
            call(source="device")
    s.close()
