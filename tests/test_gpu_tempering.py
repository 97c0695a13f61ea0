"""GPU tests of parallel tempering in the device-resident sampler (include/magprop_amd.h mp_sampler_set_temperatures)."""
import ctypes as C

import numpy as np
import pytest

from conftest import TRUTHS
from moves_restated import STRETCH
from raw_abi import dp, ip, lp, swap_counts, synth_handle
from sampler_restated import run as restate

pytestmark = pytest.mark.gpu


def _swap_counts(s):
    return swap_counts(s._L, s._s, s.ngroups, s.ntemps)


def test_tempered_gaussian_chain_matches_the_restatement_bit_for_bit():
    """4 temperatures x 16 walkers, 3 dims, 200 steps: chain, lnprob, acceptance and swap counts equal the numpy restatement
    exactly, with a whole step per launch and with two half-step launches, and continuing a run equals one run."""
    from magprop_amd import EnsembleSampler
    betas = (1.0, 0.5, 0.2, 0.05)
    seed = 20261015
    rng = np.random.default_rng(12)
    pos = rng.normal(size=(4 * 16, 3)) * 1.5
    ref = restate(pos.copy(), 200, seed, [(STRETCH, 1.0, 2.0, 0.0)], n_ensembles=4, n_temps=4,
                  betas=[betas[e % 4] for e in range(4)])           # (the restatement takes one beta per ensemble)
    chain, lnp, acc, swaps = ref.chain, ref.lnp, ref.acc, ref.swaps
    assert 0 < swaps.sum() < 200 * 16 * 3                     # swaps both accepted and refused
    for whole in (True, False):
        s = EnsembleSampler(16, 3, target="gaussian", seed=seed, betas=betas, whole_step=whole)
        assert s.nensembles == 4 and s.ntotal == 64
        s.run_mcmc(pos, 200)
        assert np.array_equal(s.get_chain(), chain), whole
        assert np.array_equal(s.get_log_prob(), lnp), whole
        assert np.array_equal(s.get_last_sample()[2], acc), whole
        assert np.array_equal(_swap_counts(s), swaps), whole
        assert np.array_equal(s.swap_acceptance_fraction, swaps / (200 * 16))
        # per-temperature views: temperature t of the only group = ensemble t
        assert np.array_equal(s.get_chain(temp=2), chain[:, 32:48]) and np.array_equal(s.get_log_prob(temp=0), lnp[:, :16])
        s.close()
        s2 = EnsembleSampler(16, 3, target="gaussian", seed=seed, betas=betas, whole_step=whole)
        s2.run_mcmc(pos, 70)
        s2.run_mcmc(None, 130)
        assert np.array_equal(s2.get_chain(), chain) and np.array_equal(s2.get_log_prob(), lnp), whole
        assert np.array_equal(_swap_counts(s2), swaps), whole
        s2.close()


def test_tempered_gaussian_distributions():
    """Ladder (1, 0.5, 0.25, 0.125), 128 walkers per temperature, 6 dims, 2000 steps (first 500 discarded): the walkers at beta_t
    sample N(0, 1/beta_t) -- variance 1/beta_t and mean lnL -d/(2 beta_t) within 6 % -- and swaps are neither always nor never
    accepted."""
    from magprop_amd import EnsembleSampler
    betas = (1.0, 0.5, 0.25, 0.125)
    d = 6
    rng = np.random.default_rng(3)
    s = EnsembleSampler(128, d, target="gaussian", seed=99, betas=betas)
    s.run_mcmc(rng.normal(size=(4 * 128, d)), 2000)
    for t, b in enumerate(betas):
        x = s.get_chain(temp=t)[500:].reshape(-1, d)
        lnl = s.get_log_prob(temp=t)[500:]
        assert np.all(np.abs(x.var(axis=0) * b - 1.0) < 0.06), (t, x.var(axis=0))
        assert abs(lnl.mean() / (-d / (2.0 * b)) - 1.0) < 0.06, (t, lnl.mean())
    f = s.swap_acceptance_fraction
    assert f.shape == (1, 3) and np.all(f > 0.0) and np.all(f < 1.0), f
    print(f"swap acceptance (1, 0.5, 0.25, 0.125), d = 6: {f.ravel()}")


def test_whole_step_equals_half_steps_on_a_posterior(gsynth):
    """Humped, 4 temperatures x 32 walkers, 100 steps (the team regime: both launch forms run the same kernel variant):
    the whole-step chain equals the half-step chain bit for bit, with its acceptance, swap and failure counts."""
    from magprop_amd import EnsembleSampler
    x, y, yerr = gsynth["Humped_x"], gsynth["Humped_y"], gsynth["Humped_yerr"]
    rng = np.random.default_rng(41)
    pos = np.array(TRUTHS["Humped"]) + 0.05 * rng.standard_normal((4 * 32, 6))
    out = []
    for whole in (True, False):
        s = EnsembleSampler(32, 6, x, y, yerr, seed=5, betas=(1.0, 0.1, 0.01, 0.001), whole_step=whole)
        s.run_mcmc(pos, 100)
        nbad, bad = s.get_bad()
        out.append((s.get_chain(), s.get_log_prob(), s.acceptance_fraction, _swap_counts(s), nbad,
                    bad[np.lexsort(bad.T)] if len(bad) else bad))
        s.close()
    for a_, b_ in zip(out[0], out[1]):
        assert np.array_equal(a_, b_)
    assert out[0][3].sum() > 0


def test_cold_chain_agrees_with_an_untempered_run(gsynth):
    """Humped from the truths, 8 temperatures x 32 walkers: the medians of the beta = 1 chain lie inside the 16-84 % intervals
    of an untempered run with the same number of steps."""
    from magprop_amd import EnsembleSampler, tempering
    x, y, yerr = gsynth["Humped_x"], gsynth["Humped_y"], gsynth["Humped_yerr"]
    rng = np.random.default_rng(8)
    n_steps, discard = 1500, 500
    betas = tempering.geometric_ladder(8, 1e-3)
    pt = EnsembleSampler(32, 6, x, y, yerr, seed=11, betas=betas)
    pt.run_mcmc(np.array(TRUTHS["Humped"]) + 1.0e-4 * rng.standard_normal((8 * 32, 6)), n_steps)
    cold = pt.get_chain(temp=0)[discard:].reshape(-1, 6)
    assert np.all(np.isfinite(pt.get_log_prob(temp=0)[discard:]))
    plain = EnsembleSampler(32, 6, x, y, yerr, seed=11)
    plain.run_mcmc(np.array(TRUTHS["Humped"]) + 1.0e-4 * rng.standard_normal((32, 6)), n_steps)
    ref = plain.get_chain()[discard:].reshape(-1, 6)
    lo, hi = np.percentile(ref, [16, 84], axis=0)
    med = np.median(cold, axis=0)
    assert np.all((lo <= med) & (med <= hi)), (med, lo, hi)
    # the beta = 1 views: autocorrelation time and band are those of the cold walkers
    assert pt.get_autocorr_time(quiet=True).shape == (6,)
    band = pt.get_model_band(q=(0.5,), discard=n_steps - 4)
    assert band["n_used"] <= 4 * 32
    nbad, _ = pt.get_bad()
    print(f"cold-chain run: swap acceptance {np.round(pt.swap_acceptance_fraction.ravel(), 3)}, "
          f"failed proposals {nbad} of {n_steps * 8 * 32} ({nbad / (n_steps * 8 * 32):.2e})")


# yerr inflation of the evidence test: lnL = -chi^2 / 2 scales as 1 / F^2
EVIDENCE_INFLATION = 10.0


def test_log_evidence_against_brute_force(gsynth):
    """Humped with yerr x 10, so that the posterior fills a sizeable part of the box: the brute-force evidence over 4 x 2^20
    uniform box draws (failed models count as L = 0; effective sample size (sum w)^2 / sum w^2 asserted >= 1 000) against
    log_evidence of a tempered run, 128 temperatures geometric from 1 to 1e-12 (the prior mean of lnL is ~ -3e7 here, from
    models far off the data, so the ladder must reach down to beta ~ 1e-12 before <lnL>_beta levels off), 32 walkers each,
    2 500 steps, the first 500 discarded.  Must agree within max(3 dlnZ, 0.05).
    The inflation was chosen from the lnL of 24 000 box draws (lnL scales as 1 / F^2): F = 10 gives an ESS of ~4 % of the draws
    and a ladder model (trapezoid over the reweighted draws) predicts a discretisation bias of -0.02 for this ladder.
    Calibrated once on an MI355X: brute force -5.5046 (ESS 160 641), tempered -5.5397 +- 0.0572, difference -0.0351 (the sign
    and size of the predicted bias); 3 156 of 10 240 000 proposals failed (3.1e-4, all temperatures together)."""
    from magprop_amd import EnsembleSampler, LogProb, synth, tempering
    x, y, yerr = gsynth["Humped_x"], gsynth["Humped_y"], gsynth["Humped_yerr"] * EVIDENCE_INFLATION
    lo, hi = synth.PRIOR_LOWER, synth.PRIOR_UPPER
    lp = LogProb(x, y, yerr)
    rng = np.random.default_rng(2026)
    n_bf, chunk = 4 << 20, 1 << 18
    vals = np.concatenate([lp(lo + (hi - lo) * rng.random((chunk, 6))) for _ in range(n_bf // chunk)])
    w = np.exp(vals - vals.max())                               # (failed models: exp(-inf) = 0)
    lnz_bf = vals.max() + np.log(w.sum()) - np.log(n_bf)
    ess = w.sum() ** 2 / (w ** 2).sum()
    assert ess >= 1000.0, ess
    # a start inside the region where the model succeeds, spread over the whole box
    start = lo + (hi - lo) * rng.random((4 * 128 * 32, 6))
    start = start[np.isfinite(lp(start))][:128 * 32]
    betas = tempering.geometric_ladder(128, 1e-12)
    s = EnsembleSampler(32, 6, x, y, yerr, seed=77, betas=betas)
    s.run_mcmc(start, 2500)
    lnz, dlnz = s.log_evidence(discard=500)
    nbad, _ = s.get_bad()
    n_prop = 2500 * 128 * 32
    print(f"evidence: brute force {lnz_bf:.4f} (ESS {ess:.0f}), tempered {lnz:.4f} +- {dlnz:.4f}, difference {lnz - lnz_bf:+.4f}; "
          f"failed proposals {nbad} of {n_prop} ({nbad / n_prop:.2e}), "
          f"hottest chain's failing-state fraction {np.mean(~np.isfinite(s.get_log_prob(temp=127)))}")
    assert abs(lnz - lnz_bf) < max(3.0 * dlnz, 0.05), (lnz, dlnz, lnz_bf)


def test_tempering_argument_validation(gsynth):
    from magprop_amd import EnsembleSampler, _capi
    L = _capi.lib()
    x, y, yerr = gsynth["Humped_x"], gsynth["Humped_y"], gsynth["Humped_yerr"]
    h = synth_handle()
    h.set_prior(gsynth["prior_lower"], gsynth["prior_upper"], 0b111100)
    h.set_dataset(0, x, y, yerr)
    h.set_dataset(1, x, y, 2.0 * yerr)

    def ladder(*b):
        a = np.array(b, dtype=np.float64)
        return a, dp(a)

    ids = np.array([0, 0, 1, 1], dtype=np.int32)
    sp = L.mp_sampler_create(h._h, 8, 4, 6, ip(ids), C.c_uint64(1), C.c_double(2.0), 0)
    assert sp
    for bad in ((0.9, 0.5), (1.0, 1.0), (1.0, 0.0), (1.0, -0.5), (1.0, np.nan), (1.0, np.inf), (1.0, 0.25, 0.5, 0.1)):
        a, p = ladder(*bad)
        assert L.mp_sampler_set_temperatures(sp, a.size, p) == _capi.MP_EINVAL, bad
    a, p = ladder(1.0)
    assert L.mp_sampler_set_temperatures(sp, 1, p) == _capi.MP_EINVAL                  # T >= 2
    a, p = ladder(1.0, 0.5, 0.25)
    assert L.mp_sampler_set_temperatures(sp, 3, p) == _capi.MP_EINVAL                  # 4 ensembles, groups of 3
    a, p = ladder(1.0, 0.5, 0.25, 0.125)
    assert L.mp_sampler_set_temperatures(sp, 4, p) == _capi.MP_EINVAL                  # datasets 0 and 1 in one group
    swaps = np.zeros(2, dtype=np.int64)
    assert L.mp_sampler_get_swaps(sp, lp(swaps)) == _capi.MP_ESTATE   # not tempered
    a, p = ladder(1.0, 0.5)
    assert L.mp_sampler_set_temperatures(sp, 2, p) == _capi.MP_OK
    pos = np.ascontiguousarray(np.array(TRUTHS["Humped"]) + 1.0e-3 * np.random.default_rng(0).standard_normal((32, 6)))
    assert L.mp_sampler_set_positions(sp, dp(pos)) == _capi.MP_OK
    assert L.mp_sampler_set_temperatures(sp, 2, p) == _capi.MP_ESTATE                  # after set_positions
    # the walker-sharded entry points refuse a tempered sampler
    rows = C.c_void_p(1)
    assert L.mp_sampler_halfstep_shard(sp, 0, 0, 1, rows, None) == _capi.MP_ESTATE
    assert L.mp_sampler_halfstep_apply(sp, 0, rows, None, None, None) == _capi.MP_ESTATE
    assert L.mp_sampler_step_shard(sp, 0, 1, rows, None) == _capi.MP_ESTATE
    assert L.mp_sampler_step_apply(sp, rows, None, None, None) == _capi.MP_ESTATE
    assert L.mp_sampler_run(sp, 3, None, None) == _capi.MP_OK
    assert L.mp_sampler_get_swaps(sp, lp(swaps)) == _capi.MP_OK
    assert np.all((swaps >= 0) & (swaps <= 3 * 8))
    L.mp_sampler_destroy(sp)
    h.close()
    # Python front end: the same ladder rule, and the distributed driver refuses a tempered sampler
    with pytest.raises(ValueError):
        EnsembleSampler(8, 6, x, y, yerr, betas=(1.0, 0.0))
    with pytest.raises(ValueError):
        EnsembleSampler(8, 6, x, y, yerr, betas=(0.5, 0.25))
    s = EnsembleSampler(8, 6, x, y, yerr, betas=(1.0, 0.5))
    assert s.nensembles == 2 and s.ngroups == 1
    from magprop_amd.distributed import DistributedEnsembleSampler, HipShardEngine
    with pytest.raises(ValueError):
        DistributedEnsembleSampler(HipShardEngine(s, "cuda:0"))
    with pytest.raises(ValueError):
        s.get_chain(temp=2)
    s.close()
    plain = EnsembleSampler(8, 6, x, y, yerr)
    with pytest.raises(ValueError):
        plain.swap_acceptance_fraction
    with pytest.raises(ValueError):
        plain.log_evidence()
    plain.close()
