"""GPU tests of the proposal moves of the device-resident sampler (include/magprop_amd.h mp_sampler_set_moves): DE, snooker and
mixtures against the numpy restatement (tests/sampler_restated.py) bit for bit, moments, a posterior run and argument codes."""
import ctypes as C

import numpy as np
import pytest

from conftest import TRUTHS
from moves_restated import DE, SNOOKER, STRETCH
from raw_abi import RawSampler, dp, gaussian_run, synth_handle, table_args
from sampler_restated import run as restate

pytestmark = pytest.mark.gpu

TEAM_RTOL = 1e-11      # tests/test_gpu_parity.py: one kernel variant against another, rounding apart
DE_DEFAULT = (DE, 1.0, 0.0, 1.0e-5)
SNOOKER_DEFAULT = (SNOOKER, 1.0, 1.7, 0.0)
TABLES = {
    "de": [DE_DEFAULT],
    "snooker": [SNOOKER_DEFAULT],
    "de_snooker": [(DE, 0.8, 0.0, 1.0e-5), (SNOOKER, 0.2, 1.7, 0.0)],
    "stretch_de": [(STRETCH, 0.5, 2.0, 0.0), (DE, 0.5, 0.0, 1.0e-5)],
}


@pytest.mark.parametrize("name", list(TABLES))
def test_gaussian_chain_matches_the_restatement_bit_for_bit(name):
    """32 walkers x 2 ensembles x 3 dims x 120 steps (the team builds; stretch steps of a mixture as one launch per step):
    chain, lnprob and acceptance counts equal the restatement exactly, and 50 + 70 steps equal 120."""
    table = TABLES[name]
    seed = 20261016
    pos = np.random.default_rng(3).normal(size=(2 * 32, 3)) * 1.5
    ref = restate(pos.copy(), 120, seed, table, n_ensembles=2)
    if len(table) > 1:
        assert 0 < np.count_nonzero(ref.drawn == 1) < 120    # both moves were drawn
    assert 0 < ref.acc.sum() < 120 * 64
    for whole in (True, False):
        got = gaussian_run(32, 2, 3, seed, table, pos, (120,), whole=whole)
        for a, b in zip(got, (ref.chain, ref.lnp, ref.acc)):
            assert np.array_equal(a, b), (name, whole)
    got = gaussian_run(32, 2, 3, seed, table, pos, (50, 70), whole=True)
    for a, b in zip(got, (ref.chain, ref.lnp, ref.acc)):
        assert np.array_equal(a, b), name


@pytest.mark.parametrize("name", ["de_snooker", "stretch_de"])
def test_gaussian_chain_bit_for_bit_on_the_one_wave_builds(name):
    """2 048 walkers x 2 dims x 20 steps: the one-wavefront half-step builds (and stretch steps of two half-step launches)."""
    table = TABLES[name]
    seed = 77
    pos = np.random.default_rng(4).normal(size=(2048, 2))
    ref = restate(pos.copy(), 20, seed, table)
    got = gaussian_run(2048, 1, 2, seed, table, pos, (20,), whole=True)
    for a, b in zip(got, (ref.chain, ref.lnp, ref.acc)):
        assert np.array_equal(a, b), name


@pytest.mark.parametrize("name", ["snooker", "de"])
def test_coinciding_walkers_match_the_restatement_bit_for_bit(name):
    """12 walkers x 3 dims x 30 steps started as six pairs of coinciding walkers.  Snooker: a walker whose z is its twin in the
    other half has dd = 0, a NaN factor and a NaN Hastings term; the proposal is rejected, the walker stays and its chain row
    repeats.  DE: partners x1 == x2 make the proposal the walker itself, to the bit (and accepted: 0 > ln u).  Chain, lnprob
    and acceptance counts equal the restatement exactly, with one launch per step and with two."""
    from oracle.stretch_oracle import gaussian_lnprob
    table, seed = TABLES[name], 20261018
    half = np.random.default_rng(21).normal(size=(6, 3))
    pos = np.concatenate([half, half])
    seen = {"nan": 0, "self": 0}
    state = pos.copy()

    def lnprob(q):      # (the restated loop advances `state` in place: q is held against the positions of the moment)
        seen["nan"] += bool(np.any(np.isnan(q)))
        seen["self"] += any(np.array_equal(q, x) for x in state)
        return gaussian_lnprob(q)
    ref = restate(state, 30, seed, table, lnprob_fn=lnprob)
    assert seen["nan" if name == "snooker" else "self"] > 0, seen
    assert not np.any(np.isnan(ref.chain)) and not np.any(np.isnan(ref.lnp)) and 0 < ref.acc.sum() < 30 * 12
    for whole in (True, False):
        got = gaussian_run(12, 1, 3, seed, table, pos, (30,), whole=whole)
        for a, b in zip(got, (ref.chain, ref.lnp, ref.acc)):
            assert np.array_equal(a, b), (name, whole)


@pytest.mark.parametrize("whole", [True, False], ids=["whole-step", "half-steps"])
def test_three_ensembles_match_the_restatement_bit_for_bit(whole):
    """3 ensembles x 10 walkers x 3 dims x 40 steps of the stretch move, untempered, as one launch per step
    (stretch_step_kernel and stretch_step_commit_kernel, whose partner lookup carries the ensemble term w_ens * n_half) and as two
    half-step launches: chain, lnprob and acceptance counts equal the restatement exactly.  (tests/test_gpu_sampler.py
    test_two_ensembles_match_the_oracle runs two ensembles in the library's default mode only.)"""
    table, seed = [(STRETCH, 1.0, 2.0, 0.0)], 20261019
    pos = np.random.default_rng(22).normal(size=(3 * 10, 3)) * 1.5
    ref = restate(pos.copy(), 40, seed, table, n_ensembles=3)
    assert 0 < ref.acc.sum() < 40 * 30
    got = gaussian_run(10, 3, 3, seed, table, pos, (40,), whole=whole)
    for a, b in zip(got, (ref.chain, ref.lnp, ref.acc)):
        assert np.array_equal(a, b), whole


def test_explicit_stretch_move_is_the_default_chain(gsynth):
    """moves=[StretchMove()] runs the chain of the default sampler on Humped, 64 walkers x 100 steps, bit for bit."""
    from magprop_amd import EnsembleSampler, StretchMove
    x, y, yerr = gsynth["Humped_x"], gsynth["Humped_y"], gsynth["Humped_yerr"]
    pos = np.array(TRUTHS["Humped"]) + 1.0e-3 * np.random.default_rng(9).standard_normal((64, 6))
    out = []
    for moves in (None, [StretchMove()]):
        s = EnsembleSampler(64, 6, x, y, yerr, seed=17, moves=moves)
        s.run_mcmc(pos, 100)
        out.append((s.get_chain(), s.get_log_prob(), s.get_last_sample()[2], s.get_bad()[0]))
        s.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("name", ["de", "snooker", "de_snooker"])
def test_gaussian_target_statistics_per_move(name):
    """test_gaussian_target_statistics (tests/test_gpu_sampler.py) with each move: 256 walkers, 6 dims, 1 500 steps from a ball
    at 3, the first 500 discarded: mean within 0.05, variance within 0.06 of 1."""
    from magprop_amd import DEMove, DESnookerMove, EnsembleSampler
    moves = {"de": DEMove(), "snooker": DESnookerMove(), "de_snooker": [(DEMove(), 0.8), (DESnookerMove(), 0.2)]}[name]
    rng = np.random.default_rng(8)
    s = EnsembleSampler(256, 6, target="gaussian", seed=3, moves=moves)
    s.run_mcmc(rng.normal(size=(256, 6)) * 0.1 + 3.0, 1500)
    tail = s.get_chain()[500:].reshape(-1, 6)
    assert np.all(np.abs(tail.mean(axis=0)) < 0.05), tail.mean(axis=0)
    assert np.all(np.abs(tail.var(axis=0) - 1.0) < 0.06), tail.var(axis=0)
    af = s.acceptance_fraction.mean()
    assert 0.05 < af < 0.9, af
    print(f"{name}: acceptance {af:.3f}, tau {np.round(s.get_autocorr_time(quiet=True), 1)}")
    s.close()


def test_tempered_cold_chain_moments_with_the_mixture():
    """Ladder (1, 0.5, 0.25) with the DE + snooker mixture: the beta = 1 walkers have the moments above."""
    from magprop_amd import DEMove, DESnookerMove, EnsembleSampler
    rng = np.random.default_rng(8)
    s = EnsembleSampler(256, 6, target="gaussian", seed=3, betas=(1.0, 0.5, 0.25),
                        moves=[(DEMove(), 0.8), (DESnookerMove(), 0.2)])
    s.run_mcmc(rng.normal(size=(3 * 256, 6)) * 0.1 + 3.0, 1500)
    tail = s.get_chain(temp=0)[500:].reshape(-1, 6)
    assert np.all(np.abs(tail.mean(axis=0)) < 0.05), tail.mean(axis=0)
    assert np.all(np.abs(tail.var(axis=0) - 1.0) < 0.06), tail.var(axis=0)
    f = s.swap_acceptance_fraction
    assert np.all(f > 0.0) and np.all(f < 1.0), f
    s.close()


def test_humped_posterior_with_the_de_snooker_mixture(gsynth):
    """512 walkers x 3 000 steps from the truths, the first 1 000 discarded: the medians of the DE + snooker run lie within
    0.25 posterior sigma of a stretch run's; every stored lnprob is the log-posterior at its stored position; every logged
    failed proposal flags or goes non-finite."""
    from magprop_amd import DEMove, DESnookerMove, EnsembleSampler, _capi
    x, y, yerr = gsynth["Humped_x"], gsynth["Humped_y"], gsynth["Humped_yerr"]
    rng = np.random.default_rng(30)
    n_steps, discard = 3000, 1000
    runs = {}
    for name, moves in (("stretch", None), ("mix", [(DEMove(), 0.8), (DESnookerMove(), 0.2)])):
        s = EnsembleSampler(512, 6, x, y, yerr, seed=31, moves=moves)
        s.run_mcmc(np.array(TRUTHS["Humped"]) + 1.0e-4 * rng.standard_normal((512, 6)), n_steps)
        runs[name] = s
    ref = runs["stretch"].get_chain()[discard:].reshape(-1, 6)
    s = runs["mix"]
    chain, lnp = s.get_chain(), s.get_log_prob()
    mix = chain[discard:].reshape(-1, 6)
    sigma = ref.std(axis=0)
    dmed = np.abs(np.median(mix, axis=0) - np.median(ref, axis=0)) / sigma
    assert np.all(dmed < 0.25), dmed
    assert np.all(np.isfinite(lnp))
    # stored lnprob against the log-posterior at the stored positions, one step per call (the half-steps ran on the
    # one-wavefront builds, a 512-row call runs the team kernel: same tiles and policy, rounding apart)
    for t in range(n_steps):
        want = s.handle.lnprob_batch(chain[t])
        assert np.allclose(lnp[t], want, rtol=TEAM_RTOL, atol=0.0), t
    n_bad, rows = s.get_bad()
    assert len(rows) == n_bad
    if n_bad:
        _, st = s.handle.lnprob_batch(rows, want_status=True)
        assert np.all((st == _capi.STATUS_FLAG) | (st == _capi.STATUS_NONFINITE)), st
    tau = {k: np.mean(v.get_autocorr_time(quiet=True)) for k, v in runs.items()}
    print(f"Humped, 512 walkers: acceptance stretch {runs['stretch'].acceptance_fraction.mean():.3f}, mixture "
          f"{s.acceptance_fraction.mean():.3f}; mean tau {tau}; failed proposals {n_bad}; median shifts / sigma {np.round(dmed, 3)}")
    for v in runs.values():
        v.close()


def test_set_moves_argument_codes(gsynth):
    from magprop_amd import EnsembleSampler, _capi
    x, y, yerr = gsynth["Humped_x"], gsynth["Humped_y"], gsynth["Humped_yerr"]
    h = synth_handle()
    h.set_prior(gsynth["prior_lower"], gsynth["prior_upper"], 0b111100)
    h.set_dataset(0, x, y, yerr)
    r = RawSampler(8, 1, 6, 1, target=0, handle=h)
    L, sp = r.L, r.sp
    for bad in ([(5, 1.0, 0.0, 0.0)], [(-1, 1.0, 0.0, 0.0)], [(DE, 0.0, 0.0, 1e-5)], [(DE, -1.0, 0.0, 1e-5)],
                [(DE, np.nan, 0.0, 1e-5)], [(DE, np.inf, 0.0, 1e-5)], [(STRETCH, 1.0, 1.0, 0.0)], [(STRETCH, 1.0, np.nan, 0.0)],
                [(DE, 1.0, -0.1, 1e-5)], [(DE, 1.0, 0.0, 0.6)], [(DE, 1.0, 0.0, -1e-3)], [(DE, 1.0, 0.0, np.nan)],
                [(SNOOKER, 1.0, 0.0, 0.0)], [(SNOOKER, 1.0, -1.7, 0.0)], [(SNOOKER, 1.0, np.inf, 0.0)], [DE_DEFAULT] * 9):
        assert r.set_moves(bad, check=False) == _capi.MP_EINVAL, bad
    k, w, p = table_args([DE_DEFAULT])
    assert L.mp_sampler_set_moves(sp, 1, None, dp(w), dp(p)) == _capi.MP_EINVAL
    assert L.mp_sampler_set_moves(sp, -1, None, None, None) == _capi.MP_EINVAL
    # n_half: DE needs 2 partners, snooker 3 (8 walkers: n_half = 4; 4 walkers: 2; 2 walkers: 1)
    for nw, de_ok, sn_ok in ((8, True, True), (4, True, False), (2, False, False)):
        with RawSampler(nw, 1, 6, 1, target=0, handle=h) as s2:
            assert (s2.set_moves([DE_DEFAULT], check=False) == _capi.MP_OK) == de_ok, nw
            assert (s2.set_moves([SNOOKER_DEFAULT], check=False) == _capi.MP_OK) == sn_ok, nw
    r.set_positions(np.array(TRUTHS["Humped"]) + 1.0e-3 * np.random.default_rng(0).standard_normal((8, 6)))
    r.set_moves(TABLES["de_snooker"])
    r.run(3, store=False)
    # the walker-sharded entry points refuse a move table
    rows = C.c_void_p(1)
    assert L.mp_sampler_halfstep_shard(sp, 0, 0, 1, rows, None) == _capi.MP_ESTATE
    assert L.mp_sampler_halfstep_apply(sp, 0, rows, None, None, None) == _capi.MP_ESTATE
    assert L.mp_sampler_step_shard(sp, 0, 1, rows, None) == _capi.MP_ESTATE
    assert L.mp_sampler_step_apply(sp, rows, None, None, None) == _capi.MP_ESTATE
    # n_moves = 0 restores the default between runs: the sharded entries work again
    assert L.mp_sampler_set_moves(sp, 0, None, None, None) == _capi.MP_OK
    assert L.mp_sampler_run(sp, 2, None, None) == _capi.MP_OK
    assert L.mp_sampler_n_slots(sp) == 4
    r.close()
    h.close()
    from magprop_amd import DEMove
    from magprop_amd.distributed import DistributedEnsembleSampler, HipShardEngine
    s = EnsembleSampler(8, 6, x, y, yerr, moves=DEMove())
    with pytest.raises(ValueError, match="moves"):
        DistributedEnsembleSampler(HipShardEngine(s, "cuda:0"))
    s.close()
