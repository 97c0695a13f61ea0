"""GPU tests of the KDE move of the device-resident sampler (include/magprop_amd.h MP_MOVE_KDE): device chains against the numpy
restatement (tests/sampler_restated.py) on the unit-Gaussian target -- team and one-wavefront builds, tempered, mixtures, split
runs --, moments, a Humped posterior run, argument codes and a degenerate other half."""
import ctypes as C

import numpy as np
import pytest

from conftest import TRUTHS
from kde_restated import KDE
from moves_restated import DE, STRETCH
from raw_abi import RawSampler, gaussian_run, synth_handle
from sampler_restated import run as restate

pytestmark = pytest.mark.gpu

# The kernel sums over the other half in an order of its own and its log / exp / sqrt / cos / sin are not numpy's: the chains
# agree to rounding (absolute for coordinates of order 1), with identical decisions
RTOL, ATOL = 1e-12, 1e-12
KDE_SCOTT = (KDE, 1.0, 0.0, 0.0)
TABLES = {
    "kde": [KDE_SCOTT],
    "kde_silverman": [(KDE, 1.0, -1.0, 0.0)],
    "kde_stretch": [(KDE, 0.5, 0.0, 0.0), (STRETCH, 0.5, 2.0, 0.0)],
    "kde_de": [(KDE, 0.8, 0.5, 0.0), (DE, 0.2, 0.0, 1.0e-5)],
}


def _moved(chain, pos0):
    """accepted[s, k] of an untempered chain: the walker's row changed (a proposal equals the old position with probability 0)."""
    prev = np.concatenate([pos0[None], chain[:-1]])
    return np.any(chain != prev, axis=2)


def _assert_agrees(got, ref, pos0, tempered=False):
    chain, lnp, acc = got
    assert np.array_equal(acc, ref.acc)
    if not tempered:
        assert np.array_equal(_moved(chain, pos0), ref.accepted)
    assert np.all(np.isfinite(chain)) and np.all(np.isfinite(lnp))
    assert np.allclose(chain, ref.chain, rtol=RTOL, atol=ATOL), np.abs(chain - ref.chain).max()
    assert np.allclose(lnp, ref.lnp, rtol=RTOL, atol=ATOL), np.abs(lnp - ref.lnp).max()


@pytest.mark.parametrize("name", list(TABLES))
def test_gaussian_chain_matches_the_restatement_on_the_team_builds(name):
    """32 walkers x 2 ensembles x 3 dims x 60 steps (the team builds): decisions at every step and acceptance counts equal the
    restatement's, positions and lnprob to rounding; 25 + 35 steps equal 60."""
    table, seed = TABLES[name], 20261016
    pos = np.random.default_rng(3).normal(size=(2 * 32, 3)) * 1.5
    ref = restate(pos.copy(), 60, seed, table, n_ensembles=2)
    if len(table) > 1:
        assert 0 < np.count_nonzero(ref.drawn == 0) < 60               # both moves were drawn
    assert 0 < ref.acc.sum() < 60 * 64
    _assert_agrees(gaussian_run(32, 2, 3, seed, table, pos, (60,)), ref, pos)
    _assert_agrees(gaussian_run(32, 2, 3, seed, table, pos, (25, 35)), ref, pos)


@pytest.mark.parametrize("name", ["kde", "kde_de"])
def test_gaussian_chain_matches_the_restatement_on_the_one_wave_builds(name):
    """2 048 walkers x 2 dims x 8 steps: the one-wavefront half-step builds, 1 024 points in every density sum."""
    table, seed = TABLES[name], 77
    pos = np.random.default_rng(4).normal(size=(2048, 2))
    ref = restate(pos.copy(), 8, seed, table)
    _assert_agrees(gaussian_run(2048, 1, 2, seed, table, pos, (8,)), ref, pos)


def test_tempered_gaussian_chain_matches_the_restatement():
    """Ladder (1, 0.5, 0.25), 24 walkers x 3 dims x 40 steps, KDE + stretch: decisions against beta and the swap sweep."""
    table, seed, betas = TABLES["kde_stretch"], 5, (1.0, 0.5, 0.25)
    pos = np.random.default_rng(6).normal(size=(3 * 24, 3))
    ref = restate(pos.copy(), 40, seed, table, n_ensembles=3, betas=betas, n_temps=3)
    _assert_agrees(gaussian_run(24, 3, 3, seed, table, pos, (40,), betas=betas), ref, pos, tempered=True)


def test_gaussian_target_statistics_with_the_kde_move():
    """test_gaussian_target_statistics_per_move (tests/test_gpu_moves.py) with KDEMove: 256 walkers, 6 dims, 1 500 steps from a
    ball at 3, the first 500 discarded: mean within 0.05, variance within 0.06 of 1."""
    from magprop_amd import EnsembleSampler, KDEMove
    rng = np.random.default_rng(8)
    s = EnsembleSampler(256, 6, target="gaussian", seed=3, moves=KDEMove())
    s.run_mcmc(rng.normal(size=(256, 6)) * 0.1 + 3.0, 1500)
    tail = s.get_chain()[500:].reshape(-1, 6)
    assert np.all(np.abs(tail.mean(axis=0)) < 0.05), tail.mean(axis=0)
    assert np.all(np.abs(tail.var(axis=0) - 1.0) < 0.06), tail.var(axis=0)
    af = s.acceptance_fraction.mean()
    assert 0.05 < af < 0.98, af
    print(f"kde: acceptance {af:.3f}, tau {np.round(s.get_autocorr_time(quiet=True), 1)}")
    s.close()


def test_humped_posterior_with_the_kde_move(gsynth):
    """512 walkers x 2 000 steps from the truths with 0.8 KDE + 0.2 DE, the first 500 discarded: every truth lies inside the
    central 95 % of the chain; lnprob finite throughout."""
    from magprop_amd import DEMove, EnsembleSampler, KDEMove
    x, y, yerr = gsynth["Humped_x"], gsynth["Humped_y"], gsynth["Humped_yerr"]
    truth = np.array(TRUTHS["Humped"])
    s = EnsembleSampler(512, 6, x, y, yerr, seed=41, moves=[(KDEMove(), 0.8), (DEMove(), 0.2)])
    s.run_mcmc(truth + 1.0e-4 * np.random.default_rng(40).standard_normal((512, 6)), 2000)
    chain = s.get_chain()[500:].reshape(-1, 6)
    lo, hi = np.percentile(chain, 2.5, axis=0), np.percentile(chain, 97.5, axis=0)
    assert np.all((lo < truth) & (truth < hi)), (lo, truth, hi)
    assert np.all(np.isfinite(s.get_log_prob()))
    print(f"Humped KDE + DE: acceptance {s.acceptance_fraction.mean():.3f}, tau {np.round(s.get_autocorr_time(quiet=True), 1)}")
    s.close()


def test_set_moves_kde_argument_codes(gsynth):
    from magprop_amd import EnsembleSampler, KDEMove, _capi
    h = synth_handle()
    h.set_prior(gsynth["prior_lower"], gsynth["prior_upper"], 0b111100)
    h.set_dataset(0, gsynth["Humped_x"], gsynth["Humped_y"], gsynth["Humped_yerr"])
    r = RawSampler(16, 1, 6, 1, target=0, handle=h)
    L, sp = r.L, r.sp
    for bad in ([(KDE, 1.0, -0.5, 0.0)], [(KDE, 1.0, -2.0, 0.0)], [(KDE, 1.0, np.nan, 0.0)], [(KDE, 1.0, np.inf, 0.0)],
                [(KDE, 1.0, -np.inf, 0.0)], [(KDE, 1.0, 0.0, 1.0)], [(KDE, 1.0, 0.0, np.nan)], [(KDE, 1.0, 0.5, -1.0)],
                [(KDE, 0.0, 0.0, 0.0)], [(KDE, np.nan, 0.0, 0.0)], [(5, 1.0, 0.0, 0.0)], [(-1, 1.0, 0.0, 0.0)]):
        assert r.set_moves(bad, check=False) == _capi.MP_EINVAL, bad
    for good in ([KDE_SCOTT], [(KDE, 1.0, -1.0, 0.0)], [(KDE, 1.0, 0.7, 0.0)], TABLES["kde_de"]):
        assert r.set_moves(good, check=False) == _capi.MP_OK, good
    # n_comp = n_walkers / 2: 12 walkers give n_comp = 6 = ndim (refused), 14 walkers n_comp = 7 = ndim + 1 (accepted)
    for nw, ok in ((12, False), (14, True)):
        with RawSampler(nw, 1, 6, 1, target=0, handle=h) as s2:
            assert (s2.set_moves([KDE_SCOTT], check=False) == _capi.MP_OK) == ok, nw
    r.set_positions(np.array(TRUTHS["Humped"]) + 1.0e-3 * np.random.default_rng(0).standard_normal((16, 6)))
    r.set_moves([KDE_SCOTT])
    r.run(3, store=False)
    rows = C.c_void_p(1)
    assert L.mp_sampler_halfstep_shard(sp, 0, 0, 1, rows, None) == _capi.MP_ESTATE
    assert L.mp_sampler_step_shard(sp, 0, 1, rows, None) == _capi.MP_ESTATE
    r.close()
    h.close()
    from magprop_amd.distributed import DistributedEnsembleSampler, HipShardEngine
    s = EnsembleSampler(16, 6, gsynth["Humped_x"], gsynth["Humped_y"], gsynth["Humped_yerr"], moves=KDEMove())
    with pytest.raises(ValueError, match="moves"):
        DistributedEnsembleSampler(HipShardEngine(s, "cuda:0"))
    s.close()


@pytest.mark.parametrize("nw,n_ens,ndim", [(32, 2, 3), (2048, 1, 2)])
def test_degenerate_other_half_moves_no_walker(nw, n_ens, ndim):
    """Every walker shares one coordinate: S is singular, every KDE proposal is NaN and rejected.  The run ends MP_OK, no walker
    moves, and neither the chain nor lnprob holds a NaN."""
    pos = np.random.default_rng(9).normal(size=(nw * n_ens, ndim))
    pos[:, 1] = 0.5
    chain, lnp, acc = gaussian_run(nw, n_ens, ndim, 13, [KDE_SCOTT], pos, (5,))
    assert np.all(acc == 0)
    assert np.all(np.isfinite(chain)) and np.all(np.isfinite(lnp))
    assert np.array_equal(chain, np.broadcast_to(pos, chain.shape))
    want = -0.5 * np.sum(pos * pos, axis=1)
    assert np.allclose(lnp, want, rtol=1e-15, atol=0.0)
