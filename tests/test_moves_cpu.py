"""CPU checks of the proposal moves (include/magprop_amd.h mp_sampler_set_moves): the numpy restatement samples a correlated
Gaussian with every move, the mixture rule, the restated step loop (tests/sampler_restated.py) against the stretch oracle and
against itself (betas of 1, continued runs, swap counts), the parsing of emcee's moves= forms, and the argument checks of the
library."""
import ctypes as C
import types

import numpy as np
import pytest

from moves_restated import DE, SNOOKER, STRETCH, correlated_gaussian, draw_move, pick_skip, pick_skip2
from oracle.stretch_oracle import gaussian_lnprob
from sampler_restated import run

RHO = 0.9
# 32 walkers x 1 500 steps, the first 300 discarded: ~40 000 draws at tau ~ 20-40 steps.  Mean within 0.1, variance within
# 10 %, correlation within 0.03 (the restatement's DE / snooker / mixture runs land within 0.04 of the variance)
MEAN_TOL, VAR_TOL, CORR_TOL = 0.1, 0.1, 0.03
DE_DEFAULT = (DE, 1.0, 0.0, 1.0e-5)
SNOOKER_DEFAULT = (SNOOKER, 1.0, 1.7, 0.0)


def _moments(table, seed, zero_hastings=False):
    rng = np.random.default_rng(seed)
    pos = rng.normal(size=(32, 2))
    r = run(pos, 1500, 7000 + seed, table, lnprob_fn=correlated_gaussian(RHO), zero_hastings=zero_hastings)
    x = r.chain[300:].reshape(-1, 2)
    assert 0.1 < r.acc.mean() / 1500 < 0.9
    return x.mean(axis=0), x.var(axis=0), np.corrcoef(x.T)[0, 1]


def _within(m, v, c):
    return bool(np.all(np.abs(m) < MEAN_TOL) and np.all(np.abs(v - 1.0) < VAR_TOL) and abs(c - RHO) < CORR_TOL)


@pytest.mark.parametrize("name,table", [
    ("de", [DE_DEFAULT]),
    ("snooker", [SNOOKER_DEFAULT]),
    ("mixture", [(DE, 0.8, 0.0, 1.0e-5), (SNOOKER, 0.2, 1.7, 0.0)]),
])
def test_restated_moves_sample_a_correlated_gaussian(name, table):
    m, v, c = _moments(table, 5)
    assert _within(m, v, c), (name, m, v, c)


def test_snooker_without_its_hastings_term_fails_the_same_check():
    """The check has power: the snooker move with h = 0 samples a narrower distribution (variance ~0.66 here)."""
    m, v, c = _moments([SNOOKER_DEFAULT], 5, zero_hastings=True)
    assert not _within(m, v, c), (m, v, c)
    assert np.all(v < 1.0 - 2 * VAR_TOL), v


def test_mixture_rule_picks_moves_at_their_weights():
    n = 20000
    for weights in ((0.8, 0.2), (1.0, 2.0, 5.0)):
        cum = list(np.cumsum(weights))
        got = np.bincount([draw_move(42, s, cum) for s in range(n)], minlength=len(weights))
        p = np.asarray(weights) / sum(weights)
        assert np.all(np.abs(got / n - p) < 5 * np.sqrt(p * (1 - p) / n)), (weights, got)
    assert all(draw_move(42, s, [3.0]) == 0 for s in range(100))           # one move: no draw
    # the move of a step depends on (seed, step, table) only
    assert [draw_move(7, s, [0.5, 1.0]) for s in range(50, 70)] == [draw_move(7, s, [0.5, 1.0]) for s in range(50, 70)]


def test_distinct_index_draws():
    for m in (3, 4, 7):
        for c0 in range(m):
            seen = {pick_skip(u, m, c0) for u in np.linspace(0.0, 1.0 - 1e-12, 97)}
            assert seen == set(range(m)) - {c0}
            for c1 in set(range(m)) - {c0}:
                seen = {pick_skip2(u, m, c0, c1) for u in np.linspace(0.0, 1.0 - 1e-12, 97)}
                assert seen == set(range(m)) - {c0, c1}


STRETCH_TABLE = [(STRETCH, 1.0, 2.0, 0.0)]
MIXTURE = [(STRETCH, 0.4, 2.0, 0.0), (DE, 0.4, 0.0, 1.0e-5), (SNOOKER, 0.2, 1.7, 0.0)]


def _same_run(a, b, swaps=True):
    for f in ("chain", "lnp", "acc", "drawn", "accepted") + (("swaps",) if swaps else ()):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f


def test_restated_stretch_table_is_the_stretch_oracle():
    """A table of one stretch move restates oracle/stretch_oracle.run exactly (the moves= path with StretchMove)."""
    from oracle import stretch_oracle
    rng = np.random.default_rng(1)
    pos = rng.normal(size=(2 * 16, 3))
    ref = stretch_oracle.run(pos, 30, 99, a=2.0, n_ensembles=2)
    got = run(pos.copy(), 30, 99, STRETCH_TABLE, n_ensembles=2)
    for a, b in zip(ref, (got.chain, got.lnp, got.acc)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("n_ens", [1, 2])
def test_restated_loop_with_one_stretch_move_is_the_stretch_oracle(n_ens):
    """18 walkers (halves of 9: no power of two) x 1 and 2 ensembles x 3 dims x 40 steps: chain, lnprob and acceptance
    counts of the loop equal oracle/stretch_oracle.run bit for bit; the accepted mask adds up to the counts, no swaps."""
    from oracle import stretch_oracle
    pos = np.random.default_rng(2).normal(size=(n_ens * 18, 3)) * 1.5
    ref = stretch_oracle.run(pos, 40, 20261017, a=2.0, n_ensembles=n_ens)
    got = run(pos.copy(), 40, 20261017, STRETCH_TABLE, n_ensembles=n_ens)
    for a, b in zip(ref, (got.chain, got.lnp, got.acc)):
        assert np.array_equal(a, b)
    assert 0 < got.acc.sum() < 40 * n_ens * 18
    assert np.array_equal(got.accepted.sum(axis=0), got.acc) and np.all(got.drawn == 0) and got.swaps.shape == (0, 0)


def test_betas_of_one_without_swaps_equal_the_untempered_loop():
    """The decision (h + b lnp(q)) - b lnp(x) at b = 1 is the untempered one: betas all 1.0 with n_temps=0 equal betas=None bit
    for bit on the stretch + DE + snooker mixture, 16 walkers x 2 ensembles x 3 dims x 60 steps."""
    pos = np.random.default_rng(3).normal(size=(2 * 16, 3)) * 1.5
    plain = run(pos.copy(), 60, 5, MIXTURE, n_ensembles=2)
    ones = run(pos.copy(), 60, 5, MIXTURE, n_ensembles=2, betas=[1.0, 1.0], n_temps=0)
    _same_run(plain, ones)
    assert len(set(plain.drawn)) == 3 and 0 < plain.acc.sum() < 60 * 32         # every move was drawn, proposals both ways


@pytest.mark.parametrize("tempered", [False, True])
def test_continued_run_equals_one_run(tempered):
    """50 steps equal 20 + 30 continued through step0 / lnp / acc (16 walkers x 3 ensembles x 3 dims, the mixture; tempered:
    ladder (1, 0.5, 0.2) with its swap sweep, whose counts add up over the two calls)."""
    kw = dict(n_ensembles=3, betas=[1.0, 0.5, 0.2], n_temps=3) if tempered else dict(n_ensembles=3)
    pos = np.random.default_rng(4).normal(size=(3 * 16, 3)) * 1.5
    whole = run(pos.copy(), 50, 11, MIXTURE, **kw)
    p = pos.copy()
    first = run(p, 20, 11, MIXTURE, **kw)
    rest = run(p, 30, 11, MIXTURE, step0=20, lnp=first.lnp[-1].copy(), acc=first.acc, **kw)
    for f in ("chain", "lnp", "drawn", "accepted"):
        assert np.array_equal(np.concatenate([getattr(first, f), getattr(rest, f)]), getattr(whole, f)), f
    assert np.array_equal(rest.acc, whole.acc) and np.array_equal(first.swaps + rest.swaps, whole.swaps)
    assert np.array_equal(p, whole.chain[-1])
    assert (whole.swaps.sum() > 0) == tempered


def test_swap_counts_on_the_ladder_case():
    """The case of tests/test_gpu_tempering.py (ladder (1, 0.5, 0.2, 0.05), 16 walkers each, 3 dims, 200 steps, seed 20261015):
    swaps are both accepted and refused, between every pair of neighbours, and every stored lnprob is that of its stored
    position, so a swap moved both."""
    betas = (1.0, 0.5, 0.2, 0.05)
    pos = np.random.default_rng(12).normal(size=(4 * 16, 3)) * 1.5
    r = run(pos.copy(), 200, 20261015, STRETCH_TABLE, n_ensembles=4, betas=[betas[e % 4] for e in range(4)], n_temps=4)
    assert r.swaps.shape == (1, 3) and np.all(r.swaps > 0)
    assert 0 < r.swaps.sum() < 200 * 16 * 3
    want = np.array([[gaussian_lnprob(x) for x in row] for row in r.chain])
    assert np.array_equal(r.lnp, want)


def test_parse_emcee_move_forms():
    from magprop_amd import DEMove, DESnookerMove, StretchMove, moves
    de, sn = DEMove(), DESnookerMove()
    assert moves.parse_moves(de) == [(de, 1.0)]
    assert moves.parse_moves([de, sn]) == [(de, 1.0), (sn, 1.0)]
    assert moves.parse_moves([(de, 0.8), (sn, 0.2)]) == [(de, 0.8), (sn, 0.2)]
    kinds, weights, params = moves.move_table([(StretchMove(1.5), 1), (DEMove(sigma=0.1, gamma0=0.5), 2), (sn, 3)], 6)
    assert kinds == [0, 1, 2] and weights == [1.0, 2.0, 3.0]
    assert params == [(1.5, 0.0), (0.5, 0.1), (1.7, 0.0)]
    assert moves.move_table(DEMove(), 6)[2] == [(0.0, 1.0e-5)]              # gamma0=None: the library's 2.38 / sqrt(2 ndim)
    assert (StretchMove().a, DEMove().sigma, DEMove().gamma0, DESnookerMove().gammas) == (2.0, 1.0e-5, None, 1.7)
    assert moves.parse_spec("de:0.8,snooker:0.2") == [(DEMove(), 0.8), (DESnookerMove(), 0.2)]
    assert moves.parse_spec("stretch") == [(StretchMove(), 1.0)]
    for bad in ([], [(de, 0.0)], [(de, float("nan"))], [(de, -1.0)], [("de", 1.0)], 3, [de, (sn, 1.0)], [de] * 9):
        with pytest.raises(ValueError):
            moves.parse_moves(bad)
    for ctor in (lambda: StretchMove(1.0), lambda: DEMove(sigma=0.6), lambda: DEMove(sigma=-1e-3), lambda: DEMove(gamma0=0.0),
                 lambda: DESnookerMove(0.0), lambda: moves.parse_spec("walk:1")):
        with pytest.raises(ValueError):
            ctor()


def test_sampler_refuses_moves_with_a_non_default_scale():
    from magprop_amd import DEMove, EnsembleSampler
    with pytest.raises(ValueError, match="StretchMove"):
        EnsembleSampler(32, 3, target="gaussian", a=3.0, moves=DEMove())


def test_distributed_sampler_refuses_moves():
    from magprop_amd import DEMove
    from magprop_amd.distributed import DistributedEnsembleSampler
    eng = types.SimpleNamespace(s=types.SimpleNamespace(betas=None, moves=[(DEMove(), 1.0)]))
    with pytest.raises(ValueError, match="moves"):
        DistributedEnsembleSampler(eng)


def test_set_moves_argument_checks_on_the_built_library():
    from magprop_amd import _capi
    L = _capi.lib()
    k = (C.c_int32 * 1)(1)
    w = (C.c_double * 1)(1.0)
    p = (C.c_double * 2)(0.0, 1e-5)
    assert L.mp_sampler_set_moves(None, 1, k, w, p) == _capi.MP_EINVAL
    assert L.mp_sampler_set_moves(None, 0, None, None, None) == _capi.MP_EINVAL
    assert "mp_sampler_set_moves" in _capi.last_error()
