"""CPU checks of the proposal moves (include/magprop_amd.h mp_sampler_set_moves): the numpy restatement samples a correlated
Gaussian with every move, the mixture rule, the parsing of emcee's moves= forms, and the argument checks of the library."""
import ctypes as C
import types

import numpy as np
import pytest

from moves_restated import DE, SNOOKER, STRETCH, correlated_gaussian, draw_move, pick_skip, pick_skip2, run

RHO = 0.9
# 32 walkers x 1 500 steps, the first 300 discarded: ~40 000 draws at tau ~ 20-40 steps.  Mean within 0.1, variance within
# 10 %, correlation within 0.03 (the restatement's DE / snooker / mixture runs land within 0.04 of the variance)
MEAN_TOL, VAR_TOL, CORR_TOL = 0.1, 0.1, 0.03
DE_DEFAULT = (DE, 1.0, 0.0, 1.0e-5)
SNOOKER_DEFAULT = (SNOOKER, 1.0, 1.7, 0.0)


def _moments(table, seed, zero_hastings=False):
    rng = np.random.default_rng(seed)
    pos = rng.normal(size=(32, 2))
    chain, _, acc, _ = run(pos, 1500, 7000 + seed, table, lnprob_fn=correlated_gaussian(RHO), zero_hastings=zero_hastings)
    x = chain[300:].reshape(-1, 2)
    assert 0.1 < acc.mean() / 1500 < 0.9
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


def test_restated_stretch_table_is_the_stretch_oracle():
    """A table of one stretch move restates oracle/stretch_oracle.run exactly (the moves= path with StretchMove)."""
    from oracle import stretch_oracle
    rng = np.random.default_rng(1)
    pos = rng.normal(size=(2 * 16, 3))
    ref = stretch_oracle.run(pos, 30, 99, a=2.0, n_ensembles=2)
    got = run(pos.copy(), 30, 99, [(STRETCH, 1.0, 2.0, 0.0)], n_ensembles=2)
    for a, b in zip(ref, got[:3]):
        assert np.array_equal(a, b)


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
