"""CPU checks of the ensemble slice-sampling move (include/magprop_amd.h MP_MOVE_SLICE): the numpy restatement
(tests/slice_move_restated.py) samples the correlated Gaussian of tests/test_moves_cpu.py and fails to without the level's
ln u, its autocorrelation time against the restated stretch chain, split runs across the tuning boundary, SliceMove's
arguments and table codes, the header's constants and the argument checks of the library."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

import sampler_restated
import slice_move_restated as sm
from conftest import ROOT
from magprop_amd import SliceMove
from moves_restated import DE, STRETCH, correlated_gaussian
from test_moves_cpu import RHO, _within

SLICE_DEFAULT = [(sm.SLICE, 1.0, 1.0, 100.0)]


def _chain(seed, drop_lnu=False):
    """The case of test_moves_cpu._moments: 32 walkers x 1 500 steps from a unit normal ball, generator seed `seed`, sampler seed
    7000 + seed."""
    pos = np.random.default_rng(seed).normal(size=(32, 2))
    return sm.run(pos, 1500, 7000 + seed, SLICE_DEFAULT, lnprob_fn=correlated_gaussian(RHO), drop_lnu=drop_lnu)


def _moments(r):
    x = r.chain[300:].reshape(-1, 2)
    return x.mean(axis=0), x.var(axis=0), np.corrcoef(x.T)[0, 1]


@pytest.fixture(scope="module")
def slice_chain():
    return _chain(5)


def test_restated_slice_move_samples_a_correlated_gaussian(slice_chain):
    m, v, c = _moments(slice_chain)
    print(f"slice: mean {m}, var {v}, corr {c:.4f}, mu {slice_chain.mu[-1]}, failed slices {slice_chain.state.nfail}")
    assert _within(m, v, c), (m, v, c)
    assert np.all(slice_chain.acc == 1500) and np.all(slice_chain.state.nfail == 0)      # every update moved its walker


def test_slice_move_without_ln_u_fails_the_same_check():
    """The check has power: with the level at the walker's own lnprob (lny = lnp_x) only points of higher density are inside,
    the ensemble climbs to the mode and both variances collapse."""
    m, v, c = _moments(_chain(5, drop_lnu=True))
    assert not _within(m, v, c), (m, v, c)
    assert np.all(v < 0.5), v


def test_slice_chain_decorrelates_faster_than_the_stretch_chain(slice_chain):
    """The integrated autocorrelation time of the slice chain lies below that of the restated stretch chain of the same sizes
    (which pays one evaluation per walker and step, the slice move several)."""
    pos = np.random.default_rng(5).normal(size=(32, 2))
    st = sampler_restated.run(pos, 1500, 7005, [(STRETCH, 1.0, 2.0, 0.0)], lnprob_fn=correlated_gaussian(RHO))
    tau_slice = max(sm.autocorr_time(slice_chain.chain[300:, :, d]) for d in range(2))
    tau_stretch = max(sm.autocorr_time(st.chain[300:, :, d]) for d in range(2))
    evals = slice_chain.state.neval[0] / (1500 * 32)
    print(f"tau: slice {tau_slice:.2f} steps at {evals:.2f} evaluations per walker and step, stretch {tau_stretch:.2f} steps at 1")
    assert tau_slice < tau_stretch


def _same(whole, first, rest):
    for f in ("chain", "lnp", "drawn", "mu"):
        assert np.array_equal(np.concatenate([getattr(first, f), getattr(rest, f)]), getattr(whole, f)), f
    assert np.array_equal(rest.acc, whole.acc) and np.array_equal(first.swaps + rest.swaps, whole.swaps)
    a, b = rest.state.counters(), whole.state.counters()
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(rest.state.mu, whole.state.mu)


@pytest.mark.parametrize("n_ens,ladder", [(1, None), (3, None), (3, (1.0, 0.5, 0.2))])
def test_continued_run_equals_one_run_across_the_tuning_boundary(n_ens, ladder):
    """50 steps equal 20 + 30 continued through step0 / lnp / acc / state with tune = 25 (16 walkers per ensemble, 3 dims): chain,
    lnprob, the mu of every step, the counters and the swap counts."""
    table = [(sm.SLICE, 1.0, 0.3, 25.0)]
    kw = dict(n_ensembles=n_ens, limits=(4, 8))
    if ladder:
        kw.update(betas=list(ladder), n_temps=len(ladder))
    pos = np.random.default_rng(4).normal(size=(n_ens * 16, 3)) * 1.5
    whole = sm.run(pos.copy(), 50, 11, table, **kw)
    p = pos.copy()
    first = sm.run(p, 20, 11, table, **kw)
    rest = sm.run(p, 30, 11, table, step0=20, lnp=first.lnp[-1].copy(), acc=first.acc, state=first.state, **kw)
    _same(whole, first, rest)
    assert np.all(whole.state.n_tuned == 50)
    assert np.all(whole.mu[24] != whole.mu[23]) and np.array_equal(whole.mu[25:], np.repeat(whole.mu[24:25], 25, axis=0))
    assert np.all(whole.mu[0] != 0.3)
    assert (whole.swaps.sum() > 0) == bool(ladder)
    if ladder:
        assert len(set(whole.state.mu)) == 3            # every temperature keeps its own scale


def test_continued_mixture_equals_one_run_and_only_slice_steps_tune():
    table = [(sm.SLICE, 0.5, 1.0, 25.0), (DE, 0.5, 0.0, 1.0e-5)]
    pos = np.random.default_rng(6).normal(size=(16, 3)) * 1.5
    whole = sm.run(pos.copy(), 50, 13, table, limits=(4, 8))
    p = pos.copy()
    first = sm.run(p, 20, 13, table, limits=(4, 8))
    rest = sm.run(p, 30, 13, table, limits=(4, 8), step0=20, lnp=first.lnp[-1].copy(), acc=first.acc, state=first.state)
    _same(whole, first, rest)
    n_slice = int(np.sum(whole.drawn == 0))
    assert 10 < n_slice < 40 and whole.state.n_tuned[0] == n_slice
    de_steps = np.flatnonzero(whole.drawn == 1)
    de_steps = de_steps[de_steps > 0]
    assert np.array_equal(whole.mu[de_steps], whole.mu[de_steps - 1])           # a DE step leaves mu as it was


def test_tune_rule():
    assert sm.tune(1.0, 0, 0) == 2.0 and sm.tune(1.0, 4, 4) == 1.0 and sm.tune(3.0, 1, 5) == 3.0 * (2.0 / 6.0)
    assert sm.tune(0.7, 3, 0) == 0.7 * 2.0


def test_slice_move_arguments_and_table():
    from magprop_amd import DEMove, moves
    s = SliceMove()
    assert (s.mu, s.tune, s.max_steps_out, s.max_shrink) == (1.0, 100, 32, 64)
    assert s.kind == 4 and s.params(6) == (1.0, 100.0) and s.limits() == (32, 64)
    assert repr(s) == "SliceMove(mu=1.0, tune=100, max_steps_out=32, max_shrink=64)"
    assert s == SliceMove(mu=1, tune=100) and s != SliceMove(mu=2.0) and s != SliceMove(max_shrink=8) and s != DEMove()
    assert hash(s) == hash(SliceMove())
    assert moves.parse_moves(s) == [(s, 1.0)]
    assert moves.move_table([(SliceMove(0.5, 10), 1), (DEMove(), 3)], 6) == ([4, 1], [1.0, 3.0], [(0.5, 10.0), (0.0, 1.0e-5)])
    assert moves.parse_spec("slice:0.5,de:0.5") == [(SliceMove(), 0.5), (DEMove(), 0.5)]
    assert moves.parse_spec("slice") == [(SliceMove(), 1.0)]
    assert moves.slice_move(moves.parse_moves([DEMove(), s])) is s and moves.slice_move(moves.parse_moves(DEMove())) is None
    with pytest.raises(ValueError, match="one SliceMove"):
        moves.parse_moves([s, SliceMove(2.0)])
    for kw in (dict(mu=0.0), dict(mu=-1.0), dict(mu=float("inf")), dict(mu=float("nan")), dict(tune=-1), dict(tune=1.5),
               dict(tune=2 ** 31), dict(max_steps_out=0), dict(max_steps_out=4097), dict(max_shrink=0), dict(max_shrink=253),
               dict(max_shrink=2.5)):
        with pytest.raises(ValueError, match="SliceMove"):
            SliceMove(**kw)
    assert SliceMove(tune=0).tune == 0 and SliceMove(tune=2 ** 31 - 1).tune == 2 ** 31 - 1 and SliceMove(max_shrink=252).max_shrink == 252


def test_distributed_sampler_refuses_a_slice_table():
    from magprop_amd.distributed import DistributedEnsembleSampler
    eng = types.SimpleNamespace(s=types.SimpleNamespace(betas=None, moves=[(SliceMove(), 1.0)]))
    with pytest.raises(ValueError, match="moves"):
        DistributedEnsembleSampler(eng)


def test_python_mirror_follows_the_header():
    from magprop_amd import _capi, moves
    hdr = open(os.path.join(ROOT, "include", "magprop_amd.h")).read()

    def define(name):
        return int(re.search(r"#define\s+%s\s+(\d+)" % name, hdr).group(1))

    assert define("MP_MOVE_SLICE") == _capi.MOVE_SLICE == moves.MOVE_SLICE == sm.SLICE == 4
    assert define("MP_SLICE_MAX_SHRINK") == _capi.SLICE_MAX_SHRINK == moves.SLICE_MAX_SHRINK == 252
    assert define("MP_NEST_MAX_STEPS_OUT") == moves.SLICE_MAX_STEPS_OUT
    assert "0x51C00000" in hdr and sm.SLICE_CTR == 0x51C00000


def test_argument_checks_on_the_built_library():
    from magprop_amd import _capi
    L = _capi.lib()
    k = (C.c_int32 * 1)(4)
    w = (C.c_double * 1)(1.0)
    p = (C.c_double * 2)(1.0, 100.0)
    assert L.mp_sampler_set_moves(None, 1, k, w, p) == _capi.MP_EINVAL
    assert L.mp_sampler_set_slice_limits(None, 32, 64) == _capi.MP_EINVAL
    assert "mp_sampler_set_slice_limits" in _capi.last_error()
    assert L.mp_sampler_get_slice(None, None, None, None, None, None, None) == _capi.MP_EINVAL
    assert "mp_sampler_get_slice" in _capi.last_error()
