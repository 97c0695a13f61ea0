"""CPU tests of the evaluate= hook of the restated sampler step (tests/sampler_restated.py): with the proposals of a half-step
evaluated in ONE call, the loop gives the bits of the serial loop -- for every move table of the GPU move tests, tempered and
untempered, with an evaluator that answers -inf, NaN and failing statuses on a fixed subset of rows, and with a KDE move whose
other half is degenerate -- and its bad log and counters say what happened.  The launch rule the GPU tests restate
(stretch_class) is checked against launch_class at the thresholds."""
import numpy as np
import pytest

import sampler_restated as sr
from kde_restated import KDE
from oracle.stretch_oracle import gaussian_lnprob
from test_gpu_moves import TABLES as MOVE_TABLES
from test_gpu_moves_kde import TABLES as KDE_TABLES

TABLES = {**MOVE_TABLES, **KDE_TABLES, "stretch": [(0, 1.0, 2.0, 0.0)]}
LADDER = (1.0, 0.3)


def _start(n_ens, nw, ndim, seed):
    return np.random.default_rng(seed).normal(size=(n_ens * nw, ndim)) * 1.5


def _marked(q):
    """A fixed subset of rows, by the bits of the first coordinate: 0 none, 1 -inf / flag, 2 NaN / non-finite, 3 -inf / prior."""
    with np.errstate(invalid="ignore"):
        v = int(np.float64(q[0]).view(np.uint64)) % 11
    return v if v in (1, 2, 3) else 0


def _faulty_fn(q):
    return {0: gaussian_lnprob(q), 1: -np.inf, 2: np.nan, 3: -np.inf}[_marked(q)]


def _evaluator(fn, calls, status_of=lambda q: 0):
    def evaluate(rows, walkers):
        assert rows.ndim == 2 and len(rows) == len(walkers) and not np.isnan(rows).any()
        calls.append(np.array(walkers))
        return np.array([fn(q) for q in rows]), np.array([status_of(q) for q in rows])
    return evaluate


def _assert_same(a, b):
    for x, y in zip(a[:6], b[:6]):
        assert np.array_equal(x, y, equal_nan=True)


@pytest.mark.parametrize("tempered", [False, True])
@pytest.mark.parametrize("name", list(TABLES))
def test_one_call_per_half_step_gives_the_bits_of_the_serial_loop(name, tempered):
    """(a) the Gaussian through evaluate=; (b) the same with rows that come back -inf, NaN and with failing statuses."""
    table, seed, n_ens, nw, steps = TABLES[name], 20261201, 4, 16, 12
    kw = dict(n_ensembles=n_ens, step0=3)
    if tempered:
        kw.update(betas=[LADDER[e % 2] for e in range(n_ens)], n_temps=2)
    pos = _start(n_ens, nw, 3, 5)
    for fn in (gaussian_lnprob, _faulty_fn):
        want = sr.run(pos.copy(), steps, seed, table, lnprob_fn=fn, **kw)
        calls = []
        lnp0 = np.array([fn(p) for p in pos])
        got = sr.run(pos.copy(), steps, seed, table, lnp=lnp0, evaluate=_evaluator(fn, calls, _marked if fn is _faulty_fn else lambda q: 0),
                     box=(np.full(3, -2.0), np.full(3, 2.0)), **kw)
        _assert_same(got, want)
        assert want.bad is None and want.counts is None
        assert len(calls) == 2 * steps and all(len(set(c)) == len(c) == n_ens * nw // 2 for c in calls)
        c = got.counts
        assert np.array_equal(c["accepted"], got.accepted.reshape(steps, n_ens, nw).sum(axis=(0, 2)))
        assert np.all(c["accepted"] + c["rejected"] + c["unevaluated"] == steps * nw) and np.all(c["unevaluated"] == 0)
        assert c["outside"].sum() > 0
        if fn is _faulty_fn:      # the bad log: the rows of status 1 and 2, in the order of the decisions
            assert len(got.bad) > 0 and all(_marked(q) in (1, 2) for q in got.bad)
        else:
            assert len(got.bad) == 0
        if tempered:
            assert np.array_equal(got.swaps + c["swap_refused"], np.full((2, 1), steps * nw))
    # without lnp= the start is one more call, over every walker
    calls = []
    got = sr.run(pos.copy(), 2, seed, table, evaluate=_evaluator(gaussian_lnprob, calls), **kw)
    _assert_same(got, sr.run(pos.copy(), 2, seed, table, **kw))
    assert len(calls) == 5 and np.array_equal(calls[0], np.arange(n_ens * nw))


def test_a_degenerate_other_half_under_kde_is_not_evaluated():
    """(c) every walker of ensemble 1 shares a coordinate: its covariance is singular, its proposals are NaN, none reaches the
    evaluator and none is accepted; ensemble 0 runs as ever."""
    table, seed, nw = [(KDE, 1.0, 0.0, 0.0)], 13, 16
    pos = _start(2, nw, 3, 9)
    pos[nw:, 1] = 0.5
    want = sr.run(pos.copy(), 5, seed, table, n_ensembles=2)
    calls = []
    got = sr.run(pos.copy(), 5, seed, table, n_ensembles=2, evaluate=_evaluator(gaussian_lnprob, calls))
    _assert_same(got, want)
    assert all(np.all(c < nw) for c in calls[1:]) and len(calls) == 11
    assert got.counts["unevaluated"].tolist() == [0, 5 * nw] and np.all(got.acc[nw:] == 0) and got.acc[:nw].sum() > 0
    assert np.array_equal(got.chain[:, nw:], np.broadcast_to(pos[nw:], (5, nw, 3)))


@pytest.mark.parametrize("waves", [1, 4])
def test_the_kernel_order_of_the_kde_sums_is_the_slot_order_to_rounding(waves):
    """kde_restated.kernel_sum against an exact sum, at sizes below, at and beyond a workgroup's threads; fit(waves=) against
    the slot-order fit to rounding; normals_batch with numpy's functions against normals(); and a run with kde_device= made of
    numpy's functions decides as the plain run does."""
    import math

    import kde_restated as kr
    rng = np.random.default_rng(waves)
    for n in (1, 63, 64 * waves, 64 * waves + 1, 1000):
        x = rng.normal(size=(n, 3)) * 1.0e3
        got = kr.kernel_sum(x, waves)
        want = np.array([math.fsum(x[:, a]) for a in range(3)])
        assert np.all(np.abs(got - want) <= 64 * np.spacing(np.abs(x).sum(axis=0))), n
    ints = rng.integers(-1000, 1000, size=(777, 2, 2)).astype(float)       # (exact in any order)
    assert np.array_equal(kr.kernel_sum(ints, waves), ints.sum(axis=0))
    x = rng.normal(size=(300, 3))
    (sa, La), (sb, Lb) = kr.fit(x, 0.5), kr.fit(x, 0.5, waves)
    assert np.allclose(sa, sb, rtol=1e-13, atol=0.0) and np.allclose(La, Lb, rtol=1e-12, atol=1e-15)

    class Numpy:
        log, sqrt, cos, sin = (staticmethod(f) for f in (np.log, np.sqrt, np.cos, np.sin))
    nb = kr.normals_batch(5, 3, 1, [7, 9], 3, Numpy)
    assert np.allclose(nb, [kr.normals(5, 3, 1, k, 3) for k in (7, 9)], rtol=1e-14, atol=1e-16)
    pos = _start(2, 16, 3, 9)
    table = [(KDE, 1.0, 0.0, 0.0)]
    want = sr.run(pos.copy(), 6, 13, table, n_ensembles=2)
    got = sr.run(pos.copy(), 6, 13, table, n_ensembles=2, evaluate=_evaluator(gaussian_lnprob, []), kde_device=(waves, Numpy))
    assert np.array_equal(got.accepted, want.accepted) and np.allclose(got.chain, want.chain, rtol=1e-12, atol=1e-12)


def test_the_libm_probe_library_is_separate():
    """After a build libmp_probe_libm.so exports mpl_libm and nothing of the product; libmagprop_amd.so, the ABI's binding and the
    header do not name it."""
    import os

    from magprop_amd import _capi
    from test_math_cpu import ROOT, _exports
    pkg = os.path.dirname(os.path.abspath(_capi.__file__))
    probe = _exports(os.path.join(pkg, "libmp_probe_libm.so"))
    assert {s for s in probe if s.startswith("mpl_")} == {"mpl_libm"} and not {s for s in probe if s.startswith("mp_")}
    assert not {s for s in _exports(os.path.join(pkg, "libmagprop_amd.so")) if s.startswith("mpl_")}
    assert not [n for n in _capi.EXPORTS if n.startswith("mpl_")]
    assert "mpl_" not in open(os.path.join(ROOT, "include", "magprop_amd.h")).read()


def test_stretch_class_restates_the_launch_rule_at_its_thresholds():
    from test_gpu_sampler_posterior import stretch_class
    from test_gpu_nested import launch_class
    ns = 1024
    for n_slots, half, whole in ((1, (4, 1, 1), (4, 1, 1)), (85, (4, 1, 1), (4, 1, 1)), (86, (4, 1, 1), (4, 1, 2)),
                                 (170, (4, 1, 1), (4, 1, 2)), (171, (1, 4, 1), (1, 4, 1)), (341, (1, 4, 1), (1, 4, 1)),
                                 (342, (1, 4, 1), (1, 2, 2)), (810, (1, 4, 1), (1, 2, 2)), (1024, (1, 4, 1), None),
                                 (1025, (1, 2, 2), None)):
        assert stretch_class(n_slots, n_slots, ns) == half, n_slots
        if whole is not None:
            assert stretch_class(3 * n_slots, n_slots, ns) == whole, n_slots
    # where the launch is as large as the whole step the rule is launch_lnprob's
    for n in (1, 256, 257, 512, 513, 1024, 1025):
        assert stretch_class(3 * n, n, ns) == launch_class(3 * n, ns)
