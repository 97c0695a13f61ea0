"""CPU tests of the nested sampler's slice mode (include/magprop_amd.h mp_nested_set_slice): the numpy restatement of the slice
walk (tests/nest_slice_restated.py) leaves the constrained prior invariant and a broken rule does not, a restated run finds
the Gaussian evidence, ties and coinciding survivors behave as the header states, and the front end checks its arguments
before any device is touched."""
import functools
import math
import os
import re

import numpy as np
import pytest
from scipy import stats
from scipy.special import erf

import nest_restated as nr
import nest_slice_restated as sr
from conftest import ROOT
from test_nested_cpu import RecordingGaussian, assert_states_equal

LO, HI = np.array([-1.5, -0.7, -2.0]), np.array([2.0, 1.2, 0.8])
C_LEVEL = 1.5        # the region {0.5 |x|^2 < 1.5} cut by the asymmetric box LO, HI


def _region(rng, n):
    """n exact uniform draws of {0.5 |x|^2 < C_LEVEL} inside the box (rejection from the box)."""
    out = np.empty((0, LO.size))
    while out.shape[0] < n:
        P = LO + (HI - LO) * rng.random((4 * n, LO.size))
        out = np.concatenate([out, P[0.5 * np.sum(P * P, axis=1) < C_LEVEL]])
    return out[:n]


def _one_walk_each(starts, surv, seed, broken=None):
    res = [sr.slice_walk([float(v) for v in x], nr.gaussian_one(x)[0], 0, 0, 0, i, surv, -C_LEVEL, seed, 3, 1.0, 8, 64, LO, HI,
                         nr.gaussian_one, broken=broken) for i, x in enumerate(starts)]
    return np.array([r[0] for r in res]), np.array([r[3] for r in res]), np.array([r[7] for r in res])


@pytest.mark.parametrize("broken", [None, "forward"])
def test_slice_walk_leaves_the_constrained_prior_invariant(broken):
    """3 000 exact uniform draws of the region, one walk of 3 slices each (directions from 200 other exact draws, L* = -1.5):
    the end points are still uniform, |x|^2 against 200 000 exact draws by a two-sample KS test (p > 1e-3) and every coordinate
    mean within 4 standard errors.  The negative control steps out forward only (x at the left end of the interval): every
    slice still moves, but the walk is not reversible and fails the same check (p ~ 1e-50)."""
    rng = np.random.default_rng(0)
    ref = _region(rng, 200000)
    surv = _region(rng, 200)
    starts = _region(rng, 3000)
    X, moved, failed = _one_walk_each(starts, surv, 1, broken)
    assert np.all(0.5 * np.sum(X * X, axis=1) < C_LEVEL) and np.all((X >= LO) & (X <= HI))
    assert moved.sum() == 3 * len(starts) and failed.sum() == 0        # (this region is easy: every slice moves)
    p = stats.ks_2samp(np.sum(X * X, axis=1), np.sum(ref * ref, axis=1)).pvalue
    z = np.abs(X.mean(axis=0) - ref.mean(axis=0)) / (ref.std(axis=0) / math.sqrt(len(X)))
    ok = p > 1e-3 and np.all(z < 4.0)
    print(f"broken={broken}: KS p {p:.3g}, |z| of the means {np.round(z, 2)}")
    assert ok == (broken is None), (p, z)


def test_a_start_tied_with_lstar_and_coinciding_survivors():
    """A flat lnL: every point ties with L*, nothing is inside, so every slice rejects max_shrink points and fails where it
    started (no stepping out).  A Gaussian start exactly on L*: the slices run as any other and move it inside.  Coinciding
    survivors (d = 0): every slice fails at once, without an evaluation."""
    rng = np.random.default_rng(4)
    surv = _region(rng, 50)
    x0 = [0.3, -0.2, 0.5]
    flat = lambda q: (-1.0, 0)                                          # noqa: E731
    x, lnl, st, moved, n_eval, n_exp, n_con, n_fail = sr.slice_walk(list(x0), -1.0, 0, 0, 0, 0, surv, -1.0, 7, 3, 1.0, 8, 16,
                                                                    LO, HI, flat)
    assert x == x0 and lnl == -1.0 and moved == 0 and n_exp == 0
    assert n_fail == 3 and n_con == 3 * 16 and n_eval <= 3 * (16 + 2)
    lstar = nr.gaussian_one(np.array(x0))[0]
    x, lnl, st, moved, *_ = sr.slice_walk(list(x0), lstar, 0, 0, 0, 0, surv, lstar, 7, 3, 1.0, 8, 64, LO, HI, nr.gaussian_one)
    assert moved == 3 and lnl > lstar and 0.5 * sum(v * v for v in x) < 0.5 * sum(v * v for v in x0)
    same = np.tile(surv[:1], (50, 1))
    x, lnl, st, moved, n_eval, n_exp, n_con, n_fail = sr.slice_walk(list(x0), lstar, 0, 0, 0, 0, same, -10.0, 7, 3, 1.0, 8, 64,
                                                                    LO, HI, nr.gaussian_one)
    assert x == x0 and moved == 0 and n_eval == 0 and n_fail == 3 and n_con == 0


def test_restated_slice_run_finds_the_gaussian_evidence():
    """The restated slice mode (3 slices per walk) on the unit Gaussian in an asymmetric 3-d box, N = 64, K = 16: ln Z within
    3 logzerr of the closed form; the counters add up and the failed slices are counted."""
    from magprop_amd import nested
    lo, hi = np.array([-2.0, -1.0, -4.0]), np.array([3.0, 2.5, 1.5])
    nlive, nbatch, slices = 64, 16, 3
    live0 = lo + (hi - lo) * np.random.default_rng(1).random((1, nlive, 3))
    s = sr.start(live0, nr.gaussian)
    sr.run(s, 400, nbatch, 12345, slices, 1.0, 8, 64, 0.01, lo, hi, nr.gaussian_one)
    assert s.stopped[0] and s.nit[0] < 400
    e = nested.estimate(s.dead_lnl[0], s.dead_n[0], s.lnl[0], nlive)
    truth = sum(math.log(math.sqrt(math.pi / 2.0) * (erf(h / math.sqrt(2.0)) - erf(l / math.sqrt(2.0))) / (h - l))
                for l, h in zip(lo, hi))
    print(f"restated slice run: ln Z {e['logz']:.4f} +- {e['logzerr']:.4f} (truth {truth:.4f}), {s.nit[0]} iterations, "
          f"ncall {s.ncall[0]}, nexpand {s.nexpand[0]}, ncontract {s.ncontract[0]}, nfail {s.nfail[0]}")
    assert abs(e["logz"] - truth) < 3.0 * e["logzerr"], (e["logz"], truth, e["logzerr"])
    walks = nbatch * int(s.nit[0])
    assert s.nacc[0] + s.nfail[0] == slices * walks                    # every slice moves or fails
    assert 0 <= s.nfail[0] <= 0.01 * slices * walks and s.nzero[0] <= s.nfail[0]
    assert s.ncall[0] >= s.nacc[0] and s.ncontract[0] <= s.ncall[0]
    assert s.dead_lnl[0][-1] <= np.min(s.lnl[0])


def test_slice_rounds_leave_the_state_of_the_one_at_a_time_path():
    """3 runs on the unit Gaussian, N = 32, K = 8, 3 slices per walk, 6 iterations as run(2) + run(4): the round-batched driver
    and the one-at-a-time path leave identical States (the slice counters among them), and every row's run is handed through."""
    lo, hi = np.array([-2.0, -1.0, -4.0]), np.array([3.0, 2.5, 1.5])
    live0 = lo + (hi - lo) * np.random.default_rng(11).random((3, 32, 3))
    kw = dict(mu=1.0, max_steps_out=4, max_shrink=32, dlogz=1e-6, lower=lo, upper=hi)
    a = sr.start(live0, nr.gaussian)
    rec = RecordingGaussian()
    b = sr.start(live0, rec, with_runs=True)
    assert len(rec.calls) == 1 and np.array_equal(rec.calls[0][1], np.repeat(np.arange(3), 32))
    for n in (2, 4):
        sr.run(a, n, 8, 78, 3, evaluate_one=nr.gaussian_one, **kw)
        sr.run(b, n, 8, 78, 3, evaluate=rec, **kw)
    assert_states_equal(a, b, extra=("nexpand", "ncontract", "nfail"))
    assert np.all(a.nit == 6) and np.all(a.nexpand > 0) and np.all(a.ncontract > 0)
    for r in range(3):
        assert sum(int(np.sum(c[1] == r)) for c in rec.calls[1:]) == a.ncall[r]
    assert all(np.all(np.diff(c[1]) >= 0) for c in rec.calls[1:])


def test_the_round_driver_calls_evaluate_once_per_round_of_the_longest_slice_walk():
    """The slice walks of one iteration of 3 runs driven together: as many evaluate calls as the longest walk has evaluations,
    one row per walk still going, and the results of the walks driven one at a time."""
    lo, hi = np.array([-2.0, -1.0, -4.0]), np.array([3.0, 2.5, 1.5])
    live0 = lo + (hi - lo) * np.random.default_rng(12).random((3, 32, 3))
    s = sr.start(live0, nr.gaussian)
    jobs = nr.retire(s, 8, 1e-6)

    def gens():
        return [sr.slice_walk_rounds([float(v) for v in s.live[r, surv[0]]], float(s.lnl[r, surv[0]]), 0, t, r, j, s.live[r, surv],
                                     lstar, 5, 3, 1.0, 4, 32, lo, hi)
                for r, dead, surv, lstar, t in jobs for j in dead]             # (every walk from its run's first survivor)

    runs = [r for r, dead, *_ in jobs for _ in dead]
    rec = RecordingGaussian()
    out = nr.in_rounds(gens(), runs, rec)
    one = [nr.one_at_a_time(g, nr.gaussian_one) for g in gens()]
    assert len(out) == 24 and out == one
    evals = np.array([o[4] for o in out])
    assert len(rec.calls) == evals.max() and evals.min() < evals.max()
    for k, (rows, rr) in enumerate(rec.calls):
        assert len(rows) == np.sum(evals > k) and rr.tolist() == [runs[i] for i in np.nonzero(evals > k)[0]]


# ---------------------------------------------------------------- the edge paths of the slice state machine in slice mode
# One run on the unit Gaussian in the box EDGE_LO, EDGE_HI, seed EDGE_SEED, the live set from default_rng(18); the GPU tests
# (tests/test_gpu_nested_slice.py) hold the device to the same restated runs bit for bit.
EDGE_LO, EDGE_HI, EDGE_SEED = np.array([-2.0, -1.0, -4.0]), np.array([3.0, 2.5, 1.5]), 20261201
# (max_steps_out, max_shrink, mu) -> (nexpand, ncontract, nfail) over 6 iterations of N = 32, K = 8, 3 slices
TIGHT = {(1, 2, 0.05): (0, 7, 3), (1, 1, 5.0): (0, 103, 103)}


def edge_live(nlive):
    return EDGE_LO + (EDGE_HI - EDGE_LO) * np.random.default_rng(18).random((1, nlive, 3))


@functools.lru_cache(maxsize=None)
def tight_run(limits):
    """(live0, the restated state behind 6 iterations) under the tight limits `limits`; computed once, not to be changed."""
    live0 = edge_live(32)
    s = sr.start(live0, nr.gaussian)
    sr.run(s, 6, 8, EDGE_SEED, 3, mu=limits[2], max_steps_out=limits[0], max_shrink=limits[1], dlogz=0.05, lower=EDGE_LO,
           upper=EDGE_HI, evaluate_one=nr.gaussian_one)
    return live0, s


@functools.lru_cache(maxsize=None)
def coinciding_run():
    """(live0, the restated state behind 2 iterations) of N = 16, K = 8, 3 slices, limits 4 / 8, dlogz = 1e-9, where the eight
    highest-lnL points of the start set (the survivors of the first iteration) lie at one position."""
    live0 = edge_live(16)
    top = np.argsort(nr.gaussian(live0[0])[0])[8:]
    live0[0, top] = live0[0, top[-1]]
    s = sr.start(live0, nr.gaussian)
    sr.run(s, 2, 8, EDGE_SEED, 3, mu=1.0, max_steps_out=4, max_shrink=8, dlogz=1e-9, lower=EDGE_LO, upper=EDGE_HI,
           evaluate_one=nr.gaussian_one)
    return live0, s


@pytest.mark.parametrize("limits", sorted(TIGHT))
def test_tight_limits_take_the_slices_to_zero_budgets_and_the_shrink_cap(limits):
    """max_steps_out = 1 leaves both budgets 0: no slice steps out, every evaluation is a shrink point.  mu = 0.05 with 2 shrink
    points: a few slices fail at the cap.  mu = 5 with one shrink point: a slice moves at its first shrink point or fails at the
    cap behind exactly one contraction, most of them on points outside the box, which are not evaluated."""
    _, s = tight_run(limits)
    assert (int(s.nexpand[0]), int(s.ncontract[0]), int(s.nfail[0])) == TIGHT[limits]
    assert s.nit[0] == 6 and not s.stopped[0] and s.nacc[0] + s.nfail[0] == 3 * 8 * 6 and s.nfail[0] > 0
    assert s.ncall[0] <= s.nacc[0] + s.ncontract[0]            # nothing but shrink points was evaluated
    if limits[1] == 1:
        assert s.ncontract[0] == s.nfail[0] and s.ncall[0] < s.nacc[0] + s.ncontract[0]
    else:
        assert s.nfail[0] * limits[1] <= s.ncontract[0]


def test_coinciding_survivors_fail_every_slice_without_an_evaluation():
    """Every direction is zero: no point is evaluated, every slice fails where it starts, every walk ends at the survivor it
    started from, and the run is not stopped."""
    live0, s = coinciding_run()
    assert s.nfail[0] == 48 and s.ncall[0] == 0 and s.nzero[0] == 16 and s.nacc[0] == 0
    assert s.nexpand[0] == 0 and s.ncontract[0] == 0 and s.nit[0] == 2 and not s.stopped[0]
    assert np.all(s.live[0] == live0[0, np.argmax(nr.gaussian(live0[0])[0])])


@pytest.mark.parametrize("kw, match", [
    ({"sample": "rslice"}, "sample"),
    ({"sample": "slice", "slices": 0}, "slices"),
    ({"sample": "slice", "slices": 5000}, "slices"),
    ({"sample": "slice", "slices": 2.5}, "slices"),
    ({"slices": 3}, "sample='slice'"),
    ({"sample": "slice", "slice_mu": 0.0}, "slice_mu"),
    ({"sample": "slice", "slice_mu": np.inf}, "slice_mu"),
    ({"sample": "slice", "slice_mu": np.nan}, "slice_mu"),
    ({"sample": "slice", "slice_mu": "1"}, "slice_mu"),
    ({"sample": "slice", "max_steps_out": 0}, "max_steps_out"),
    ({"sample": "slice", "max_shrink": 0}, "max_shrink"),
    ({"sample": "slice", "max_shrink": 255}, "max_shrink"),
])
def test_slice_arguments_are_checked_before_any_device_is_touched(monkeypatch, kw, match):
    from magprop_amd import _capi, nested

    def no_device(*a, **k):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(_capi, "lib", no_device)
    monkeypatch.setattr(_capi, "Handle", no_device)
    monkeypatch.setattr(_capi, "cfg_synth", no_device)
    monkeypatch.setattr(_capi, "cfg_lib", no_device)
    x = np.linspace(1.0, 10.0, 5)
    with pytest.raises(ValueError, match=match):
        nested.NestedSampler(x, x, x, **kw)
    s = nested.NestedSampler(x, x, x, sample="slice")
    assert s.slices == 6 and s.sample == "slice"
    assert nested.NestedSampler(x, x, x).slices == 0


def test_header_states_the_slice_limits_and_counters_and_the_library_exports_them():
    from magprop_amd import _capi
    hdr = open(os.path.join(ROOT, "include", "magprop_amd.h")).read()

    def define(name):
        return int(re.search(r"#define\s+%s\s+(\d+)" % name, hdr).group(1))

    assert define("MP_NEST_MAX_SLICES") == _capi.NEST_MAX_SLICES
    assert define("MP_NEST_MAX_STEPS_OUT") == _capi.NEST_MAX_STEPS_OUT
    assert define("MP_NEST_MAX_SHRINK") == _capi.NEST_MAX_SHRINK
    assert 2 + _capi.NEST_MAX_SHRINK - 1 < 0x100                        # c = 2 + i stays inside its slice's 0x100
    for name in ("mp_nested_set_slice", "mp_nested_get_slice_stats"):
        assert name in _capi.EXPORTS and hasattr(_capi.lib(), name) and name in hdr
    # the slice counters 0x4E400000 + 0x100 s + c against every other c3 range the header lists
    assert "0x4E400000 + 0x100 s + c" in hdr and sr.SLICE_CTR == 0x4E400000
    lo, hi = 0x4E400000, 0x4E400000 + 0x100 * _capi.NEST_MAX_SLICES
    others = [(0, 3), (0x4B00, 0x4B05), (0x5117, 0x5117), (0x30FE, 0x30FE), (0xDE00, 0xDEFF),
              (nr.CTR, nr.CTR + 2 * _capi.NEST_MAX_WALKS)]
    for a, b in others:
        assert b < lo or a >= hi, (hex(a), hex(b))
    assert hi <= 0xFFFFFFFF
    line = hdr[hdr.index("Philox counters c3 in use"):hdr.index("Mixtures:")]
    for tok in ("0x4B00", "0x5117", "0x30FE", "0xDE00", "0x4E000000", "0x4E400000"):
        assert tok in line, tok
