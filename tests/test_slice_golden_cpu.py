"""The two slice restatements (tests/slice_move_restated.py, tests/nest_slice_restated.py) against results recorded from them
before they were put on one slice generator (tests/walk_restated.py slice_rounds): every array equal bit for bit.  The GPU tests tie the
device to the restatements; these fixtures tie the restatements to what they were.  tests/golden/make_slice_golden.py records
the fixtures from the two functions below."""
import os

import numpy as np

import nest_restated as nr
import nest_slice_restated as sr
import slice_move_restated as sm
from conftest import GOLDEN

MOVE_FIXTURE = os.path.join(GOLDEN, "golden_slice_move.npz")
NEST_FIXTURE = os.path.join(GOLDEN, "golden_nest_slice.npz")


def move_run():
    """The case of test_gpu_moves_slice.py::test_tight_limits_exhaust_budgets_and_fail_slices: 18 walkers x 3 ensembles, 3 dims,
    40 steps, tune 10, mu0 = 0.05, limits 2 / 2."""
    seed = 20261102
    pos = np.random.default_rng(seed).normal(size=(18 * 3, 3)) * 1.5
    ref = sm.run(pos, 40, seed, [(sm.SLICE, 1.0, 0.05, 10.0)], limits=(2, 2), n_ensembles=3)
    out = {"chain": ref.chain, "lnp": ref.lnp, "acc": ref.acc, "mu": ref.mu}
    out.update(ref.state.counters())
    return out


def nest_run():
    """The first six iterations of test_gpu_nested_slice.py::test_slice_state_matches_the_restatement_bit_for_bit, n_runs = 3."""
    n_runs, ndim, nlive, nbatch, slices = 3, 3, 32, 8, 3
    seed = 20261016 + n_runs
    lo, hi = np.array([-2.0, -1.0, -4.0]), np.array([3.0, 2.5, 1.5])
    live0 = lo + (hi - lo) * np.random.default_rng(17 + n_runs).random((n_runs, nlive, ndim))
    s = sr.start(live0, nr.gaussian)
    sr.run(s, 6, nbatch, seed, slices, mu=1.0, max_steps_out=4, max_shrink=32, dlogz=0.05, lower=lo, upper=hi,
           evaluate_one=nr.gaussian_one)
    out = {"live": s.live, "lnl": s.lnl, "status": s.status, "acc": s.acc, "dead_pars": np.array(s.dead_pars),
           "dead_lnl": np.array(s.dead_lnl), "dead_n": np.array(s.dead_n)}
    out.update({k: getattr(s, k) for k in ("nit", "stopped", "ncall", "nacc", "nzero", "nexpand", "ncontract", "nfail")})
    return out


def _assert_holds(got, path):
    want = np.load(path)
    assert sorted(want.files) == sorted(got)
    for k in want.files:
        a = np.asarray(got[k])
        assert a.dtype == want[k].dtype and np.array_equal(a, want[k]), k


def test_slice_move_restatement_reproduces_its_recorded_run():
    got = move_run()
    assert got["chain"].shape == (40, 54, 3) and np.all(got["nfail"] > 0) and np.all(got["n_tuned"] == 40)
    _assert_holds(got, MOVE_FIXTURE)


def test_nested_slice_restatement_reproduces_its_recorded_run():
    got = nest_run()
    assert got["dead_lnl"].shape == (3, 48) and np.all(got["nit"] == 6) and np.all(got["nexpand"] > 0)
    _assert_holds(got, NEST_FIXTURE)
