"""GPU tests of the tempered sampler's ladder adaptation and of its thermodynamic monitor (include/magprop_amd.h
mp_sampler_set_ladder_adaptation, mp_sampler_set_thermo): the device's chains, ladders and sums against the restated step loop
with the restated rule between its steps (tests/ladder_restated.py run_adaptive, with the device's exp and log), the paths that
must not have moved, the evidence from the device sums, the real posterior and the argument codes."""
import ctypes as C

import numpy as np
import pytest

import ladder_restated as lr
from conftest import TRUTHS
from moves_restated import STRETCH
from raw_abi import RawSampler, dp, lp, swap_counts
from sampler_restated import run as restate
from test_gpu_ladder_kernels import device_exp, device_log

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
TABLE = [(STRETCH, 1.0, 2.0, 0.0)]
BETAS = (1.0, 0.5, 0.2, 0.05)
NW, ND, T, GROUPS = 16, 3, 4, 2
N_STEPS, N_ADAPT, LAG, TIME = 200, 120, 20.0, 5.0
SEED = 20261020


def temperatures(r, n_groups, n_temps):
    """mp_sampler_get_temperatures of RawSampler r: (betas[n_groups, n_temps], n_updates, n_dropped[n_groups])."""
    b, n, d = np.full((n_groups, n_temps), -7.0), C.c_int64(-7), np.full(n_groups, -7, dtype=np.int64)
    r._ok(r.L.mp_sampler_get_temperatures(r.sp, dp(b), C.byref(n), lp(d)))
    return b, n.value, d


def history(r, group, n_temps, first=0, rows=N_ADAPT + 5):
    buf, n = np.full((rows, n_temps), -7.0), C.c_int64(-7)
    r._ok(r.L.mp_sampler_get_ladder_history(r.sp, group, first, rows, dp(buf), C.byref(n)))
    assert np.all(buf[n.value:] == -7.0)
    return buf[:n.value]


def thermo(r):
    s, nf, nn, n = np.empty(r.ne), np.empty(r.ne, dtype=np.int64), np.empty(r.ne, dtype=np.int64), C.c_int64(-7)
    r._ok(r.L.mp_sampler_get_thermo(r.sp, dp(s), lp(nf), lp(nn), C.byref(n)))
    return s, nf, nn, n.value


@pytest.fixture(scope="module")
def gaussian():
    """The start and the restated adaptive run of the Gaussian case: two groups of 4 temperatures x 16 walkers in 3 dimensions,
    200 steps of which the first 120 adapt (lag 20, time 5)."""
    rng = np.random.default_rng(12)
    pos = rng.normal(size=(GROUPS * T * NW, ND)) * 1.5
    ref = lr.run_adaptive(pos.copy(), N_STEPS, SEED, TABLE, GROUPS, BETAS, N_ADAPT, LAG, TIME, exp=device_exp, log=device_log)
    ref.run.chain.setflags(write=False)
    ref.run.lnp.setflags(write=False)
    return pos, ref


def adaptive_sampler(whole):
    r = RawSampler(NW, GROUPS * T, ND, SEED)
    r.set_temperatures(BETAS)
    r._ok(r.L.mp_sampler_set_ladder_adaptation(r.sp, N_ADAPT, LAG, TIME, 1))
    r.set_whole_step(whole)
    r._ok(r.L.mp_sampler_set_thermo(r.sp, 0))
    return r


@pytest.mark.parametrize("whole", [True, False])
def test_adaptive_gaussian_run_matches_the_restatement_bit_for_bit(gaussian, whole):
    pos, ref = gaussian
    assert ref.n_updates == N_ADAPT and not np.array_equal(ref.betas[0], ref.betas[1])     # the two groups' ladders differ
    assert 0 < ref.run.swaps.sum() < N_STEPS * NW * GROUPS * (T - 1)
    want_thermo = lr.thermo(ref.run.lnp[N_ADAPT:].reshape(-1, GROUPS * T, NW))
    outs = []
    for runs in ((N_STEPS,), (70, 130)):
        with adaptive_sampler(whole) as r:
            r.set_positions(pos)
            chain, lnp, acc = r.run_chunks(runs)
            b, n_upd, dropped = temperatures(r, GROUPS, T)
            assert np.array_equal(chain, ref.run.chain) and np.array_equal(lnp, ref.run.lnp), (whole, runs)
            assert np.array_equal(acc, ref.run.acc) and np.array_equal(r.swaps(GROUPS, T), ref.run.swaps), (whole, runs)
            assert np.array_equal(b, ref.betas) and n_upd == N_ADAPT and np.array_equal(dropped, ref.dropped), (whole, runs)
            for g in range(GROUPS):
                h = history(r, g, T)
                assert np.array_equal(h, ref.history[:, g]), (whole, runs, g)
                assert np.array_equal(history(r, g, T, first=100, rows=7), ref.history[100:107, g])
            s, nf, nn, n = thermo(r)
            assert n == N_STEPS - N_ADAPT and np.array_equal(s, want_thermo[0]), (whole, runs)
            assert np.array_equal(nf, want_thermo[1]) and np.array_equal(nn, want_thermo[2]) and not nn.any()
            outs.append((chain, lnp, b, s))
            # further steps are frozen steps: the ladder stays bit for bit, no update is counted, no history row is added
            r.run(30, store=False)
            b2, n_upd2, _ = temperatures(r, GROUPS, T)
            assert np.array_equal(b2, b) and n_upd2 == N_ADAPT and len(history(r, 0, T)) == N_ADAPT
            assert thermo(r)[3] == N_STEPS - N_ADAPT + 30
    assert all(np.array_equal(x, y) for x, y in zip(*outs))                                # split as 70 + 130: one run
    assert b[0, 0] == 1.0 and b[0, -1] == BETAS[-1] and np.all(np.diff(b, axis=1) < 0.0)


def test_frozen_steps_are_a_fixed_ladder_run(gaussian):
    """Steps >= n_adapt of the adaptive run equal the restated FIXED-ladder loop started from the state and the frozen ladder at
    step n_adapt, and a device sampler that is handed the frozen ladder as a fixed one has the same ladder bit for bit."""
    pos, ref = gaussian
    with adaptive_sampler(True) as r:
        r.set_positions(pos)
        chain, lnp = r.run(N_ADAPT)
        _, _, acc = r.state()
        frozen, _, _ = temperatures(r, GROUPS, T)
        tail, tail_lnp = r.run(N_STEPS - N_ADAPT)
    fixed = restate(chain[-1].copy(), N_STEPS - N_ADAPT, SEED, TABLE, n_ensembles=GROUPS * T, step0=N_ADAPT, lnp=lnp[-1].copy(),
                    acc=acc.copy(), betas=frozen.ravel(), n_temps=T)
    assert np.array_equal(tail, fixed.chain) and np.array_equal(tail_lnp, fixed.lnp)
    assert np.array_equal(tail, ref.run.chain[N_ADAPT:])


def test_fixed_and_untempered_samplers_are_untouched():
    """A fixed-ladder sampler and an untempered one give the chains of the restated step loop as before; the fixed one reports
    its ladder as set and no update."""
    rng = np.random.default_rng(5)
    pos = rng.normal(size=(T * NW, ND))
    ref = restate(pos.copy(), 60, SEED, TABLE, n_ensembles=T, n_temps=T, betas=list(BETAS))
    with RawSampler(NW, T, ND, SEED) as r:
        r.set_temperatures(BETAS)
        r.set_positions(pos)
        chain, lnp, acc = r.run_chunks((25, 35))
        assert np.array_equal(chain, ref.chain) and np.array_equal(lnp, ref.lnp) and np.array_equal(acc, ref.acc)
        assert np.array_equal(r.swaps(1, T), ref.swaps)
        b, n_upd, dropped = temperatures(r, 1, T)
        assert np.array_equal(b[0], BETAS) and n_upd == 0 and not dropped.any()
        n = C.c_int64(0)
        assert r.L.mp_sampler_get_ladder_history(r.sp, 0, 0, 1, dp(np.zeros(T)), C.byref(n)) == r.cap.MP_ESTATE
    plain = restate(pos.copy(), 60, SEED, TABLE, n_ensembles=T)
    with RawSampler(NW, T, ND, SEED) as r:
        r.set_positions(pos)
        chain, lnp, acc = r.run_chunks((60,))
        assert np.array_equal(chain, plain.chain) and np.array_equal(lnp, plain.lnp) and np.array_equal(acc, plain.acc)
        assert r.L.mp_sampler_get_temperatures(r.sp, dp(np.zeros(T)), None, None) == r.cap.MP_ESTATE


def test_log_evidence_from_the_device_sums():
    """The Gaussian run through the front end: log_evidence(device=True), from the monitor's sums over the frozen steps, against
    log_evidence(discard=n_adapt) from the stored chain.  Every lnL of the Gaussian target is <= 0, so a sum of the N = 80 x 16
    cells of a temperature in any order is within (N - 1) 2^-53 relative of the exact sum; the mean adds one rounding on either
    side: the two means agree to N 2^-52 relative.  The integral is a sum of terms of one sign, linear in the means; evaluating it
    twice adds the roundings of its T + 3 operations per term on either side."""
    from magprop_amd import EnsembleSampler
    pos = np.random.default_rng(3).normal(size=(T * NW, ND))
    s = EnsembleSampler(NW, ND, target="gaussian", seed=SEED, betas=BETAS,
                        adapt_ladder={"steps": N_ADAPT, "lag": LAG, "time": TIME, "history": True})
    assert s.ladder_frozen_at == N_ADAPT and np.array_equal(s.get_betas(), [BETAS]) and np.array_equal(s.betas, BETAS)
    with pytest.raises(RuntimeError):
        s.log_evidence(device=True)                       # the monitor is off
    s.monitor_thermo()
    s.run_mcmc(pos, 50)
    with pytest.raises(ValueError):
        s.log_evidence(device=True)                       # on, but no frozen step yet
    with pytest.raises(ValueError):
        s.log_evidence()                                  # every stored step lies before the freeze
    s.run_mcmc(None, N_STEPS - 50)
    frozen = s.get_betas()
    assert np.array_equal(s.ladder_history()[-1], frozen[0]) and len(s.ladder_history()) == N_ADAPT
    assert s.ladder_updates[0] == N_ADAPT and not np.array_equal(frozen[0], BETAS)
    th = s.get_thermo()
    N = (N_STEPS - N_ADAPT) * NW
    assert th["n_steps"] == N_STEPS - N_ADAPT and np.all(th["n_finite"] == N) and not th["n_nonfinite"].any()
    host_means = s.get_log_prob()[N_ADAPT:].reshape(-1, T, NW).transpose(1, 0, 2).reshape(T, -1).mean(axis=1)
    dev_means = th["sum_lnl"][0] / N
    assert np.all(host_means < 0.0) and np.all(np.abs(dev_means - host_means) <= N * EPS * np.abs(host_means)), (dev_means, host_means)
    lnz_d, dlnz_d = s.log_evidence(device=True)
    lnz_h, dlnz_h = s.log_evidence(discard=N_ADAPT)
    tol = (N + 2 * (T + 3)) * EPS
    print(f"lnZ from the device sums {lnz_d!r}, from the stored chain {lnz_h!r}, bound {tol * abs(lnz_h):.3e}")
    # (dlnZ = |fine - coarse|, two such integrals: |coarse| <= |fine| + dlnZ)
    assert abs(lnz_d - lnz_h) <= tol * abs(lnz_h) and abs(dlnz_d - dlnz_h) <= tol * (2.0 * abs(lnz_h) + dlnz_h)
    for discard in (0, N_ADAPT - 1):
        with pytest.raises(ValueError):
            s.log_evidence(discard=discard)               # a step before the freeze
    s.close()


EVIDENCE_INFLATION = 10.0      # tests/test_gpu_tempering.py's brute-force case


def test_adaptation_on_the_real_posterior(gsynth):
    """The brute-force case of tests/test_gpu_tempering.py (Humped, yerr x 10, 32 walkers per temperature, geometric start ladder
    1 .. 1e-12, started from box draws with a finite lnprob), 400 steps, once fixed and once with the first 200 adapting (lag 50,
    time 5), same seed: the adapted ladder is finite, strictly decreasing with both ends bit-fixed, no update was dropped, the cold
    chain's lnprob is finite, and over the frozen window (steps 200 .. 399) the smallest pair acceptance of the adapted run is
    larger than the fixed run's.
    T = 16.  Measured once on an MI355X, smallest pair acceptance over that window, fixed / adapted: T = 16: 0.443 / 0.773;
    T = 32: 0.639 / 0.880; T = 64: 0.802 / 0.927 (largest - smallest: 0.557 / 0.090, 0.361 / 0.115, 0.198 / 0.073).  On this
    posterior the geometric ladder's smallest acceptance, which is the coldest pair's, stays above 0.05 at all three sizes, so the
    smallest of them is taken: it is where the fixed ladder is starved most."""
    from magprop_amd import EnsembleSampler, LogProb, synth, tempering
    n_temps, half = 16, 200
    x, y, yerr = gsynth["Humped_x"], gsynth["Humped_y"], gsynth["Humped_yerr"] * EVIDENCE_INFLATION
    lo, hi = synth.PRIOR_LOWER, synth.PRIOR_UPPER
    lnprob = LogProb(x, y, yerr)
    rng = np.random.default_rng(2026)
    start = lo + (hi - lo) * rng.random((4 * n_temps * 32, 6))
    start = start[np.isfinite(lnprob(start))][:n_temps * 32]
    betas = tempering.geometric_ladder(n_temps, 1e-12)
    window = {}
    for adapt in (None, {"steps": half, "lag": 50.0, "time": 5.0}):
        s = EnsembleSampler(32, 6, x, y, yerr, seed=77, betas=betas, adapt_ladder=adapt)
        s.run_mcmc(start, half, store=False)
        before = swap_counts(s._L, s._s, 1, n_temps)
        s.run_mcmc(None, half)
        acc = (swap_counts(s._L, s._s, 1, n_temps) - before)[0] / (half * 32)
        window[adapt is not None] = acc
        lad = s.get_betas()[0]
        n_upd, dropped = s.ladder_updates
        if adapt is None:
            assert np.array_equal(lad, betas) and n_upd == 0
        else:
            assert np.all(np.isfinite(lad)) and np.all(np.diff(lad) < 0.0) and lad[0] == 1.0 and lad[-1] == betas[-1]
            assert n_upd == half and not dropped.any() and not np.array_equal(lad, betas)
            assert np.all(np.isfinite(s.get_log_prob(temp=0)))
        s.close()
    print(f"smallest pair acceptance over the frozen window: fixed {window[False].min():.4f}, adapted {window[True].min():.4f}; "
          f"spread {tempering.swap_spread(window[False]):.4f} / {tempering.swap_spread(window[True]):.4f}")
    assert window[True].min() > window[False].min(), (window[True], window[False])


def test_ladder_argument_validation(gsynth):
    from magprop_amd import EnsembleSampler, _capi
    OK, EINVAL, ESTATE = _capi.MP_OK, _capi.MP_EINVAL, _capi.MP_ESTATE
    with RawSampler(8, 6, ND, 1) as r:
        L, sp = r.L, r.sp
        assert L.mp_sampler_set_ladder_adaptation(sp, 10, 20.0, 5.0, 0) == ESTATE            # before set_temperatures
        assert L.mp_sampler_get_temperatures(sp, None, None, None) == ESTATE                # untempered
        assert L.mp_sampler_get_thermo(sp, None, None, None, None) == ESTATE                # the monitor is off
        assert L.mp_sampler_set_thermo(sp, -2) == EINVAL
        r.set_temperatures((1.0, 0.5))
        assert L.mp_sampler_set_ladder_adaptation(sp, 10, 20.0, 5.0, 0) == EINVAL            # n_temps < 3
        r.set_temperatures((1.0, 0.5, 0.1))
        for bad in ((0, 20.0, 5.0, 0), (-1, 20.0, 5.0, 0), (10, 0.0, 5.0, 0), (10, -1.0, 5.0, 0), (10, np.nan, 5.0, 0),
                    (10, np.inf, 5.0, 0), (10, 20.0, 0.0, 0), (10, 20.0, np.nan, 0), (10, 20.0, np.inf, 0),
                    ((1 << 28) // (8 * 6) + 1, 20.0, 5.0, 1)):                              # a history beyond 256 MB
            assert L.mp_sampler_set_ladder_adaptation(sp, *bad) == EINVAL, bad
        assert L.mp_sampler_set_ladder_adaptation(sp, (1 << 28) // (8 * 6) + 1, 20.0, 5.0, 0) == OK   # without a history it may
        assert L.mp_sampler_set_ladder_adaptation(sp, 10, 20.0, 5.0, 0) == OK
        n = C.c_int64(0)
        assert L.mp_sampler_get_ladder_history(sp, 0, 0, 1, dp(np.zeros(3)), C.byref(n)) == ESTATE   # no history kept
        assert L.mp_sampler_set_ladder_adaptation(sp, 10, 20.0, 5.0, 1) == OK
        assert L.mp_sampler_get_ladder_history(sp, 2, 0, 1, dp(np.zeros(3)), C.byref(n)) == EINVAL   # 2 groups: 0, 1
        assert L.mp_sampler_get_ladder_history(sp, 0, -1, 1, dp(np.zeros(3)), C.byref(n)) == EINVAL
        assert L.mp_sampler_get_ladder_history(sp, 0, 0, 1, None, C.byref(n)) == EINVAL
        assert L.mp_sampler_get_ladder_history(sp, 1, 0, 4, dp(np.zeros(12)), C.byref(n)) == OK and n.value == 0
        assert L.mp_sampler_set_thermo(sp, 3) == OK and L.mp_sampler_set_thermo(sp, -1) == OK
        assert L.mp_sampler_get_thermo(sp, None, None, None, None) == ESTATE
        assert L.mp_sampler_set_thermo(sp, 0) == OK
        r.set_positions(np.random.default_rng(0).normal(size=(48, ND)))
        assert L.mp_sampler_set_ladder_adaptation(sp, 10, 20.0, 5.0, 0) == ESTATE            # after set_positions
        r.run(4, store=False)
        assert L.mp_sampler_get_ladder_history(sp, 1, 0, 9, dp(np.zeros(27)), C.byref(n)) == OK and n.value == 4
        assert L.mp_sampler_get_thermo(sp, None, None, None, C.byref(n)) == OK and n.value == 0      # no frozen step yet
    # the front end
    x, y, yerr = gsynth["Humped_x"], gsynth["Humped_y"], gsynth["Humped_yerr"]
    with pytest.raises(ValueError):
        EnsembleSampler(8, 6, x, y, yerr, adapt_ladder=10)                                  # untempered
    with pytest.raises(ValueError):
        EnsembleSampler(8, 6, x, y, yerr, betas=(1.0, 0.5), adapt_ladder=10)                # 2 temperatures
    for bad in (0, {"steps": 10, "lag": 0.0}, {"steps": 10, "time": -1.0}, {"lag": 5.0}, {"steps": 10, "rate": 1.0}):
        with pytest.raises(ValueError):
            EnsembleSampler(8, 6, x, y, yerr, betas=(1.0, 0.5, 0.1), adapt_ladder=bad)
    s = EnsembleSampler(8, 6, x, y, yerr, betas=(1.0, 0.5, 0.1), adapt_ladder=10)
    assert s.ladder_frozen_at == 10 and s.ladder_updates[0] == 0
    with pytest.raises(ValueError):
        s.ladder_history()                                                                  # no history asked for
    with pytest.raises(_capi.MagpropAmdError):
        s.get_thermo()
    s.close()
    fixed = EnsembleSampler(8, 6, x, y, yerr, betas=(1.0, 0.5, 0.1))
    assert fixed.ladder_frozen_at is None and np.array_equal(fixed.get_betas(), [[1.0, 0.5, 0.1]])
    fixed.close()
    plain = EnsembleSampler(8, 6, x, y, yerr)
    with pytest.raises(ValueError):
        plain.get_betas()
    plain.close()
