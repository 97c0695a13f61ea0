"""The kernels of the ladder adaptation and of the thermodynamic monitor (magprop_amd/csrc/mp_ladder.hip ladder_init_kernel,
ladder_adapt_kernel, thermo_kernel) on the named cases of tests/ladder_cases.py, reached through the probe library
libmp_probe_ladder.so (csrc/mp_probe_ladder.hip), which is test infrastructure, no part of the product's ABI, and linked from the
product's own object, so that the kernels under test are the ones libmagprop_amd.so runs.

Held: bit for bit.  The restatement (tests/ladder_restated.py) forms its three sums in index order and the monitor's row sums in
the order of mp_wg.h, and takes the device's exp and log (mpt_libm), so no bound on a sum in another order is needed."""
import ctypes as C

import numpy as np
import pytest

import ladder_cases as lc
import ladder_restated as lr
import probe_lib
from raw_abi import dp, lp

pytestmark = pytest.mark.gpu


def probe():
    """libmp_probe_ladder.so, behind the product's library so that one HIP runtime is shared."""
    from magprop_amd import _capi
    _capi.lib()
    return probe_lib.load("ladder")


def _libm(func, x):
    a = np.atleast_1d(np.asarray(x, dtype=np.float64))
    if a.size == 0:
        return a.copy()
    buf, out = np.ascontiguousarray(a.ravel()), np.empty(a.size)
    assert probe().mpt_libm(func, dp(buf), dp(out), C.c_int(buf.size)) == 0
    out = out.reshape(a.shape)
    return float(out[0]) if np.ndim(x) == 0 else out


def device_exp(x):
    """The device runtime's exp, element by element (mpt_libm)."""
    return _libm(0, x)


def device_log(x):
    return _libm(1, x)


def init_launch(betas, swaps):
    """mpt_init over betas[n_groups, T]: gap, span, prev as the device left them (canaries where it left them alone)."""
    n_groups, T = betas.shape
    gap, span = np.full((n_groups, T - 1), -7.0), np.full(n_groups, -7.0)
    prev = np.full((n_groups, T - 1), -7, dtype=np.int64)
    rc = probe().mpt_init(T, n_groups, dp(np.ascontiguousarray(betas)), lp(np.ascontiguousarray(swaps, dtype=np.int64)), dp(gap), dp(span), lp(prev))
    assert rc == 0, rc
    return gap, span, prev


def adapt_launch(case, gap, span, history=True):
    """mpt_adapt of one case: betas, gap, prev, dropped (started at 3 per group) and the history row as the device left them."""
    n_groups, T = case.betas.shape
    betas, gap, prev = case.betas.copy(), np.array(gap, dtype=np.float64), np.array(case.prev, dtype=np.int64)
    dropped = np.full(n_groups, 3, dtype=np.int64)
    hist = np.full((n_groups, T), -7.0) if history else None
    rc = probe().mpt_adapt(T, n_groups, case.n_walkers, C.c_double(case.kappa), dp(np.ascontiguousarray(span, dtype=np.float64)),
                           lp(np.ascontiguousarray(case.swaps, dtype=np.int64)), dp(betas), dp(gap), lp(prev), lp(dropped), dp(hist))
    assert rc == 0, rc
    return betas, gap, prev, dropped, hist


def check_adapt(case):
    n_groups, T = case.betas.shape
    if case.gap is None:
        gap, span, prev0 = init_launch(case.betas, case.prev)
        assert np.array_equal(prev0, case.prev), case.name
        for g in range(n_groups):
            rg, rs, _ = lr.init(case.betas[g], case.prev[g], device_log)
            assert np.array_equal(gap[g], rg) and span[g] == rs, case.name
    else:
        gap, span = case.gap, case.span
    betas, new_gap, prev, dropped, hist = adapt_launch(case, gap, span)
    for g in range(n_groups):
        rb, rg, rp, taken = lr.adapt(case.betas[g], gap[g], span[g], case.prev[g], case.swaps[g], case.n_walkers, case.kappa, device_exp)
        assert taken != case.drops, case.name
        assert np.array_equal(betas[g], rb) and np.array_equal(new_gap[g], rg), (case.name, g)
        assert np.array_equal(prev[g], rp) and np.array_equal(prev[g], case.swaps[g]), (case.name, g)
        assert dropped[g] == 3 + (0 if taken else 1), (case.name, g)
        assert np.array_equal(hist[g], rb), (case.name, g)
        assert betas[g, 0] == case.betas[g, 0] == 1.0 and betas[g, -1] == case.betas[g, -1], case.name
        assert np.all(np.diff(betas[g]) < 0.0), case.name
        if not taken:
            assert np.array_equal(betas[g], case.betas[g]) and np.array_equal(new_gap[g], gap[g]), case.name


@pytest.mark.parametrize("n_temps", lc.N_TEMPS)
def test_init_and_update_kernels_equal_the_restatement_bit_for_bit(n_temps):
    cases = lc.adapt_cases(n_temps)
    assert {c.betas.shape[0] for c in cases} == set(lc.N_GROUPS)
    for case in cases:
        check_adapt(case)


def test_dropped_updates_leave_the_state_and_count():
    for case in lc.dropped_cases():
        check_adapt(case)
    # without a history nothing but the state is written
    case = lc.adapt_cases(4)[3]
    gap, span, _ = init_launch(case.betas, case.prev)
    a, b = adapt_launch(case, gap, span, history=False), adapt_launch(case, gap, span)
    assert all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4]))


@pytest.mark.parametrize("n_walkers", lc.THERMO_WALKERS)
def test_thermo_kernel_equals_the_restatement_bit_for_bit(n_walkers):
    lnp = lc.thermo_rows(n_walkers)
    n_rows, n_ens, _ = lnp.shape
    L = probe()
    s, nf, nn = np.zeros(n_ens), np.zeros(n_ens, dtype=np.int64), np.zeros(n_ens, dtype=np.int64)
    ref = None
    # rows 1 .. 2, then 3 .. 5 of the same slab, continued: row 0 is passed over
    for first, rows in ((1, 2), (3, 3), (0, 0)):
        assert L.mpt_thermo(n_walkers, n_ens, n_rows, first, rows, dp(lnp), dp(s), lp(nf), lp(nn)) == 0
        ref = lr.thermo(lnp[first:first + rows], *(ref or ()))
        assert np.array_equal(s, ref[0]) and np.array_equal(nf, ref[1]) and np.array_equal(nn, ref[2]), (first, rows)
    assert np.all(nf + nn == 5 * n_walkers) and nn[2] >= n_walkers and np.all(np.isfinite(s))
    one = lr.thermo(lnp[1:])
    assert np.array_equal(s, one[0])                      # (a function of the rows alone, not of how they were fed)


def test_the_probe_refuses_bad_arguments():
    L = probe()
    b, sw = np.array([[1.0, 0.5, 0.1]]), np.zeros((1, 2), dtype=np.int64)
    gap, span, prev = np.zeros((1, 2)), np.zeros(1), np.zeros((1, 2), dtype=np.int64)
    assert L.mpt_init(2, 1, dp(b), lp(sw), dp(gap), dp(span), lp(prev)) == -1
    assert L.mpt_init(3, 0, dp(b), lp(sw), dp(gap), dp(span), lp(prev)) == -1
    assert L.mpt_init(3, 1, None, lp(sw), dp(gap), dp(span), lp(prev)) == -1
    assert L.mpt_adapt(3, 1, 0, C.c_double(0.1), dp(span), lp(sw), dp(b), dp(gap), lp(prev), lp(prev), None) == -1
    assert L.mpt_thermo(4, 1, 2, 1, 2, dp(np.zeros(8)), dp(span), lp(prev), lp(prev)) == -1
    assert L.mpt_libm(2, dp(span), dp(span), C.c_int(1)) == -1
    x = np.array([0.0, 1.0, -700.0, 709.0])
    assert np.allclose(device_exp(x), np.exp(x), rtol=4e-16) and device_exp(0.0) == 1.0 and device_log(1.0) == 0.0
