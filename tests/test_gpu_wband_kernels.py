"""The weighted select of the band, one launch at a time: band_wselect_kernel (magprop_amd/csrc/mp_band.hip; wg_wradix_select of
mp_wg.h) on every case of tests/wband_cases.py, through the probe library libmp_probe_wselect.so (csrc/mp_probe_wselect.hip:
test infrastructure, no part of the product's ABI, linked from the product's own kernel object).  The reference is the
restatement tests/wband_restated.py; everything is compared bit for bit, every assertion is on every element.
tests/test_wband_cpu.py checks the cases and the restatement themselves."""
import ctypes as C

import numpy as np
import pytest

import probe_lib
import wband_cases as wc
import wband_restated as wr

pytestmark = pytest.mark.gpu

_dp, _up, _i = C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.c_int
NAN_CANARY = np.array([0x7FF8C0FFEE15BAD1], dtype=np.uint64).view(np.float64)[0]   # (NaN is a result: a NaN no arithmetic makes)


class Probe:
    def __init__(self):
        from magprop_amd import _capi
        _capi.lib()                                        # first, so that one HIP runtime is shared
        self.L = probe_lib.load("wselect")
        self.L.mpv_max_grid.restype, self.L.mpv_max_grid.argtypes = _i, []
        self.L.mpv_wselect.restype, self.L.mpv_wselect.argtypes = _i, [_dp, _up, _i, _i, _dp, _i, _dp]

    def raw(self, cols, units, n, n_grid, q, nq, out):
        p = lambda a, t: None if a is None else a.ctypes.data_as(t)
        return self.L.mpv_wselect(p(cols, _dp), p(units, _up), n, n_grid, p(q, _dp), nq, p(out, _dp))

    def wselect(self, cols, units, q):
        cols, q = np.ascontiguousarray(cols, dtype=np.float64), np.ascontiguousarray(q, dtype=np.float64)
        units = np.ascontiguousarray(units, dtype=np.uint32)
        out = np.full((q.size, cols.shape[0]), NAN_CANARY)
        rc = self.raw(cols, units, cols.shape[1], cols.shape[0], q, q.size, out)
        assert rc == 0, f"mpv_wselect returned {rc}"
        return out


@pytest.fixture(scope="module")
def probe():
    return Probe()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _canonical(a):
    """the bits, every NaN but the canary as one pattern (NaN is the kernel's answer for a column without units)"""
    b = _bits(a).copy()
    b[np.isnan(a) & (b != _bits([NAN_CANARY])[0])] = 0x7FF8000000000000
    return b


def test_probe_refuses_bad_arguments(probe):
    x, u, q, y = np.ones(64), np.ones(8, dtype=np.uint32), np.full(17, 0.5), np.full(64, 7.0)
    assert probe.L.mpv_max_grid() == 1 << 16
    for n, g in ((0, 1), (-1, 1), (wc.BAND_MAX_SAMPLES + 1, 1), (1, 0), (1, -3), (1, (1 << 16) + 1)):
        assert probe.raw(x, u, n, g, q, 1, y) == -1
    for nq in (0, -1, wc.BAND_MAX_Q + 1):
        assert probe.raw(x, u, 8, 8, q, nq, y) == -1
    for bad in (-2.0 ** -1074, np.nextafter(1.0, 2.0), np.nan, np.inf):
        assert probe.raw(x, u, 8, 8, np.array([0.5, bad]), 2, y) == -1
    big = u.copy()
    big[5] = (1 << 31) + 1
    assert probe.raw(x, big, 8, 8, q, 1, y) == -1
    for k in range(4):
        args = [x, u, q, y]
        args[k] = None
        assert probe.raw(args[0], args[1], 8, 8, args[2], 1, args[3]) == -1
    assert np.all(y == 7.0)


@pytest.mark.parametrize("case", wc.CASES, ids=[c.name for c in wc.CASES])
def test_kernel_equals_the_restatement_bit_for_bit(probe, case):
    want = wr.weighted_band(case.cols, case.units, case.q)
    got = probe.wselect(case.cols, case.units, case.q)
    assert got.shape == want.shape and np.array_equal(_canonical(got), _canonical(want)), case.name


def test_result_does_not_depend_on_the_order_of_the_rows(probe):
    """the sums are integer sums: a permutation of the rows changes which wavefront adds what and nothing else"""
    c = wc.BY_NAME["ties-n1000"]
    rng = np.random.default_rng(3)
    first = probe.wselect(c.cols, c.units, c.q)
    for _ in range(2):
        p = rng.permutation(c.units.size)
        assert np.array_equal(_bits(probe.wselect(c.cols[:, p], c.units[p], c.q)), _bits(first))


def test_quantiles_and_columns_are_independent(probe):
    """16 quantiles of 5 columns in one launch equal the launches of one quantile of one column"""
    c = wc.BY_NAME["random-n257"]
    rng = np.random.default_rng(4)
    cols = np.concatenate([c.cols, rng.standard_normal((5 - c.cols.shape[0], c.units.size))]) if c.cols.shape[0] < 5 else c.cols
    whole = probe.wselect(cols, c.units, wc.Q16)
    assert whole.shape == (16, 5)
    for g in (0, 4):
        for j in (0, 7, 15):
            assert _bits(probe.wselect(cols[g:g + 1], c.units, wc.Q16[j:j + 1]))[0, 0] == _bits(whole)[j, g]
