"""The derived-quantity kernel on its own (magprop_amd/csrc/mp_derive.hip derive_kernel) on the cases of tests/derive_cases.py:
grid sizes that leave segments empty, short or full, zero and constant curves, peaks at the ends and on a plateau, all the energy
in one interval at the ends of a segment and of the row, a cumulative energy that meets its threshold exactly, tiny and huge
values, failed rows between finished ones and row counts around a wavefront.  The kernel is reached through the probe library
libmp_probe_derive.so (csrc/mp_probe_derive.hip), which is test infrastructure, no part of the product's ABI, and linked from the
product's own kernel object.  The reference is the numpy restatement (tests/derive_restated.py) and every column is compared bit
for bit (NaNs by position, signs of zero included): the header promises it, so there is no tolerance here.
tests/test_derive_cases_cpu.py checks the cases and the restatement themselves."""
import ctypes as C
import os

import numpy as np
import pytest

import derive_cases as dc
import derive_restated as dr
import probe_lib

pytestmark = pytest.mark.gpu

_dp, _ip, _i = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_int


class Probe:
    """libmp_probe_derive.so behind numpy arrays"""

    def __init__(self):
        from magprop_amd import _capi
        _capi.lib()                                        # first, so that one HIP runtime is shared
        self.L = probe_lib.load("derive")
        for name in ("mpd_threads", "mpd_window", "mpd_columns", "mpd_max_rows", "mpd_max_grid"):
            getattr(self.L, name).restype = _i
            getattr(self.L, name).argtypes = []
        self.L.mpd_seg.restype, self.L.mpd_seg.argtypes = _i, [_i]
        self.L.mpd_run_derive.restype = _i
        self.L.mpd_run_derive.argtypes = [_dp, _ip, _dp, _i, _i, _dp]

    def run(self, t, curves, status):
        curves = np.ascontiguousarray(curves, dtype=np.float64)
        status = np.ascontiguousarray(status, dtype=np.int32)
        t = np.ascontiguousarray(t, dtype=np.float64)
        out = np.full((curves.shape[1], dr.N), -777.0)     # a canary the kernel must overwrite
        rc = self.L.mpd_run_derive(curves.ctypes.data_as(_dp), status.ctypes.data_as(_ip), t.ctypes.data_as(_dp), curves.shape[1],
                                   t.size, out.ctypes.data_as(_dp))
        assert rc == 0, f"mpd_run_derive returned {rc}"
        return out


@pytest.fixture(scope="module")
def probe():
    return Probe()


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a), np.signbit(b))


def test_probe_shares_the_restatement_constants(probe):
    assert probe.L.mpd_threads() == dr.SEGMENTS and probe.L.mpd_columns() == dr.N
    assert probe.L.mpd_window() == dc.WINDOW                # (the corners dc.WINDOW_GRID_SIZES sit on)
    for G in dc.GRID_SIZES + dc.WINDOW_GRID_SIZES + (1000, 130):
        assert probe.L.mpd_seg(G) == dr.seg_len(G)
    t = np.arange(1.0, 4.0)
    z = np.zeros((5, 1, 3))
    st = np.zeros(1, dtype=np.int32)
    out = np.empty((1, 16))
    a = lambda x, p: x.ctypes.data_as(p)                   # noqa: E731
    assert probe.L.mpd_run_derive(None, a(st, _ip), a(t, _dp), 1, 3, a(out, _dp)) == -1
    assert probe.L.mpd_run_derive(a(z, _dp), a(st, _ip), a(t, _dp), 0, 3, a(out, _dp)) == -1
    assert probe.L.mpd_run_derive(a(z, _dp), a(st, _ip), a(t, _dp), 1, 1, a(out, _dp)) == -1


@pytest.mark.parametrize("name", dc.names())
def test_kernel_equals_the_restatement_bit_for_bit(probe, name):
    _, t, curves, status = dc.case(name)
    got = probe.run(t, curves, status)
    want = dr.derive(curves, status, t)
    assert np.all(np.isnan(got[status != 0])) and not np.any(np.isnan(got[status == 0]))
    bad = [(r, c) for r in range(got.shape[0]) for c in range(dr.N) if not same(got[r, c:c + 1], want[r, c:c + 1])]
    assert not bad, (name, bad[:5], [(got[r, c], want[r, c]) for r, c in bad[:5]])


def test_a_row_does_not_depend_on_its_place_in_the_batch(probe):
    _, t, curves, status = dc.case("rows_257")
    whole = probe.run(t, curves, status)
    for r in (0, 63, 64, 256):
        alone = probe.run(t, curves[:, r:r + 1], status[r:r + 1])
        assert same(alone[0], whole[r]), r
    perm = np.random.default_rng(3).permutation(257)
    assert same(probe.run(t, curves[:, perm], status[perm]), whole[perm])
