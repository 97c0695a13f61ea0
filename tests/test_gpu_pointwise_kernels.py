"""The three kernels of the pointwise scores on their own (magprop_amd/csrc/mp_pointwise.hip: pointwise_cells_kernel,
pointwise_select_kernel, pointwise_reduce_kernel) on the cases of tests/pointwise_cases.py.  The kernels are reached through the
probe library libmp_probe_pointwise.so (csrc/mp_probe_pointwise.hip), which is test infrastructure, no part of the product's ABI,
and linked from the product's own kernel object.

The reference is the numpy restatement (tests/pointwise_restated.py).  The cells, the cut, the tail and every column without an
exp in it are compared bit for bit (NaNs by position, signs of zero included): the header promises it.  The S halves of the
log-sum-exp pairs depend on the device's exp and are held, as log S + M, to the long-double definition within the bound
tests/test_pointwise_cases_cpu.py derives (lse_bound there: (K + 9) 3 eps + 0.5 eps (1 + log n) + 2^-63 |want|, K = ceil(n /
256)); the worst ratio to the bound is reported.  Every output buffer starts as a canary the kernel must overwrite."""
import ctypes as C
import os

import numpy as np
import pytest

import pointwise_cases as pc
import pointwise_restated as pr
import probe_lib
from test_pointwise_cases_cpu import lse_bound, lse_error, same

pytestmark = pytest.mark.gpu

_dp, _ip, _i, _i64 = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_int, C.c_int64
CANARY = -777.0


def _d(a):
    return a.ctypes.data_as(_dp)


class Probe:
    """libmp_probe_pointwise.so behind numpy arrays"""

    def __init__(self):
        from magprop_amd import _capi
        _capi.lib()                                        # first, so that one HIP runtime is shared
        self.L = probe_lib.load("pointwise")
        for name in ("mpw_threads", "mpw_tile", "mpw_columns", "mpw_max_tail", "mpw_sort_cap", "mpw_max_rows", "mpw_max_obs"):
            getattr(self.L, name).restype = _i
            getattr(self.L, name).argtypes = []
        self.L.mpw_tail_len.restype, self.L.mpw_tail_len.argtypes = _i, [_i64]
        self.L.mpw_cells.restype = _i
        self.L.mpw_cells.argtypes = [_dp, _ip, _ip, _dp, _dp, _dp, _dp, _i, _i, _i, _i64, _i64, _dp]
        self.L.mpw_select.restype, self.L.mpw_select.argtypes = _i, [_dp, _i64, _i, _i, _dp, _dp]
        self.L.mpw_reduce.restype, self.L.mpw_reduce.argtypes = _i, [_dp, _i64, _i, _dp]

    def cells(self, c, z=None, chunks=None):
        """the case's chunks, one launch each, into z (a canary matrix unless given)"""
        n, n_obs = c.status.size, c.g.size
        z = np.full((n_obs, n), CANARY) if z is None else z
        arr = [np.ascontiguousarray(a) for a in (c.g, c.dx, c.idt, c.y, c.yerr)]
        for lo, cnt in (chunks or c.chunks):
            ltot = np.ascontiguousarray(c.ltot[lo:lo + cnt])
            st = np.ascontiguousarray(c.status[lo:lo + cnt])
            rc = self.L.mpw_cells(_d(ltot), st.ctypes.data_as(_ip), arr[0].ctypes.data_as(_ip), _d(arr[1]), _d(arr[2]), _d(arr[3]),
                                  _d(arr[4]), cnt, c.t.size, n_obs, n, lo, _d(z))
            assert rc == 0, f"mpw_cells returned {rc}"
        return z

    def select(self, z, stride=None, want_tail=True):
        z = np.ascontiguousarray(z)
        n_obs, n = z.shape
        stride = pr.tail_len(n) if stride is None else stride
        obs = np.full((n_obs, pr.N), CANARY)
        tail = np.full((n_obs, stride), CANARY)
        rc = self.L.mpw_select(_d(z), n, n_obs, stride, _d(obs), _d(tail) if want_tail else None)
        assert rc == 0, f"mpw_select returned {rc}"
        return obs, tail

    def reduce(self, z, obs):
        z, obs = np.ascontiguousarray(z), np.array(obs)
        rc = self.L.mpw_reduce(_d(z), z.shape[1], z.shape[0], _d(obs))
        assert rc == 0, f"mpw_reduce returned {rc}"
        return obs


@pytest.fixture(scope="module")
def probe():
    return Probe()


def test_probe_shares_the_restatement_constants(probe):
    L = probe.L
    assert L.mpw_threads() == pr.THREADS and L.mpw_tile() == 64 and L.mpw_columns() == pr.N
    assert L.mpw_max_tail() == pr.MAX_TAIL == pr.tail_len(pr.MAX_SAMPLES) <= L.mpw_sort_cap() == 2048
    for n in (-1, 0, 1, 2, 5, 6, 224, 225, 226, 4096, 100000, pr.MAX_SAMPLES):
        assert L.mpw_tail_len(n) == pr.tail_len(n)
    assert L.mpw_max_rows() >= max(pc.SAMPLES) and L.mpw_max_obs() >= max(pc.N_OBS)
    z, obs = np.zeros((2, 8)), np.zeros((2, pr.N))
    assert L.mpw_select(None, 8, 2, 3, _d(obs), None) == -1
    assert L.mpw_select(_d(z), 0, 2, 3, _d(obs), None) == -1
    assert L.mpw_select(_d(z), 8, 2, 2, _d(obs), None) == -1          # a tail row shorter than T(8) = 3
    assert L.mpw_reduce(_d(z), 8, 0, _d(obs)) == -1
    g = np.array([5, 7], dtype=np.int32)
    one = np.ones(2)
    st = np.zeros(1, dtype=np.int32)
    lt = np.ones((1, 7))
    assert L.mpw_cells(_d(lt), st.ctypes.data_as(_ip), g.ctypes.data_as(_ip), _d(one), _d(one), _d(one), _d(one), 1, 7, 2, 1, 0,
                       _d(z)) == -1                                    # g = 7 is outside a grid of 7 points: refused, not launched


@pytest.mark.parametrize("name", pc.names())
def test_kernels_equal_the_restatement(probe, name):
    c, z_want = pc.case(name)
    n_obs, n = z_want.shape
    # cells
    z = probe.cells(c)
    assert not np.any(z == CANARY)
    bad = np.argwhere(~((z == z_want) | (np.isnan(z) & np.isnan(z_want))) | (np.signbit(z) != np.signbit(z_want)) & ~np.isnan(z))
    assert bad.size == 0, (name, bad[:5], [(z[j, s], z_want[j, s]) for j, s in bad[:5]])
    # select
    want_obs, want_tail = pr.pointwise(z_want)
    obs, tail = probe.select(z_want)
    assert not np.any(tail == CANARY) and not np.any(obs[:, pr.CUT] == CANARY)
    assert np.all(np.delete(obs, pr.CUT, axis=1) == CANARY)             # its only column
    assert same(obs[:, pr.CUT], want_obs[:, pr.CUT]), (name, obs[:, pr.CUT], want_obs[:, pr.CUT])
    badt = [j for j in range(n_obs) if not same(tail[j], want_tail[j])]
    assert not badt, (name, badt[:5], tail[badt[0]], want_tail[badt[0]])
    # reduce, with the select kernel's cut in place
    obs = probe.reduce(z_want, obs)
    assert not np.any(obs == CANARY)
    for col in pr.EXACT:
        assert same(obs[:, col], want_obs[:, col]), (name, col, obs[:, col], want_obs[:, col])
    d = pr.definition(z_want)
    worst = 0.0
    for mcol, scol, key in ((pr.LPPD_M, pr.LPPD_S, "lppd"), (pr.NONTAIL_M, pr.NONTAIL_S, "nontail")):
        for j in range(n_obs):
            want = d[key][j]
            err = lse_error(obs[j, mcol], obs[j, scol], want)
            lim = lse_bound(n, float(want)) if np.isfinite(want) else 0.0
            print(f"{name} {key}[{j}]: |log S + M - want| = {err:.3e}, bound {lim:.3e}") if err > lim else None
            assert err <= lim, (name, key, j, err, lim)
            if lim:
                worst = max(worst, err / lim)
    print(f"{name}: device log-sum-exp worst/bound {worst:.3f}")


def test_chunking_and_tail_stride_do_not_show(probe):
    c, z_want = pc.case("failed_between")
    n = c.status.size
    whole = probe.cells(c, chunks=((0, n),))
    parts = probe.cells(c, chunks=((0, 1), (1, 63), (64, 64), (128, 129)))
    assert same(whole, z_want) and same(parts, z_want)
    # a chunk writes its own columns only
    z = probe.cells(c, chunks=((64, 64),))
    assert same(z[:, 64:128], z_want[:, 64:128]) and np.all(z[:, :64] == CANARY) and np.all(z[:, 128:] == CANARY)
    # a wider tail row is NaN behind the tail; without a tail row the cut is the same
    _, want_tail = pr.pointwise(z_want)
    obs, tail = probe.select(z_want, stride=100)
    T = want_tail.shape[1]
    assert same(tail[:, :T], want_tail) and np.all(np.isnan(tail[:, T:]))
    obs2, _ = probe.select(z_want, want_tail=False)
    assert same(obs2[:, pr.CUT], obs[:, pr.CUT])
    # the order of the samples moves no order-free column and no tail
    perm = np.random.default_rng(8).permutation(n)
    zp = np.ascontiguousarray(z_want[:, perm])
    obs_p, tail_p = probe.select(zp)
    assert same(tail_p, want_tail)
    full, full_p = probe.reduce(z_want, obs2), probe.reduce(zp, obs_p)
    for col in pr.ORDER_FREE:
        assert same(full[:, col], full_p[:, col]), col
