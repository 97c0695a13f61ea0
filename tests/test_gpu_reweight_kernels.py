"""The three kernels of the importance reweighting on their own (magprop_amd/csrc/mp_reweight.hip: reweight_rows_kernel,
reweight_select_kernel, reweight_reduce_kernel) on the cases of tests/reweight_cases.py.  The kernels are reached through the
probe library libmp_probe_reweight.so (csrc/mp_probe_reweight.hip), which is test infrastructure, no part of the product's ABI,
and linked from the product's own kernel object.

The reference is the numpy restatement (tests/reweight_restated.py) with the device runtime's log, log1p and exp (mpr_libm), so
that every number -- the log weights, the cut, the tail and all twelve columns, the S halves of the log-sum-exp pairs included --
is compared bit for bit (NaNs by position, signs of zero included).  Every output buffer starts as a canary the kernel must
overwrite."""
import ctypes as C

import numpy as np
import pytest

import pointwise_restated as pr
import probe_lib
import reweight_cases as rc
import reweight_restated as rr
from raw_abi import dp, ip

pytestmark = pytest.mark.gpu

CANARY = -777.0


def same(a, b):
    """bit for bit, NaN equal to NaN"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


class Probe:
    """libmp_probe_reweight.so behind numpy arrays"""

    def __init__(self):
        from magprop_amd import _capi
        _capi.lib()                                        # first, so that one HIP runtime is shared
        self.L = probe_lib.load("reweight")
        self.L.mpr_libm.argtypes = [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int]
        self.L.mpr_rows.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int32)] + [C.POINTER(C.c_double)] * 4 + \
            [C.c_int] * 4 + [C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int64, C.c_int64, C.POINTER(C.c_double)]
        self.L.mpr_cols.argtypes = [C.POINTER(C.c_double), C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        self.libm = rr.Libm(log=self._fn(0), log1p=self._fn(1), exp=self._fn(2))

    def _fn(self, func):
        def f(x):
            a = np.ascontiguousarray(np.asarray(x, dtype=np.float64)).ravel()
            out = np.empty(a.size)
            if a.size:
                assert self.L.mpr_libm(func, dp(a), dp(out), a.size) == 0
            return out.reshape(np.shape(x))
        return f

    def rows(self, c, lw=None, chunks=None, obs_w="case"):
        """the case's rows, one launch per chunk (lo, cnt), into lw (a canary matrix unless given)"""
        n, n_obs, n_alt = c.status.size, c.g.size, c.kind.size
        lw = np.full((n_alt, n), CANARY) if lw is None else lw
        w = c.obs_w if isinstance(obs_w, str) else obs_w
        w = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
        arr = [np.ascontiguousarray(a) for a in (c.g, c.dx, c.idt, c.y, c.yerr, c.kind, c.alt)]
        for lo, cnt in (chunks or ((0, n),)):
            ltot, st = np.ascontiguousarray(c.ltot[lo:lo + cnt]), np.ascontiguousarray(c.status[lo:lo + cnt])
            rc_ = self.L.mpr_rows(dp(ltot), ip(st), ip(arr[0]), dp(arr[1]), dp(arr[2]), dp(arr[3]), dp(arr[4]), cnt, c.t.size, n_obs,
                                  n_alt, ip(arr[5]), dp(arr[6]), dp(w), n, lo, dp(lw))
            assert rc_ == 0, f"mpr_rows returned {rc_}"
        return lw

    def cols(self, lw, stride=None, want_tail=True):
        lw = np.ascontiguousarray(lw)
        n_alt, n = lw.shape
        stride = pr.tail_len(n) if stride is None else stride
        out, tail = np.full((n_alt, rr.N), CANARY), np.full((n_alt, stride), CANARY)
        rc_ = self.L.mpr_cols(dp(lw), n, n_alt, stride, dp(out), dp(tail) if want_tail else None)
        assert rc_ == 0, f"mpr_cols returned {rc_}"
        return out, tail


@pytest.fixture(scope="module")
def probe():
    return Probe()


def want_rows(probe, c):
    return rr.rows(c.ltot, c.status, c.g, c.dx, c.idt, c.y, c.yerr, c.kind, c.alt, c.obs_w, probe.libm)


def test_probe_shares_the_restatement_constants(probe):
    L = probe.L
    assert L.mpr_group() == rc.GROUP and L.mpr_threads() == rr.THREADS and L.mpr_columns() == rr.N and L.mpr_max_alt() == rr.MAX_ALT
    assert L.mpr_max_rows() >= max(rc.COLUMN_N) and L.mpr_max_obs() >= max(rc.N_OBS)
    x = np.array([1.0, 2.5, 1e-300, 4.9e-324])
    assert np.allclose(probe.libm.log(x), np.log(x), rtol=4e-16) and probe.libm.log(1.0) == 0.0 and probe.libm.log1p(0.0) == 0.0
    assert np.allclose(probe.libm.log1p(np.array([1e-12, 0.5, 1e9])), np.log1p(np.array([1e-12, 0.5, 1e9])), rtol=4e-16)
    assert probe.libm.exp(0.0) == 1.0 and L.mpr_libm(3, dp(x), dp(x), 4) == -1
    # refused, not launched: a bracket outside the grid, a bad alternative, a bad weight, a tail row shorter than T(n)
    c = rc.row_case("obs1_rows1_alt1")
    lw = np.zeros((1, 1))

    def rows(**kw):
        a = dict(g=c.g, kind=c.kind, alt=c.alt, w=None, n_alt=1)
        a.update(kw)
        return L.mpr_rows(dp(c.ltot), ip(c.status), ip(np.ascontiguousarray(a["g"], dtype=np.int32)), dp(c.dx), dp(c.idt), dp(c.y), dp(c.yerr),
                          1, c.t.size, 1, a["n_alt"], ip(np.ascontiguousarray(a["kind"], dtype=np.int32)),
                          dp(np.ascontiguousarray(a["alt"], dtype=np.float64)), dp(a["w"]), 1, 0, dp(lw))
    assert rows() == 0
    assert rows(g=[c.t.size - 1]) == -1 and rows(kind=[2]) == -1 and rows(alt=[[0.0, 0.0, 0.0]]) == -1
    assert rows(w=np.array([-1.0])) == -1 and rows(n_alt=65) == -1 and rows(n_alt=0) == -1
    out = np.zeros((1, rr.N))
    assert L.mpr_cols(dp(np.zeros((1, 8))), 8, 1, 2, dp(out), None) == -1


@pytest.mark.parametrize("name", rc.row_names())
def test_rows_equal_the_restatement(probe, name):
    c = rc.row_case(name)
    lw = probe.rows(c)
    want = want_rows(probe, c)
    assert not np.any(lw == CANARY)
    bad = np.argwhere(~((lw.view(np.uint64) == want.view(np.uint64)) | (np.isnan(lw) & np.isnan(want))))
    assert bad.size == 0, (name, bad[:5], [(lw[k, s], want[k, s]) for k, s in bad[:5]])
    ok = c.status == 0
    assert np.all(np.isnan(lw[:, ~ok]))
    if c.obs_w is None and tuple(c.alt[0]) == (1.0, 0.0, 0.0) and c.kind[0] == rr.GAUSS and c.definition:
        assert same(lw[0, ok], np.zeros(int(ok.sum())))     # the identity alternative: exactly +0.0


def test_rows_do_not_depend_on_chunks_places_or_company(probe):
    c = rc.row_case("failed_rows")
    n = c.status.size
    whole = probe.rows(c)
    parts = probe.rows(c, chunks=((0, 1), (1, 3), (4, 4), (8, 1)))
    assert same(whole, parts)
    # a chunk writes its own columns only
    lw = probe.rows(c, chunks=((4, 4),))
    assert same(lw[:, 4:8], whole[:, 4:8]) and np.all(lw[:, :4] == CANARY) and np.all(lw[:, 8:] == CANARY)
    # an alternative's row is the same alone, whatever group it sat in, and the rows reversed give the reversed sums
    for k in (0, rc.GROUP - 1, rc.GROUP):
        one = c._replace(kind=c.kind[k:k + 1], alt=c.alt[k:k + 1], obs_w=c.obs_w[k:k + 1])
        assert same(probe.rows(one)[0], whole[k]), k
    rev = c._replace(ltot=c.ltot[::-1], status=c.status[::-1])
    assert same(probe.rows(rev), whole[:, ::-1])
    # weights of 1 are no weights
    c2 = rc.row_case("obs65_rows5_alt9")
    assert same(probe.rows(c2, obs_w=np.ones((c2.kind.size, c2.g.size))), probe.rows(c2))


def test_leave_one_out_is_minus_the_base_term(probe):
    c = rc.row_case("leave_one_out")
    gauss1 = c._replace(kind=np.zeros_like(c.kind), alt=np.tile([1.0, 0.0, 0.0], (c.kind.size, 1)))
    lw = probe.rows(gauss1)
    mod, res = rr.model(c.ltot, c.g, c.dx, c.idt, c.y)
    t0 = rr.base_term(mod, res, c.yerr, probe.libm)
    for k in range(c.kind.size):
        assert same(lw[k], -t0[:, k % c.g.size]), k


@pytest.mark.parametrize("n", rc.COLUMN_N)
def test_columns_equal_the_restatement(probe, n):
    lw = rc.column_case(n)
    want, want_tail = rr.cols(lw, libm=probe.libm)
    out, tail = probe.cols(lw)
    assert not np.any(out == CANARY) and not np.any(tail == CANARY)
    for col in range(rr.N):
        assert same(out[:, col], want[:, col]), (n, col, out[:, col], want[:, col])
    badt = [k for k in range(lw.shape[0]) if not same(tail[k], want_tail[k])]
    assert not badt, (n, badt, tail[badt[0]], want_tail[badt[0]])


def test_columns_tail_stride_and_alternative_count(probe):
    lw = rc.column_case(257)
    out, tail = probe.cols(lw)
    wide, wide_tail = probe.cols(lw, stride=100)
    T = tail.shape[1]
    assert same(wide, out) and same(wide_tail[:, :T], tail) and np.all(np.isnan(wide_tail[:, T:]))
    none, _ = probe.cols(lw, want_tail=False)
    assert same(none, out)
    # an alternative's row of the table is its column's alone: 64 alternatives, each the same as on its own
    many = np.ascontiguousarray(np.tile(lw, (8, 1)))
    out64, tail64 = probe.cols(many)
    assert same(out64, np.tile(out, (8, 1))) and same(tail64, np.tile(tail, (8, 1)))
