"""The kernels that decide which values a result is built from, one launch at a time: band_transpose_kernel and
band_select_kernel (magprop_amd/csrc/mp_band.hip), nest_select_kernel (mp_nest.hip) and opt_reduce_kernel (mp_opt.hip), on the
cases of tests/select_cases.py: ties, NaNs, infinities, keys that differ in one digit, sizes around every stride and threshold.
They are reached through the probe library libmp_probe_select.so (csrc/mp_probe_select.hip), which is test infrastructure, no
part of the product's ABI, and linked from the product's own kernel objects.  References: np.nanquantile and the restated rule of
mp_band.h; tests/nest_restated.py's select step; tests/de_restated.py's reduce.  Everything is compared bit for bit but ln X and
ln Z (rtol 1e-14 as in tests/test_gpu_nested.py: the device's log1p / exp / expm1 are not numpy's); every assertion is on
every element.  tests/test_select_cases_cpu.py checks the cases and the references themselves."""
import ctypes as C
import os
import warnings

import numpy as np
import pytest

import probe_lib
import select_cases as sc

pytestmark = pytest.mark.gpu

_dp, _ip, _lp, _i, _d = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.c_int, C.c_double
GETTERS = ("mps_band_max_samples", "mps_band_max_q", "mps_band_max_grid", "mps_nest_min_live", "mps_nest_max_live", "mps_opt_min_pop",
           "mps_opt_max_pop", "mps_max_ndim", "mps_max_runs", "mps_max_chunk")


NAN_CANARY = np.array([0x7FF8C0FFEE15BAD1], dtype=np.uint64).view(np.float64)[0]


def _p(a):
    assert a.flags.c_contiguous and a.flags.writeable
    return a.ctypes.data_as({np.dtype(np.float64): _dp, np.dtype(np.int32): _ip, np.dtype(np.int64): _lp}[a.dtype])


class Probe:
    """libmp_probe_select.so behind numpy arrays.  The raw functions are in .L; the methods raise unless the probe returns 0."""

    def __init__(self):
        from magprop_amd import _capi
        _capi.lib()                                        # first, so that one HIP runtime is shared
        self.L = probe_lib.load("select")
        for name in GETTERS:
            getattr(self.L, name).restype = _i
            getattr(self.L, name).argtypes = []
        self.L.mps_band_transpose.argtypes = [_dp, _dp, _i, _i]
        self.L.mps_band_select.argtypes = [_dp, _i, _i, _dp, _i, _dp]
        self.L.mps_nest_select.argtypes = [_i] * 7 + [_d, _dp, _dp, _ip, _ip, _dp, _dp, _dp, _ip, _dp, _dp, _ip, _ip]
        self.L.mps_opt_reduce.argtypes = [_i] * 4 + [_d, _d, _dp, _dp, _dp, _dp, _ip, _ip, _ip, _ip, _ip, _lp]
        for name in ("mps_band_transpose", "mps_band_select", "mps_nest_select", "mps_opt_reduce"):
            getattr(self.L, name).restype = _i

    def transpose(self, src):
        src = np.ascontiguousarray(src, dtype=np.float64)
        dst = np.full(src.shape[::-1], np.nan)
        rc = self.L.mps_band_transpose(_p(src), _p(dst), *src.shape)
        assert rc == 0, f"mps_band_transpose returned {rc}"
        return dst

    def band(self, cols, q):
        cols, q = np.ascontiguousarray(cols, dtype=np.float64), np.ascontiguousarray(q, dtype=np.float64)
        out = np.full((q.size, cols.shape[0]), NAN_CANARY)  # (NaN is a result of this kernel: the canary is a NaN no arithmetic makes)
        rc = self.L.mps_band_select(_p(cols), cols.shape[1], cols.shape[0], _p(q), q.size, _p(out))
        assert rc == 0, f"mps_band_select returned {rc}"
        return out

    def nest(self, c):
        o = sc.nest_outputs(c)
        live, lnl = np.ascontiguousarray(c.live), np.ascontiguousarray(c.lnl)
        rc = self.L.mps_nest_select(c.nlive, c.nbatch, c.n_runs, c.ndim, c.mode, c.slot, c.chunk, c.dlogz, _p(live), _p(lnl),
                                    _p(o["dead_slot"]), _p(o["surv"]), _p(o["lstar"]), _p(o["dead_pars"]), _p(o["dead_lnl"]),
                                    _p(o["dead_n"]), _p(o["lnx"]), _p(o["lnz"]), _p(o["stopped"]), _p(o["nit"]))
        assert rc == 0, f"mps_nest_select returned {rc}"
        return o

    def opt(self, c):
        o = sc.opt_outputs(c)
        rc = self.L.mps_opt_reduce(c.popsize, c.n_pops, c.ndim, c.trial, c.tol, c.atol, _p(o["pop_cur"]), _p(o["pop_next"]),
                                   _p(o["lnp_cur"]), _p(o["lnp_next"]), _p(o["st_cur"]), _p(o["st_next"]), _p(o["best"]),
                                   _p(o["converged"]), _p(o["nit"]), _p(o["nfev"]))
        assert rc == 0, f"mps_opt_reduce returned {rc}"
        return o


@pytest.fixture(scope="module")
def probe():
    return Probe()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits_or_nan(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(_bits(a)[~np.isnan(a)], _bits(b)[~np.isnan(b)])


# ---------------------------------------------------------------- argument checks of the probe itself
def test_probe_refuses_bad_sizes(probe):
    L = probe.L
    assert [getattr(L, g)() for g in GETTERS[:8]] == [sc.BAND_MAX_SAMPLES, sc.BAND_MAX_Q, 1 << 16, sc.NEST_MIN_LIVE, sc.NEST_MAX_LIVE,
                                                       sc.OPT_MIN_POP, sc.OPT_MAX_POP, sc.MAX_NDIM]
    max_runs, max_chunk = L.mps_max_runs(), L.mps_max_chunk()
    x, y, q = np.ones(64), np.full(64, 7.0), np.full(17, 0.5)
    for n, g in ((0, 1), (-1, 1), (sc.BAND_MAX_SAMPLES + 1, 1), (1, 0), (1, -3), (1, (1 << 16) + 1)):
        assert L.mps_band_transpose(_p(x), _p(y), n, g) == -1
        assert L.mps_band_select(_p(x), n, g, _p(q), 1, _p(y)) == -1
    for nq in (0, -1, sc.BAND_MAX_Q + 1):
        assert L.mps_band_select(_p(x), 8, 8, _p(q), nq, _p(y)) == -1
    for bad in (-2.0 ** -1074, np.nextafter(1.0, 2.0), np.nan, np.inf):
        assert L.mps_band_select(_p(x), 8, 8, _p(np.array([0.5, bad])), 2, _p(y)) == -1
    assert L.mps_band_transpose(None, _p(y), 8, 8) == L.mps_band_transpose(_p(x), None, 8, 8) == -1
    assert L.mps_band_select(None, 8, 8, _p(q), 1, _p(y)) == L.mps_band_select(_p(x), 8, 8, None, 1, _p(y)) == -1
    assert L.mps_band_select(_p(x), 8, 8, _p(q), 1, None) == -1
    assert np.all(y == 7.0)

    c = next(c for c in sc.NEST_CASES if c.name == "nest-distinct-n16-k2")

    def nest(o=None, null=None, **kw):
        o = o or sc.nest_outputs(c)
        a = dict(nlive=c.nlive, nbatch=c.nbatch, n_runs=c.n_runs, ndim=c.ndim, mode=c.mode, slot=c.slot, chunk=c.chunk)
        a.update(kw)
        ptrs = [_p(np.ascontiguousarray(c.live)), _p(np.ascontiguousarray(c.lnl))] + \
            [_p(o[k]) for k in ("dead_slot", "surv", "lstar", "dead_pars", "dead_lnl", "dead_n", "lnx", "lnz", "stopped", "nit")]
        if null is not None:
            ptrs[null] = None
        return L.mps_nest_select(a["nlive"], a["nbatch"], a["n_runs"], a["ndim"], a["mode"], a["slot"], a["chunk"], c.dlogz, *ptrs)

    for kw in (dict(nlive=sc.NEST_MIN_LIVE - 1, nbatch=1), dict(nlive=sc.NEST_MAX_LIVE + 1), dict(nlive=0), dict(nlive=-16),
               dict(nbatch=0), dict(nbatch=-1), dict(nbatch=c.nlive // 2 + 1), dict(n_runs=0), dict(n_runs=max_runs + 1),
               dict(ndim=0), dict(ndim=sc.MAX_NDIM + 1), dict(mode=2), dict(mode=-1), dict(slot=-1), dict(slot=1), dict(chunk=0),
               dict(chunk=max_chunk + 1)):
        o = sc.nest_outputs(c)
        assert nest(o, **kw) == -1, kw
        assert np.all(o["dead_slot"] == sc.ICANARY) and np.all(np.isnan(o["lstar"])) and np.array_equal(o["nit"], c.nit)
    for k in range(12):
        assert nest(null=k) == -1

    c2 = next(c for c in sc.OPT_CASES if c.name == "opt-distinct-p5")

    def opt(o=None, null=None, **kw):
        o = o or sc.opt_outputs(c2)
        a = dict(popsize=c2.popsize, n_pops=c2.n_pops, ndim=c2.ndim, trial=c2.trial)
        a.update(kw)
        ptrs = [_p(o[k]) for k in ("pop_cur", "pop_next", "lnp_cur", "lnp_next", "st_cur", "st_next", "best", "converged", "nit", "nfev")]
        if null is not None:
            ptrs[null] = None
        return L.mps_opt_reduce(a["popsize"], a["n_pops"], a["ndim"], a["trial"], c2.tol, c2.atol, *ptrs)

    for kw in (dict(popsize=sc.OPT_MIN_POP - 1), dict(popsize=0), dict(popsize=-5), dict(popsize=sc.OPT_MAX_POP + 1), dict(n_pops=0),
               dict(n_pops=max_runs + 1), dict(ndim=0), dict(ndim=sc.MAX_NDIM + 1), dict(trial=2), dict(trial=-1)):
        o = sc.opt_outputs(c2)
        assert opt(o, **kw) == -1, kw
        assert np.all(o["best"] == sc.ICANARY) and np.array_equal(o["nfev"], c2.nfev)
    for k in range(10):
        assert opt(null=k) == -1


# ---------------------------------------------------------------- band
@pytest.mark.parametrize("shape", sc.TRANSPOSE_SHAPES, ids=lambda s: f"n{s[0]}-g{s[1]}")
def test_band_transpose_is_the_transpose(probe, shape):
    src = sc.transpose_input(*shape)
    assert np.array_equal(probe.transpose(src), src.T)


@pytest.mark.parametrize("case", sc.BAND_CASES, ids=lambda c: c.name)
def test_band_select_is_nanquantile_bit_for_bit(probe, case):
    """Every column against np.nanquantile: the same NaNs, the same bits (the sign of a zero with them) everywhere else; a column
    that holds both zeros (numpy leaves their order open) by value.  And every column, those included, bit for bit against
    mp_band.h's rule restated (select_cases.band_rule), which puts -0.0 first as the kernel does."""
    got = probe.band(case.cols, case.q)
    assert not np.any(_bits(got) == _bits(NAN_CANARY))                         # every element written
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        want = np.nanquantile(case.cols, case.q, axis=1).reshape(got.shape)
    for g, col in enumerate(case.cols):
        rule = sc.band_rule(col, case.q)
        assert _same_bits_or_nan(got[:, g], rule), (g, got[:, g], rule)
        if g in sc.BAND_NOT_NANQUANTILE.get(case.name, ()):
            continue
        if sc.has_both_zeros(col):
            assert np.array_equal(got[:, g], want[:, g], equal_nan=True), (g, got[:, g], want[:, g])
        else:
            assert _same_bits_or_nan(got[:, g], want[:, g]), (g, got[:, g], want[:, g])


# ---------------------------------------------------------------- nested select
@pytest.mark.parametrize("case", sc.NEST_CASES, ids=lambda c: c.name)
def test_nest_select_is_the_restated_select(probe, case):
    got, want = probe.nest(case), sc.nest_expected(case)
    for name in ("dead_slot", "surv", "dead_n", "stopped", "nit"):
        assert np.array_equal(got[name], want[name]), name
    for name in ("lstar", "dead_pars", "dead_lnl"):                            # (NaN: the canary of what must stay unwritten)
        assert np.array_equal(got[name], want[name], equal_nan=True), name
    assert not np.any(np.isnan(got["lnx"])) and not np.any(np.isnan(got["lnz"]))
    assert np.array_equal(got["lnz"] == -np.inf, want["lnz"] == -np.inf)
    assert np.allclose(got["lnx"], want["lnx"], rtol=1e-14, atol=0.0)
    assert np.allclose(got["lnz"], want["lnz"], rtol=1e-14, atol=0.0)
    for r in range(case.n_runs):                                               # untouched runs: to the bit
        if case.stopped[r] or case.mode == 1 or want["stopped"][r]:
            assert got["lnx"][r] == case.lnx[r] and got["lnz"][r] == case.lnz[r]


# ---------------------------------------------------------------- optimizer reduce
@pytest.mark.parametrize("case", sc.OPT_CASES, ids=lambda c: c.name)
def test_opt_reduce_is_the_restated_reduce(probe, case):
    got, want = probe.opt(case), sc.opt_expected(case)
    for name in ("best", "converged", "nit", "nfev", "st_cur", "st_next"):
        assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), name
    for name in ("pop_cur", "pop_next", "lnp_cur", "lnp_next"):
        assert np.array_equal(_bits(got[name]), _bits(want[name])), name
