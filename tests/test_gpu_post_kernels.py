"""The kernels of the posterior monitor on their own (magprop_amd/csrc/mp_post.hip: post_hist1_kernel, post_hist2_kernel,
post_moments_kernel, post_best_kernel, post_reset_kernel), on the cases of tests/post_cases.py: a whole ensemble in one bin, the
corners of the bin rule, non-finite coordinates, bin counts and dimensions at both ends, walker counts around a wavefront,
several ensembles, chunk lists of every kind and the corners of the best-sample rule.  They are reached through the probe
library libmp_probe_post.so (csrc/mp_probe_post.hip), which is test infrastructure, no part of the product's ABI, and linked
from the product's own kernel object.  The reference is the numpy restatement (tests/post_restated.py) and every accumulator
is compared with array_equal (NaNs by position): the header promises it, so there is no tolerance here.
tests/test_post_cases_cpu.py checks the cases and the restatement themselves."""
import ctypes as C
import os

import numpy as np
import pytest

import post_cases as pc
import probe_lib

pytestmark = pytest.mark.gpu

_dp, _ip, _lp, _i = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.c_int
OUTS = ("hist1", "hist2", "outside2", "mom", "nfin", "best_x", "best_lnp", "best_idx")


def _p(a):
    if a is None:
        return None
    assert a.flags.c_contiguous
    return a.ctypes.data_as({np.dtype(np.float64): _dp, np.dtype(np.int32): _ip, np.dtype(np.int64): _lp}[a.dtype])


class Probe:
    """libmp_probe_post.so behind numpy arrays: run(case, chunk_rows) returns the accumulators as the device holds them."""

    def __init__(self):
        from magprop_amd import _capi
        _capi.lib()                                        # first, so that one HIP runtime is shared
        self.L = probe_lib.load("post")
        for name in ("mpq_threads", "mpq_max_bins", "mpq_max_bins2", "mpq_max_ndim", "mpq_max_rows", "mpq_max_elements"):
            getattr(self.L, name).restype = _i
            getattr(self.L, name).argtypes = []
        self.L.mpq_run_posterior.restype = _i
        self.L.mpq_run_posterior.argtypes = [_dp, _dp] + [_i] * 6 + [_dp, _dp, _i, _ip, _lp, _lp, _lp, _dp, _lp, _dp, _dp, _lp]

    def outputs(self, c):
        """Buffers of the device layout's shapes, filled with a canary every kernel or memset must overwrite."""
        want = pc.device_layout(c)
        return {k: None if want[k] is None else np.full(want[k].shape, -777, dtype=want[k].dtype) for k in OUTS}

    def raw(self, c, rows, o, **kw):
        a = dict(n=len(c.chain), n_walkers=c.n_walkers, n_ensembles=c.n_ensembles, ndim=c.ndim, bins1=c.bins1, bins2=c.bins2,
                 lower=c.lower, upper=c.upper, n_chunks=len(rows))
        a.update(kw)
        chunk = np.ascontiguousarray(rows, dtype=np.int32)
        return self.L.mpq_run_posterior(_p(np.ascontiguousarray(c.chain)), _p(np.ascontiguousarray(c.lnp)), a["n"], a["n_walkers"],
                                        a["n_ensembles"], a["ndim"], a["bins1"], a["bins2"], _p(np.ascontiguousarray(a["lower"])),
                                        _p(np.ascontiguousarray(a["upper"])), a["n_chunks"], _p(chunk), *(_p(o[k]) for k in OUTS))

    def run(self, c, rows):
        o = self.outputs(c)
        rc = self.raw(c, rows, o)
        assert rc == 0, f"mpq_run_posterior returned {rc}"
        return o


@pytest.fixture(scope="module")
def probe():
    return Probe()


def same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype == np.float64)


def test_probe_refuses_what_the_product_refuses(probe):
    L = probe.L
    assert [L.mpq_threads(), L.mpq_max_bins(), L.mpq_max_bins2(), L.mpq_max_ndim()] == [pc.THREADS, pc.MAX_BINS, pc.MAX_BINS2, pc.MAX_NDIM]
    assert L.mpq_max_rows() >= max(len(c.chain) for c in pc.cases()) and L.mpq_max_elements() >= max((len(c.chain) + 2) * c.chain[0].size for c in pc.cases())
    c = pc.by_name("bins-7-and-1")
    n = len(c.chain)
    nan_lo, inf_hi, empty = c.lower.copy(), c.upper.copy(), c.upper.copy()
    nan_lo[1], inf_hi[2], empty[0] = np.nan, np.inf, c.lower[0]
    bad = [dict(n_walkers=0), dict(n_walkers=3), dict(n_ensembles=0), dict(ndim=0), dict(ndim=pc.MAX_NDIM + 1), dict(bins1=0), dict(bins1=-1),
           dict(bins1=pc.MAX_BINS + 1), dict(bins2=-1), dict(bins2=pc.MAX_BINS2 + 1), dict(n=0), dict(n=n - 1), dict(n=L.mpq_max_rows() + 1),
           dict(n_chunks=0), dict(lower=nan_lo), dict(upper=inf_hi), dict(upper=empty), dict(lower=c.upper, upper=c.lower)]
    for kw in bad:
        o = probe.outputs(c)
        assert probe.raw(c, [n], o, **kw) == -1, kw
        assert all(np.all(v == -777) for v in o.values()), kw
    o = probe.outputs(c)
    assert probe.raw(c, [n - 1], o) == -1 and probe.raw(c, [-1, n + 1], o) == -1


@pytest.mark.parametrize("case", pc.cases(), ids=lambda c: c.name)
def test_kernels_equal_the_restatement(probe, case):
    """Every run of the case: every accumulator equals the restatement on every element, so every chunking of the sequence
    gives the same accumulators."""
    want = pc.device_layout(case)
    for name, rows in case.runs.items():
        got = probe.run(case, rows)
        for key in OUTS:
            assert same(got[key], want[key]), (name, key, got[key], want[key])
