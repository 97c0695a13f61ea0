"""The four kernels of the autocorrelation monitor on their own (magprop_amd/csrc/mp_acf.hip: acf_ingest_kernel,
acf_accumulate_kernel, acf_rho_kernel, acf_final_kernel), on the cases of tests/acf_cases.py: rings that wrap many times from
any first row, chunks of every length around the lag block, junk rows around a chunk, finalisations between chunks, every
max_lag around a multiple of the lag block, series counts around the workgroup, constant, stuck, huge, tiny, NaN and infinite
values, and the corners of the window rule.  They are reached through the probe library libmp_probe_acf.so
(csrc/mp_probe_acf.hip), which is test infrastructure, no part of the product's ABI, and linked from the product's own kernel
object.  The reference is the numpy restatement (tests/acf_restated.py) and everything is compared bit for bit on every element
(NaNs by position): the header promises it, so there is no tolerance here.  tests/test_acf_cases_cpu.py checks the cases and the
restatement themselves."""
import ctypes as C
import os

import numpy as np
import pytest

import acf_cases as ac
import probe_lib

pytestmark = pytest.mark.gpu

_dp, _ip, _i, _d = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_int, C.c_double
GETTERS = ("mpa_lag_block", "mpa_threads", "mpa_max_lag", "mpa_max_ndim", "mpa_max_series", "mpa_max_rows", "mpa_max_chunks",
           "mpa_max_lead", "mpa_max_ring", "mpa_max_ring_doubles")
OUTS = ("S", "T", "H", "pivot", "hist", "rho", "f", "tau", "window")


def _p(a):
    assert a.flags.c_contiguous
    return a.ctypes.data_as({np.dtype(np.float64): _dp, np.dtype(np.int32): _ip}[a.dtype])


def _i32(v):
    return np.ascontiguousarray(v, dtype=np.int32)


class Probe:
    """libmp_probe_acf.so behind numpy arrays.  The raw function is .L.mpa_run_monitor; run() raises unless it returns 0."""

    def __init__(self):
        from magprop_amd import _capi
        _capi.lib()                                        # first, so that one HIP runtime is shared
        self.L = probe_lib.load("acf")
        for name in GETTERS:
            getattr(self.L, name).restype = _i
            getattr(self.L, name).argtypes = []
        self.L.mpa_run_monitor.restype = _i
        self.L.mpa_run_monitor.argtypes = [_dp] + [_i] * 8 + [_ip] * 3 + [_d, _d] + [_dp] * 8 + [_ip]

    def raw(self, case, run, o, /, null=None, **kw):
        """One call with the arguments of (case, run), any of them replaced through kw; null: the index of a pointer to pass as
        NULL (0: x; 1 .. 3: chunk_rows, lead, finalise_after; 4 ..: OUTS)."""
        x = np.ascontiguousarray(case.x.reshape(len(case.x), -1))
        a = dict(n=len(case.x), n_walkers=case.n_walkers, n_ensembles=case.n_ensembles, ndim=case.ndim, max_lag=case.max_lag,
                 ring_rows=run.ring_rows, head0=run.head0, n_chunks=len(run.chunk_rows), chunk_rows=run.chunk_rows, lead=run.lead,
                 finalise_after=run.finalise_after, c_mid=run.c_mid, c=case.c)
        a.update(kw)
        ptrs = [_p(x)] + [_p(_i32(a[k])) for k in ("chunk_rows", "lead", "finalise_after")] + [_p(o[k]) for k in OUTS]
        if null is not None:
            ptrs[null] = None
        return self.L.mpa_run_monitor(ptrs[0], a["n"], a["n_walkers"], a["n_ensembles"], a["ndim"], a["max_lag"], a["ring_rows"], a["head0"],
                                      a["n_chunks"], ptrs[1], ptrs[2], ptrs[3], a["c_mid"], a["c"], *ptrs[4:])

    def run(self, c, run):
        o = ac.outputs(c, run)
        rc = self.raw(c, run, o)
        assert rc == 0, f"mpa_run_monitor returned {rc}"
        return o


@pytest.fixture(scope="module")
def probe():
    return Probe()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    """The same bits everywhere but in NaNs, and NaNs at the same places (the canary is a NaN and is compared as one)."""
    if a.dtype != np.float64:
        return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(_bits(a)[~np.isnan(a)], _bits(b)[~np.isnan(b)])


def canary_at(a):
    return _bits(a) == _bits(ac.NAN_CANARY)


# ---------------------------------------------------------------- argument checks of the probe itself
def test_probe_refuses_what_the_product_refuses(probe):
    L = probe.L
    assert [getattr(L, g)() for g in GETTERS[:4]] == [ac.LAG_BLOCK, ac.THREADS, ac.ACF_MAX_LAG, ac.MAX_NDIM]
    max_series, max_rows, max_chunks, max_lead, max_ring, max_ring_doubles = (getattr(L, g)() for g in GETTERS[4:])
    assert max_series >= max(ac.n_series(c) for c in ac.CASES) and max_rows >= max(len(c.x) for c in ac.CASES)
    c = ac.BY_NAME["lag-17"]
    run = next(r for r in c.runs if r.name.startswith("by17"))
    nch, kp = len(run.chunk_rows), ac.kp_of(c.max_lag)
    short = list(run.chunk_rows)
    short[0] -= 1
    neg = list(run.chunk_rows)
    neg[0], neg[1] = -1, neg[1] + neg[0] + 1
    bad = [dict(n_walkers=0), dict(n_walkers=-2), dict(n_walkers=3), dict(n_walkers=1), dict(n_ensembles=0), dict(n_ensembles=-1),
           dict(ndim=0), dict(ndim=-1), dict(ndim=ac.MAX_NDIM + 1), dict(n_walkers=max_series + 2), dict(n_ensembles=max_series),
           dict(max_lag=0), dict(max_lag=-1), dict(max_lag=ac.ACF_MAX_LAG + 1), dict(n=1, chunk_rows=[1], n_chunks=1, lead=[0], finalise_after=[0]),
           dict(n=0), dict(n=-5), dict(n=max_rows + 1), dict(c=0.0), dict(c=-5.0), dict(c=np.nan), dict(c=np.inf), dict(c_mid=0.0),
           dict(c_mid=np.nan), dict(c_mid=np.inf), dict(head0=-1), dict(head0=run.ring_rows), dict(ring_rows=0), dict(ring_rows=-1),
           dict(ring_rows=max_ring + 1), dict(ring_rows=max_ring_doubles // ac.n_series(c) + 1), dict(ring_rows=kp + max(run.chunk_rows) - 1),
           dict(ring_rows=kp - 1, head0=0), dict(n_chunks=0), dict(n_chunks=-1), dict(n_chunks=max_chunks + 1), dict(n_chunks=nch - 1),
           dict(chunk_rows=short), dict(chunk_rows=neg), dict(lead=[-1] + [0] * (nch - 1)), dict(lead=[max_lead + 1] + [0] * (nch - 1))]
    for kw in bad:
        o = ac.outputs(c, run)
        assert probe.raw(c, run, o, **kw) == -1, kw
        assert all(np.all(canary_at(o[k])) for k in OUTS[:-1]) and np.all(o["window"] == ac.ICANARY), kw
    for k in range(4 + len(OUTS)):
        o = ac.outputs(c, run)
        assert probe.raw(c, run, o, null=k) == -1, k
        assert all(np.all(canary_at(o[k])) for k in OUTS[:-1]) and np.all(o["window"] == ac.ICANARY)


# ---------------------------------------------------------------- the cases
@pytest.mark.parametrize("case", ac.CASES, ids=lambda c: c.name)
def test_kernels_equal_the_restatement_bit_for_bit(probe, case):
    """Every run of the case: S, T, H, pivot, the ring, rho, f, tau and window equal the restatement on every element; what no
    kernel defines keeps its canary (f from lag min(n, max_lag) on); so every chunking, first row, junk and intermediate
    finalisation of the sequence gives the same outputs."""
    want = ac.expected(case)
    n, K = len(case.x), case.max_lag
    lim = min(n, K)
    first = None
    for run in case.runs:
        got = probe.run(case, run)
        for key in ("S", "T", "H", "pivot", "rho", "tau", "window"):
            assert not np.any(canary_at(got[key])) if key != "window" else not np.any(got[key] == ac.ICANARY), (run.name, key)
            assert same(got[key], want[key]), (run.name, key, got[key], want[key])
        assert np.all(canary_at(got["f"][:, lim:])) and not np.any(canary_at(got["f"][:, :lim])), run.name
        assert same(got["f"][:, :lim], want["f"][:, :lim]), (run.name, "f")
        assert same(got["hist"], ac.expected_hist(case, run)), (run.name, "hist")
        if first is None:
            first = got
        for key in OUTS:
            if key != "hist":
                assert same(got[key], first[key]), (run.name, key)


@pytest.mark.parametrize("case", [c for c in ac.CASES if c.poison], ids=lambda c: c.name)
def test_a_nan_or_an_infinity_poisons_its_own_dimension_only(probe, case):
    """One NaN or +inf in one sample of one series: tau and f of its (ensemble, dimension) are NaN, and every other (ensemble,
    dimension) and every other series is bit for bit what the same sequence without it gives, whatever the run."""
    base = ac.BY_NAME[case.base]
    t, e, w, d = case.poison
    one = e * case.ndim + d
    j = (e * case.n_walkers + w) * case.ndim + d
    others, series = np.delete(np.arange(case.n_ensembles * case.ndim), one), np.delete(np.arange(ac.n_series(case)), j)
    lim = min(len(case.x), case.max_lag)
    for run, base_run in zip(case.runs, base.runs):
        assert run == base_run
        got, clean = probe.run(case, run), probe.run(base, base_run)
        assert np.isnan(got["tau"][one]) and np.all(np.isnan(got["f"][one, :lim])) and np.all(np.isfinite(clean["tau"])), run.name
        for key in ("tau", "window", "f"):
            assert same(got[key][others], clean[key][others]), (run.name, key)
        for key in ("S", "H", "rho", "hist"):
            assert same(got[key][:, series], clean[key][:, series]), (run.name, key)
        for key in ("T", "pivot"):
            assert same(got[key][series], clean[key][series]), (run.name, key)
