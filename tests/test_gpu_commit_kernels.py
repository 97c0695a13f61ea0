"""The sampler's deciding kernels on their own (magprop_amd/csrc/mp_kernels.hip: stretch_step_commit_kernel<TEMPERED>,
stretch_apply_kernel, stretch_swap_kernel, order_kernel), on the cases of tests/commit_cases.py: decisions with ties and
non-finite values on either side, partners in another ensemble, every beta rule, launch orders of up to 16 ensembles, sweeps of
up to 600 walkers and 8 temperatures, logs of failed proposals filled past their capacity, class thresholds of the launch order.
They are reached through the probe library libmp_probe_commit.so (csrc/mp_probe_commit.hip), which is test infrastructure, no
part of the product's ABI, and linked from the product's own kernel object.  The reference is the numpy restatement
(tests/commit_restated.py) and every output is compared with array_equal (NaNs by position): there is no tolerance here.
Two outputs are compared as sets, because the restatement itself leaves their order open: the rows of the log of failed proposals
(their order is the order of an atomic) and the order of the walkers inside a length class.
tests/test_commit_cases_cpu.py checks the cases and the restatement themselves."""
import ctypes as C
import os

import numpy as np
import pytest

import commit_cases as cc
import commit_restated as cr
import probe_lib

pytestmark = pytest.mark.gpu

_dp, _ip, _lp, _up, _i = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_uint32), C.c_int
_TYPES = {np.dtype(np.float64): _dp, np.dtype(np.int32): _ip, np.dtype(np.int64): _lp, np.dtype(np.uint32): _up}
CAPS = ("mpc_max_ndim", "mpc_spec_extra", "mpc_max_walkers", "mpc_max_ensembles", "mpc_max_total", "mpc_max_rows", "mpc_max_bad_cap",
        "mpc_max_order_n", "mpc_max_datasets")


def _p(a):
    if a is None:
        return None
    assert a.flags.c_contiguous
    return a.ctypes.data_as(_TYPES[a.dtype])


class Probe:
    """libmp_probe_commit.so behind numpy arrays.  Every run_* takes a case and keyword overrides of the probe's arguments,
    launches once and returns (code, outputs as the device holds them); the outputs go in filled as cc.state_of fills them."""

    def __init__(self):
        from magprop_amd import _capi
        _capi.lib()                                        # first, so that one HIP runtime is shared
        self.L = L = probe_lib.load("commit")
        for name in CAPS:
            getattr(L, name).restype = _i
            getattr(L, name).argtypes = []
        state, chain = [_dp, _dp, _lp, _ip], [_dp, _dp, _i, _i]
        L.mpc_commit.restype = L.mpc_apply.restype = L.mpc_swap.restype = L.mpc_order.restype = _i
        L.mpc_commit.argtypes = state + [_dp, _i, _i, _i] + chain + [_dp, _dp, _up, _i]
        L.mpc_apply.argtypes = state + [_dp, _i, _i, _i, _i, C.c_uint64] + chain + [_dp, _up, _i]
        L.mpc_swap.argtypes = state + [_dp, _i, _i, _i, _i, C.c_uint64, C.c_uint32, _lp] + chain
        L.mpc_order.argtypes = [_ip, _i, _ip, _i, _ip]
        self.launches = 0

    def _args(self, c, kw):
        a = dict(n_walkers=c.n_walkers, n_ensembles=c.n_ensembles, ndim=c.ndim, perm=c.perm, chain_row=c.chain_row, n_rows=c.chain_rows)
        a.update(kw)
        return a

    def run_commit(self, c, **kw):
        s = cc.state_of(c)
        s["bad_log"], s["bad_count"] = cc.bad_buffers(c)
        a = self._args(c, kw)
        a = dict(dict(spec=c.spec, betas=c.betas, bad_cap=c.bad_cap or 0), **a)
        rc = self.L.mpc_commit(_p(s["pos"]), _p(s["lnprob"]), _p(s["n_accepted"]), _p(np.ascontiguousarray(a["perm"])),
                               _p(np.ascontiguousarray(a["spec"])), a["n_walkers"], a["n_ensembles"], a["ndim"], _p(s["chain"]),
                               _p(s["chain_lnp"]), a["chain_row"], a["n_rows"], _p(a["betas"]), _p(s["bad_log"]), _p(s["bad_count"]),
                               a["bad_cap"])
        self.launches += rc == 0
        return rc, s

    def run_apply(self, c, **kw):
        s = cc.state_of(c)
        s["bad_log"], s["bad_count"] = cc.bad_buffers(c)
        a = self._args(c, kw)
        a = dict(dict(half=c.half, ens_order=c.ens_order, bad_cap=c.bad_cap or 0), **a)
        rc = self.L.mpc_apply(_p(s["pos"]), _p(s["lnprob"]), _p(s["n_accepted"]), _p(np.ascontiguousarray(a["perm"])), _p(c.upd),
                              a["n_walkers"], a["n_ensembles"], a["ndim"], a["half"], a["ens_order"], _p(s["chain"]), _p(s["chain_lnp"]),
                              a["chain_row"], a["n_rows"], _p(s["bad_log"]), _p(s["bad_count"]), a["bad_cap"])
        self.launches += rc == 0
        return rc, s

    def run_swap(self, c, **kw):
        s = cc.state_of(c)
        s["n_swaps"] = c.swaps0.copy()
        a = self._args(c, kw)
        a = dict(dict(n_temps=c.n_temps, betas=c.betas), **a)
        rc = self.L.mpc_swap(_p(s["pos"]), _p(s["lnprob"]), _p(s["n_accepted"]), _p(np.ascontiguousarray(a["perm"])), _p(a["betas"]),
                             a["n_walkers"], a["n_ensembles"], a["ndim"], a["n_temps"], c.seed, c.step, _p(s["n_swaps"]), _p(s["chain"]),
                             _p(s["chain_lnp"]), a["chain_row"], a["n_rows"])
        self.launches += rc == 0
        return rc, s

    def run_order(self, c, **kw):
        a = dict(dict(n_ds=len(c.n_obs), n=len(c.ds_id)), **kw)
        out = np.full(len(c.ds_id), cc.ICANARY, dtype=np.int32)
        rc = self.L.mpc_order(_p(c.n_obs) if len(c.n_obs) else None, a["n_ds"], _p(c.ds_id), a["n"], _p(out))
        self.launches += rc == 0
        return rc, out


@pytest.fixture(scope="module")
def probe():
    return Probe()


STATE = ("pos", "lnprob", "n_accepted", "chain", "chain_lnp")


def same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype == np.float64)


def assert_state(got, want, name):
    for key in STATE:
        assert same(got[key], want[key]), (name, key)


def _sorted_rows(rows, ndim):
    rows = np.asarray(rows, dtype=np.float64).reshape(len(rows), ndim)
    return rows[np.lexsort(rows.T[::-1])]


def assert_bad_log(c, got, failed):
    """The log of failed proposals against the restatement's list.  The count is exact.  The rows are compared as a sorted multiset:
    their order is the order of an atomic, which the restatement leaves open.  Past the capacity every logged row must be one of
    the failing rows, no row more often than it failed, and the guard row behind the log keeps its canary."""
    if c.bad_cap is None:
        assert got["bad_log"] is None and got["bad_count"][0] == 0, c.name       # no log: nothing is counted either
        return
    assert got["bad_count"][0] == len(failed), (c.name, got["bad_count"], len(failed))
    log, n = got["bad_log"], min(len(failed), c.bad_cap)
    assert np.all(np.isnan(log[n:])), (c.name, "rows behind the logged ones and the guard row keep their canaries")
    want = _sorted_rows(failed, c.ndim)
    if len(failed) <= c.bad_cap:
        assert np.array_equal(_sorted_rows(log[:n], c.ndim), want), c.name
    else:
        pool = [tuple(r) for r in want]
        for r in log[:n]:
            assert tuple(r) in pool, (c.name, r)
            pool.remove(tuple(r))


def test_probe_refuses_what_the_product_refuses(probe):
    """Refused arguments return -1 and leave every canary: the sizes mp_sampler_create and the launchers refuse and every index a
    kernel would address memory with."""
    L, launches = probe.L, probe.launches
    assert [L.mpc_max_ndim(), L.mpc_spec_extra()] == [cc.MAX_NDIM, cc.SPEC_EXTRA]
    for c in cc.commit_cases() + cc.apply_cases() + cc.swap_cases():
        assert c.n_walkers <= L.mpc_max_walkers() and c.n_ensembles <= L.mpc_max_ensembles() and c.chain_rows <= L.mpc_max_rows()
        assert c.n_walkers * c.n_ensembles <= L.mpc_max_total() and (getattr(c, "bad_cap", None) or 0) <= L.mpc_max_bad_cap()
    assert all(len(c.ds_id) <= L.mpc_max_order_n() and len(c.n_obs) <= L.mpc_max_datasets() for c in cc.order_cases())

    def untouched(c, s):
        want = cc.state_of(c)
        return all(same(s[k], want[k]) for k in STATE) and (s.get("bad_log") is None or np.all(np.isnan(s["bad_log"])))

    def bad_perm(c, v):
        p = c.perm.copy()
        p[-1, 1] = v
        return p

    def bad_partner(c, blk, v):
        s = c.spec.copy()
        s[blk, -1, c.ndim + 5] = v
        return s

    c = cc.by_name("commit-258-3-ensembles")
    n_half = c.n_walkers // 2
    for kw in (dict(n_walkers=85), dict(n_walkers=0), dict(ndim=0), dict(ndim=cc.MAX_NDIM + 1), dict(n_ensembles=0),
               dict(perm=bad_perm(c, c.n_walkers)), dict(perm=bad_perm(c, -1)), dict(spec=bad_partner(c, 1, n_half)),
               dict(spec=bad_partner(c, 1, -1.0)), dict(spec=bad_partner(c, 1, np.nan)), dict(spec=bad_partner(c, 2, 1.0e10)),
               dict(spec=bad_partner(c, 0, 0.5)), dict(chain_row=3), dict(chain_row=-1), dict(n_rows=0), dict(bad_cap=-1)):
        rc, s = probe.run_commit(c, **kw)
        assert rc == -1 and untouched(c, s) and s["bad_count"][0] == 0, kw
    c = cc.by_name("apply-two-swapped")
    for kw in (dict(half=2), dict(half=-1), dict(ens_order=0x11), dict(ens_order=0x12), dict(ens_order=0x110), dict(n_walkers=7),
               dict(perm=bad_perm(c, c.n_walkers)), dict(chain_row=3), dict(ndim=0)):
        rc, s = probe.run_apply(c, **kw)
        assert rc == -1 and untouched(c, s) and s["bad_count"][0] == 0, kw
    big = cc.ApplyCase("seventeen", "", 2, 17, 1, np.zeros((34, 1)), np.zeros(34), np.zeros((17, 2), dtype=np.int32), np.zeros((17, 4)),
                       0, 0x10, 0, 0, 0)
    assert probe.run_apply(big)[0] == -1                           # ens_order != 0 with more than 16 ensembles
    c = cc.by_name("swap-62-three-groups")
    for kw in (dict(n_temps=1), dict(n_temps=0), dict(n_temps=2), dict(n_temps=4), dict(betas=None), dict(n_walkers=61),
               dict(perm=bad_perm(c, c.n_walkers)), dict(chain_row=3)):
        rc, s = probe.run_swap(c, **kw)
        assert rc == -1 and untouched(c, s) and np.array_equal(s["n_swaps"], c.swaps0), kw
    c = cc.by_name("order-12-every-length")
    for kw in (dict(n=0), dict(n=-1), dict(n_ds=-1), dict(n=L.mpc_max_order_n() + 1)):
        rc, out = probe.run_order(c, **kw)
        assert rc == -1 and np.all(out == cc.ICANARY), kw
    assert probe.launches == launches                              # nothing was launched


@pytest.mark.parametrize("case", cc.commit_cases(), ids=lambda c: c.name)
def test_commit_kernel_equals_the_restatement(probe, case):
    want, _, _, failed = cc.commit_expected(case.name)
    rc, got = probe.run_commit(case)
    assert rc == 0, f"mpc_commit returned {rc}"
    assert_state(got, want, case.name)
    assert_bad_log(case, got, failed)
    if case.twin and case.betas is not None:
        # betas all 1 through the TEMPERED build: the untempered build's outputs to the bit, device against device
        rc, plain = probe.run_commit(cc.by_name(case.twin))
        assert rc == 0
        assert_state(got, plain, case.name)
        assert plain["bad_count"][0] == got["bad_count"][0]


@pytest.mark.parametrize("case", cc.apply_cases(), ids=lambda c: c.name)
def test_apply_kernel_equals_the_restatement(probe, case):
    want, _, _, failed = cc.apply_expected(case.name)
    rc, got = probe.run_apply(case)
    assert rc == 0, f"mpc_apply returned {rc}"
    assert_state(got, want, case.name)
    assert_bad_log(case, got, failed)


@pytest.mark.parametrize("case", cc.swap_cases(), ids=lambda c: c.name)
def test_swap_kernel_equals_the_restatement(probe, case):
    want, counts, _, _ = cc.swap_expected(case.name)
    rc, got = probe.run_swap(case)
    assert rc == 0, f"mpc_swap returned {rc}"
    assert_state(got, want, case.name)                         # (n_accepted among them: the counters stay with the walkers)
    assert np.array_equal(got["n_swaps"], case.swaps0 + counts), (case.name, got["n_swaps"] - case.swaps0, counts)


@pytest.mark.parametrize("case", cc.order_cases(), ids=lambda c: c.name)
def test_order_kernel_sorts_longest_first(probe, case):
    """`order` is a permutation of 0 .. n - 1, the classes along it never fall, and every class holds the walkers the restatement
    puts there.  The order inside a class is the order of an atomic, which the restatement leaves open: each class is compared as
    a sorted set."""
    cls, counts = cr.order(case.n_obs, case.ds_id)
    rc, got = probe.run_order(case)
    assert rc == 0, f"mpc_order returned {rc}"
    n = len(case.ds_id)
    assert np.array_equal(np.sort(got), np.arange(n, dtype=np.int32)), case.name
    along = cls[got]
    assert np.all(np.diff(along) >= 0), case.name
    assert np.array_equal(np.bincount(along, minlength=len(counts)), counts)
    start = 0
    for k, m in enumerate(counts):
        assert np.array_equal(np.sort(got[start:start + m]), np.flatnonzero(cls == k)), (case.name, k)
        start += m
