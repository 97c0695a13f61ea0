"""The kernels of the sampler's sample reservoir (magprop_amd/csrc/mp_reservoir.hip res_filter_kernel, res_merge_kernel) and the
host unit that drives them (ResMonitor, mp_monitor.cpp) on the named cases of tests/reservoir_cases.py, reached through the probe
library libmp_probe_reservoir.so (csrc/mp_probe_reservoir.hip), which is test infrastructure, no part of the product's ABI, and
linked from the product's own objects, so that the code under test is what libmagprop_amd.so runs.

Held: bit for bit.  The held set is a set of (key, step, walker), all integers, and every row and lnprob is a copy, so the
restatement (tests/reservoir_restated.py) is compared for equality after the canonical sort by (step, walker); NaN cells compare
by their bytes."""
import ctypes as C

import numpy as np
import pytest

import probe_lib
import reservoir_cases as rc
import reservoir_restated as rr
from raw_abi import dp, ip, lp

pytestmark = pytest.mark.gpu


def up(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


def probe():
    """libmp_probe_reservoir.so, behind the product's library so that one HIP runtime is shared."""
    from magprop_amd import _capi
    _capi.lib()
    return probe_lib.load("reservoir")


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def run_probe(case, chunks, chain, lnp):
    n, ne, k, nd = rc.n_steps(case), case.n_ensembles, case.size, case.ndim
    x, lnprob = np.full((ne, k, nd), -7.0), np.full((ne, k), -7.0)
    step, walker, key = np.full((ne, k), -7, dtype=np.int64), np.full((ne, k), -7, dtype=np.int32), np.full((ne, k), 7, dtype=np.uint64)
    n_rows, n_seen = np.full(ne, -7, dtype=np.int32), np.full(ne, -7, dtype=np.int64)
    ch = np.ascontiguousarray(chunks, dtype=np.int32)
    rc_ = probe().mpr_run_reservoir(dp(chain), dp(lnp), n, case.n_walkers, ne, nd, k, C.c_uint64(case.seed), C.c_int64(case.discard),
                                    C.c_int64(case.step0), len(ch), ip(ch), case.restart_before, dp(x), dp(lnprob), lp(step),
                                    ip(walker), up(key), ip(n_rows), lp(n_seen))
    assert rc_ == 0, (case.name, rc_)
    return x, lnprob, step, walker, key, n_rows, n_seen


@pytest.mark.parametrize("case", rc.run_cases(), ids=lambda c: c.name)
def test_monitor_equals_the_restatement_bit_for_bit(case):
    assert probe().mpr_cand_cap() == rr.CAND_CAP
    chain, lnp = rc.run_chain(case)
    nw = case.n_walkers
    ref = rr.Reservoir(case.size, case.seed, case.discard, nw, case.n_ensembles).run(case.chunks[0], case.step0, case.restart_before)
    for chunks in case.chunks:
        x, lnprob, step, walker, key, n_rows, n_seen = run_probe(case, chunks, chain, lnp)
        for e in range(case.n_ensembles):
            t, w, k = rr.as_arrays(ref.result(e))
            rows = len(t)
            assert n_rows[e] == rows and n_seen[e] == ref.n_seen[e], (case.name, chunks, e)
            assert np.array_equal(step[e, :rows], t) and np.array_equal(walker[e, :rows], w) and np.array_equal(key[e, :rows], k), (case.name, chunks, e)
            at = (t - case.step0, e * nw + w)
            assert same_bytes(x[e, :rows], chain[at]) and same_bytes(lnprob[e, :rows], lnp[at]), (case.name, chunks, e)
            assert np.all(x[e, rows:] == -7.0) and np.all(key[e, rows:] == 7)          # (nothing written behind the rows)


def held_row(t, w, ndim):
    """What a held entry (t, w) of a merge case holds before the launch: its own mark, so that a slot that moved shows."""
    return t * 1000.0 + w + np.arange(ndim) / 16.0


@pytest.mark.parametrize("case", rc.merge_cases(), ids=lambda c: c.name)
def test_merge_kernel_on_crafted_keys(case):
    L = probe()
    ne, k, nd, nw, cap, words = len(case.held), case.size, case.ndim, case.n_walkers, 512, L.mpr_meta_words()
    chain, lnp = rc.merge_slab(case)
    key, step = np.full((ne, k), 7, dtype=np.uint64), np.full((ne, k), -7, dtype=np.int64)
    walker, x, lnprob = np.full((ne, k), -7, dtype=np.int32), np.full((ne, k, nd), -7.0), np.full((ne, k), -7.0)
    meta = np.zeros((ne, words), dtype=np.int64)
    ckey, cstep = np.zeros((ne, cap), dtype=np.uint64), np.zeros((ne, cap), dtype=np.int64)
    cwalker, n_cand = np.zeros((ne, cap), dtype=np.int32), np.zeros(ne, dtype=np.uint32)
    for e in range(ne):
        for i, (kk, t, w) in enumerate(case.held[e]):
            key[e, i], step[e, i], walker[e, i], x[e, i], lnprob[e, i] = kk, t, w, held_row(t, w, nd), -float(t)
        meta[e, 4], meta[e, 5] = len(case.held[e]), 1000 + e            # n_held, n_seen
        for j, (kk, t, w) in enumerate(case.cand[e]):
            ckey[e, j], cstep[e, j], cwalker[e, j] = kk, t, w
        n_cand[e] = len(case.cand[e])
    rows_seen = 3
    rc_ = L.mpr_merge(nw, ne, nd, k, cap, case.n_rows, C.c_int64(case.t0), rows_seen, dp(chain), dp(lnp), up(key), lp(step), ip(walker),
                      dp(x), dp(lnprob), lp(meta), up(ckey), lp(cstep), ip(cwalker), n_cand.ctypes.data_as(C.POINTER(C.c_uint32)))
    assert rc_ == 0, (case.name, rc_)
    for e in range(ne):
        want, thr = rr.merge_launch(case.held[e], case.cand[e], k)
        if not case.cand[e]:
            want, thr = set(case.held[e]), None
        n = len(want)
        assert meta[e, 4] == n and meta[e, 5] == 1000 + e + rows_seen * nw and n_cand[e] == 0, (case.name, e)
        got = sorted(zip(key[e, :n].tolist(), step[e, :n].tolist(), walker[e, :n].tolist()))
        assert got == sorted(want), (case.name, e)
        if thr is None:
            assert meta[e, 3] == 0
        else:
            assert meta[e, 3] == 1 and int(meta[e, 0]) & rc.U64_MAX == thr[0] and tuple(meta[e, 1:3]) == thr[1:], (case.name, e)
        was_held = set(case.held[e])
        for i in range(n):
            t, w = int(step[e, i]), int(walker[e, i])
            if (int(key[e, i]), t, w) in was_held:
                assert same_bytes(x[e, i], held_row(t, w, nd)) and lnprob[e, i] == -float(t), (case.name, e, i)
            else:
                assert same_bytes(x[e, i], chain[t - case.t0, e * nw + w]), (case.name, e, i)
                assert same_bytes(lnprob[e, i], lnp[t - case.t0, e * nw + w]), (case.name, e, i)
        assert np.all(key[e, n:] == 7) and np.all(x[e, n:] == -7.0)


def test_the_probe_refuses_bad_arguments():
    L = probe()
    case = rc.run_cases()[0]
    chain, lnp = rc.run_chain(case)
    out = (np.zeros((2, 1, 6)), np.zeros((2, 1)), np.zeros((2, 1), dtype=np.int64), np.zeros((2, 1), dtype=np.int32),
           np.zeros((2, 1), dtype=np.uint64), np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int64))
    tail = (dp(out[0]), dp(out[1]), lp(out[2]), ip(out[3]), up(out[4]), ip(out[5]), lp(out[6]))
    ch = np.array([4], dtype=np.int32)

    def call(n=4, size=1, discard=0, step0=1, chunks=ch, restart=-1):
        return L.mpr_run_reservoir(dp(chain), dp(lnp), n, 64, 2, 6, size, C.c_uint64(1), C.c_int64(discard), C.c_int64(step0),
                                   len(chunks), ip(chunks), restart, *tail)

    assert call() == 0
    assert call(size=0) == -1 and call(size=L.mpr_max_rows() + 1) == -1 and call(discard=-1) == -1
    assert call(step0=0) == -1 and call(chunks=np.array([3], dtype=np.int32)) == -1 and call(restart=1) == -1
