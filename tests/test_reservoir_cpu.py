"""The sample reservoir's rule on the CPU (include/magprop_amd.h mp_sampler_set_reservoir): the restatement of the device's way
through a stream (tests/reservoir_restated.py Reservoir) against the definition, a sort of all keys; the merge property; the
uniformity of the held set; the named cases' own claims; the bindings; and the argument checks of magprop_amd.reservoir.merge and
of source="reservoir", which need no device."""
import os
import re

import numpy as np
import pytest

import reservoir_cases as rc
import reservoir_restated as rr
from conftest import ROOT
from magprop_amd import _capi, ensemble, reservoir

SEED = 0xC0FFEE1234


def as_dict(rows, ndim=2):
    """A list of (key, t, w) as get_samples returns a reservoir (x: the step and the walker)."""
    t, w, k = rr.as_arrays(rows)
    x = np.zeros((len(rows), ndim))
    if len(rows):
        x[:, 0], x[:, 1] = t, w
    return {"x": x, "log_prob": -t.astype(float), "step": t, "walker": w, "key": k, "n_seen": 0}


@pytest.mark.parametrize("size", (1, 7, 64, 100))
def test_the_restatement_holds_the_definitions_set_however_the_stream_is_chunked(size):
    nw, ne, n, step0 = 6, 2, 308, 5
    for discard in (0, 3, 150):
        want = [rr.brute(SEED, range(step0 + discard, step0 + n), nw, e, size) for e in range(ne)]
        assert all(len(w) == min(size, (n - discard) * nw) for w in want)
        for chunks in ([n], [1] * n, [7, 300, 1], [0, 200, 0, 108]):
            for cap in (rr.CAND_CAP, 6, 13):       # (a slice of many steps, of one step, of two)
                r = rr.Reservoir(size, SEED, discard, nw, ne, cand_cap=cap).run(chunks, step0)
                for e in range(ne):
                    assert r.result(e) == want[e], (discard, chunks, cap, e)
                    assert r.n_seen[e] == (n - discard) * nw


def test_restart_drops_what_was_held_and_discards_again():
    nw, size, step0 = 6, 20, 9
    r = rr.Reservoir(size, SEED, 2, nw, 1).run([10, 4, 30, 5], step0, restart_before=2)
    assert r.result(0) == rr.brute(SEED, range(step0 + 14 + 2, step0 + 49), nw, 0, size) and r.n_seen[0] == 33 * nw


def test_merging_the_parts_reservoirs_gives_the_whole_streams():
    nw, n, size, step0 = 4, 30, 16, 3
    whole = as_dict(rr.brute(SEED, range(step0, step0 + n), nw, 0, size))
    for cut in range(n + 1):
        a = as_dict(rr.brute(SEED, range(step0, step0 + cut), nw, 0, size))
        b = as_dict(rr.brute(SEED, range(step0 + cut, step0 + n), nw, 0, size))
        a["n_seen"], b["n_seen"] = cut * nw, (n - cut) * nw
        m = reservoir.merge(a, b, size)
        assert m["n_seen"] == n * nw
        for k in ("x", "log_prob", "step", "walker", "key"):
            assert np.array_equal(m[k], whole[k]) and m[k].dtype == whole[k].dtype, (cut, k)
    # two seeds: the least by (key, step, walker) of both, whatever their steps
    a = as_dict(rr.brute(SEED, range(step0, step0 + n), nw, 0, size))
    b = as_dict(rr.brute(SEED + 1, range(step0, step0 + n), nw, 0, size))
    a["n_seen"] = b["n_seen"] = n * nw
    m = reservoir.merge(a, b, size)
    both = sorted(rr.brute(SEED, range(step0, step0 + n), nw, 0, size) + rr.brute(SEED + 1, range(step0, step0 + n), nw, 0, size))[:size]
    assert sorted(zip(m["key"].tolist(), m["step"].tolist(), m["walker"].tolist())) == both and m["n_seen"] == 2 * n * nw


def test_merge_refuses_what_it_cannot_merge():
    rows = rr.brute(SEED, range(1, 11), 4, 0, 8)
    a = dict(as_dict(rows), n_seen=40)
    with pytest.raises(ValueError, match="share a sample"):
        reservoir.merge(a, a, 8)
    with pytest.raises(ValueError, match="cannot be merged to size 16"):
        reservoir.merge(a, dict(as_dict(rr.brute(SEED + 1, range(1, 11), 4, 0, 8)), n_seen=40), 16)
    with pytest.raises(ValueError, match="size must be >= 1"):
        reservoir.merge(a, a, 0)
    with pytest.raises(ValueError, match="different dimensions"):
        reservoir.merge(a, dict(as_dict(rr.brute(SEED + 1, range(1, 11), 4, 0, 8), ndim=3), n_seen=40), 8)


def test_the_products_keys_are_the_restated_keys():
    for seed, e, nw in ((0, 0, 4), (SEED, 3, 20), ((1 << 64) - 1, 1, 65)):
        steps = np.array([0, 1, 77, (1 << 32) - 1, 1 << 32, (1 << 40) + 5])
        got = reservoir.keys(seed, steps[:, None], np.arange(nw)[None, :], e, nw)
        assert got.dtype == np.uint64 and got.shape == (len(steps), nw)
        want = [[rr.key(seed, int(t), e * nw + w) for w in range(nw)] for t in steps]
        assert got.tolist() == want
    assert reservoir.RES_CTR == rr.RES_CTR
    hdr = open(os.path.join(ROOT, "magprop_amd", "csrc", "mp_reservoir.h")).read()
    assert int(re.search(r"kResCtr\s*=\s*(0x[0-9A-Fa-f]+)u", hdr).group(1), 16) == rr.RES_CTR
    assert int(re.search(r"kResCandCap\s*=\s*(\d+)", hdr).group(1)) == rr.CAND_CAP


def test_the_held_set_is_uniform_over_steps_and_walkers():
    """100 steps x 20 walkers, K = 100, seeds 1 .. 200: the held samples' counts pooled in 20 equal step bins and in the 20
    walkers, Pearson's chi^2 against equal expectation with 19 degrees of freedom (conservative: sampling without replacement
    has less variance than the multinomial), below the 1 - 1e-6 quantile."""
    from scipy.stats import chi2
    n, nw, size = 100, 20, 100
    steps, walkers = np.repeat(np.arange(n), nw), np.tile(np.arange(nw), n)
    by_step, by_walker = np.zeros(20), np.zeros(20)
    for seed in range(1, 201):
        k = reservoir.keys(seed, steps, walkers, 0, nw)
        held = np.lexsort((walkers, steps, k))[:size]
        if seed <= 3:
            want = rr.brute(seed, range(n), nw, 0, size)
            assert sorted(zip(steps[held].tolist(), walkers[held].tolist())) == [(t, w) for _, t, w in want]
        by_step += np.bincount(steps[held] // 5, minlength=20)
        by_walker += np.bincount(walkers[held], minlength=20)
    bound = chi2.ppf(1.0 - 1.0e-6, 19)
    for counts in (by_step, by_walker):
        expect = 200 * size / 20
        stat = float(np.sum((counts - expect) ** 2 / expect))
        print("chi2", stat, "bound", bound)
        assert counts.sum() == 200 * size and stat < bound, (stat, bound)


def test_the_named_cases_are_what_their_names_say():
    cases = {c.name: c for c in rc.run_cases()}
    assert len(cases) == len(rc.run_cases())
    for c in cases.values():
        assert all(sum(ch) == rc.n_steps(c) for ch in c.chunks) and c.step0 >= 1
    assert {c.size for c in cases.values()} >= {1, 63, 64, 65, 255, 256, 257}
    assert {c.n_walkers for c in cases.values()} >= {63, 64, 65} and {c.ndim for c in cases.values()} == {6, 9}
    assert {c.n_ensembles for c in cases.values()} == {1, 2, 16}
    c = cases["chunks without a candidate"]
    r = rr.Reservoir(c.size, c.seed, c.discard, c.n_walkers, c.n_ensembles).run(c.chunks[0], c.step0)
    assert sum(1 for counts in r.n_cand if max(counts) == 0) > 200 and sum(1 for counts in r.n_cand if min(counts) == 0 < max(counts)) >= 1
    per = rr.CAND_CAP // 64
    assert cases["a slice at the candidate capacity"].chunks[0] == (per,) and per * 64 == rr.CAND_CAP
    c = cases["one step past the candidate capacity"]
    r = rr.Reservoir(c.size, c.seed, 0, c.n_walkers, 1).run(c.chunks[0], c.step0)
    assert len(r.n_cand) == 2 and r.n_cand[0] == [rr.CAND_CAP]
    for c in rc.merge_cases():
        ne = len(c.held)
        assert len(c.cand) == ne
        for e in range(ne):
            assert len(c.held[e]) <= c.size and len(set((t, w) for _, t, w in c.held[e] + c.cand[e])) == len(c.held[e]) + len(c.cand[e])
            assert all(c.t0 <= t < c.t0 + c.n_rows and 0 <= w < c.n_walkers for _, t, w in c.cand[e])
            assert all(0 <= k <= rc.U64_MAX for k, _, _ in c.held[e] + c.cand[e])
    by = {c.name: c for c in rc.merge_cases()}
    c = by["K=64 ties straddle the cut"]
    _, thr = rr.merge_launch(c.held[0], c.cand[0], c.size)
    tied = [k for k in c.held[0] + c.cand[0] if k[0] == thr[0]]
    assert len(tied) > 100 and any(k > thr for k in tied) and any(k < thr for k in tied)
    c = by["the whole reservoir replaced"]
    assert rr.merge_launch(c.held[0], c.cand[0], c.size)[0] == set(c.cand[0])


def test_bindings_and_header():
    assert "mp_sampler_set_reservoir" in _capi.EXPORTS and "mp_sampler_get_reservoir" in _capi.EXPORTS
    assert _capi.ABI_VERSION == 5
    hdr = open(os.path.join(ROOT, "include", "magprop_amd.h")).read()
    assert int(re.search(r"#define\s+MP_RESERVOIR_MAX_ROWS\s+(\d+)", hdr).group(1)) == _capi.RESERVOIR_MAX_ROWS == 65536
    assert int(re.search(r"#define\s+MP_ABI_VERSION\s+(\d+)", hdr).group(1)) == 5


def test_source_argument_checks_need_no_device():
    rows = np.arange(12.0).reshape(4, 3)
    calls = []

    def get_samples(e):
        calls.append(e)
        return {"x": rows}

    assert np.array_equal(ensemble.reservoir_selection(get_samples, 0, 1, 1, 2), rows) and calls == [1]
    for kw in (dict(discard=1), dict(thin=2)):
        with pytest.raises(ValueError, match="discard and thin must be 0 and 1"):
            ensemble.reservoir_selection(get_samples, ensemble=0, nensembles=1, **kw)
    with pytest.raises(ValueError, match=r"ensemble must be in 0\.\.1"):
        ensemble.reservoir_selection(get_samples, ensemble=2, nensembles=2)
    with pytest.raises(ValueError, match="the reservoir is empty"):
        ensemble.reservoir_selection(lambda e: {"x": np.empty((0, 3))})
    with pytest.raises(ValueError, match="MP_BAND_MAX_SAMPLES"):
        ensemble.reservoir_selection(lambda e: {"x": np.zeros((_capi.BAND_MAX_SAMPLES + 1, 3))})
    # every summary takes source= as its last keyword, "chain" by default
    import inspect
    for name in ("get_model_band", "get_derived", "get_flows", "get_flow_band", "get_pointwise"):
        params = list(inspect.signature(getattr(ensemble.EnsembleSampler, name)).parameters.values())
        assert params[-1].name == "source" and params[-1].default == "chain", name
