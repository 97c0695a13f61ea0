"""CPU checks of the weighted band (mp_model_band_weighted): the two inlines of magprop_amd/csrc/mp_band.h compiled for the host
against the restatement (tests/wband_restated.py) bit for bit, the restatement against derived.weighted_quantile and numpy's
method="inverted_cdf", the cases of tests/wband_cases.py, the conversion the library exports and the Python argument checks."""
import ctypes
import subprocess
import warnings

import numpy as np
import pytest

import wband_cases as wc
import wband_restated as wr
from conftest import ROOT
from magprop_amd import _capi, derived, nested

QS = np.array([0.0, 0.025, 0.16, 0.5, 0.84, 0.975, 1.0])


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    """bit for bit, NaN where NaN (whatever its payload)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(_bits(a)[~np.isnan(a)], _bits(b)[~np.isnan(b)])


# ---------------------------------------------------------------- the header's inlines, built with g++
@pytest.fixture(scope="module")
def rule_exe(tmp_path_factory):
    """band_weight_units and band_weight_target built for the host.  stdin: `U n` and n weights as hex bits -> `1 u0 u1 ..` or `0`;
    `T q W` (q as hex bits, W decimal) -> the target."""
    d = tmp_path_factory.mktemp("wband")
    src = d / "wband.cpp"
    src.write_text(r'''
#include <cstdio>
#include <cstring>
#include <vector>
#include "magprop_amd/csrc/mp_band.h"
static double d_of(unsigned long long b) { double v; std::memcpy(&v, &b, 8); return v; }
int main() {
    char kind;
    while (std::scanf(" %c", &kind) == 1) {
        if (kind == 'U') {
            int n;
            if (std::scanf("%d", &n) != 1) return 1;
            std::vector<double> w(n);
            std::vector<uint32_t> u(n);
            for (auto &v : w) { unsigned long long b; if (std::scanf("%llx", &b) != 1) return 1; v = d_of(b); }
            if (!mp::band_weight_units(w.data(), n, u.data())) { std::printf("0\n"); continue; }
            std::printf("1");
            for (auto v : u) std::printf(" %u", (unsigned)v);
            std::printf("\n");
        } else {
            unsigned long long qb, W;
            if (std::scanf("%llx %llu", &qb, &W) != 2) return 1;
            std::printf("%llu\n", (unsigned long long)mp::band_weight_target(d_of(qb), W));
        }
    }
}
''')
    exe = d / "wband"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", ROOT, str(src), "-o", str(exe)], check=True)
    return exe


def _weight_vectors():
    rng = np.random.default_rng(11)
    tiny = 5e-324
    vs = [np.array([1.0]), np.array([3.0, 3.0, 3.0]), np.array([0.0, 2.5, 0.0]), np.array([1.7976931348623157e308, 1.0, 1e300]),
          np.array([tiny, 2 * tiny, 3 * tiny]),                      # wmax denormal itself: ratios 1/3, 2/3, 1
          np.array([tiny, 1.0, 2.0 ** -1022, 2.0 ** -31, 2.0 ** -32, np.nextafter(2.0 ** -31, 0.0), np.nextafter(2.0 ** -31, 1.0)]),
          np.array([1.0, 2.0 ** -1074 * 2.0 ** 1000, 1e-320, 1e308]),  # denormal ratios
          np.array([np.nan, 1.0]), np.array([1.0, -1.0]), np.array([-0.0, 0.0]), np.array([np.inf, 1.0]), np.array([0.0, 0.0, 0.0]),
          np.array([1.0, -np.inf]), np.array([-0.0, 1.0])]
    # ratios on and just below a whole number of units, under several wmax
    for wmax in (1.0, 3.0, 0.1, 1e-300, 7e300):
        k = np.concatenate([[1, 2, 3, (1 << 31) - 1, 1 << 30], rng.integers(1, 1 << 31, 40)]).astype(np.float64)
        on = wmax * (k / 2147483648.0)
        vs.append(np.concatenate([[wmax], on, np.nextafter(on, 0.0), np.nextafter(on, np.inf), [np.nextafter(wmax, 0.0)]]))
    for n in (1, 2, 17, 1000):
        vs.append(np.exp(3.0 * rng.standard_normal(n)))
        vs.append(rng.random(n) * 10.0 ** rng.integers(-300, 300, n))
    return vs


def _targets():
    rng = np.random.default_rng(12)
    out = []
    for W in [1, 2, 3, 1 << 31, (1 << 31) + 1, 3 << 31, (1 << 46) - 1, 1 << 46] + [int(w) for w in rng.integers(1, 1 << 46, 60)]:
        qs = [0.0, 1.0, 0.5, 2.0 ** -1074, 1.0 - 2.0 ** -53, 2.0 ** -46, 0.025, 0.975] + list(rng.random(6))
        for k in rng.integers(1, W + 1, 4):                   # on a whole number of units and next to it
            qk = float(k) / float(W)
            qs += [qk, np.nextafter(qk, 0.0), min(np.nextafter(qk, 1.0), 1.0)]
        out += [(float(q), W) for q in qs]
    return out


def test_header_inlines_equal_the_restatement_bit_for_bit(rule_exe):
    vectors, targets = _weight_vectors(), _targets()
    stdin = "".join(f"U {w.size} " + " ".join(f"{b:x}" for b in _bits(w)) + "\n" for w in vectors)
    stdin += "".join(f"T {_bits([q])[0]:x} {W}\n" for q, W in targets)
    lines = subprocess.run([str(rule_exe)], input=stdin, capture_output=True, text=True, check=True).stdout.split("\n")
    refused = 0
    for w, line in zip(vectors, lines):
        want = wr.weight_units(w)
        got = line.split()
        if want is None:
            assert got == ["0"], w
            refused += 1
            continue
        assert got[0] == "1" and np.array_equal(np.array(got[1:], dtype=np.uint64), want.astype(np.uint64)), w
        assert want.max() == 1 << 31 and np.all(want[w == w.max()] == 1 << 31)      # the heaviest row: exactly 2^31
        assert np.all(want[w < w.max() * 2.0 ** -32] == 0)
    assert refused == 6
    for (q, W), line in zip(targets, lines[len(vectors):]):
        assert int(line) == wr.weight_target(q, W), (q, W)
        assert 1 <= int(line) <= W
    assert len(targets) > 1500


def test_library_conversion_is_the_restatement_and_refuses_bad_weights():
    L = _capi.lib()
    up = ctypes.POINTER(ctypes.c_uint32)
    for w in _weight_vectors():
        want = wr.weight_units(w)
        u = np.full(w.size, 12345, dtype=np.uint32)
        rc = L.mp_band_weight_units(_capi._dptr(np.ascontiguousarray(w)), int(w.size), u.ctypes.data_as(up))
        if want is None:
            assert rc == _capi.MP_EINVAL and "finite" in _capi.last_error(), w
            with pytest.raises(ValueError):
                _capi.band_weight_units(w)
        else:
            assert rc == _capi.MP_OK and np.array_equal(u, want), w
            assert np.array_equal(_capi.band_weight_units(w), want)
    for bad in ([np.nan, 1.0], [1.0, -1.0], [np.inf, 1.0], [0.0, 0.0]):      # NaN, negative, infinite, all zero
        w = np.array(bad)
        u = np.zeros(2, dtype=np.uint32)
        assert L.mp_band_weight_units(_capi._dptr(w), 2, u.ctypes.data_as(up)) == _capi.MP_EINVAL
    w, u = np.ones(4), np.zeros(4, dtype=np.uint32)
    assert L.mp_band_weight_units(None, 4, u.ctypes.data_as(up)) == _capi.MP_EINVAL
    assert L.mp_band_weight_units(_capi._dptr(w), 4, None) == _capi.MP_EINVAL
    assert L.mp_band_weight_units(_capi._dptr(w), 0, u.ctypes.data_as(up)) == _capi.MP_EINVAL


def test_weighted_entry_judges_its_arguments_without_a_handle():
    L = _capi.lib()
    p, q, band = np.zeros((4, 6)), np.array([0.5]), np.empty(10)

    def call(w, h=None, n=4):
        return L.mp_model_band_weighted(h, _capi._dptr(p), n, 6, 0, None if w is None else _capi._dptr(np.asarray(w, dtype=np.float64)),
                                        _capi._dptr(q), 1, 1, _capi._dptr(band), None, None)

    assert call(np.ones(4)) == _capi.MP_EINVAL and "NULL" in _capi.last_error()          # a null handle
    assert call(None) == _capi.MP_EINVAL and "NULL" in _capi.last_error()
    for bad in ([np.nan, 1, 1, 1], [1, -1, 1, 1], [np.inf, 1, 1, 1], [0, 0, 0, 0]):
        assert call(bad) == _capi.MP_EINVAL and "finite" in _capi.last_error(), bad
    assert call(np.ones(4), n=0) == _capi.MP_EINVAL and "MP_BAND_MAX_SAMPLES" in _capi.last_error()
    assert "mp_model_band_weighted" in _capi.EXPORTS and "mp_band_weight_units" in _capi.EXPORTS and _capi.ABI_VERSION == 5


# ---------------------------------------------------------------- the restatement
def test_cases_have_the_properties_their_names_claim():
    names = [c.name for c in wc.CASES]
    for n in wc.SIZES:
        assert f"random-n{n}" in names and f"one-row-n{n}" in names
    for c in wc.CASES:
        assert c.cols.dtype == np.float64 and c.units.dtype == np.uint32 and c.q.dtype == np.float64
        assert c.cols.flags.c_contiguous and 1 <= c.cols.shape[0] <= 5 and c.units.max() <= 1 << 31
        assert np.all((c.q >= 0.0) & (c.q <= 1.0))
        want = wr.weighted_band(c.cols, c.units, c.q)
        assert _same(want, np.stack([wr.weighted_quantile(col, c.units, c.q) for col in c.cols], axis=1)), c.name
        if c.name.startswith("one-row"):
            i = int(np.argmax(c.units))
            assert np.count_nonzero(c.units) == 1 and _same(want, np.broadcast_to(c.cols[:, i], want.shape))
        if c.name.startswith("zero-ends"):
            for g, col in enumerate(c.cols):
                assert c.units[np.argmin(col)] == 0 and c.units[np.argmax(col)] == 0
                assert want[0, g] > col.min() and want[-1, g] < col.max() and c.q[0] == 0.0 and c.q[-1] == 1.0
        if c.name.startswith("nan-heaviest"):
            assert all(np.isnan(col[np.argmax(c.units)]) for col in c.cols) and not np.any(np.isnan(want))
    c = wc.BY_NAME["all-nan-column"]
    want = wr.weighted_band(c.cols, c.units, c.q)
    assert np.all(np.isnan(want[:, 1])) and not np.any(np.isnan(want[:, [0, 2]]))
    c = wc.BY_NAME["used-rows-without-units"]
    want = wr.weighted_band(c.cols, c.units, c.q)
    assert np.any(~np.isnan(c.cols[0])) and np.all(c.units[~np.isnan(c.cols[0])] == 0)
    assert np.all(np.isnan(want[:, 0])) and not np.any(np.isnan(want[:, 1]))
    c = wc.BY_NAME["signed-zeros"]
    want = wr.weighted_band(c.cols, c.units, c.q)
    z = want[np.argsort(c.q), 3]                           # a column of zeros of both signs: -0.0 first, then +0.0
    assert np.all(z == 0.0) and np.signbit(z[0]) and not np.signbit(z[-1]) and np.all(np.diff(np.signbit(z).astype(int)) <= 0)
    c = wc.BY_NAME["infinities"]
    want = wr.weighted_band(c.cols, c.units, c.q)
    assert c.q[0] == 0.0 and c.q[6] == 1.0 and np.all(want[0] == -np.inf) and np.all(want[6] == np.inf)
    for name in ("overflow-n3", "overflow-n300"):
        c = wc.BY_NAME[name]
        assert int(c.units.astype(np.int64).sum()) >= 3 << 31 and np.all(c.units == 1 << 31)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            assert _same(wr.weighted_band(c.cols, c.units, c.q), np.quantile(c.cols, c.q, axis=1, method="inverted_cdf"))
    on, beyond = wc.BY_NAME["boundary-on"], wc.BY_NAME["boundary-beyond"]
    assert wr.weight_target(0.5, int(on.units.astype(np.int64).sum())) == 1 << 32 == int(on.units[[1, 3]].astype(np.int64).sum())
    assert wr.weight_target(0.5, int(beyond.units.astype(np.int64).sum())) == 1 << 32 == int(beyond.units[[1, 3]].astype(np.int64).sum()) + 1
    assert wr.weighted_band(on.cols, on.units, on.q)[0, 0] == 2.0 and wr.weighted_band(beyond.cols, beyond.units, beyond.q)[0, 0] == 3.0
    for byte in range(8):
        c = wc.BY_NAME[f"one-key-byte-{byte}"]
        k = wr.band_key(c.cols[0])
        assert np.unique(k).size == k.size >= 240 and np.all((k ^ k[0]) & ~(np.uint64(255) << np.uint64(8 * byte)) == 0)
    sizes = sorted(c.units.size for c in wc.CASES if c.name.startswith("lds-"))
    assert sizes == [wc.N_LAST_PLAIN, wc.N_LAST_PLAIN + 1, 8188, wc.BAND_MAX_SAMPLES]
    assert wc.LDS_HEADER + 8 * wc.N_LAST_PLAIN == wc.LDS_PLAIN and 8 * 8188 < wc.LDS_PLAIN < wc.LDS_HEADER + 8 * 8188
    hip = open(ROOT + "/magprop_amd/csrc/mp_band.hip").read()
    assert f"kWKeysOffset == {wc.LDS_HEADER}" in hip and "lds > 65536" in hip


def test_restatement_equals_weighted_quantile_on_every_case():
    """derived.weighted_quantile over the rows with units, the units as float weights: integer-valued sums below 2^53 are exact,
    so the two walk the same cumulative sums.  (Values compare as values: derived.weighted_quantile keeps tied -0.0 / +0.0 in the
    order of the rows, the band puts -0.0 first.)"""
    for c in wc.CASES:
        want = wr.weighted_band(c.cols, c.units, c.q)
        for g, col in enumerate(c.cols):
            keep = ~np.isnan(col) & (c.units > 0)
            if not keep.any():
                assert np.all(np.isnan(want[:, g])), c.name
                continue
            ref = derived.weighted_quantile(col[keep], c.q, c.units[keep].astype(np.float64))
            assert np.array_equal(want[:, g], ref), (c.name, g)
            if not np.any(ref == 0.0):
                assert _same(want[:, g], ref), (c.name, g)


def test_equal_weights_are_numpys_inverted_cdf():
    rng = np.random.default_rng(5)
    for n in wc.SIZES:
        for x in (rng.standard_normal(n), rng.integers(-3, 4, n).astype(float) * 0.5 + 0.25, 10.0 ** rng.uniform(-5, 3, n)):
            for units in (np.full(n, 1 << 31, dtype=np.uint32), np.full(n, 12345, dtype=np.uint32), wr.weight_units(np.full(n, 0.3))):
                assert _same(wr.weighted_quantile(x, units, QS), np.quantile(x, QS, method="inverted_cdf")), n


def test_integer_units_agree_with_float_weights_on_seeded_columns():
    """derived.weighted_quantile with the FLOAT weights against the restatement with their units: n = 1 .. 2 000 and five sizes up
    to the cap, log-weights 3 N(0, 1), default_rng(0), seven quantiles each; none left out."""
    rng = np.random.default_rng(0)
    count = 0
    for n in list(range(1, 2001)) + [2048, 4096, 8188, 16383, 16384]:
        x = rng.standard_normal(n)
        w = np.exp(3.0 * rng.standard_normal(n))
        got = wr.weighted_quantile(x, wr.weight_units(w), QS)
        assert np.array_equal(got, derived.weighted_quantile(x, QS, w)), n
        count += QS.size
    assert count == 14035


# ---------------------------------------------------------------- Python argument checks
def test_python_weight_validation():
    assert _capi.band_weights([1, 2, 0], 3).dtype == np.float64
    for w in (np.ones(4), np.ones((3, 1)), 1.0):
        with pytest.raises(ValueError, match="shape"):
            _capi.band_weights(w, 3)
    for w in ([1, np.nan, 1], [1, -1, 1], [1, np.inf, 1], [0, 0, 0]):
        with pytest.raises(ValueError, match="finite"):
            _capi.band_weights(w, 3)
    st = np.array([0, 1, 0, 3], dtype=np.int32)
    assert _capi.kish_n_eff([1.0, 5.0, 1.0, 9.0], st) == 2.0 and _capi.kish_n_eff([3.0, 5.0, 1.0, 9.0], st) == 16.0 / 10.0
    assert _capi.kish_n_eff([0.0, 5.0, 0.0, 9.0], st) == 0.0


def test_nested_sampler_weights_argument_and_exact_selection():
    x = np.array([1.0, 2.0, 3.0])
    s = nested.NestedSampler(x, x, x, nlive=64)
    for bad in ("nope", None, "Exact", 1):
        with pytest.raises(ValueError, match="'resample' or 'exact'"):
            s.get_model_band(weights=bad)
    with pytest.raises(ValueError, match="run_nested first"):
        s.get_model_band(weights="exact")
    g = nested.NestedSampler(nlive=64, target="gaussian", bounds=[(-1.0, 1.0)] * 2)
    with pytest.raises(ValueError, match="gaussian"):
        g.get_model_band(weights="exact")
    # the selection: rows of zero units out, then the heaviest `cap` in the run's order; weight_dropped is what the cap cut
    rng = np.random.default_rng(1)
    samples = rng.standard_normal((50, 6))
    logwt = rng.standard_normal(50)
    logwt[[3, 7]] = -100.0                                   # far below 2^-31 of the heaviest: no unit
    rows, w, dropped = nested.band_exact_selection(samples, logwt)
    keep = np.setdiff1d(np.arange(50), [3, 7])
    wall = np.exp(logwt - logwt.max())
    assert np.array_equal(rows, samples[keep]) and np.array_equal(w, wall[keep]) and w.max() == 1.0 and dropped == 0.0
    assert np.all(wr.weight_units(w) > 0) and np.all(wr.weight_units(wall)[[3, 7]] == 0)
    rows, w, dropped = nested.band_exact_selection(samples, logwt, cap=10)
    order = np.argsort(-wall[keep], kind="stable")
    top, cut = np.sort(keep[order[:10]]), np.sort(keep[order[10:]])
    assert np.array_equal(rows, samples[top]) and np.array_equal(w, wall[top])
    assert dropped == float(np.sum(wall[cut])) / float(np.sum(wall)) and dropped > 1e-3
    rows, w, dropped = nested.band_exact_selection(samples, np.zeros(50))
    assert rows.shape == (50, 6) and dropped == 0.0
    with pytest.raises(ValueError, match="log-weight"):
        nested.band_exact_selection(samples, logwt[:-1])
