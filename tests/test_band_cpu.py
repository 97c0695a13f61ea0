"""CPU checks of the posterior-predictive band (mp_model_band): the quantile rule of magprop_amd/csrc/mp_band.h compiled for
the host against np.nanquantile, the key mapping, the ABI constants and the Python argument checks."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from magprop_amd import _capi, ensemble


@pytest.fixture(scope="module")
def rule_exe(tmp_path_factory):
    """mp_band.h's key mapping, rank rule and lerp, built for the host: reads columns on stdin, writes quantile / key bits."""
    d = tmp_path_factory.mktemp("band")
    src = d / "band.cpp"
    src.write_text(r'''
#include <cstdio>
#include <cstring>
#include <vector>
#include <algorithm>
#include "magprop_amd/csrc/mp_band.h"
static double d_of(unsigned long long b) { double v; std::memcpy(&v, &b, 8); return v; }
static unsigned long long b_of(double v) { unsigned long long b; std::memcpy(&b, &v, 8); return b; }
int main() {
    int n, nq;
    while (std::scanf("%d %d", &n, &nq) == 2) {
        std::vector<double> x(n), q(nq);
        for (auto &v : x) { unsigned long long b; if (std::scanf("%llx", &b) != 1) return 1; v = d_of(b); }
        for (auto &v : q) { unsigned long long b; if (std::scanf("%llx", &b) != 1) return 1; v = d_of(b); }
        std::vector<unsigned long long> k;
        for (double v : x) if (!__builtin_isnan(v)) k.push_back(mp::band_key(v));
        std::sort(k.begin(), k.end());
        for (auto kk : k) std::printf("%llx ", b_of(mp::band_value(kk)));
        std::printf("\n");
        const int m = (int)k.size();
        for (double qq : q) {
            double r = __builtin_nan("");
            if (m) {
                const mp::BandRank rk = mp::band_rank(m, qq);
                r = mp::band_lerp(mp::band_value(k[rk.lo]), mp::band_value(k[rk.hi]), rk.gamma);
            }
            std::printf("%llx ", b_of(r));
        }
        std::printf("\n");
    }
}
''')
    exe = d / "band"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", ROOT, str(src), "-o", str(exe)], check=True)
    return exe


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def _cases(rng):
    cases = []
    for n in list(range(1, 12)) + [17, 64, 100, 255, 256, 257, 1000, 5000] + list(rng.integers(1, 5001, 40)):
        for kind in range(4):
            if kind == 0:
                x = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4)
            elif kind == 1:                                   # ties
                x = rng.integers(-3, 4, n).astype(float) * 0.5
            elif kind == 2:                                   # +-0.0 among other values
                x = rng.choice([0.0, -0.0, 1.5, -2.0, np.inf, -np.inf], n)
            else:                                             # light-curve-like: positive, many decades
                x = 10.0 ** rng.uniform(-5, 3, n)
            frac = rng.choice([0.0, 0.1, 0.5, 0.9, 1.0])
            x[rng.random(n) < frac] = np.nan
            q = np.concatenate([[0.0, 1.0, 0.025, 0.5, 0.975], rng.random(3)])
            cases.append((x, q))
    return cases


def test_rule_is_nanquantile_bit_for_bit(rule_exe):
    rng = np.random.default_rng(7)
    cases = _cases(rng)
    stdin = "".join(f"{x.size} {q.size}\n" + " ".join(f"{b:x}" for b in _bits(x)) + "\n" + " ".join(f"{b:x}" for b in _bits(q)) + "\n"
                    for x, q in cases)
    lines = subprocess.run([str(rule_exe)], input=stdin, capture_output=True, text=True, check=True).stdout.split("\n")
    import warnings
    for c, (x, q) in enumerate(cases):
        keys_sorted = np.array([int(t, 16) for t in lines[2 * c].split()], dtype=np.uint64).view(np.float64)
        got = np.array([int(t, 16) for t in lines[2 * c + 1].split()], dtype=np.uint64).view(np.float64)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            want = np.nanquantile(x, q)
        # key order is value order: the values come back sorted (NaNs dropped), and every value is there
        fin = x[~np.isnan(x)]
        assert keys_sorted.size == fin.size and np.array_equal(keys_sorted, np.sort(fin))
        if fin.size:
            neg0 = np.signbit(keys_sorted) & (keys_sorted == 0)
            # -0.0 sorts below +0.0 (numpy's partition leaves tied zeros in any order)
            assert not np.any(neg0[1:] & ~neg0[:-1] & (keys_sorted[:-1] == 0))
        same_bits = _bits(got) == _bits(want)
        both_nan = np.isnan(got) & np.isnan(want)
        # numpy's partition puts tied +-0.0 in an arbitrary order, so where the quantile is a zero only the value is defined
        zero = (got == 0) & (want == 0)
        assert np.all(same_bits | both_nan | zero), (c, x.size, q, got, want)
    assert len(cases) > 200


def test_key_mapping_preserves_order():
    rng = np.random.default_rng(3)
    # numpy restatement of the header's mapping, checked against the compiled one above through the sorted output; here the
    # property itself on a wide spread of values, signed zeros and infinities
    x = np.concatenate([rng.standard_normal(2000) * 10.0 ** rng.integers(-300, 300, 2000), [0.0, -0.0, np.inf, -np.inf,
                                                                                            5e-324, -5e-324]])
    b = x.view(np.uint64)
    k = np.where(b >> np.uint64(63), ~b, b | np.uint64(1 << 63))
    o_k, o_v = np.argsort(k, kind="stable"), np.argsort(x, kind="stable")
    assert np.array_equal(x[o_k], x[o_v])


def test_header_constants_match_python():
    hdr = open(os.path.join(ROOT, "include", "magprop_amd.h")).read()

    def define(name):
        return int(re.search(r"#define\s+%s\s+([0-9]+)u?\b" % name, hdr).group(1))

    assert define("MP_BAND_MAX_SAMPLES") == _capi.BAND_MAX_SAMPLES == 16384
    assert define("MP_BAND_MAX_Q") == _capi.BAND_MAX_Q == 16
    assert (define("MP_BAND_LTOT"), define("MP_BAND_LPROP"), define("MP_BAND_LDIP")) == \
        (_capi.BAND_LTOT, _capi.BAND_LPROP, _capi.BAND_LDIP) == (1, 2, 4)
    assert "mp_model_band" in _capi.EXPORTS and _capi.ABI_VERSION == 5


def test_null_handle_is_einval():
    L = _capi.lib()
    p = np.zeros((4, 6))
    q = np.array([0.5])
    band = np.empty(10)
    dp = ctypes.POINTER(ctypes.c_double)
    rc = L.mp_model_band(None, p.ctypes.data_as(dp), 4, 6, 0, q.ctypes.data_as(dp), 1, 1, band.ctypes.data_as(dp), None, None)
    assert rc == _capi.MP_EINVAL
    assert "NULL" in _capi.last_error()


def test_python_argument_validation():
    qa, mask, names = _capi.band_args((0.975, 0.025), ("Ldip", "Ltot"))
    assert list(qa) == [0.975, 0.025] and mask == 5 and names == ("Ltot", "Ldip")
    assert _capi.band_args(0.5, "Lprop")[1:] == (2, ("Lprop",))
    for q in ([], np.zeros(17), [np.nan], [-0.1], [1.5], [np.inf]):
        with pytest.raises(ValueError, match=r"q must|quantile"):
            _capi.band_args(q, ("Ltot",))
    for comps in ((), ("L",), ("Ltot", "Ltot")):
        with pytest.raises(ValueError, match="components"):
            _capi.band_args(0.5, comps)
    with pytest.raises(ValueError, match="16384"):
        _capi.band_rows(np.zeros((16385, 6)))
    with pytest.raises(ValueError, match="16384"):
        _capi.band_rows(np.zeros((0, 6)))
    with pytest.raises(ValueError, match="2-D"):
        _capi.band_rows(np.zeros(6))
    assert _capi.band_rows(np.zeros((16384, 6))).shape == (16384, 6)


def test_sampler_row_selection():
    nsteps, nw, ne, nd = 20, 4, 2, 6
    chain = np.arange(nsteps * nw * ne * nd, dtype=float).reshape(nsteps, nw * ne, nd)
    rows = ensemble.band_selection(chain, nw, ne, discard=10, thin=5, ensemble=1)
    want = np.concatenate([chain[s, nw:2 * nw] for s in (10, 15)])
    assert np.array_equal(rows, want)
    assert np.array_equal(ensemble.band_selection(chain, nw, ne), chain[:, :nw].reshape(-1, nd))
    with pytest.raises(ValueError, match="empty"):
        ensemble.band_selection(None, nw, ne)
    with pytest.raises(ValueError, match="empty"):
        ensemble.band_selection(chain[:0], nw, ne)
    with pytest.raises(ValueError, match="leaves no step"):
        ensemble.band_selection(chain, nw, ne, discard=20)
    with pytest.raises(ValueError, match="ensemble"):
        ensemble.band_selection(chain, nw, ne, ensemble=2)
    with pytest.raises(ValueError, match="thin"):
        ensemble.band_selection(chain, nw, ne, thin=0)
    big = np.zeros((4097, 8, nd))
    with pytest.raises(ValueError, match="16384"):
        ensemble.band_selection(big, 4, 2)
    assert ensemble.band_selection(big, 4, 2, thin=2).shape == (2049 * 4, nd)
