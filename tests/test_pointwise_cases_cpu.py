"""CPU checks of the pointwise-score kernels' restatement (tests/pointwise_restated.py) on the named cases of
tests/pointwise_cases.py, against a long-double definition that prescribes no order, and of the tail-length rule of
magprop_amd/csrc/mp_pointwise.h compiled for the host.

Bounds (eps = 2^-52, K = ceil(n / 256) cells per thread, D = K + 6 + 3 the depth of a sum: a thread's K additions, six butterfly
levels, three additions over the wavefronts):
  * counts, extrema, the cut, the tail and the M halves of the log-sum-exp pairs involve no rounding: equal.
  * a sum of terms x_i carries at most D roundings on any path from a term to the total: |error| <= 1.01 D eps sum |x_i|; a
    mean adds the division's eps / 2.
  * the variance's deviations are taken from the ROUNDED mean: with delta the error of that mean, a squared deviation is off by
    at most 2 |d| delta + delta^2 + 2 eps d^2, and the sum adds its D eps sum d^2.
  * a log-sum-exp pair: as tests/test_gpu_math.py lse_bound derives for wave_lse with K folds and six merges, here with K
    folds, six butterfly merges and three merges over the wavefronts.  Every fold or merge scales S by an exp (1 ulp = eps),
    multiplies (eps / 2) and adds (eps / 2), 2 eps, budgeted as 3 eps with the second-order terms: (K + 9) 3 eps on log S.
    The rounded exponent v - m of a term is off by eps |v - m| / 2, which moves its exp by (d e^-d) eps / 2 <= eps / (2 e)
    relative to the largest term, and the long-double log of S rounds: 0.5 eps (1 + log n) covers both for up to n terms.
    The expectation itself is a long double: 2^-63 |want|."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import pointwise_cases as pc
import pointwise_restated as pr

EPS = 2.0 ** -52
L = np.longdouble


def depth(n):
    return (n + pr.THREADS - 1) // pr.THREADS + 6 + 3


def lse_bound(n, want):
    K = (n + pr.THREADS - 1) // pr.THREADS
    return (K + 9) * 3.0 * EPS + 0.5 * EPS * (1.0 + np.log(max(n, 2))) + 2.0 ** -63 * abs(want)


def lse_error(m, s, want):
    """|m + log s - want| in long double; (-inf, 0) and an infinite want are matched exactly (error 0 or inf)"""
    if want == -np.inf:
        return 0.0 if (m == -np.inf and s == 0.0) else np.inf
    if not np.isfinite(want):
        return 0.0 if (np.isnan(want) or m == want) else np.inf
    return float(abs(L(m) + np.log(L(s)) - want))


def same(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a) & ~np.isnan(a), np.signbit(b) & ~np.isnan(b))


def test_case_list_covers_the_sizes():
    names = pc.names()
    assert len(names) == len(set(names)) >= 25
    seen_n, seen_o = set(), set()
    for name in names:
        c, z = pc.case(name)
        assert c.ltot.shape == (c.status.size, pc.GRID) and z.shape == (c.g.size, c.status.size)
        assert np.all((c.g >= 0) & (c.g <= pc.GRID - 2)) and np.all(np.diff(c.t[c.g] + c.dx) >= 0)
        assert sum(cnt for _, cnt in c.chunks) == c.status.size
        assert np.all(np.isfinite(c.ltot[c.status == 0])) and np.all(np.isnan(c.ltot[c.status != 0]))
        assert np.all(np.isnan(z[:, c.status != 0])) and not np.any(np.isnan(z[:, c.status == 0]))
        seen_n.add(c.status.size)
        seen_o.add(c.g.size)
    assert set(pc.SAMPLES) <= seen_n and set(pc.N_OBS) <= seen_o
    c, _ = pc.case("s1000_o63")
    # observations on knots, between knots, in the first and in the last interval, on the first and the last grid point
    assert np.any(c.dx == 0.0) and np.any(c.dx > 0.0) and np.any(c.g == 0) and np.any(c.g == pc.GRID - 2)
    assert np.any((c.g == pc.GRID - 2) & (c.t[c.g] + c.dx == c.t[-1])) and np.any((c.g == 0) & (c.dx == 0.0))


def test_planted_cells_are_what_they_claim():
    c, z = pc.case("planted_226")
    with np.errstate(over="ignore"):
        r = 0.5 * z * z
    obs, tail = pr.pointwise(z)
    T = pr.tail_len(226)
    assert T == 47
    assert np.all(z[0] == z[0, 0]) and obs[0, pr.NONTAIL_COUNT] == 226 and np.all(tail[0, :T] == r[0, 0])   # nothing above the cut
    assert 0 < 226 - obs[1, pr.NONTAIL_COUNT] < T - 1 and np.sum(r[1] == obs[1, pr.CUT]) > 1              # ties straddle the cut
    assert np.sum(z[2] == 0.0) >= 30 and obs[2, pr.R_MIN] == 0.0
    assert np.sum(np.isinf(r[3])) == 2 and np.isfinite(r[3, 225]) and r[3, 225] > 1e307
    assert obs[3, pr.R_MAX] == np.inf and np.isnan(obs[3, pr.LL_VAR]) and obs[3, pr.LPPD_S] > 0 and np.isfinite(obs[3, pr.CUT])
    assert np.all(tail[3, T - 2:T] == np.inf)
    assert z[4, 77] == -c.ltot[77, c.g[4]] == 40.0 and tail[4, T - 1] == 800.0
    assert obs[5, pr.LPPD_M] == -0.5e-6 and 1.0 < obs[5, pr.LPPD_S] < 1.0 + 1e-6                         # one dominant likelihood: the others are e^-25 and less
    assert obs[7, pr.CUT] == 0.125 and obs[7, pr.NONTAIL_COUNT] == 180                                    # T = 47 > the 46 cells of the upper level
    c, z = pc.case("all_failed")
    obs, tail = pr.pointwise(z)
    assert np.all(obs[:, pr.N_USED] == 0) and np.all(obs[:, pr.NONTAIL_COUNT] == 0) and np.all(np.isnan(tail))
    assert np.all(obs[:, pr.LPPD_M] == -np.inf) and np.all(obs[:, pr.LPPD_S] == 0) and np.all(np.isnan(obs[:, [pr.Z_MEAN, pr.CUT, pr.R_MIN]]))
    c, z = pc.case("failed_leave_one")
    obs, tail = pr.pointwise(z)
    assert np.all(obs[:, pr.N_USED] == 1) and np.all(np.isnan(obs[:, pr.LL_VAR])) and np.all(obs[:, pr.NONTAIL_COUNT] == 1)
    assert same(tail[:, 0], 0.5 * z[:, 64] ** 2) and np.all(np.isnan(tail[:, 1:]))


@pytest.mark.parametrize("name", pc.names())
def test_restatement_against_the_long_double_definition(name):
    c, z = pc.case(name)
    n = z.shape[1]
    obs, tail = pr.pointwise(z)
    d = pr.definition(z)
    assert tail.shape == (z.shape[0], pr.tail_len(n))
    worst = 0.0
    for j in range(z.shape[0]):
        col = z[j][~np.isnan(z[j])]
        with np.errstate(over="ignore"):
            r = 0.5 * col * col
        m = col.size
        # the tail and the cut against a plain sort, the tail length against the real-valued rule
        T = int(np.ceil(min(L(m) / 5, 3 * np.sqrt(L(m))))) + 1 if m else 0
        want_tail = np.sort(r)[::-1][:T][::-1]
        assert same(tail[j, :want_tail.size], want_tail) and np.all(np.isnan(tail[j, want_tail.size:])), (name, j)
        assert same(obs[j, pr.CUT], want_tail[0] if m else np.nan), (name, j)
        assert obs[j, pr.N_USED] == m == d["n"][j] and obs[j, pr.NONTAIL_COUNT] == d["nontail_count"][j] == np.sum(r <= obs[j, pr.CUT])
        assert m - obs[j, pr.NONTAIL_COUNT] <= max(T - 1, 0)
        for col_id, key in ((pr.R_MIN, "r_min"), (pr.R_MAX, "r_max")):
            assert same(obs[j, col_id], np.float64(d[key][j])), (name, j, key)
        assert same(obs[j, pr.LPPD_M], -np.min(r) if m else -np.inf)
        nt = r[r <= obs[j, pr.CUT]]
        assert same(obs[j, pr.NONTAIL_M], np.max(nt) if nt.size else -np.inf)
        # sums
        D = depth(n)
        for col_id, key, terms in ((pr.Z_MEAN, "z_mean", col), (pr.R_MEAN, "r_mean", r)):
            want = d[key][j]
            if not np.isfinite(want):
                assert same(obs[j, col_id], np.float64(want)), (name, j, key)
                continue
            lim = (1.01 * D * EPS * float(np.sum(np.abs(terms.astype(L)))) / m + EPS * abs(float(want))) if m else 0.0
            assert abs(L(obs[j, col_id]) - want) <= lim, (name, j, key, float(abs(L(obs[j, col_id]) - want)), lim)
        want = d["ll_var"][j]
        if not np.isfinite(want):
            assert np.isnan(obs[j, pr.LL_VAR]) == bool(np.isnan(want)), (name, j)
        else:
            dev = np.abs(-r.astype(L) + d["r_mean"][j])
            delta = abs(L(obs[j, pr.R_MEAN]) - d["r_mean"][j])
            lim = (float(np.sum(2 * dev * delta + delta * delta + 2 * EPS * dev * dev)) + 1.01 * D * EPS * float(np.sum(dev * dev))) / (m - 1) \
                + EPS * float(want)
            assert abs(L(obs[j, pr.LL_VAR]) - want) <= lim, (name, j, float(abs(L(obs[j, pr.LL_VAR]) - want)), lim)
        # log-sum-exp pairs
        for mcol, scol, key in ((pr.LPPD_M, pr.LPPD_S, "lppd"), (pr.NONTAIL_M, pr.NONTAIL_S, "nontail")):
            want = d[key][j]
            err = lse_error(obs[j, mcol], obs[j, scol], want)
            lim = lse_bound(n, float(want)) if np.isfinite(want) else 0.0
            assert err <= lim, (name, j, key, err, lim)
            if lim:
                worst = max(worst, err / lim)
    print(f"{name}: restated log-sum-exp worst/bound {worst:.3f}")


@pytest.fixture(scope="module")
def tail_exe(tmp_path_factory):
    """pointwise_tail_len of mp_pointwise.h built for the host: reads n on stdin, writes T(n)"""
    d = tmp_path_factory.mktemp("pointwise")
    src = d / "tail.cpp"
    src.write_text(r'''
#include <cstdio>
#include "magprop_amd/csrc/mp_pointwise.h"
int main() {
    long long n;
    while (std::scanf("%lld", &n) == 1) std::printf("%d\n", mp::pointwise_tail_len((int64_t)n));
    std::printf("%d %d %d\n", mp::kPointwiseMaxTail, mp::kPointwiseSortCap, mp::kPointwiseThreads);
}
''')
    exe = d / "tail"
    subprocess.run(["g++", "-std=c++17", "-O2", "-I", ROOT, str(src), "-o", str(exe)], check=True)
    return exe


def test_tail_length_rule_of_the_header(tail_exe):
    ns = set(range(-2, 5001))
    for k in range(1, 513):                                    # around every square up to 262 144 (where 9 n is a square too)
        ns.update((k * k - 1, k * k, k * k + 1))
    for m in range(1, 1537):                                   # and around every n at which m * m crosses 9 n
        ns.update((m * m // 9 - 1, m * m // 9, m * m // 9 + 1))
    ns.update((262143, 262144))
    ns = sorted(n for n in ns if n <= pr.MAX_SAMPLES)
    out = subprocess.run([str(tail_exe)], input="\n".join(str(n) for n in ns) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    got = [int(v) for v in out[:len(ns)]]
    assert [int(v) for v in out[len(ns)].split()] == [pr.MAX_TAIL, 2048, pr.THREADS]
    from magprop_amd import pointwise
    for n, T in zip(ns, got):
        assert T == pr.tail_len(n) == pointwise.tail_len(n), n
        if n >= 1:
            real = int(np.ceil(min(L(n) / 5, 3 * np.sqrt(L(n))))) + 1
            assert T == real, (n, T, real)
        else:
            assert T == 0
    assert got[-1] == pr.MAX_TAIL == max(got) and all(a <= b for a, b in zip(got, got[1:]))   # non-decreasing: T(n) bounds every column's
    assert pr.tail_len(1) == 2 and pr.tail_len(2) == 2 and pr.tail_len(5) == 2 and pr.tail_len(6) == 3 and pr.tail_len(225) == 46
