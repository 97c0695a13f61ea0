"""CPU side of tests/select_cases.py: every generated case runs through the restatements, has the property its name claims, and
(band) np.nanquantile equals the rule of magprop_amd/csrc/mp_band.h on every generated column: as a Python restatement and as
the host build of the header that tests/test_band_cpu.py compiles.  tests/test_gpu_select.py holds the kernels against the same
cases."""
import subprocess
import warnings

import numpy as np
import pytest

import de_restated as de
import nest_restated as nr
import select_cases as sc
from test_band_cpu import rule_exe  # noqa: F401  (the fixture: mp_band.h built for the host)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits_or_nan(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(_bits(a)[~np.isnan(a)], _bits(b)[~np.isnan(b)])


def nanquantile(cols, q):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return np.nanquantile(cols, q, axis=1).reshape(len(q), len(cols))


# ================================================================ band
def test_case_names_are_unique_and_cover_the_sizes():
    for cases in (sc.BAND_CASES, sc.NEST_CASES, sc.OPT_CASES):
        names = [c.name for c in cases]
        assert len(set(names)) == len(names)
    assert {c.cols.shape[1] for c in sc.BAND_CASES} == set(sc.BAND_NS) | {7}
    assert {c.cols.shape[0] for c in sc.BAND_CASES} >= set(sc.BAND_GRIDS)
    assert {c.q.size for c in sc.BAND_CASES} >= {1, sc.BAND_MAX_Q}
    for c in sc.BAND_CASES:
        assert np.all((c.q >= 0.0) & (c.q <= 1.0))
        if c.cols.shape[1] in sc.BAND_LARGE:
            assert c.cols.shape[0] <= 8 and c.kind in ("distinct", "equal", "two-valued", "low-byte", "digit-levels", "nan", "rounds-up")
    assert max(c.cols.size for c in sc.BAND_CASES) == 8 * sc.BAND_MAX_SAMPLES
    kinds = {c.kind for c in sc.BAND_CASES}
    assert kinds == {"distinct", "equal", "two-valued", "low-byte", "top-byte", "digit-levels", "denormal", "zeros", "inf", "dbl-max",
                     "nan", "integer-h", "rounds-up", "nq"}
    # the sample counts either side of the 64 KiB of dynamic LDS (4 160 bytes of histograms and words, 8 per key)
    assert 4160 + 8 * 7672 <= 65536 < 4160 + 8 * 7673
    assert {c.nlive for c in sc.NEST_CASES} == {16, 17, 64, 1000, 1023, 1024, 1025, 4096}
    assert {c.n_runs for c in sc.NEST_CASES} == {1, 3} and {c.n_pops for c in sc.OPT_CASES} == {1, 3}
    assert {c.popsize for c in sc.OPT_CASES} == {5, 63, 64, 65, 200, 1024}
    for n in (16, 17, 1000, 1023, 1024, 1025, 4096):
        assert {c.nbatch for c in sc.NEST_CASES if c.nlive == n} >= {1, 2, n // 2}
    assert max(c.n_runs * c.nlive for c in sc.NEST_CASES) == sc.NEST_MAX_LIVE


@pytest.mark.parametrize("case", sc.BAND_CASES, ids=lambda c: c.name)
def test_band_case_has_the_property_its_name_claims(case):
    cols, q, n = case.cols, case.q, case.cols.shape[1]
    nn = [col[~np.isnan(col)] for col in cols]
    keys = [sc.band_key(v) for v in nn]
    for v, k in zip(nn, keys):
        assert np.array_equal(_bits(sc.band_value(k)), _bits(v))                  # the key mapping inverts bit for bit
    if case.kind not in ("nan", "nq"):
        assert all(v.size == n for v in nn)
    if case.kind in ("distinct", "integer-h", "rounds-up"):
        assert np.unique(cols[0]).size == n and (n < 2 or (cols[0].min() < 0.0 < cols[0].max()))
    if case.kind == "distinct":
        assert all(np.unique(col).size == n for col in cols)
    elif case.kind == "equal":
        assert all(np.unique(k).size == 1 for k in keys)
    elif case.kind == "two-valued":
        counts = [int(np.sum(col == col.min())) if np.unique(col).size == 2 else (0 if col[0] == 2.5 else n) for col in cols]
        assert all(np.unique(col).size <= 2 for col in cols)
        for qq in ((0.5, 0.975) if n in sc.BAND_LARGE else sc.Q7):
            lo = sc.band_rank(n, qq)[0]
            # the boundary below lo (rank lo holds the upper value), between lo and hi, and above hi (both hold the lower value)
            want = {c for c in (lo, lo + 1, lo + 2) if 0 <= c <= n}
            assert want <= set(counts), (qq, lo, sorted(want - set(counts)))
    elif case.kind == "low-byte":
        for k in keys:
            assert np.unique(k >> np.uint64(8)).size == 1 and (n < 2 or np.unique(k & np.uint64(255)).size > 1 or n < 4)
        assert cols[0][0] > 0.0 > cols[1][0]
    elif case.kind == "top-byte":
        for k in keys:
            assert np.unique(k & np.uint64((1 << 56) - 1)).size <= 2              # (negative values: the low bits flipped)
            assert np.unique(k >> np.uint64(56)).size == min(n, 256)
        assert np.all(np.isfinite(cols))
    elif case.kind == "digit-levels":
        assert len(cols) == 8 and np.all(np.isfinite(cols))
        for level, k in enumerate(keys):
            above = k >> np.uint64(8 * level + 8) if level < 7 else np.zeros(n, dtype=np.uint64)
            assert np.unique(above).size == 1
            assert np.unique((k >> np.uint64(8 * level)) & np.uint64(255)).size == 256
    elif case.kind == "denormal":
        assert np.all((np.abs(cols) < np.finfo(np.float64).tiny) & (cols != 0.0))
        assert all(5e-324 in col and -5e-324 in col for col in cols if n >= 2)
    elif case.kind == "zeros":
        assert np.all(cols[:3] == 0.0) and not np.any(np.signbit(cols[0])) and np.all(np.signbit(cols[1]))
        assert n < 2 or sc.has_both_zeros(cols[2])
    elif case.kind == "inf":
        assert np.all(cols[1] == np.inf) and np.all(cols[2] == -np.inf)
        assert n < 3 or (np.inf in cols[0] and -np.inf in cols[0] and np.any(np.isfinite(cols[0])))
    elif case.kind == "dbl-max":
        big = np.finfo(np.float64).max
        assert np.all(np.abs(cols[0]) == big) and (n < 2 or (big in cols[0] and -big in cols[0]))
    elif case.kind == "nan":
        m = [v.size for v in nn]
        assert set(m) == ({n, n - 1, 1, 0} if n > 1 else {1, 0})
        assert np.any(np.signbit(cols[np.isnan(cols)])) and not np.all(np.signbit(cols[np.isnan(cols)]))
        default = np.uint64(0x7FF8000000000000)
        assert np.any(_bits(cols[np.isnan(cols)]) & ~sc._SIGN != default)
        one = [np.flatnonzero(np.isnan(col))[0] for col, mm in zip(cols, m) if mm == n - 1 and n > 1]
        assert n == 1 or set(one) >= {0, n - 1} | ({63, 64} if n > 65 else set())
    elif case.kind == "integer-h":
        for qq in q:
            h = float(n - 1) * qq
            assert h == np.floor(h)
    elif case.kind == "rounds-up":
        for qq in q:
            h = float(n - 1) * qq
            assert h == np.floor(h) and qq < h / (n - 1)
    elif case.kind == "nq":
        assert q.size in (1, sc.BAND_MAX_Q) and [v.size for v in nn] == [n, 1, n]


def test_integer_and_rounding_quantiles_exist_for_every_small_count():
    for n in (2, 3, 63, 64, 65):
        assert len(sc.integer_h_quantiles(n)) >= (n + 1) // 2
        assert sum(c.q.size for c in sc.BAND_CASES if c.name.startswith(f"band-integer-h-n{n}-")) == len(sc.integer_h_quantiles(n))
    assert [len(sc.rounding_up_quantiles(n)) for n in (7, 63, 255)] == [1, 1, 1] and len(sc.rounding_up_quantiles(7673)) >= 16
    # the largest q below 1 never reaches band_rank's first branch ((m - 1) 2^-53 is at least half an ulp below m - 1): lo = m - 2
    for m in (2, 3, 65, 7673, 16384):
        assert sc.band_rank(m, 1.0 - 2.0 ** -53)[:2] == (m - 2, m - 1) and sc.band_rank(m, 1.0)[:2] == (m - 1, m - 1)
    assert sc.band_rank(16384, 2.0 ** -1074) == (0, 1, 16383 * 2.0 ** -1074)


@pytest.mark.parametrize("case", sc.BAND_CASES, ids=lambda c: c.name)
def test_nanquantile_is_the_header_rule_on_every_generated_column(case):
    """np.nanquantile, the reference of the GPU test, against the restated rule: bit for bit, NaN positions included; on a
    column with both zeros (numpy's partition leaves their order open) by value."""
    want = nanquantile(case.cols, case.q)
    for g, col in enumerate(case.cols):
        rule = sc.band_rule(col, case.q)
        if g in sc.BAND_NOT_NANQUANTILE.get(case.name, ()):
            continue
        if sc.has_both_zeros(col):
            assert np.array_equal(rule, want[:, g], equal_nan=True), (g, rule, want[:, g])
        else:
            assert _same_bits_or_nan(rule, want[:, g]), (g, rule, want[:, g])
    # the all-zero columns: +0.0 stays +0.0; of -0.0 the lerp's own sums make either zero (b - a = +0.0, and then -0.0 + 0.0 =
    # +0.0 but -0.0 - 0.0 = -0.0), in numpy as in the header: compared bit for bit above, as the kernel is with numpy
    if case.kind == "zeros":
        assert not np.any(np.signbit(want[:, 0])) and np.all(want[:, 1] == 0.0) and np.any(np.signbit(want[:, 1]))


def test_restated_rule_is_the_compiled_header_on_every_generated_column(rule_exe):  # noqa: F811
    """The Python restatement of band_key / band_rank / band_lerp against mp_band.h itself, built for the host."""
    items = [(col, c.q) for c in sc.BAND_CASES for col in c.cols]
    stdin = "".join(f"{x.size} {q.size}\n" + " ".join(f"{b:x}" for b in _bits(x)) + "\n" + " ".join(f"{b:x}" for b in _bits(q)) + "\n"
                    for x, q in items)
    lines = subprocess.run([str(rule_exe)], input=stdin, capture_output=True, text=True, check=True).stdout.split("\n")
    for i, (x, q) in enumerate(items):
        sorted_vals = np.array([int(t, 16) for t in lines[2 * i].split()], dtype=np.uint64)
        got = np.array([int(t, 16) for t in lines[2 * i + 1].split()], dtype=np.uint64).view(np.float64)
        assert np.array_equal(sorted_vals, _bits(sc.band_value(np.sort(sc.band_key(x[~np.isnan(x)])))))
        assert _same_bits_or_nan(got, sc.band_rule(x, q)), i
    assert len(items) > 1000


def test_transpose_input_codes_every_index():
    for n, g in sc.TRANSPOSE_SHAPES:
        src = sc.transpose_input(n, g)
        assert src.shape == (n, g) and np.unique(src).size == n * g
    assert {g for _, g in sc.TRANSPOSE_SHAPES} >= set(sc.BAND_GRIDS)


# ================================================================ nested select
def _keys(lnl):
    return np.where(np.isnan(lnl), -np.inf, lnl)


@pytest.mark.parametrize("case", sc.NEST_CASES, ids=lambda c: c.name)
def test_nest_case_runs_through_the_restatement_and_is_what_its_name_claims(case):
    c, exp, before = case, sc.nest_expected(case), sc.nest_outputs(case)
    K, n = c.nbatch, c.nlive
    assert sc.NEST_MIN_LIVE <= n <= sc.NEST_MAX_LIVE and 1 <= K <= n // 2 and 0 <= c.slot < c.chunk
    for r in range(c.n_runs):
        key = _keys(c.lnl[r])
        o = np.lexsort((np.arange(n), key))                    # ascending (lnL, slot), by numpy
        went = not c.stopped[r] and c.mode == 0 and not exp["stopped"][r]
        if went:
            assert np.array_equal(exp["dead_slot"][r], o[:K]) and np.array_equal(exp["surv"][r], np.sort(o[K:]))
            assert exp["lstar"][r] == key[o[K - 1]] and np.array_equal(exp["dead_lnl"][c.slot, r], key[o[:K]])
            assert np.array_equal(exp["dead_n"][c.slot, r], n - np.arange(K))
            assert np.array_equal(exp["dead_pars"][c.slot, r], c.live[r, o[:K]])
            assert exp["nit"][r] == c.nit[r] + 1
            with np.errstate(all="ignore"):                    # the chain, by numpy's own logaddexp
                lnx, lnz = c.lnx[r], c.lnz[r]
                for k in range(K):
                    lnz = np.logaddexp(lnz, key[o[k]] + lnx + np.log(-np.expm1(-1.0 / (n - k))))
                    lnx = lnx - 1.0 / (n - k)
            assert np.isclose(exp["lnx"][r], lnx, rtol=1e-13, atol=0.0)
            assert (exp["lnz"][r] == lnz == -np.inf) if lnz == -np.inf else np.isclose(exp["lnz"][r], lnz, rtol=1e-12, atol=0.0)
            assert not np.isnan(exp["lnz"][r])
            for s in range(c.chunk):                            # the other chunk slots keep their canaries
                if s != c.slot:
                    assert np.all(np.isnan(exp["dead_pars"][s, r])) and np.all(exp["dead_n"][s, r] == sc.ICANARY)
        else:
            for name in ("dead_slot", "surv", "lstar", "dead_lnl", "dead_n", "dead_pars", "lnx", "lnz", "nit"):
                a, b = (exp[name][:, r], before[name][:, r]) if name.startswith("dead_") and name != "dead_slot" else \
                    (exp[name][r], before[name][r])
                assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), name
            assert exp["stopped"][r] in (c.stopped[r], 1)
    kinds = {c.kind} if c.n_runs == 1 or c.kind in ("distinct", "equal") else set()
    key0, o0 = _keys(c.lnl[0]), np.lexsort((np.arange(n), _keys(c.lnl[0])))
    if "distinct" in kinds:
        assert np.unique(key0).size == n and np.all(np.isfinite(key0))
    if "equal" in kinds:
        assert np.unique(key0).size == 1 and np.array_equal(exp["dead_slot"][0], np.arange(K))
    if c.kind == "boundary-tie":
        assert key0[o0[K - 1]] == key0[o0[K]] and np.isfinite(key0[o0[K]])
        tied = np.flatnonzero(key0 == key0[o0[K]])
        dead = set(exp["dead_slot"][0].tolist())
        assert max(t for t in tied if t in dead) < min(t for t in tied if t not in dead)      # the slot decides
    if c.kind.startswith("minf-") or c.kind == "all-minf":
        b = int(np.sum(key0 == -np.inf))
        assert {"minf-below": b == K - 1 >= 1, "minf-equal": b == K, "minf-above": b > K, "all-minf": b == n}[c.kind]
        assert exp["lstar"][0] == (-np.inf if b >= K else key0[o0[K - 1]])
        assert exp["lnz"][0] == -np.inf if b >= K else np.isfinite(exp["lnz"][0])
        assert exp["stopped"][0] == 0
    if c.kind == "nan":
        assert np.sum(np.isnan(c.lnl[0])) == 3 and np.sum(c.lnl[0] == -np.inf) == 2 and K == 4
        assert np.all(exp["dead_lnl"][0, 0] == -np.inf) and exp["lstar"][0] == -np.inf
        assert np.array_equal(exp["dead_slot"][0], np.sort(np.flatnonzero(key0 == -np.inf))[:K])
    if c.kind == "three-runs":
        assert np.any(np.isnan(c.lnl[2])) and np.all(exp["nit"] == c.nit + 1) and np.all(np.isfinite(exp["lnz"][1:]))
    if c.kind == "mid-run":
        assert c.ndim == sc.MAX_NDIM and np.isfinite(c.lnz[0]) and exp["nit"][0] == c.nit[0] + 1
    if c.kind == "stopped-beside":
        assert list(c.stopped) == [0, 1, 0] and list(exp["stopped"]) == [0, 1, 0] and list(exp["nit"] - c.nit) == [1, 0, 1]
    if c.kind == "stop-fires":
        assert list(exp["stopped"]) == [1, 0, 1] and list(exp["nit"] - c.nit) == [0, 1, 0]
    if c.kind == "mode1":
        assert c.mode == 1 and list(exp["stopped"]) == [1, 0, 0] and np.array_equal(exp["nit"], c.nit)
        assert np.all(exp["dead_slot"] == sc.ICANARY) and np.all(exp["surv"] == sc.ICANARY)
    if c.kind == "slot":
        assert c.slot > 0 and c.chunk == 4 and np.all(exp["dead_n"][c.slot] != sc.ICANARY)


def test_restated_select_is_the_step_inside_iteration():
    """nest_restated.select on a tied live set with a NaN, against the order and the chain written out by hand."""
    lnl = np.array([-1.0, -np.inf, -1.0, np.nan, -2.0, -0.5])
    dead, surv, lstar, dead_lnl, dead_n, lnx, lnz = nr.select(lnl, 0.0, -np.inf, 3, 0.01)
    assert (dead, surv, lstar, dead_lnl, dead_n) == ([1, 3, 4], [0, 2, 5], -2.0, [-np.inf, -np.inf, -2.0], [6, 5, 4])
    assert lnx == ((0.0 - 1.0 / 6.0) - 1.0 / 5.0) - 1.0 / 4.0
    assert np.isclose(lnz, -2.0 + (0.0 - 1.0 / 6.0 - 1.0 / 5.0) + np.log(-np.expm1(-0.25)), rtol=1e-15)
    assert nr.select(lnl, -30.0, 40.0, 3, 0.01) is None


# ================================================================ optimizer reduce
@pytest.mark.parametrize("case", sc.OPT_CASES, ids=lambda c: c.name)
def test_opt_case_runs_through_the_restatement_and_is_what_its_name_claims(case):
    c, exp, before = case, sc.opt_expected(case), sc.opt_outputs(case)
    assert sc.OPT_MIN_POP <= c.popsize <= sc.OPT_MAX_POP
    assert not np.array_equal(c.pop_cur, c.pop_next) and not np.any(c.st_cur == c.st_next) and not np.any(c.lnp_cur == c.lnp_next)
    for p in range(c.n_pops):
        lnp = c.lnp_next[p]
        fresh = not c.converged[p]
        for name in ("pop_next", "lnp_next", "st_next"):
            assert np.array_equal(exp[name][p], before[name][p])
        if not fresh:
            for name in before:
                assert np.array_equal(exp[name][p], before[name][p]), name
            continue
        assert exp["best"][p] == int(np.argmax(lnp))            # numpy's argmax: the first of the largest
        assert exp["nfev"][p] == c.nfev[p] + c.popsize and exp["nit"][p] == c.nit[p] + c.trial
        e = -lnp
        with np.errstate(all="ignore"):
            conv = bool(c.trial and np.all(np.isfinite(lnp)) and np.std(e) <= c.atol + c.tol * abs(np.mean(e)))
        assert exp["converged"][p] == int(conv)
        src = "pop_next" if conv else "pop_cur"
        assert np.array_equal(exp["pop_cur"][p], before[src][p])
        assert np.array_equal(exp["lnp_cur"][p], before["lnp_next" if conv else "lnp_cur"][p])
        assert np.array_equal(exp["st_cur"][p], before["st_next" if conv else "st_cur"][p])
    kinds = {"three-pops": ["tight", "equal", "best-tie"], "three-pops-gen0": ["tight", "best-tie", "equal"], "atol": ["tight"],
             "all-converged": ["tight", "distinct", "best-tie"], "equal-gen0": ["equal"]}.get(c.kind, [c.kind])
    for p, kind in enumerate(kinds):
        lnp, conv, best = c.lnp_next[p], exp["converged"][p], exp["best"][p]
        if c.converged[p]:
            assert conv == 1 and best == sc.ICANARY
            continue
        if kind == "distinct":
            assert np.unique(lnp).size == c.popsize and not conv
        elif kind == "best-tie":
            assert sorted(set(np.flatnonzero(lnp == lnp.max()))) == sorted({2, c.popsize // 2, c.popsize - 1}) and best == 2
            assert not conv
        elif kind == "tight":
            assert np.unique(lnp).size > 1 and conv == c.trial
        elif kind == "tight-minf":
            assert np.sum(lnp == -np.inf) == 1 and not conv
            assert de.reduce(np.where(np.isinf(lnp), -12.5, lnp), c.tol, c.atol)[1]          # tight but for that member
        elif kind == "equal":
            assert np.unique(lnp).size == 1 and best == 0 and conv == c.trial
    if c.kind == "three-pops":
        assert list(c.converged) == [0, 1, 0] and list(exp["converged"]) == [1, 1, 0]
    if c.kind == "atol":
        assert c.tol == 0.0 and exp["converged"][0] == 1
