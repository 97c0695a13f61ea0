"""The definition of the simulated light curves (tests/simulate_restated.py, the header's mp_simulate in numpy) on the crafted
cases of tests/simulate_cases.py, without a GPU: its model value against exact rational interpolation, its knots, and its noise
stream against the chunking.

Bound of the model value.  Off a knot mod = fl(fl(fl(fl(Lb - La) * idt) * dx) + La) with idt = fl(1 / fl(t1 - t0)) and dx =
fl(x - t0): seven roundings, each of relative size u = 2^-53 at most, six of them in the rise r = (Lb - La) (x - t0) / (t1 - t0)
and one in the final sum.  To first order |mod - exact| <= 6 u |r| + u |mod| <= 7 u max(|La|, |Lb|) for curve values of one sign
(|r| <= |Lb - La| <= max, |mod| <= max), and u |v| < ulp(v): the test asks for 8 ulp(max(|La|, |Lb|)), which leaves the second-order
terms a whole ulp.  The bound is about normal numbers: cells whose max(|La|, |Lb|) is below 1e-290 (the subnormal case) are
left to the knot and chunking tests."""
from fractions import Fraction

import numpy as np
import pytest

import simulate_cases as sc
import simulate_restated as sr

ULPS = 8


def _rows(case):
    """(row index, x[n_obs]) of every row with a usable curve"""
    x = case["x"]
    for s in range(case["ltot"].shape[0]):
        if case["status"][s] == sr.STATUS_OK:
            yield s, (x if x.ndim == 1 else x[s])


@pytest.mark.parametrize("name", list(sc.CASES))
def test_model_value_against_exact_interpolation(name):
    case = sc.CASES[name]
    t = case["t"]
    checked = 0
    for s, x in _rows(case):
        L = case["ltot"][s]
        g, dx, idt = sr.bracket(t, x)
        mod = sr.model_value(L, g.astype(np.int64), dx, idt)
        for j in range(x.size):
            a = min(int(g[j]), t.size - 2)
            La, Lb = L[a], L[a + 1]
            top = max(abs(La), abs(Lb))
            if top < 1.0e-290:
                continue
            exact = Fraction(La) + (Fraction(Lb) - Fraction(La)) * (Fraction(x[j]) - Fraction(t[a])) / (Fraction(t[a + 1]) - Fraction(t[a]))
            err = abs(Fraction(float(mod[j])) - exact)
            assert err <= ULPS * Fraction(float(np.spacing(top))), (name, s, j, float(err / Fraction(float(np.spacing(top)))))
            checked += 1
    assert checked or name == "subnormal_error"


@pytest.mark.parametrize("name", list(sc.CASES))
def test_knots_are_exact(name):
    """a time that IS a grid point reads its curve value and nothing else: the last point included, and with a NaN or infinite
    neighbour"""
    case = sc.CASES[name]
    t = case["t"]
    for s, x in _rows(case):
        L = case["ltot"][s]
        g, dx, idt = sr.bracket(t, x)
        mod = sr.model_value(L, g.astype(np.int64), dx, idt)
        on = np.isin(x, t)
        assert np.array_equal(dx == 0.0, on)
        assert np.array_equal(t[g[on]], x[on])
        assert np.array_equal(mod[on].view(np.uint64), L[g[on]].view(np.uint64))
    # every knot of a curve whose other values are poison
    L = np.full(t.size, np.nan)
    for k in (0, 17, t.size - 1):
        L[:] = np.nan
        L[k] = 3.25
        g, dx, idt = sr.bracket(t, t[k:k + 1])
        assert g[0] == k and sr.model_value(L, g.astype(np.int64), dx, idt)[0] == 3.25


def test_the_bracket_is_the_largest_knot_at_or_below():
    t = sc.CASES["every_knot"]["t"]
    x = np.concatenate([t, np.nextafter(t[:-1], np.inf), np.nextafter(t[1:], -np.inf), [1.5, 999.0]])
    g, dx, idt = sr.bracket(t, x)
    for j in range(x.size):
        assert t[g[j]] <= x[j] and (g[j] == t.size - 1 or x[j] < t[g[j] + 1])
        if g[j] < t.size - 1:
            assert dx[j] == x[j] - t[g[j]] and idt[j] == 1.0 / (t[g[j] + 1] - t[g[j]])
    for bad in (t[0] - 1.0e-9, t[-1] + 1.0e-6, np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError):
            sr.bracket(t, np.array([1.5, bad]))


def _same(a, b):
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


@pytest.mark.parametrize("name", list(sc.CASES))
def test_nothing_depends_on_the_chunking(name):
    """the whole call at once, row by row, and in chunks of 7 and 64 rows: the same bits, the noise included"""
    case = sc.CASES[name]
    args = (case["t"], case["ltot"], case["status"], case["x"], case["yerr"], case["frac_err"], case["seed"])
    whole = sr.simulate(*args)
    for chunk in (1, 7, 64):
        part = sr.simulate(*args, chunk=chunk)
        for k in ("y", "yerr", "model", "z"):
            assert _same(whole[k], part[k]), (name, chunk, k)
        assert np.array_equal(whole["status"], part["status"])


def test_noise_stream():
    """the normal of a cell is a function of seed, row index and observation: odd counts leave a pair's second normal unused,
    rows and seeds differ, and the pair is one Box-Muller step"""
    z257, z256 = sr.normals(11, 5, 257), sr.normals(11, 5, 256)
    assert np.array_equal(z257[:256], z256) and np.array_equal(sr.normals(11, 5, 1), z257[:1])
    assert not np.any(np.isin(sr.normals(11, 6, 257), z257)) and not np.any(np.isin(sr.normals(12, 5, 257), z257))
    assert np.array_equal(sr.normals(11 + (1 << 32), 5, 4) == z257[:4], np.zeros(4, dtype=bool))   # the high word of the seed is keyed
    z = np.concatenate([sr.normals(3, i, 64) for i in range(400)])
    assert abs(z.mean()) < 5.0 / np.sqrt(z.size) and abs(z.var() - 1.0) < 5.0 * np.sqrt(2.0 / z.size)


def test_zero_error_and_failed_rows():
    c = sc.CASES["curve_value_zero"]
    out = sr.simulate(c["t"], c["ltot"], c["status"], c["x"], None, c["frac_err"], c["seed"])
    assert list(out["status"]) == [0, sr.STATUS_ZEROERR, 0]
    assert np.all(np.isnan(out["y"][1])) and np.all(np.isnan(out["model"][1])) and np.all(np.isfinite(out["y"][[0, 2]]))
    kernel = sr.cells(c["ltot"], c["status"], *sr.bracket(c["t"], c["x"]), None, c["frac_err"], c["seed"], 0)
    assert list(kernel["zero"]) == [0, 1, 0] and kernel["model"][1, 0] == 0.0 and kernel["y"][1, 0] == 0.0   # what the kernel itself writes
    c = sc.CASES["subnormal_error"]
    assert list(sr.simulate(c["t"], c["ltot"], c["status"], c["x"], None, c["frac_err"], c["seed"])["status"]) == [sr.STATUS_ZEROERR]
    c = sc.CASES["failed_row"]
    out = sr.simulate(c["t"], c["ltot"], c["status"], c["x"], None, c["frac_err"], c["seed"])
    assert list(out["status"]) == [0, 0, 1, 0]
    for k in ("y", "yerr", "model", "z"):
        assert np.all(np.isnan(out[k][2])) and np.all(np.isfinite(out[k][[0, 1, 3]]))


def test_given_errors_are_used_as_they_are():
    c = sc.CASES["given_errors_per_row"]
    out = sr.simulate(c["t"], c["ltot"], c["status"], c["x"], c["yerr"], c["frac_err"], c["seed"])
    assert np.array_equal(out["yerr"], c["yerr"])
    assert np.array_equal(out["y"], out["model"] + c["yerr"] * out["z"])


def test_the_header_states_the_constants():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "magprop_amd.h")).read()
    assert int(re.search(r"#define MP_SIM_MAX_ROWS\s+(\d+)", text).group(1)) == sr.MAX_ROWS
    assert int(re.search(r"#define MP_SIM_MAX_CELLS\s+(\d+)", text).group(1)) == sr.MAX_CELLS
    assert int(re.search(r"#define MP_STATUS_ZEROERR\s+(\d+)", text).group(1)) == sr.STATUS_ZEROERR
    assert "0x%08X" % sr.CTR in text
    from magprop_amd import _capi
    assert (_capi.SIM_MAX_ROWS, _capi.SIM_MAX_CELLS, _capi.STATUS_ZEROERR) == (sr.MAX_ROWS, sr.MAX_CELLS, sr.STATUS_ZEROERR)
    assert "mp_simulate" in _capi.SIGNATURES
