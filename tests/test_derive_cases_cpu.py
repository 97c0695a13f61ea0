"""The numpy restatement of mp_model_derived's definition (tests/derive_restated.py) on every case of tests/derive_cases.py,
against an independent definition: plain Python loops in np.longdouble for the energies and the cumulative energy, np.argmax and
first-crossing loops for the rest.

Bounds.  A sum of G - 1 non-negative terms in any order is within (G - 1) eps relative of the exact one, and every term carries
three roundings: energies must agree to 4 G eps relative.  The index-valued columns must agree exactly, except that a crossing
may differ where the long-double cumulative energy at either answer is within 4 G eps E_tot of the threshold; the cases in which
that happens must be among derive_cases.AT_THRESHOLD, at most 2."""
import numpy as np
import pytest

import derive_cases as dc
import derive_restated as dr

EPS = np.finfo(np.float64).eps
LD = np.longdouble


def independent_row(curves, t):
    """(the 16 columns, the long-double cumulative energy after every interval) of one finished row"""
    G = t.size
    out = np.empty(dr.N)
    cum = None
    for col, L in ((dr.E_TOT, curves[0]), (dr.E_PROP, curves[1]), (dr.E_DIP, curves[2])):
        acc, run = LD(0.0), []
        for i in range(G - 1):
            acc += LD(0.5) * (LD(t[i + 1]) - LD(t[i])) * (LD(L[i]) + LD(L[i + 1]))
            run.append(acc)
        out[col] = float(acc)
        if col == dr.E_TOT:
            cum, e_tot = run, acc
    for col, v in ((dr.L_PEAK, curves[0]), (dr.LPROP_PEAK, curves[1]), (dr.OMEGA_MAX, curves[4]), (dr.MDISC_MAX, curves[3])):
        best = 0
        for i in range(1, G):
            if v[i] > v[best]:
                best = i
        assert best == int(np.argmax(v))
        out[col], out[col + 1] = v[best], t[best]
    for col, f in zip((dr.T10, dr.T50, dr.T90), dr.FRACTIONS):
        i = 0
        if e_tot != 0:
            while i < G - 2 and not cum[i] >= LD(f) * e_tot:
                i += 1
        out[col] = t[i + 1]
    out[dr.OMEGA_END], out[dr.MDISC_END] = curves[4][-1], curves[3][-1]
    return out, np.array(cum, dtype=LD)


EXACT = (dr.L_PEAK, dr.T_PEAK, dr.LPROP_PEAK, dr.T_LPROP_PEAK, dr.OMEGA_END, dr.OMEGA_MAX, dr.T_OMEGA_MAX, dr.MDISC_END,
         dr.MDISC_MAX, dr.T_MDISC_MAX)


def check_case(name):
    """Holds the restatement of one case against the independent definition; returns whether a crossing needed the exemption."""
    _, t, curves, status = dc.case(name)
    G = t.size
    got = dr.derive(curves, status, t)
    exempt = False
    for r in range(curves.shape[1]):
        if status[r] != 0:
            assert np.all(np.isnan(got[r])), (name, r)
            continue
        want, cum = independent_row(curves[:, r], t)
        for col in (dr.E_TOT, dr.E_PROP, dr.E_DIP):
            assert abs(got[r, col] - want[col]) <= 4 * G * EPS * abs(want[col]), (name, r, col, got[r, col], want[col])
        for col in EXACT:
            assert got[r, col] == want[col], (name, r, col, got[r, col], want[col])
        for col, f in zip((dr.T10, dr.T50, dr.T90), dr.FRACTIONS):
            if got[r, col] == want[col]:
                continue
            slack = 4 * G * EPS * abs(cum[-1])
            thr = LD(f) * cum[-1]
            for tt in (got[r, col], want[col]):
                i = int(np.nonzero(t == tt)[0][0]) - 1
                near = [j for j in (i - 1, i) if 0 <= j < G - 1]
                assert any(abs(cum[j] - thr) <= slack for j in near), (name, r, col, got[r, col], want[col])
            exempt = True
    return exempt


@pytest.fixture(scope="module")
def exempted():
    return {name for name in dc.names() if check_case(name)}


def test_every_case_against_the_independent_definition(exempted):
    assert exempted <= set(dc.AT_THRESHOLD) and len(dc.AT_THRESHOLD) <= 2, exempted


def test_the_cases_cover_what_they_are_named_for():
    names = dc.names()
    assert len(names) == len(set(names))
    for G in (2, 3, 256, 257, 258, 513, 514, 10001):
        assert dc.case(f"grid_{G}")[1].size == G
    for n in (1, 63, 64, 65, 257):
        assert dc.case(f"rows_{n}")[2].shape[1] == n
    assert sorted(set(dc.case("failed_rows_between")[3].tolist())) == [0, 1, 2, 3]
    assert dr.seg_len(2) == 1 and dr.seg_len(257) == 1 and dr.seg_len(258) == 2 and dr.seg_len(514) == 3 and dr.seg_len(10001) == 40
    # one interval holds all the energy, and it sits where the name says (seg = 4 at G = 1 000)
    for name, i in (("energy_segment_first", 28), ("energy_segment_last", 31), ("energy_row_first", 0), ("energy_row_last", 998)):
        _, t, curves, _ = dc.case(name)
        terms = (0.5 * np.diff(t)) * (curves[0, 0, :-1] + curves[0, 0, 1:])
        assert np.count_nonzero(terms) == 1 and terms[i] > 0 and dr.seg_len(t.size) == 4
        row = dr.derive_row(curves[:, 0], t)
        assert row[dr.T10] == row[dr.T50] == row[dr.T90] == t[i + 1] and row[dr.E_TOT] == terms[i]
    # ties go to the first occurrence; the ends
    _, t, curves, _ = dc.case("peak_plateau")
    assert dr.derive_row(curves[:, 0], t)[dr.T_PEAK] == t[100]
    _, t, curves, _ = dc.case("peak_first")
    assert dr.derive_row(curves[:, 0], t)[dr.T_PEAK] == t[0]
    _, t, curves, _ = dc.case("peak_last")
    assert dr.derive_row(curves[:, 0], t)[dr.T_OMEGA_MAX] == t[-1]
    # E_tot == 0 answers t_1, with +0.0 energies whatever the sign of the zeros
    for name in ("all_zero", "negative_zero"):
        _, t, curves, _ = dc.case(name)
        row = dr.derive_row(curves[:, 0], t)
        assert row[dr.T10] == row[dr.T50] == row[dr.T90] == t[1]
        assert row[dr.E_TOT] == 0.0 and not np.signbit(row[dr.E_TOT])
    assert np.signbit(dr.derive_row(dc.case("negative_zero")[2][:, 0], dc.case("negative_zero")[1])[dr.L_PEAK])
    # the exact threshold: 0.5 * 8 is met at the end of the fourth interval
    _, t, curves, _ = dc.case("exact_threshold")
    row = dr.derive_row(curves[:, 0], t)
    assert row[dr.E_TOT] == 8.0 and row[dr.T50] == t[4]


def test_the_order_is_the_two_level_one():
    """The restatement's energies equal a plain loop in the stated order (segments from 0.0, then totals from 0.0)."""
    for name in ("grid_258", "grid_10001", "tiny_1e-300"):
        _, t, curves, _ = dc.case(name)
        G, seg = t.size, dr.seg_len(t.size)
        L = curves[0, 0]
        total = 0.0
        for k in range(dr.SEGMENTS):
            s = 0.0
            for i in range(k * seg, min((k + 1) * seg, G - 1)):
                s = s + (0.5 * (t[i + 1] - t[i])) * (L[i] + L[i + 1])
            total = total + s
        assert dr.derive_row(curves[:, 0], t)[dr.E_TOT] == total
