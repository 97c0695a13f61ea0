"""CPU checks of the importance-reweighting kernels' restatement (tests/reweight_restated.py) on the named cases of
tests/reweight_cases.py, against the definition in long double, which prescribes no order (reweight_restated.definition_rows:
mod and res are the float64 restatement's, their roundings being part of the definition).

Allowance of a row sum: per term 32 x 2^-53 (|w t_k| + |t_0| + 1) -- a term is at most 16 rounded operations on numbers no
larger than that, and log(var) inherits an absolute error of up to 2 x 2^-53 from the three roundings of var -- plus (ceil(n_obs
/ 64) + 6) 2^-53 sum |d| for the sum, whose depth is a lane's additions and the butterfly's six.  The exact properties are held
exactly: the identity alternative gives +0.0, a leave-one-out mask -t_0 of the observation left out."""
import numpy as np
import pytest
from scipy.special import logsumexp

import pointwise_restated as pr
import reweight_cases as rc
import reweight_restated as rr
from test_pointwise_cases_cpu import same


def _lw(c, libm=rr.NUMPY):
    return rr.rows(c.ltot, c.status, c.g, c.dx, c.idt, c.y, c.yerr, c.kind, c.alt, c.obs_w, libm)


def test_case_list_covers_the_sizes():
    cases = [rc.row_case(name) for name in rc.row_names()]
    assert {c.g.size for c in cases} >= set(rc.N_OBS) and {c.status.size for c in cases} >= set(rc.ROWS)
    assert {c.kind.size for c in cases} >= set(rc.N_ALT) and max(rc.N_ALT) == rr.MAX_ALT
    assert any(c.obs_w is not None and np.any(c.obs_w == 0.0) for c in cases)
    assert any(c.obs_w is not None and np.any((c.obs_w % 1.0) != 0.0) for c in cases)
    k = rc.row_case("knots")
    assert np.any(k.dx == 0.0) and 0 in k.g and k.t.size - 2 in k.g and np.any((k.dx > 0.0) & (k.g == 0))
    assert np.any(rc.row_case("failed_rows").status != 0) and np.all(np.isnan(rc.row_case("failed_rows").ltot[0]))
    assert set(rc.row_case("nu_extremes").alt[:, 2]) == {0.5, 1.0e12}
    u = rc.row_case("underflow")
    assert np.any(u.yerr * u.yerr == 0.0) and np.any((u.yerr * u.yerr > 0.0) & (u.yerr * u.yerr < 2.3e-308))
    for n in rc.COLUMN_N:
        lw = rc.column_case(n)
        assert lw.shape == (8, n) and np.all(np.isnan(lw[6])) and np.sum(~np.isnan(lw[7])) == 1 and np.any(lw[4] == -np.inf)
    assert pr.tail_len(224) == 46 and pr.tail_len(225) == 46 and pr.tail_len(226) == 47     # (n / 5 and 3 sqrt(n) cross at 225)


@pytest.mark.parametrize("name", rc.row_names())
def test_rows_against_the_definition(name):
    c = rc.row_case(name)
    lw = _lw(c)
    ok = c.status == 0
    assert lw.shape == (c.kind.size, c.status.size) and np.all(np.isnan(lw[:, ~ok]))
    # the identity alternative (the first of every generated table) without weights: exactly +0.0
    if c.obs_w is None and tuple(c.alt[0]) == (1.0, 0.0, 0.0) and c.kind[0] == rr.GAUSS and c.definition:
        assert same(lw[0, ok], np.zeros(int(ok.sum()))), lw[0]
    if not c.definition:
        return
    mod, res = rr.model(c.ltot[ok], c.g, c.dx, c.idt, c.y)
    want, allow = rr.definition_rows(mod, res, c.yerr, c.kind, c.alt, c.obs_w)
    err = np.abs(lw[:, ok].astype(np.longdouble) - want)
    assert np.all(err <= allow), (name, float(np.max(err / allow)))
    print(f"{name}: worst error / allowance {float(np.max(err / allow)):.3f}")


def test_leave_one_out_is_minus_the_base_term():
    c = rc.row_case("leave_one_out")
    gauss1 = c._replace(kind=np.zeros_like(c.kind), alt=np.tile([1.0, 0.0, 0.0], (c.kind.size, 1)))
    lw = _lw(gauss1)
    mod, res = rr.model(c.ltot, c.g, c.dx, c.idt, c.y)
    t0 = rr.base_term(mod, res, c.yerr)
    for k in range(c.kind.size):
        assert same(lw[k], -t0[:, k % c.g.size]), k


def test_student_t_of_large_nu_is_the_gaussian():
    """nu = 1e12: the sum stays within the allowance of the Gaussian alternative's, once the difference the two laws have on
    paper is set aside.  With u = q / nu, (nu + 1) / 2 log1p(u) - q / 2 lies in [-q^2 / (4 nu), q / (2 nu)], so a term differs
    from the Gaussian one by at most q (q + 2) / (4 nu).  (A log(1 + u) in place of log1p(u) misses the allowance of the
    Student-t definition itself, which test_rows_against_the_definition holds on this case.  Within the bare allowance the two agree only for q below about 1e-2: the
    difference on paper is 1e-12 (1 + q / 2) of the term, the allowance 4e-15 of it.)"""
    c = rc.row_case("nu_extremes")
    big = c.alt[:, 2] == 1.0e12
    mod, res = rr.model(c.ltot, c.g, c.dx, c.idt, c.y)
    want, allow = rr.definition_rows(mod, res, c.yerr, np.zeros(int(big.sum()), dtype=np.int32), c.alt[big])
    lw = _lw(c)[big]
    for k, (scale, jitter, nu) in enumerate(c.alt[big]):
        q = res * res / ((scale * c.yerr) ** 2 + (jitter * mod) ** 2)
        paper = 1.001 * np.sum(q * (q + 2.0), axis=1) / (4.0 * nu)
        err = np.abs(lw[k].astype(np.longdouble) - want[k])
        assert np.all(err <= allow[k] + paper), (k, err, allow[k], paper)


def test_student_t_of_large_nu_within_the_bare_allowance_at_small_residuals():
    """The same without setting anything aside, where it can hold: with q < 1e-2 the two laws differ on paper by less than 1e-12
    (1 + q / 2) of a term of at most q / 2, below the allowance of 32 x 2^-53 per term.  The Student-t rows of `small_q` are held
    to the GAUSSIAN definition of their scale and jitter within the bare allowance."""
    c = rc.row_case("small_q")
    mod, res = rr.model(c.ltot, c.g, c.dx, c.idt, c.y)
    assert float(np.max(res * res / (c.yerr * c.yerr))) < 1.0e-2
    st = c.kind == rr.STUDENT
    assert np.all(c.alt[st, 2] == 1.0e12) and int(st.sum()) == 2
    want, allow = rr.definition_rows(mod, res, c.yerr, np.zeros(2, dtype=np.int32), c.alt[st])
    err = np.abs(_lw(c)[st].astype(np.longdouble) - want)
    assert np.all(err <= allow), float(np.max(err / allow))
    print(f"nu = 1e12 at q < 1e-2 against the Gaussian definition: worst error / allowance {float(np.max(err / allow)):.3f}")


@pytest.mark.parametrize("n", rc.COLUMN_N)
def test_columns_against_direct_numpy(n):
    lw = rc.column_case(n)
    table, tail = rr.cols(lw)
    assert tail.shape == (8, pr.tail_len(n))
    for k, col in enumerate(lw):
        v = np.sort(col[~np.isnan(col)])                     # (numpy's sort leaves -0.0 and +0.0 in either order: compared by value)
        m = v.size
        assert table[k, rr.N_USED] == m
        if m == 0:
            assert np.all(np.isnan(table[k, [rr.LW_MEAN, rr.LW_MIN, rr.LW_MAX, rr.CUT]])) and np.all(np.isnan(tail[k]))
            assert table[k, rr.LSE1_M] == -np.inf and table[k, rr.LSE1_S] == 0.0 and table[k, rr.NONTAIL_COUNT] == 0
            continue
        tm = min(pr.tail_len(m), m)
        assert table[k, rr.LW_MIN] == v[0] and table[k, rr.LW_MAX] == v[-1] and table[k, rr.CUT] == v[m - tm]
        assert np.array_equal(tail[k, :tm], v[m - tm:]) and np.all(np.isnan(tail[k, tm:])) and np.all(np.diff(rr.key(tail[k, :tm]).astype(float)) >= 0)
        nontail = rr.key(col) <= rr.key(table[k, rr.CUT:rr.CUT + 1])[0]
        nontail &= ~np.isnan(col)
        assert table[k, rr.NONTAIL_COUNT] == nontail.sum() >= m - tm + 1 - np.sum(v[m - tm:] == v[m - tm]) + 1 - 1
        with np.errstate(divide="ignore", invalid="ignore"):
            got = [table[k, a] + np.log(table[k, b]) for a, b in ((rr.LSE1_M, rr.LSE1_S), (rr.LSE2_M, rr.LSE2_S), (rr.NONTAIL_M, rr.NONTAIL_S))]
        want = [logsumexp(v), logsumexp(2.0 * v), logsumexp(col[nontail])]
        for g, w in zip(got, want):
            assert (g == w) if not np.isfinite(w) else abs(g - w) <= 1e-12 * max(1.0, abs(w)), (k, g, w)
        if np.all(np.isfinite(v)):
            assert abs(table[k, rr.LW_MEAN] - np.mean(v)) <= 1e-12 * max(1.0, np.max(np.abs(v)))
    # -0.0 sits below +0.0: the row of mixed zeros
    z = lw[5]
    if np.any((z == 0.0) & np.signbit(z)) and np.any((z == 0.0) & ~np.signbit(z)):
        srt = z[np.argsort(rr.key(z), kind="stable")]
        zeros = srt[srt == 0.0]
        assert np.all(np.diff(np.signbit(zeros).astype(int)) <= 0)
