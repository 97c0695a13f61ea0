"""GPU tests of the derived quantities (mp_model_derived, run with -m gpu on an MI355X): the device table against the numpy
restatement (tests/derive_restated.py) applied to the five curves mp_model_lc returns for the same rows one by one, bit for bit;
independence of the batch size across the chunk boundary; the front ends; and the reference's own values
(tests/golden/golden_derived.npz).

The bit-for-bit comparison with mp_model_lc and the physical / sampler-coordinate test run on a handle whose prior box is in
physical units with no log mask (`phys`), not on the log-masked Humped handle: mp_model_lc takes physical parameters, and the
device's 10^x and numpy's need not agree to the bit, so a log-masked row has no physical twin that is the same numbers.  On
`phys` the two forms of a row ARE the same numbers, so that test pins the prior and the `physical` flag, not the un-logging.  The
log-masked path of model_derived is compared bit for bit only with itself (independence of n, repeat, the sampler wiring) and,
to a tolerance, with its physical twin (test_log_masked_rows_against_their_physical_twins)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, LC_REF_RTOL, LC_TIGHT_RTOL, TRUTHS

import derive_restated as dr

pytestmark = pytest.mark.gpu

# the synthetic prior box in PHYSICAL units with no log mask: on such a handle a row means the same numbers with physical = 0
# (prior applied) and physical = 1, and mp_model_lc takes it as it is
PHYS_LOWER = np.array([1.0e-3, 0.69, 1.0e-6, 50.0, 1.0e-2, 1.0e-1])
PHYS_UPPER = np.array([10.0, 10.0, 1.0e-2, 2000.0, 1.0e2, 1.0e3])
# rows of the fixture whose recorded neighbourhood cannot decide the peak time (at most 2)
UNDECIDED = ()


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a), np.signbit(b))


@pytest.fixture(scope="module")
def humped(tarr, gsynth):
    from magprop_amd import _capi, synth
    h = _capi.Handle(_capi.cfg_synth(), tarr)
    h.set_dataset(0, gsynth["Humped_x"], gsynth["Humped_y"], gsynth["Humped_yerr"])
    h.set_prior(synth.PRIOR_LOWER, synth.PRIOR_UPPER, synth.LOG_MASK)
    yield h
    h.close()


@pytest.fixture(scope="module")
def phys(tarr):
    from magprop_amd import _capi
    h = _capi.Handle(_capi.cfg_synth(), tarr)
    h.set_prior(PHYS_LOWER, PHYS_UPPER, 0)
    yield h
    h.close()


def _unlog(S):
    P = np.array(S, dtype=np.float64)
    P[:, 2:6] = 10.0 ** P[:, 2:6]
    return P


def _rows70(gflag):
    """near-truth rows, prior-wide rows, two rows outside the prior and flagged rows of the flag scan, in physical units"""
    from magprop_amd import synth
    rng = np.random.default_rng(11)
    flag = gflag["pars"][gflag["status"] == 1][:12]
    near = np.array(TRUTHS["Humped"]) + 0.02 * rng.standard_normal((28, 6))
    wide = synth.PRIOR_LOWER + (synth.PRIOR_UPPER - synth.PRIOR_LOWER) * rng.random((70 - 28 - 2 - len(flag), 6))
    out = np.array(TRUTHS["Humped"]) + np.zeros((2, 6))
    out[0, 0], out[1, 1] = 50.0, 0.1                           # B above, P below the box
    P = _unlog(np.concatenate([near, wide, out, flag]))
    return P[rng.permutation(len(P))]


def _host_path(h, P, inside):
    """(table, status) of mp_model_lc row by row and the restatement; rows outside the prior: status 3"""
    out = np.full((len(P), dr.N), np.nan)
    st = np.full(len(P), 3, dtype=np.int32)
    for i in np.nonzero(inside)[0]:
        s, lc, traj = h.model_lc(P[i], want_traj=True)
        st[i] = s
        if s == 0:
            out[i] = dr.derive_row(np.stack([lc[1], lc[2], lc[3], traj[0], traj[1]]), lc[0])
    return out, st


@pytest.fixture(scope="module")
def rows70(phys, gflag):
    P = _rows70(gflag)
    inside = np.all((P >= PHYS_LOWER) & (P <= PHYS_UPPER), axis=1)
    return P, inside, _host_path(phys, P, inside)


def test_table_equals_the_restatement_of_model_lc_curves(phys, rows70):
    P, inside, (want, st_want) = rows70
    assert len(P) == 70 and int((~inside).sum()) == 2
    got, st, used = phys.model_derived(P)
    assert np.array_equal(st, st_want)
    assert np.sum(st == 0) >= 40 and np.sum(st == 1) >= 1 and np.sum(st == 3) == 2
    assert used == int(np.sum(st == 0))
    assert np.all(np.isnan(got[st != 0])) and np.all(np.isfinite(got[st == 0]))
    bad = np.nonzero([not _same(got[i], want[i]) for i in range(70)])[0]
    assert bad.size == 0, (bad[:5], got[bad[:2]], want[bad[:2]])


def test_physical_and_sampler_coordinates_agree(phys, rows70):
    P, inside, _ = rows70
    a, sta, ua = phys.model_derived(P[inside])
    b, stb, ub = phys.model_derived(P[inside], physical=True)
    assert np.array_equal(sta, stb) and ua == ub and _same(a, b)


def test_log_masked_rows_against_their_physical_twins(humped):
    """model_derived(S) under the log mask against model_derived(10 ** S, physical=True).  The two parameter sets differ by a
    few ulp (the device's 10^x is held to 2 ulp, numpy's to 1), the solver then runs twice on its own: each curve is within
    1e-12 + LC_TIGHT_RTOL |ref| of the tight reference point by point (the bound of the parity tests), so the two agree to
    twice that, and so do trapezoids (non-negative combinations; the 1e-12 over t_end - t_0) and maxima and end values
    (1-Lipschitz).  The trajectory columns have no such recorded bound and are held to the same relative figure, which is four
    orders above what a perturbation of a few ulp does near the truths.  The time-valued columns are not compared: a peak that
    is flat to a few ulp may sit at another grid point."""
    rng = np.random.default_rng(15)
    S = np.array(TRUTHS["Humped"]) + 0.02 * rng.standard_normal((48, 6))
    a, sta, _ = humped.model_derived(S)
    b, stb, _ = humped.model_derived(_unlog(S), physical=True)
    assert np.all(sta == 0) and np.all(stb == 0)
    span = humped.tgrid[-1] - humped.tgrid[0]
    for col, atol in ((dr.E_TOT, 1e-12 * span), (dr.E_PROP, 1e-12 * span), (dr.E_DIP, 1e-12 * span), (dr.L_PEAK, 1e-12),
                      (dr.LPROP_PEAK, 1e-12), (dr.OMEGA_END, 0.0), (dr.OMEGA_MAX, 0.0), (dr.MDISC_END, 0.0), (dr.MDISC_MAX, 0.0)):
        d = np.abs(a[:, col] - b[:, col])
        print(f"column {col}: largest relative difference {np.max(d / np.maximum(np.abs(b[:, col]), 1e-300)):.3e}")
        assert np.all(d <= 2.0 * (atol + LC_TIGHT_RTOL * np.abs(b[:, col]))), (col, np.max(d))


def test_a_row_does_not_depend_on_the_batch(humped):
    n = humped.n_simd + 6                                       # one full chunk and a short one
    rng = np.random.default_rng(12)
    S = np.array(TRUTHS["Humped"]) + 0.05 * rng.standard_normal((n, 6))
    S[5::97, 0] = 50.0                                          # some rows outside the prior
    got, st, used = humped.model_derived(S)
    assert got.shape == (n, 16) and used == int(np.sum(st == 0)) and used > n - 40 and np.sum(st == 3) >= 10
    for r in (0, humped.n_simd - 1, humped.n_simd, n - 1):
        alone, st1, u1 = humped.model_derived(S[r:r + 1])
        assert st1[0] == st[r] == 0 and u1 == 1 and _same(alone[0], got[r]), r
    assert np.all(np.isnan(got[st != 0])) and np.all(np.isfinite(got[st == 0]))


def test_all_rows_fail(humped):
    from magprop_amd import _capi
    S = np.array(TRUTHS["Humped"]) + np.zeros((64, 6))
    S[:, 0] = 50.0                                              # B outside the prior
    got, st, used = humped.model_derived(S)
    assert used == 0 and np.all(st == 3) and got.shape == (64, 16) and np.all(np.isnan(got))
    out = np.empty((64, 16))
    assert _capi.lib().mp_model_derived(humped._h, _capi._dptr(S), 64, 6, 0, _capi._dptr(out), None, None) == _capi.MP_OK
    assert np.all(np.isnan(out))
    with pytest.raises(ValueError, match="ndim"):
        humped.model_derived(np.zeros((3, 5)))
    with pytest.raises(ValueError, match="2-D"):
        humped.model_derived(np.zeros((0, 6)))


def test_repeat_is_bitwise(humped):
    rng = np.random.default_rng(13)
    S = np.array(TRUTHS["Humped"]) + 0.05 * rng.standard_normal((300, 6))
    a, b = humped.model_derived(S), humped.model_derived(S)
    assert _same(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


def test_library_variant_front_end_with_nine_parameters():
    """A smoke of magprop_amd.mcmc_eqns.model_derived: finite values and E_tot within 1e-12 relative of E_prop + E_dip.
    Ltot is not Lprop + Ldip point by point: the kernel forms f_beam (ld + lp) / 1e50 next to lp / 1e50 and ld / 1e50
    (mp_eval.hpp luminosity), three roundings apart, <= 4 u relative with u = 2^-53 where f_beam = 1, as in these rows.  The
    terms are non-negative, so each of the three sums is within (seg + 256 + 3) u = 299 u of its exact value; together
    <= 3 x 299 u + 4 u = 1.0e-13 relative, inside the 1e-12 asked for."""
    from magprop_amd import _capi, derived, engine, mcmc_eqns
    rng = np.random.default_rng(14)
    # the point-wise figure, measured on three curves of these rows (printed; the docstring's bound is the analytic one)
    with engine.use(_capi.cfg_lib(), "L", -1) as eng:
        for p in ([1.0, 5.0, 1e-2, 100.0, 1.0, 1.0, 0.5, 0.5, 1.0], [2.0, 3.0, 3e-2, 300.0, 0.5, 2.0, 0.3, 0.7, 1.0],
                  [0.5, 8.0, 5e-3, 80.0, 3.0, 0.3, 0.9, 0.1, 1.0]):
            s_, lc = eng.handle.model_lc(np.array(p))
            if s_ == 0:
                rel = np.abs(lc[1] - (lc[2] + lc[3])) / np.maximum(lc[1], 1e-300)
                print(f"Ltot against Lprop + Ldip point by point: largest relative difference {np.max(rel):.3e}, "
                      f"{int(np.count_nonzero(rel))} of {rel.size} points differ")
    S = np.array([1.0, 5.0, -2.0, 2.0, 0.0, 0.0, 0.5, 0.5, 1.0]) + np.zeros((40, 9))
    S[:, :6] += 0.05 * rng.standard_normal((40, 6))
    S[7, 0] = 50.0
    res = mcmc_eqns.model_derived(S, "L")
    v, st = res["values"], res["status"]
    assert v.shape == (40, 16) and st[7] == 3 and res["n_used"] == int(np.sum(st == 0)) >= 35
    ok = st == 0
    assert np.all(np.isfinite(v[ok])) and np.all(np.isnan(v[~ok]))
    d = derived.as_dict(v[ok])
    assert np.all(d["E_tot"] > 0.0)
    assert np.all(np.abs(d["E_tot"] - (d["E_prop"] + d["E_dip"])) <= 1e-12 * d["E_tot"])
    assert res["summary"]["n_used"] == res["n_used"] and res["summary"]["E_tot"].shape == (3,)


def test_sampler_wiring(gsynth):
    from magprop_amd import EnsembleSampler, derived, synth
    x, y, yerr = gsynth["Humped_x"], gsynth["Humped_y"], gsynth["Humped_yerr"]
    rng = np.random.default_rng(4)
    p0 = np.array(TRUTHS["Humped"]) + 1e-3 * rng.standard_normal((64, 6))
    s = EnsembleSampler(64, 6, x, y, yerr, seed=5)
    s.run_mcmc(p0, 200)
    got = s.get_derived(discard=100, thin=5)
    rows = s.get_chain()[100::5].reshape(-1, 6)
    want = synth.model_derived(rows)
    assert got["values"].shape == (20 * 64, 16) and got["n_used"] == want["n_used"] > 0
    assert _same(got["values"], want["values"]) and np.array_equal(got["status"], want["status"])
    for name in derived.NAMES:
        assert _same(got["summary"][name], want["summary"][name]), name
    assert _same(got["summary"]["t50"], np.nanquantile(got["values"][:, dr.T50], (0.16, 0.5, 0.84)))
    s.close()
    # two ensembles: ensemble=1 takes the second dataset's walkers
    xc, yc, ec = gsynth["Classic_x"], gsynth["Classic_y"], gsynth["Classic_yerr"]
    s2 = EnsembleSampler(32, 6, datasets=[(x, y, yerr), (xc, yc, ec)], seed=6)
    p2 = np.concatenate([np.array(TRUTHS["Humped"]) + 1e-3 * rng.standard_normal((32, 6)),
                         np.array(TRUTHS["Classic"]) + 1e-3 * rng.standard_normal((32, 6))])
    s2.run_mcmc(p2, 20)
    d1 = s2.get_derived(q=(0.5,), ensemble=1)
    want1 = synth.model_derived(s2.get_chain()[:, 32:].reshape(-1, 6), q=(0.5,))
    assert _same(d1["values"], want1["values"])
    d0 = s2.get_derived(q=(0.5,), ensemble=0)
    assert not np.array_equal(d0["values"], d1["values"], equal_nan=True)
    s2.close()
    g = EnsembleSampler(8, 2, target="gaussian")
    g.run_mcmc(rng.standard_normal((8, 2)), 5)
    with pytest.raises(ValueError, match="gaussian"):
        g.get_derived()
    g.close()


def test_against_the_reference(tarr):
    """Columns 0 to 2 are trapezoids (non-negative combinations of the curve's points, weights summing to t_end - t_0) and
    columns 3 and 5 maxima (1-Lipschitz), so the point-wise curve bound |d| <= 1e-12 + rtol |ref| of the parity tests carries
    over: 1e-12 (t_end - t_0) + rtol |ref| and 1e-12 + rtol |ref|.  The peak times: the device's time must be a grid time at
    which the reference's tight curve is within 2 LC_TIGHT_RTOL relative of its own peak, judged on the recorded neighbours."""
    from magprop_amd import _capi
    g = np.load(os.path.join(GOLDEN, "golden_derived.npz"))
    span = float(g["t_last"] - g["t_first"])
    assert tarr[0] == g["t_first"] and tarr[-1] == g["t_last"]
    h = _capi.Handle(_capi.cfg_synth(), tarr)
    got, st, used = h.model_derived(g["pars"], physical=True)
    h.close()
    n = len(g["pars"])
    assert used == n and np.all(st == 0)
    for ref, rtol in ((g["tight"], LC_TIGHT_RTOL), (g["ref"], LC_REF_RTOL)):
        for col in (0, 1, 2):
            d = np.abs(got[:, col] - ref[:, col])
            assert np.all(d <= 1e-12 * span + rtol * np.abs(ref[:, col])), (col, rtol, np.max(d / np.abs(ref[:, col])))
        for col in (3, 5):
            d = np.abs(got[:, col] - ref[:, col])
            assert np.all(d <= 1e-12 + rtol * np.abs(ref[:, col])), (col, rtol, d, ref[:, col])
    nbr = g["tight_peak_nbr"]
    K = (nbr.shape[2] - 1) // 2
    undecided = []
    for r in range(n):
        for k, col in enumerate((4, 6)):
            j = int(np.nonzero(tarr == got[r, col])[0][0])      # (a grid time: exactly one hit)
            off = j - int(g["tight_peak_idx"][r, k])
            if abs(off) > K or np.isnan(nbr[r, k, off + K]):
                undecided.append(r)
                continue
            peak = nbr[r, k, K]
            assert nbr[r, k, off + K] >= peak - 2.0 * LC_TIGHT_RTOL * abs(peak), (r, col, off, nbr[r, k, off + K], peak)
    assert set(undecided) <= set(UNDECIDED) and len(UNDECIDED) <= 2, undecided


def test_nested_results_helper(gsynth):
    """The weighted samples of a short nested run through model_derived and the weighted summary, no resampling."""
    from magprop_amd import NestedSampler, derived
    x, y, yerr = gsynth["Humped_x"], gsynth["Humped_y"], gsynth["Humped_yerr"]
    s = NestedSampler(x, y, yerr, nlive=64, nbatch=16, seed=3)
    res = s.run_nested(dlogz=0.5, maxiter=30)
    d = s.get_derived()
    assert d["values"].shape == (len(res.samples), 16) and d["n_used"] > 0
    want = derived.summarize(d["values"], (0.16, 0.5, 0.84), np.exp(res.logwt - np.max(res.logwt)))
    for name in derived.NAMES:
        assert _same(d["summary"][name], want[name]), name
    direct = s.handle.model_derived(res.samples)
    assert _same(d["values"], direct[0])
    s.close()
