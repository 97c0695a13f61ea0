"""GPU tests of the importance reweighting end to end (mp_model_reweight, run with -m gpu on an MI355X) on the synthetic Humped
set: the log weights against the probe's row kernel on the curve mp_model_lc returns for the same rows one by one, bit for bit;
independence of the chunking; the identity and leave-one-out alternatives; statuses; the columns against the restatement of
the returned log weights; the refusals behind a handle; the front ends; and one statistical check against a second run.

As in tests/test_gpu_pointwise.py the bit-for-bit comparisons with mp_model_lc run on a handle whose prior box is in physical
units with no log mask (`phys`)."""
import math

import numpy as np
import pytest

from conftest import TRUTHS

import pointwise_restated as pr
import reweight_restated as rr
from test_gpu_bridge import EVIDENCE_INFLATION, box_start
from test_gpu_derived import PHYS_LOWER, PHYS_UPPER, _unlog
from test_gpu_reweight_kernels import Probe, same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe():
    return Probe()


@pytest.fixture(scope="module")
def phys(tarr, gsynth):
    from magprop_amd import _capi
    h = _capi.Handle(_capi.cfg_synth(), tarr)
    h.set_prior(PHYS_LOWER, PHYS_UPPER, 0)
    h.set_dataset(0, gsynth["Humped_x"], gsynth["Humped_y"], gsynth["Humped_yerr"])
    yield h
    h.close()


def _dataset(h, gsynth):
    """the Humped set as the library keeps it: ascending time (stable), digested on the handle's grid"""
    x, y, yerr = gsynth["Humped_x"], gsynth["Humped_y"], gsynth["Humped_yerr"]
    order = np.argsort(x, kind="stable")
    g, dx, idt = pr.digest(h.tgrid, x[order])
    return g, dx, idt, np.ascontiguousarray(y[order]), np.ascontiguousarray(yerr[order])


@pytest.fixture(scope="module")
def big(phys, gsynth, gcorners):
    """n = mp_n_simd + 7 rows, two chunks: a ball about the truth, one row outside the box and a break-up corner the model flags
    in the first chunk, a row outside the box in the second; nine alternatives with and without weights."""
    from magprop_amd import reweight
    n = phys.n_simd + 7
    rng = np.random.default_rng(61)
    P = _unlog(np.array(TRUTHS["Humped"]) + 0.02 * rng.standard_normal((n, 6)))
    P[40, 0] = 50.0                                           # B above the box
    P[71] = np.clip(_unlog(gcorners["pars"][gcorners["status"] == 1]), PHYS_LOWER, PHYS_UPPER)[0]
    P[n - 3, 1] = 0.1                                         # outside the box, in the second chunk
    n_obs = phys.dataset_size(0)
    alts = [reweight.gaussian(), reweight.gaussian(1.3), reweight.gaussian(1.0, 0.1), reweight.student_t(4.0), reweight.student_t(0.5, 0.8, 0.05),
            reweight.gaussian(leave_out=[7]), reweight.gaussian(power=0.5), reweight.student_t(30.0, weights=rng.uniform(0.0, 2.0, n_obs)),
            reweight.gaussian(1.1, leave_out=np.arange(n_obs) % 3 == 0)]
    kind, alt, obs_w = reweight.pack(alts, n_obs)             # (weights in the library's order here)
    lw, table, tail, st, used = phys.model_reweight(P, kind, alt, obs_w)
    return dict(P=P, n=n, kind=kind, alt=alt, obs_w=obs_w, lw=lw, table=table, tail=tail, st=st, used=used, alts=alts)


def test_rows_equal_the_probe_on_model_lc(phys, probe, gsynth, big):
    import reweight_cases as rc
    n, st = big["n"], big["st"]
    assert n > phys.n_simd and big["lw"].shape == (9, n) and big["table"].shape == (9, 12) and big["tail"].shape == (9, pr.tail_len(n))
    assert st[40] == 3 and st[71] == 1 and st[n - 3] == 3 and big["used"] == int(np.sum(st == 0)) >= n - 12
    assert np.array_equal(st, phys.lnprob_batch(big["P"], ds_id=0, want_status=True)[1])
    assert np.array_equal(np.isnan(big["lw"]), np.broadcast_to(st != 0, big["lw"].shape))       # NaN in every alternative, and nowhere else
    g, dx, idt, y, yerr = _dataset(phys, gsynth)
    rows = [i for i in list(range(6)) + [39, 41, 70, 72, phys.n_simd - 1] + list(range(phys.n_simd, n)) if st[i] == 0]
    ltot = np.empty((len(rows), phys.tgrid.size))
    for r, i in enumerate(rows):
        s, lc = phys.model_lc(big["P"][i])
        assert s == 0
        ltot[r] = lc[1]
    case = rc.RowCase(phys.tgrid, ltot, np.zeros(len(rows), dtype=np.int32), g, dx, idt, y, yerr, big["kind"], big["alt"], big["obs_w"])
    want = probe.rows(case)
    assert same(big["lw"][:, rows], want), (big["lw"][:, rows] - want)
    assert same(want, rr.rows(ltot, case.status, g, dx, idt, y, yerr, big["kind"], big["alt"], big["obs_w"], probe.libm))
    # the identity alternative: exactly +0.0
    assert same(big["lw"][0, st == 0], np.zeros(big["used"]))


def test_a_row_is_the_same_alone(phys, big):
    n = big["n"]
    for i in (0, 1, phys.n_simd - 1, phys.n_simd, n - 1):
        lw1, table1, tail1, st1, used1 = phys.model_reweight(big["P"][i:i + 1], big["kind"], big["alt"], big["obs_w"])
        assert st1[0] == big["st"][i] == 0 and used1 == 1 and same(lw1[:, 0], big["lw"][:, i]), i
        assert same(table1[:, rr.LW_MEAN], lw1[:, 0]) and same(tail1[:, 0], lw1[:, 0]) and tail1.shape == (9, pr.tail_len(1))
        assert np.all(np.isnan(tail1[:, 1:]))
    # a failed row alone
    lw1, table1, tail1, st1, used1 = phys.model_reweight(big["P"][40:41], big["kind"], big["alt"], big["obs_w"])
    assert st1[0] == 3 and used1 == 0 and np.all(np.isnan(lw1)) and np.all(table1[:, rr.N_USED] == 0) and np.all(np.isnan(tail1))
    # the rows in another order and company: the same numbers in their new places
    idx = np.array([n - 1, 5, 40, phys.n_simd, 3])
    lw5 = phys.model_reweight(big["P"][idx], big["kind"][2:5], big["alt"][2:5], None)[0]
    full = phys.model_reweight(big["P"][idx], big["kind"], big["alt"], big["obs_w"])[0]
    assert same(full, big["lw"][:, idx]) and same(lw5, big["lw"][2:5][:, idx])


def test_columns_equal_the_restatement_of_the_log_weights(probe, big):
    want, want_tail = rr.cols(big["lw"], libm=probe.libm)
    for col in range(rr.N):
        assert same(big["table"][:, col], want[:, col]), (col, big["table"][:, col], want[:, col])
    assert same(big["tail"], want_tail)
    assert np.all(big["table"][:, rr.N_USED] == big["used"])


def _raw(h, P, kind, alt, obs_w=None, ds_id=0, out=None):
    """mp_model_reweight itself with the table as the only output: (code, message)"""
    from magprop_amd import _capi
    from raw_abi import dp, ip
    kind, alt = np.ascontiguousarray(kind, dtype=np.int32), np.ascontiguousarray(alt, dtype=np.float64)
    out = np.empty((kind.size, 12)) if out is None else out
    rc_ = _capi.lib().mp_model_reweight(h._h, dp(P), len(P), P.shape[1], 0, ds_id, kind.size, ip(kind), dp(alt), dp(obs_w), None, dp(out), None,
                                        None, None)
    return rc_, _capi.last_error()


def test_table_without_the_optional_outputs(phys, big):
    out = np.full((9, 12), -7.0)
    assert _raw(phys, big["P"], big["kind"], big["alt"], big["obs_w"], out=out)[0] == 0 and same(out, big["table"])


def test_leave_one_out_against_the_pointwise_cells(phys, probe, gsynth, big):
    """Alternative j leaves observation j out: lw = -t_0 of that observation = 0.5 q + 0.5 log(ye^2), q = res^2 / ye^2, and
    mp_model_pointwise's cell r = 0.5 (res / ye)^2.  The quotient res / ye carries half an ulp, so its square 1 ulp and a
    rounding, against q's two roundings: 0.5 q lies within 4 ulp of r, and lw = fl(0.5 q + g) within 4 ulp(r) + ulp(lw) / 2 of
    r + g, g the device's 0.5 log(ye ye) to the bit; the float64 sum r + g it is held to adds half an ulp of its own."""
    from magprop_amd import reweight
    P = big["P"][:64]
    n_obs = phys.dataset_size(0)
    alts = [reweight.gaussian(leave_out=[j]) for j in range(n_obs)]
    kind, alt, obs_w = reweight.pack(alts, n_obs)
    lw, table, tail, st, used = phys.model_reweight(P, kind, alt, obs_w)
    obs, ptail, pst, pused, z = phys.model_pointwise(P, ds_id=0, cells=True)
    assert np.array_equal(st, pst) and used == pused and lw.shape == z.shape == (n_obs, 64)
    yerr = _dataset(phys, gsynth)[4]
    g = 0.5 * probe.libm.log(yerr * yerr)
    r = 0.5 * (z * z)
    ok = st == 0
    want = r[:, ok] + g[:, None]
    tol = 4.0 * np.spacing(r[:, ok]) + 0.5 * np.spacing(np.abs(lw[:, ok])) + 0.5 * np.spacing(np.abs(want))
    err = np.abs(lw[:, ok] - want)
    print(f"leave-one-out against the pointwise cells: worst error / tolerance {np.max(err / tol):.3f}")
    assert np.all(err <= tol), float(np.max(err / tol))
    assert np.all(np.isnan(lw[:, ~ok])) and int((~ok).sum()) == 1


def test_refusals_behind_a_handle(phys):
    from magprop_amd import _capi
    P = _unlog(np.array([TRUTHS["Humped"]] * 4))
    n_obs = phys.dataset_size(0)
    good = (np.zeros(1, dtype=np.int32), np.array([[1.2, 0.0, 0.0]]))
    with pytest.raises(_capi.MagpropAmdError, match="unset dataset 7"):
        phys.model_reweight(P, *good, ds_id=7)
    # the unset dataset comes before a bad obs_w, a bad alternative before the unset dataset
    rc_, msg = _raw(phys, P, *good, obs_w=np.full((1, n_obs), -1.0), ds_id=7)
    assert rc_ == _capi.MP_ESTATE and "unset dataset 7" in msg
    rc_, msg = _raw(phys, P, [0], [[-1.0, 0.0, 0.0]], obs_w=np.full((1, n_obs), -1.0), ds_id=7)
    assert rc_ == _capi.MP_EINVAL and "alternative 0" in msg
    rc_, msg = _raw(phys, P, *good, obs_w=np.full((1, n_obs), -1.0))
    assert rc_ == _capi.MP_EINVAL and "obs_w[0][0]" in msg
    for bad in (-1.0, np.nan, np.inf):
        w = np.ones((1, n_obs))
        w[0, n_obs - 1] = bad
        with pytest.raises(ValueError, match="obs_w"):
            phys.model_reweight(P, *good, obs_w=w)
    for kind, alt in ((2, [1.0, 0.0, 1.0]), (0, [0.0, 0.0, 0.0]), (0, [np.inf, 0.0, 0.0]), (0, [1.0, -0.1, 0.0]), (1, [1.0, 0.0, 0.0]),
                      (1, [1.0, 0.0, np.nan])):
        with pytest.raises(ValueError, match="alternative 1"):
            phys.model_reweight(P, np.array([0, kind], dtype=np.int32), np.array([[1.0, 0.0, 0.0], alt]))
    assert phys.model_reweight(P, np.zeros(1, dtype=np.int32), np.array([[1.0, 0.0, np.nan]]))[4] == 4    # a Gaussian's nu is not read
    with pytest.raises(ValueError, match="MP_REWEIGHT_MAX_ALT"):
        phys.model_reweight(P, np.zeros(65, dtype=np.int32), np.tile([1.0, 0.0, 0.0], (65, 1)))
    with pytest.raises(ValueError, match="MP_POINTWISE_MAX_SAMPLES"):
        phys.model_reweight(np.zeros((_capi.POINTWISE_MAX_SAMPLES + 1, 6)), *good)
    with pytest.raises(ValueError, match="2-D"):
        phys.model_reweight(np.zeros(6), *good)


def test_front_ends(gsynth):
    from magprop_amd import EnsembleSampler, mcmc_eqns, reweight, synth
    x, y, yerr = gsynth["Humped_x"], gsynth["Humped_y"], gsynth["Humped_yerr"]
    rev = np.arange(x.size)[::-1]                             # the caller's order is not the library's
    rng = np.random.default_rng(62)
    w = rng.uniform(0.0, 2.0, x.size)
    s = EnsembleSampler(32, 6, x[rev], y[rev], yerr[rev], seed=5)
    s.monitor_samples(128)
    s.run_mcmc(np.array(TRUTHS["Humped"]) + 1.0e-3 * rng.standard_normal((32, 6)), 6)
    alts = [reweight.gaussian(1.2), reweight.student_t(4.0, weights=w[rev]), reweight.gaussian(leave_out=[0])]
    a = s.get_reweight(alts)
    flat = s.get_chain(flat=True)
    b = synth.model_reweight(flat, x[rev], y[rev], yerr[rev], alts)
    assert a["n_used"] == b["n_used"] == 192 and np.array_equal(a["status"], b["status"])
    for k in ("lw", "table", "tail", "n_eff", "khat", "log_evidence_ratio", "log_evidence_ratio_err"):
        assert same(a[k], b[k]), k
    assert a["lw"].shape == (3, 192) and a["table"].shape == (3, 12) and np.all(np.isfinite(a["log_evidence_ratio"]))
    # per-observation weights follow the caller's order of x: the same light curve given in ascending time
    c = synth.model_reweight(flat, x, y, yerr, [reweight.gaussian(1.2), reweight.student_t(4.0, weights=w), reweight.gaussian(leave_out=[x.size - 1])])
    assert same(c["lw"], b["lw"]) and same(c["table"], b["table"])
    assert s.get_reweight(alts, discard=2, thin=2)["n_used"] == 64
    r = s.get_reweight(alts[0], source="reservoir")
    assert r["lw"].shape == (1, 128) and r["n_used"] == 128
    wk = reweight.weights(a["lw"], 0)
    band = s.get_model_band(weights=wk)
    assert abs(band["n_eff"] - a["n_eff"][0]) < 1e-9 * band["n_eff"]
    s.close()
    with pytest.raises(ValueError, match="samples must be 2-D"):
        synth.model_reweight(flat[:, :5], x, y, yerr, alts)
    # the library variant: finite weights under the variant's prior box, the identity exactly 0
    data = {"t": x, "Lum50": y, "Lum50err": yerr}
    S = np.array(TRUTHS["Humped"]) + 0.01 * np.abs(rng.standard_normal((8, 6)))
    lib = mcmc_eqns.model_reweight(S, data, "L", [reweight.gaussian(), reweight.gaussian(1.3, 0.05)])
    ok = lib["status"] == 0
    assert lib["lw"].shape == (2, 8) and lib["n_used"] == int(ok.sum()) >= 1
    assert same(lib["lw"][0, ok], np.zeros(int(ok.sum()))) and np.all(np.isfinite(lib["lw"][1, ok])) and np.all(np.isnan(lib["lw"][:, ~ok]))


def test_reweighted_chain_against_a_second_run(gsynth):
    """The brute-force case of tests/test_gpu_bridge.py (Humped with yerr x 10, KDE move, 512 walkers, 400 steps from box draws,
    the first 100 discarded).  The chain, thinned by ceil(tau), is reweighted to scale = 1.2; a second run samples yerr x 12.
    Both runs sample the unnormalised lnlike = -0.5 chi^2, whose evidence misses prod 1 / (scale yerr): log_evidence_ratio +
    n_obs ln 1.2 is the difference of the two runs' log_evidence(method="bridge"), and the weighted parameter means are the
    second run's.  Margins: 5 combined standard errors of the estimators' own reported errors -- the delta-method error of the
    ratio and the two dlnz; sensitivity's weighted_mean_err of the reweighted, thinned rows and its mean_err of the second run's
    rows thinned by its own ceil(tau)."""
    from magprop_amd import EnsembleSampler, KDEMove, LogProb, reweight, synth
    x, y = gsynth["Humped_x"], gsynth["Humped_y"]
    runs = []
    for k, factor in enumerate((EVIDENCE_INFLATION, 1.2 * EVIDENCE_INFLATION)):
        yerr = gsynth["Humped_yerr"] * factor
        s = EnsembleSampler(512, 6, x, y, yerr, seed=3100 + k, moves=KDEMove())
        s.run_mcmc(box_start(LogProb(x, y, yerr), 512, np.random.default_rng(3200 + k)), 400)
        ev = s.log_evidence(method="bridge", discard=100)
        tau = s.get_autocorr_time(tol=0, quiet=True)
        assert np.all(np.isfinite(tau)), tau
        thin = int(math.ceil(float(np.max(tau))))
        rows = np.ascontiguousarray(s.get_chain()[100::thin].reshape(-1, 6))
        runs.append(dict(ev=ev, rows=rows, yerr=yerr, thin=thin))
        s.close()
    assert runs[0]["ev"].ok and runs[1]["ev"].ok
    a, b = runs
    alt = [reweight.gaussian(scale=1.2)]
    res = synth.model_reweight(a["rows"], x, y, a["yerr"], alt)
    got = res["log_evidence_ratio"][0] + x.size * math.log(1.2)
    want = b["ev"].lnz - a["ev"].lnz
    se = math.sqrt(res["log_evidence_ratio_err"][0] ** 2 + a["ev"].dlnz ** 2 + b["ev"].dlnz ** 2)
    print(f"thin {a['thin']} and {b['thin']}: {a['rows'].shape[0]} rows reweighted, n_eff {res['n_eff'][0]:.0f}, khat {res['khat'][0]:.3f}; "
          f"ln Z ratio {got:+.4f} against {want:+.4f} from two bridge estimates, combined se {se:.4f}: {(got - want) / se:+.2f} se")
    assert res["n_used"] == a["rows"].shape[0]                # (a chain holds no row whose model failed)
    assert abs(got - want) < 5.0 * se
    sens = reweight.sensitivity(a["rows"], res["lw"])
    se_w = sens["weighted_mean_err"][0]
    se_b = reweight.sensitivity(b["rows"], np.zeros((1, b["rows"].shape[0])))["mean_err"]
    dev = (sens["weighted_mean"][0] - b["rows"].mean(axis=0)) / np.hypot(se_w, se_b)
    print(f"weighted means against the second run's, in combined se: {np.round(dev, 2).tolist()}; unweighted: "
          f"{np.round((sens['mean'] - b['rows'].mean(axis=0)) / np.hypot(sens['mean_err'], se_b), 2).tolist()}; weighted_mean_err over "
          f"weighted_std / sqrt(n_eff): {np.round(se_w / (sens['weighted_std'][0] / math.sqrt(sens['n_eff'][0])), 2).tolist()}")
    assert np.all(np.abs(dev) < 5.0)
