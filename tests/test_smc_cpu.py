"""CPU tests of the tempered SMC sampler (include/magprop_amd.h mp_smc_*, magprop_amd.smc): the resampling rule and the bisection
of the numpy restatement (tests/smc_restated.py, which the GPU tests hold the device to bit for bit), the whole scheme against
the closed-form evidence and posterior of the unit Gaussian in a box, and the argument checks of SMCSampler and of the C entry
points on a machine without a device."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import smc_restated as sm
from conftest import ROOT

U31 = 1 << 31


# ---------------------------------------------------------------- the resampling rule
@pytest.mark.parametrize("n", [4, 63, 257])
def test_equal_weights_give_the_identity_genealogy(n):
    """Every unit 2^31: whatever the offset s < U, slot j continues particle j."""
    units = [U31] * n
    total = n * U31
    for s in (0, 1, U31 - 1, U31, total // 2, total - 1):
        anc, pos = sm.resample(units, s)
        assert np.array_equal(anc, np.arange(n)), s
        assert max(pos) < total
    out = sm.stage(np.full(n, -3.25), 0.0, 0.0, 0.5, 7, 0, 0)
    assert out["beta"] == 1.0 and np.all(out["units"] == U31) and np.array_equal(out["anc"], np.arange(n))


def test_one_dominant_particle_is_every_ancestor():
    """The others' weights round to zero units: every slot continues the dominant particle."""
    lnl = np.full(65, -1.0e300)                                        # (no increment the bisection reaches bridges this range)
    lnl[41] = 0.0
    out = sm.stage(lnl, 0.0, 0.0, 0.5, 11, 3, 2)
    assert out["units"][41] == U31 and out["units"].sum() == U31
    assert np.array_equal(sm.units_of(np.array([1.0, 0.2e-9, 0.3e-9, 0.5]), 1.0), [U31, 0, 1, U31 // 2])   # rint of 0.43, 0.64
    assert np.all(out["anc"] == 41)
    anc, _ = sm.resample([0, 0, 5, 0], 4)
    assert np.all(anc == 2)


def test_failed_particles_are_never_ancestors():
    rng = np.random.default_rng(5)
    lnl = -10.0 * rng.random(255)
    dead = np.r_[0, 1, 2, 100, 253, 254]
    lnl[dead] = -np.inf
    for t in range(8):
        out = sm.stage(lnl, 0.0, 0.0, 0.5, 20261020, t, 1)
        assert np.all(out["units"][dead] == 0) and not np.any(np.isin(out["anc"], dead))
        assert np.all(np.diff(out["anc"]) >= 0)                        # systematic resampling keeps the order


def test_positions_stay_below_the_total_and_offspring_follow_the_units():
    """P_j < U for every offset; the offspring count of particle i differs from N u_i / U by less than 1; over every offset
    s = 0 .. U-1 its mean is N u_i / U exactly."""
    rng = np.random.default_rng(9)
    n = 37
    units = [int(v) for v in rng.integers(0, 9, n)]
    units[5] = 0
    total = sum(units)
    tot = np.zeros(n, dtype=np.int64)
    for s in range(total):
        anc, pos = sm.resample(units, s)
        assert 0 <= min(pos) and max(pos) < total
        cnt = np.bincount(anc, minlength=n)
        assert np.all(np.abs(cnt - n * np.array(units) / total) < 1.0)
        tot += cnt
    assert np.array_equal(tot, n * np.array(units))                     # mean over s: N u_i / U
    # at the kernel's scale: units up to 2^31, N = 16 384 (j U < 2^59)
    n = 16384
    units = [int(v) for v in np.rint(U31 * rng.random(n) ** 8)]
    total = sum(units)
    for s in (0, total - 1, total // 3):
        anc, pos = sm.resample(units, s)
        assert max(pos) < total and (n - 1) * total + s < 1 << 59
        assert np.all(np.abs(np.bincount(anc, minlength=n) - n * np.array(units, dtype=np.float64) / total) < 1.0 + 1e-9)


def test_the_offset_is_one_rounded_product_below_the_total():
    for total in (1, 5, U31, 16384 * U31, 12345678901234):
        for t in range(4):
            s = sm.offset(99, t, 3, total)
            k = sm.draws(99, t, 3, [0], 0)
            assert 0 <= s < total and s == int(float(sm.u01(k[0], k[1])[0]) * float(total))


# ---------------------------------------------------------------- the bisection
def test_beta_lands_on_exactly_one_when_the_last_increment_keeps_the_ess():
    rng = np.random.default_rng(3)
    lnl = -0.1 * rng.random(256)
    for beta in (0.0, 0.7, 1.0 - 2.0 ** -53):
        d, last, big, n_fin = sm.next_increment(lnl, beta, 0.5)
        assert last and d == 1.0 - beta and n_fin == 256 and big == lnl.max()
        assert sm.stage(lnl, beta, 0.0, 0.5, 1, 0, 0)["beta"] == 1.0
    # ... and does not where it would not
    d, last, _, _ = sm.next_increment(-50.0 * rng.random(256), 0.0, 0.5)
    assert not last and 0.0 < d < 1.0


@pytest.mark.parametrize("scale", [30.0, 1.0e9])
def test_the_increment_brackets_the_target(scale):
    """ESS(d) >= target > ESS(the next double above d): lo and hi ended as neighbours."""
    rng = np.random.default_rng(4)
    lnl = -scale * rng.random(1025)
    lnl[[0, 1024]] = -np.inf
    d, last, big, n_fin = sm.next_increment(lnl, 0.25, 0.5)
    assert not last and n_fin == 1023
    target = 0.5 * n_fin
    assert sm.ess_of(*sm.sums(lnl, big, d)[:2]) >= target > sm.ess_of(*sm.sums(lnl, big, np.nextafter(d, 1.0))[:2])
    if scale == 1.0e9:
        assert 1e-10 < d < 1e-8


def test_the_rule_for_a_lower_end_that_stays_zero():
    """A range no increment above 2^-128 (1 - beta) can bridge: lo stays 0 and d is hi, the last midpoint tried."""
    lnl = np.array([0.0, -1.0e300, -1.0e300, -1.0e300])
    d, last, big, n_fin = sm.next_increment(lnl, 0.0, 0.5)
    assert not last and d == 2.0 ** -128 and sm.ess_of(*sm.sums(lnl, big, d)[:2]) == 1.0 < 0.5 * n_fin
    out = sm.stage(lnl, 0.0, 0.0, 0.5, 1, 0, 0)
    assert np.all(out["anc"] == 0) and out["beta"] == d


def test_no_finite_particle_fails_the_run():
    assert sm.next_increment(np.full(16, -np.inf), 0.0, 0.5) is None
    x0 = np.zeros((2, 16, 2))
    s = sm.start(x0, lambda rows, runs: (np.where(runs == 0, -np.inf, 0.0), np.where(runs == 0, 1, 0)))
    sm.run(s, 5, 1, 3, 0.5, 0.0, 0.1, [-1.0, -1.0], [1.0, 1.0], sm.gaussian)
    assert s.run_status.tolist() == [sm.FAILED, sm.DONE] and s.nstage.tolist() == [0, 1] and s.nfail.tolist() == [16, 0]
    assert np.array_equal(s.x[0], x0[0]) and s.log[0] == []


def test_wg_sum_is_a_sum():
    rng = np.random.default_rng(8)
    for n in (1, 4, 255, 256, 257, 1025, 16384):
        v = rng.random(n)
        assert abs(sm.wg_sum(v) - math.fsum(v)) <= 4.0 * n * 2.0 ** -52 * math.fsum(v)
    assert sm.wg_sum(np.arange(1.0, 301.0)) == 45150.0


# ---------------------------------------------------------------- the whole scheme against a closed form
SEED, NDIM, HALF, NRUNS, NPART, WALKS = 1, 6, 10.0, 8, 1024, 10


def scheme(walks=WALKS, norm_term=True):
    """8 runs of N = 1 024 on the unit Gaussian in [-10, 10]^6: (z of the mean ln Z against the closed form, in standard errors;
    the pooled sample variance per coordinate; the state)."""
    lo, hi = np.full(NDIM, -HALF), np.full(NDIM, HALF)
    x0 = lo + (hi - lo) * np.random.default_rng(SEED).random((NRUNS, NPART, NDIM))
    s = sm.start(x0, sm.gaussian)
    sm.run(s, 1000, SEED, walks, 0.5, 0.0, 0.1, lo, hi, sm.gaussian, norm_term=norm_term)
    se = np.std(s.lnz, ddof=1) / math.sqrt(NRUNS)
    return (np.mean(s.lnz) - sm.box_lnz(HALF, NDIM)) / se, np.var(s.x.reshape(-1, NDIM), axis=0), s


def passes(z, var):
    """The check of the evidence and the posterior: within 4 standard errors, every variance within 5 % of 1."""
    return bool(abs(z) < 4.0 and np.all(np.abs(var - 1.0) < 0.05))


def test_the_scheme_gives_the_evidence_and_the_posterior_of_the_box_gaussian():
    z, var, s = scheme()
    print(f"z = {z:.2f} standard errors, variances {np.round(var, 3).tolist()}, stages {s.nstage.tolist()}, ln Z {s.lnz.tolist()}")
    assert np.all(s.run_status == sm.DONE) and np.all(s.beta == 1.0)
    assert abs(z) < 3.0                       # (the seed's own margin; the check is 4)
    assert passes(z, var)
    for r in range(NRUNS):                    # the log: beta rises to 1, ESS(d) sits at the target until the last stage
        beta, d, ess, lnz, accept, ncall = sm.stages_of(s, r, NPART, WALKS)
        assert np.all(np.diff(beta) > 0.0) and beta[-1] == 1.0 and np.allclose(np.cumsum(d)[:-1], beta[:-1], rtol=1e-12)
        assert np.all(ess[:-1] >= 0.5 * NPART) and np.all(ess[:-1] < 0.5 * NPART + 1.0) and ess[-1] >= 0.5 * NPART
        assert lnz[-1] == s.lnz[r] and np.all((accept > 0.05) & (accept < 0.9)) and ncall.sum() + NPART == s.ncall[r]


def test_the_check_fails_without_the_normalising_term_and_without_moves():
    """The same check on two broken schemes: ln Z without ln(sum w / N), and resampling with no moves behind it."""
    z, var, _ = scheme(norm_term=False)
    print(f"without ln(sum w / N): z = {z:.1f}")
    assert not passes(z, var) and abs(z) > 4.0 and np.all(np.abs(var - 1.0) < 0.05)
    z, var, s = scheme(walks=0)
    print(f"without moves: z = {z:.1f}, variances {np.round(var, 3).tolist()}")
    assert not passes(z, var) and np.any(np.abs(var - 1.0) > 0.05)
    assert len(np.unique(s.x[0], axis=0)) < NPART // 4        # copies of a few prior draws


# ---------------------------------------------------------------- argument checks
def _kw(**kw):
    return kw


@pytest.mark.parametrize("kw, match", [
    (_kw(nparticles=3), "nparticles"),
    (_kw(nparticles=16385), "nparticles"),
    (_kw(nparticles=100.5), "nparticles"),
    (_kw(walks=0), "walks"),
    (_kw(walks=5000), "walks"),
    (_kw(ess=0.0), "ess"),
    (_kw(ess=1.0), "ess"),
    (_kw(ess=float("nan")), "ess"),
    (_kw(sigma=0.6), "sigma"),
    (_kw(g0=np.inf), "g0"),
    (_kw(n_runs=0), "n_runs"),
    (_kw(n_runs=65), "at most"),
    (_kw(variant="other"), "variant"),
    (_kw(ndim=7), "6 parameters"),
    (_kw(variant="lib", ndim=10), "6 to 9"),
    (_kw(bounds=[(1.0, 0.0)] * 6), "lower < upper"),
    (_kw(bounds=[(0.0, 1.0)] * 5), "pairs"),
    (_kw(target="other"), "target"),
    (_kw(target=3), "target"),
    (_kw(target=1), "bounds"),
])
def test_argument_checks_raise_before_any_device_is_touched(monkeypatch, kw, match):
    from magprop_amd import _capi, smc

    def no_device(*a, **k):
        raise AssertionError("the device was touched")

    for name in ("lib", "Handle", "cfg_synth", "cfg_lib"):
        monkeypatch.setattr(_capi, name, no_device)
    x = np.linspace(1.0, 10.0, 5)
    with pytest.raises(ValueError, match=match):
        smc.SMCSampler(x, x, x, **kw)


def test_run_arguments_are_checked_before_any_device_is_touched(monkeypatch):
    from magprop_amd import _capi, smc

    def no_device(*a, **k):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(_capi, "lib", no_device)
    monkeypatch.setattr(_capi, "Handle", no_device)
    x = np.linspace(1.0, 10.0, 5)
    s = smc.SMCSampler(x, x, x, nparticles=64, n_runs=3)
    assert s.n_runs == 3 and s.initial_particles().shape == (3, 64, 6)
    assert np.all((s.initial_particles() >= s.lower) & (s.initial_particles() <= s.upper))
    for bad in (dict(max_stages=-1), dict(max_stages=2.5)):
        with pytest.raises(ValueError):
            s.run(**bad)
    with pytest.raises(ValueError, match="run first"):
        s.get_derived()
    with pytest.raises(ValueError, match="dataset"):
        smc.SMCSampler()
    g = smc.SMCSampler(target="gaussian", bounds=[(-1.0, 1.0)] * 3)
    assert g.target == 1 and g.ndim == 3 and g.datasets == []


def test_c_entry_points_refuse_bad_arguments_without_a_device():
    """NULL objects are MP_EINVAL everywhere; without a device the front end fails with the library's MP_ENODEV message."""
    import torch

    from magprop_amd import _capi, smc
    L = _capi.lib()
    lo, hi = np.zeros(2), np.ones(2)
    assert not L.mp_smc_create(None, 64, 1, 2, None, 1, _capi.ptr(lo), _capi.ptr(hi), 0.5, 3, 0.0, 0.1, 1)
    assert "NULL" in _capi.last_error()
    assert L.mp_smc_set_particles(None, _capi.ptr(lo)) == _capi.MP_EINVAL
    assert L.mp_smc_run(None, 1, None) == _capi.MP_EINVAL
    assert L.mp_smc_get_state(None, *([None] * 11)) == _capi.MP_EINVAL
    assert L.mp_smc_get_stages(None, 0, 0, *([None] * 7)) == _capi.MP_EINVAL
    assert L.mp_smc_get_ancestors(None, None) == _capi.MP_EINVAL
    assert L.mp_smc_destroy(None) == _capi.MP_OK
    if not torch.cuda.is_available():
        with pytest.raises(_capi.MagpropAmdError, match="no HIP device"):
            smc.SMCSampler(target=1, bounds=[(-1.0, 1.0)] * 2, nparticles=16).run()
        assert L.mp_create(C.byref(_capi.ModelCfg()), None, 0, 0) is None


def test_header_states_the_limits_and_the_library_exports_the_entry_points():
    from magprop_amd import _capi
    hdr = open(os.path.join(ROOT, "include", "magprop_amd.h")).read()
    for name, val in (("MP_SMC_MIN_PARTICLES", _capi.SMC_MIN_PARTICLES), ("MP_SMC_MAX_PARTICLES", _capi.SMC_MAX_PARTICLES),
                      ("MP_SMC_MAX_WALKS", _capi.SMC_MAX_WALKS), ("MP_SMC_MAX_STAGES", _capi.SMC_MAX_STAGES),
                      ("MP_SMC_RUNNING", _capi.SMC_RUNNING), ("MP_SMC_DONE", _capi.SMC_DONE), ("MP_SMC_FAILED", _capi.SMC_FAILED),
                      ("MP_SMC_STAGE_LIMIT", _capi.SMC_STAGE_LIMIT)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, hdr).group(1)) == val
    assert (sm.RUNNING, sm.DONE, sm.FAILED, sm.STAGE_LIMIT, sm.MAX_STAGES) == (0, 1, 2, 3, _capi.SMC_MAX_STAGES)
    assert "0x534D0000" in hdr and sm.CTR == 0x534D0000
    for name in ("mp_smc_create", "mp_smc_set_particles", "mp_smc_run", "mp_smc_get_state", "mp_smc_get_stages",
                 "mp_smc_get_ancestors", "mp_smc_destroy"):
        assert name in _capi.EXPORTS and hasattr(_capi.lib(), name)
    import magprop_amd
    assert magprop_amd.SMCSampler is magprop_amd.smc.SMCSampler
