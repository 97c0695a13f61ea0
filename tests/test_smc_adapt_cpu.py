"""CPU tests of the adaptive moves of the tempered SMC sampler (include/magprop_amd.h mp_smc_set_adaptive): the restatement
(tests/smc_adapt_restated.py, which the GPU tests hold the device to bit for bit) against the fixed-length restatement, its tune
rule on the crafted cases (tests/smc_adapt_cases.py) against a long-double correlation, the whole adaptive scheme against the
closed-form evidence of the unit Gaussian in a box, and the argument checks on a machine without a device."""
import math

import numpy as np
import pytest

import smc_adapt_cases as cases
import smc_adapt_restated as ad
import smc_restated as sm
from test_smc_cpu import HALF, NDIM, NPART, NRUNS, SEED, passes

U = 2.0 ** -53


def test_fixed_rounds_without_gain_equal_the_fixed_length_run_bit_for_bit():
    """min_rounds = max_rounds = R, gain = 0: the adaptive run of rounds of `walks` steps is smc_restated.run with walks * R
    steps: particles, lnl, status, accepted counts, ln Z, betas, the log, the counters and the ancestors, at every stage."""
    n_runs, n, ndim, walks, R, seed = 2, 64, 3, 2, 3, 20261020
    lo, hi = np.full(ndim, -4.0), np.linspace(3.0, 5.0, ndim)
    x0 = lo + (hi - lo) * np.random.default_rng(11).random((n_runs, n, ndim))
    fixed = sm.start(x0, sm.gaussian)
    s = ad.begin(sm.start(x0, sm.gaussian), 0.0, 0.1)
    cfg = ad.Adapt(s.g[0], min_rounds=R, max_rounds=R, corr=0.0, gain=0.0)
    for _ in range(40):
        sm.run(fixed, 1, seed, walks * R, 0.5, 0.0, 0.1, lo, hi, sm.gaussian)
        ad.run(s, 1, seed, walks, 0.5, 0.0, 0.1, lo, hi, sm.gaussian, cfg)
        for k in ("x", "lnl", "status", "acc", "anc", "beta", "lnz", "nstage", "run_status", "ncall", "nacc", "nfail"):
            assert np.array_equal(getattr(s, k), getattr(fixed, k)), k
        assert s.log == fixed.log
        if not np.any(fixed.run_status == sm.RUNNING):
            break
    assert np.all(s.run_status == sm.DONE) and np.all(s.nstage > 2) and np.all(s.nacc > 0)
    for r in range(n_runs):
        rounds, g, rho = ad.tuning_of(s, r)
        assert np.all(rounds == R) and np.all(g == s.g[0]) and len(rounds) == s.nstage[r] and np.all(np.abs(rho) <= 1.0)
        for got, want in zip(ad.stages_of(s, r, n, walks), sm.stages_of(fixed, r, n, walks * R)):
            assert np.array_equal(got, want)


def long_double_rho(a, b):
    """The Pearson correlation of two columns in long double, as it is defined."""
    a, b = a.astype(np.longdouble), b.astype(np.longdouble)
    da, db = a - np.sum(a) / a.size, b - np.sum(b) / b.size
    return np.sum(da * db) / (np.sqrt(np.sum(da * da)) * np.sqrt(np.sum(db * db)))


def rho_bound(n, ka, kb):
    """|rho_d - the exact correlation| for N slots, first order in u = 2^-53.  A centred value carries one rounding of its
    subtraction (the scaling by a power of two is exact), a product of two a third, and a sum of N terms in any order at most
    (N - 1) u of the sum of their sizes, which Cauchy-Schwarz bounds by sqrt(Saa Sbb): |dSab| <= (N + 2) u sqrt(Saa Sbb), and the
    same relative bound for Saa and Sbb.  Each of the two enters the denominator under a square root, so the denominator carries
    (N + 2) u, its product, root and the quotient 3 u more: (2 N + 7) u with |rho| <= 1.  The error e of a mean (|e| <= N u mean|x|)
    shifts every centred value alike and so enters Sab only as N e_a e_b, that is k_a k_b (N u)^2 of sqrt(Saa Sbb) with k =
    mean|x| / sd of the column, taken from the case itself.  The long-double reference's own error, 2 N 2^-64, is 16 u at the
    largest N."""
    return (2 * n + 7 + 16 + 9) * U + ka * kb * (n * U) ** 2


@pytest.mark.parametrize("ndim", cases.NDIMS)
@pytest.mark.parametrize("n", cases.SIZES)
def test_the_tune_rule_on_the_crafted_cases(n, ndim):
    """rho_d against its exact value where the case has one, and against the long-double definition within rho_bound(N)
    elsewhere; the largest is rho; the decision and the scale update follow the rule."""
    rng = np.random.default_rng(7000 + n + ndim)
    cfg = ad.Adapt(cases.G0, min_rounds=1, max_rounds=4, corr=0.3, gain=1.0)
    for made in (1, 4):
        for name, start, now, acc, g in cases.runs(n, ndim, made, rng, cfg.g_min, cfg.g_max):
            rho_d, rho, go_on, g_next = ad.tune(start, now, acc, cases.WALKS, made, g, cfg)
            exact = cases.exact_rho(name, ndim)
            if exact is not None:
                assert np.array_equal(rho_d, exact), (name, rho_d)
            else:
                for d in range(ndim):
                    if name == "constant dimension" and d == 1:
                        assert rho_d[d] == 1.0
                        continue
                    ka, kb = (float(np.mean(np.abs(col)) / np.std(col)) for col in (start[:, d].astype(np.longdouble),
                                                                                    now[:, d].astype(np.longdouble)))
                    assert ka < 100.0 and kb < 100.0, name   # (the means' term stays far below the first)
                    assert abs(rho_d[d] - float(long_double_rho(start[:, d], now[:, d]))) <= rho_bound(n, ka, kb), (name, d)
            assert rho == np.max(rho_d) and go_on == (made < cfg.max_rounds and not rho <= cfg.corr), name
            share = float(np.sum(acc)) / (float(n) * float(made * cases.WALKS))   # every product rounded on its own
            want = g if go_on else min(max(g * np.exp(cfg.gain * (share - cfg.accept_target)), cfg.g_min), cfg.g_max)
            assert g_next == want, name
            if not go_on:                                      # the cases the update is there for
                if name == "accept 0":
                    assert g_next == g * np.exp(-cfg.accept_target) < g
                if name == "accept 1":
                    assert g_next == g * np.exp(1.0 - cfg.accept_target) > g
                if name.startswith("g at"):
                    assert g_next == g and g in (cfg.g_min, cfg.g_max)
            if name in ("tiny", "huge"):                       # neither squares that underflow nor products that overflow
                assert np.all(np.isfinite(rho_d)) and np.all(np.abs(rho_d) <= 1.0)
                assert n < 255 or ((0.4 < rho < 0.8) if name == "tiny" else (rho < 0.4)), (name, rho)


def test_rho_one_ulp_on_either_side_of_corr_and_the_round_limits():
    rng = np.random.default_rng(5)
    name, start, now, acc, g = cases.runs(257, 6, 2, rng, 0.1, 2.0)[5]
    assert name == "mixed"
    base = ad.Adapt(cases.G0, min_rounds=1, max_rounds=4, corr=0.3)
    rho = ad.tune(start, now, acc, cases.WALKS, 2, g, base)[1]
    assert 0.3 < rho < 1.0
    at = ad.Adapt(cases.G0, min_rounds=1, max_rounds=4, corr=rho)
    below = ad.Adapt(cases.G0, min_rounds=1, max_rounds=4, corr=float(np.nextafter(rho, -1.0)))
    above = ad.Adapt(cases.G0, min_rounds=1, max_rounds=4, corr=float(np.nextafter(rho, 2.0)))
    assert not ad.tune(start, now, acc, cases.WALKS, 2, g, at)[2]          # rho <= corr: stop
    assert not ad.tune(start, now, acc, cases.WALKS, 2, g, above)[2]
    assert ad.tune(start, now, acc, cases.WALKS, 2, g, below)[2]           # one ulp above corr: another round ...
    assert not ad.tune(start, now, acc, cases.WALKS, 4, g, below)[2]       # ... up to max_rounds
    held = ad.Adapt(cases.G0, min_rounds=3, max_rounds=4, corr=rho)
    assert ad.tune(start, now, acc, cases.WALKS, 2, g, held)[2] and not ad.tune(start, now, acc, cases.WALKS, 3, g, held)[2]
    nan = now.copy()
    nan[3, 2] = np.nan                                                      # a NaN rho goes on, up to the cap
    with np.errstate(invalid="ignore"):
        out = ad.tune(start, nan, acc, cases.WALKS, 2, g, at), ad.tune(start, nan, acc, cases.WALKS, 4, g, at)
    assert math.isnan(out[0][1]) and out[0][2] and not out[1][2]
    still = ad.Adapt(cases.G0, gain=0.0)                                    # gain = 0 leaves g exactly
    assert ad.tune(start, now, acc, cases.WALKS, 16, 0.123456789, still)[3] == 0.123456789


ADAPT, ROUND = dict(min_rounds=1, max_rounds=80, corr=0.5, gain=1.0, accept_target=0.234), 2


def test_the_adaptive_scheme_gives_the_evidence_of_the_box_gaussian():
    """The closed-form case of tests/test_smc_cpu.py (8 runs, N = 1 024, d = 6, [-10, 10]^6, the same seed and particles) with
    the shipped adaptation settings: the mean ln Z within 4 standard errors of box_lnz, the variances within 5 % of 1."""
    from magprop_amd import smc
    assert {k: smc.ADAPT_DEFAULTS[k] for k in ADAPT} == ADAPT and smc.WALKS_ADAPTIVE == ROUND
    lo, hi = np.full(NDIM, -HALF), np.full(NDIM, HALF)
    x0 = lo + (hi - lo) * np.random.default_rng(SEED).random((NRUNS, NPART, NDIM))
    s = ad.begin(sm.start(x0, sm.gaussian), 0.0, 0.1)
    ad.run(s, 1000, SEED, ROUND, 0.5, 0.0, 0.1, lo, hi, sm.gaussian, ad.Adapt(s.g[0], **ADAPT))
    se = np.std(s.lnz, ddof=1) / math.sqrt(NRUNS)
    z = (np.mean(s.lnz) - sm.box_lnz(HALF, NDIM)) / se
    var = np.var(s.x.reshape(-1, NDIM), axis=0)
    rounds = [ad.tuning_of(s, r)[0].tolist() for r in range(NRUNS)]
    print(f"z = {z:.2f} standard errors (se {se:.4f}), variances {np.round(var, 3).tolist()}, rounds of run 0 {rounds[0]}, "
          f"g of run 0 {np.round(ad.tuning_of(s, 0)[1], 3).tolist()}")
    assert np.all(s.run_status == sm.DONE) and np.all(s.beta == 1.0)
    assert passes(z, var)
    assert all(len(rounds[r]) == s.nstage[r] for r in range(NRUNS))
    assert all(1 <= k < ADAPT["max_rounds"] for row in rounds for k in row)      # the rule stopped every stage, not the cap
    for r in range(NRUNS):
        accept = ad.stages_of(s, r, NPART, ROUND)[4]
        assert np.all((accept > 0.02) & (accept < 0.9))


def _kw(**kw):
    return kw


@pytest.mark.parametrize("kw, match", [
    (_kw(adapt="yes"), "adapt must be"),
    (_kw(adapt=dict(rounds=3)), "adapt must be"),
    (_kw(adapt=dict(min_rounds=0)), "min_rounds"),
    (_kw(adapt=dict(min_rounds=5, max_rounds=4)), "min_rounds"),
    (_kw(adapt=dict(max_rounds=2.5)), "integer"),
    (_kw(adapt=dict(max_rounds=2049)), "walks \\* max_rounds"),
    (_kw(adapt=True, walks=52), "walks \\* max_rounds"),
    (_kw(adapt=dict(corr=1.0)), "corr"),
    (_kw(adapt=dict(corr=-0.1)), "corr"),
    (_kw(adapt=dict(gain=-1.0)), "gain"),
    (_kw(adapt=dict(gain=float("inf"))), "gain"),
    (_kw(adapt=dict(accept_target=0.0)), "accept_target"),
    (_kw(adapt=dict(accept_target=1.0)), "accept_target"),
    (_kw(adapt=dict(g_min=2.0)), "g_min"),
    (_kw(adapt=dict(g_max=0.1)), "g_min"),
    (_kw(adapt=dict(g_max=float("inf"))), "g_min"),
])
def test_adapt_arguments_raise_before_any_device_is_touched(monkeypatch, kw, match):
    from magprop_amd import _capi, smc

    def no_device(*a, **k):
        raise AssertionError("the device was touched")

    for name in ("lib", "Handle", "cfg_synth", "cfg_lib"):
        monkeypatch.setattr(_capi, name, no_device)
    x = np.linspace(1.0, 10.0, 5)
    with pytest.raises(ValueError, match=match):
        smc.SMCSampler(x, x, x, **kw)


def test_adapt_settings_are_resolved_without_a_device(monkeypatch):
    from magprop_amd import _capi, smc
    monkeypatch.setattr(_capi, "lib", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the device was touched")))
    x = np.linspace(1.0, 10.0, 5)
    assert smc.SMCSampler(x, x, x).adapt is None and smc.SMCSampler(x, x, x, adapt=False).adapt is None
    assert smc.SMCSampler(x, x, x, adapt=True).adapt == smc.ADAPT_DEFAULTS
    assert smc.SMCSampler(x, x, x).walks == 10 and smc.SMCSampler(x, x, x, adapt=True).walks == smc.WALKS_ADAPTIVE == 2
    assert smc.SMCSampler(x, x, x, adapt=True, walks=5).walks == 5
    got = smc.SMCSampler(x, x, x, walks=2, adapt=dict(max_rounds=8, corr=0.1, g_min=0.2)).adapt
    assert got == {**smc.ADAPT_DEFAULTS, "max_rounds": 8, "corr": 0.1, "g_min": 0.2} and list(got) == list(smc.ADAPT_DEFAULTS)


def test_c_entry_points_refuse_a_null_sampler_and_are_exported():
    from magprop_amd import _capi
    L = _capi.lib()
    assert L.mp_smc_set_adaptive(None, 1, 4, 0.3, 1.0, 0.234, 0.0, 0.0) == _capi.MP_EINVAL and "NULL" in _capi.last_error()
    assert L.mp_smc_get_tuning(None, 0, 0, None, None, None, None) == _capi.MP_EINVAL
    assert "mp_smc_set_adaptive" in _capi.EXPORTS and "mp_smc_get_tuning" in _capi.EXPORTS and L.mp_abi_version() == 5
