"""The reference side of tests/test_gpu_math.py, without a GPU: the fixture tests/golden/golden_math.npz regenerates
identically, its double-double pairs are valid, the numpy restatements of exp_fast, the phi formulas and the affine scan
(tests/math_restated.py) meet the bounds the device is held to, and the probe library stays apart from the product's."""
import importlib.util
import json
import os
import subprocess

import numpy as np
import pytest

import math_restated as mr
from math_restated import EPS, err_rel, err_ulps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")
LARGEST_OTHER_FIXTURE = 356030          # golden_holdout.npz: no fixture may be larger


@pytest.fixture(scope="module")
def g():
    return np.load(mr.GOLDEN)


def _generator():
    spec = importlib.util.spec_from_file_location("make_math_golden", os.path.join(GOLDEN_DIR, "make_math_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("group", ["recip", "exp10", "phi", "scan", "lse", "merge"])
def test_fixture_regenerates(g, group):
    pytest.importorskip("mpmath")
    arrays = _generator().parts(group)
    assert arrays
    for key, want in arrays.items():
        assert mr.same_bits(g[key].ravel(), np.asarray(want, float).ravel()), key


def test_fixture_is_recorded_and_small():
    man = json.load(open(os.path.join(GOLDEN_DIR, "MANIFEST.json")))["golden_math.npz"]
    gen = _generator()
    assert man["generator"] == "tests/golden/make_math_golden.py" and man["seed"] == gen.SEED and man["mpmath"]
    assert os.path.getsize(mr.GOLDEN) <= LARGEST_OTHER_FIXTURE


def test_double_double_pairs_are_valid(g):
    """hi is the nearest double of hi + lo: |lo| <= ulp(hi) / 2."""
    keys = [k[:-3] for k in g.files if k.endswith("_hi")]
    assert len(keys) >= 11
    for k in keys:
        hi, lo = g[k + "_hi"], g[k + "_lo"]
        fin = np.isfinite(hi)
        assert np.all(np.isfinite(lo)) and np.all(lo[~fin] == 0.0)
        assert np.all(np.abs(lo[fin]) <= 0.5 * mr.ulp(hi[fin])), k
    for k in ("recip_x", "root_x"):
        assert np.all(g[k] >= 2.0 ** -1022) and np.all(np.isfinite(g[k]))
    assert g["root_x"].min() >= 2.0 ** -126 and g["root_x"].max() < 2.0 ** 127 and g["root_x"].max() > 1e34


def _dd_of(f, xs):
    """hi, lo of f(mpf(x)) for every x, by the fixture's own generator."""
    gen = _generator()
    mp = gen._mp()
    return gen.dd(mp, [f(mp, mp.mpf(float(v))) for v in xs])


def test_exp_restatement(g):
    from test_gpu_math import EXP_MAX_ULPS
    x, hi, lo = g["exp_x"], g["exp_hi"], g["exp_lo"]
    e = err_ulps(mr.exp_fast(x), hi, lo)
    sub = np.abs(hi) < 2.0 ** -1022
    assert sub.sum() >= 64 and np.all(e[sub] <= 1.0)
    assert np.all(e[~sub] <= EXP_MAX_ULPS)
    assert {-750.0, 700.0, 0.0} <= set(x.tolist())
    # the fixture holds k ln2 / 2 for every odd k inside the domain
    worst = mr.exp_worst_inputs()
    centres = np.arange(-2163, 2020, 2) * (np.log(2.0) / 2.0)
    centres = centres[(centres >= -750.0) & (centres <= 700.0)]
    assert centres.size >= 2090 and set(centres.tolist()) <= set(x.tolist()) and set(centres.tolist()) <= set(worst.tolist())
    # all of them with both neighbours, against mpmath: the constant is the measured maximum
    pytest.importorskip("mpmath")
    whi, wlo = _dd_of(lambda mp, v: mp.exp(v), worst)
    ew = err_ulps(mr.exp_fast(worst), whi, wlo)
    nrm = np.abs(whi) >= 2.0 ** -1022
    assert nrm.sum() >= 6000
    top = max(ew[nrm].max(), e[~sub].max())
    print(f"MATH-MAX exp_fast restated {top:.4f} ulp at x = {worst[nrm][np.argmax(ew[nrm])]!r}")
    assert np.all(ew[~nrm] <= 1.0)
    assert EXP_MAX_ULPS - 0.01 < top <= EXP_MAX_ULPS


def test_exp10_inputs_are_the_prior_boxes(g):
    """The generator's bounds are the product's: the un-logged coordinates (log mask 0b111100) of both prior boxes."""
    from magprop_amd import mcmc_eqns, synth
    gen = _generator()
    assert synth.LOG_MASK == 0b111100 and mcmc_eqns.LIB_LOG_MASK == 0b111100
    assert gen.SYNTH_LOWER == synth.PRIOR_LOWER[2:6].tolist() and gen.SYNTH_UPPER == synth.PRIOR_UPPER[2:6].tolist()
    assert gen.LIB_LOWER == mcmc_eqns.DEFAULT_LIMITS_LOWER[2:6].tolist()
    assert gen.LIB_UPPER == mcmc_eqns.DEFAULT_LIMITS_UPPER[2:6].tolist()
    x = g["exp10_x"]
    bounds = np.array(gen.SYNTH_LOWER + gen.SYNTH_UPPER + gen.LIB_LOWER + gen.LIB_UPPER)
    for b in bounds:
        assert {np.nextafter(b, -np.inf), b, np.nextafter(b, np.inf)} <= set(x.tolist())
    assert ((x >= bounds.min()) & (x <= bounds.max())).sum() >= 1000
    assert set(np.arange(-300.0, 301.0).tolist()) <= set(x.tolist())


def test_exp10_restatement(g):
    """The restatement of exp10_fast within the 2 ulp the device is held to: on the fixture, and against mpmath on 20 000
    uniform inputs over the span of the prior boxes and 5 000 over [-300, 300]."""
    x = g["exp10_x"]
    e = err_ulps(mr.exp10_fast(x), g["exp10_hi"], g["exp10_lo"])
    assert np.all(e <= 2.0), e.max()
    pytest.importorskip("mpmath")
    rng = np.random.default_rng(11)
    xs = np.concatenate([rng.uniform(-6.0, np.log10(2000.0), 20000), rng.uniform(-300.0, 300.0, 5000)])
    hi, lo = _dd_of(lambda mp, v: mp.power(10, v), xs)
    ed = err_ulps(mr.exp10_fast(xs), hi, lo)
    print(f"MATH-MAX exp10_fast restated {max(e.max(), ed.max()):.4f} ulp")
    assert np.all(ed <= 2.0), (ed.max(), xs[np.argmax(ed)])


@pytest.mark.parametrize("N", [1, 2, 4])
def test_phi_plain_formulas_within_the_table(g, N):
    """The plain-fp64 formulas on the fixture's inputs: within 1.5 x the table's figures (the constructed bounds where the
    table has none), every range present."""
    z, hi, lo = g["phi_z"], g["phi_hi"], g["phi_lo"]
    path = mr.wave_paths(z, N)
    plain = mr.phi_plain(z, path)
    E = mr.phi_errors(plain, z, path, hi, lo)
    assert not np.isnan(E).any()
    for r, rng in enumerate(mr.PHI_RANGES):
        for c in range(7):
            assert E[r, c] <= mr.phi_cap(rng, c), (rng, c, E[r, c])
    sub = np.abs(hi[:, 0]) < 2.0 ** -1022
    assert np.all(err_ulps(plain[sub, 0], hi[sub, 0], lo[sub, 0]) <= 1.0)
    for v in (0.0, 1e-300, 5e-324, 0.03125, -0.03125, 0.5, -0.5, -750.0, -1000.0):
        assert v in z
    for v in (0.03125, 0.5):
        for s in (1.0, -1.0):
            assert s * np.nextafter(v, 0) in z and s * np.nextafter(v, 1) in z


def test_scan_restatement(g):
    a, b = mr.scan_affine(g["scan_a"], g["scan_b"])
    assert np.all(err_rel(a.ravel(), g["scan_a_hi"], g["scan_a_lo"]) <= 128 * EPS)
    assert np.all(err_rel(b.ravel(), g["scan_b_hi"], g["scan_b_lo"]) <= 128 * EPS)
    # against the serial composition in fp64 on small integers, where every operation is exact
    rng = np.random.default_rng(0)
    ai, bi = rng.integers(-1, 2, (4, 64)).astype(float), rng.integers(-3, 4, (4, 64)).astype(float)
    A, B = mr.scan_affine(ai, bi)
    pa, pb = np.ones(4), np.zeros(4)
    for l in range(64):
        pb = ai[:, l] * pb + bi[:, l]
        pa = ai[:, l] * pa
        assert np.array_equal(A[:, l], pa) and np.array_equal(B[:, l], pb)


def test_wave_sum_and_extrema_restatements():
    v = np.arange(128.0).reshape(2, 64)
    assert np.array_equal(mr.wave_sum(v), np.repeat(v.sum(axis=1), 64).reshape(2, 64))
    x = np.array([[np.nan, -3.0, 2.0], [-0.0, 0.0, -0.0], [np.nan, np.nan, np.nan]])
    assert mr.same_bits(mr.lane_ext(2, x), np.array([2.0, 0.0, np.nan]))
    assert mr.same_bits(mr.lane_ext(3, x), np.array([-3.0, -0.0, np.nan]))
    assert mr.same_bits(mr.lane_ext(0, x), np.array([3.0, 0.0, np.nan]))
    assert mr.same_bits(mr.lane_ext(1, x), np.array([2.0, 0.0, np.nan]))


def test_quadrature_table_restatement():
    """Rows of W sum to the moments of the Lagrange basis: sum_k W[k][m] x_k^j = m! [j == m] for j, m < 5."""
    for lnq in (mr.LNQ_GRID, mr.LNQ_GRID_S):
        T = mr.wtab(lnq)
        assert T.size == mr.WTAB_SIZE
        for kind in range(mr.KINDS):
            Q = np.exp(lnq / 8.0 if kind == 0 else lnq * (1 << (kind - 1)))
            x = np.array([1.0, 0.0, -1 / Q, -1 / Q - 1 / Q ** 2, -1 / Q - 1 / Q ** 2 - 1 / Q ** 3], dtype=np.longdouble)
            W = T[kind * 40: kind * 40 + 30].reshape(5, 6)[:, :5].astype(np.longdouble)
            fact = np.array([1.0, 1.0, 2.0, 6.0, 24.0])
            for j in range(5):
                mom = (W * (x ** j)[:, None]).sum(axis=0)
                want = np.where(np.arange(5) == j, fact, 0.0)
                assert np.all(np.abs(mom - want) <= 1e-9 * np.abs(W).max()), (kind, j)


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_probe_library_is_separate():
    """After a build libmp_probe.so exports the mpp_* functions and libmagprop_amd.so none of them; the ABI's binding and
    header do not name them."""
    from magprop_amd import _capi
    pkg = os.path.dirname(os.path.abspath(_capi.__file__))
    probe = _exports(os.path.join(pkg, "libmp_probe.so"))
    assert set(mr.PROBE_EXPORTS) <= probe
    assert {s for s in probe if s.startswith("mpp_")} == set(mr.PROBE_EXPORTS)
    assert not {s for s in probe if s.startswith("mp_")}
    product = _exports(os.path.join(pkg, "libmagprop_amd.so"))
    assert not {s for s in product if s.startswith("mpp_")}
    assert not [n for n in _capi.EXPORTS if n.startswith("mpp_")]
    assert "mpp_" not in open(os.path.join(ROOT, "include", "magprop_amd.h")).read()
