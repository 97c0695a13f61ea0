"""CPU checks of the derived quantities (mp_model_derived): the host helpers of magprop_amd/derived.py, the column names against
the header's indices, the entry point's argument checks without a device, and the reference fixture's shape."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, LC_REF_RTOL, ROOT
from magprop_amd import _capi, derived

import derive_restated as dr


def _table(rng, n=200):
    v = rng.standard_normal((n, 16)) * np.arange(1, 17)
    v[::9] = np.nan                                            # rows that did not finish
    return v


def test_names_follow_the_header_indices():
    hdr = open(os.path.join(ROOT, "include", "magprop_amd.h")).read()
    defs = dict((k, int(v)) for k, v in re.findall(r"#define\s+MP_DERIVED_([A-Z0-9_]+)\s+([0-9]+)\b", hdr))
    assert defs.pop("N") == len(derived.NAMES) == _capi.DERIVED_N == dr.N == 16
    assert sorted(defs.values()) == list(range(16))
    assert [k.lower() for k, _ in sorted(defs.items(), key=lambda kv: kv[1])] == [n.lower() for n in derived.NAMES]
    # the restatement's indices are the header's
    for k, v in defs.items():
        assert getattr(dr, k) == v, k
    d = derived.as_dict(np.arange(32.0).reshape(2, 16))
    assert list(d) == list(derived.NAMES) and np.array_equal(d["t_peak"], [4.0, 20.0])
    assert derived.as_dict(np.arange(16.0))["Mdisc_max"] == 14.0
    with pytest.raises(ValueError, match="16 columns"):
        derived.as_dict(np.zeros((3, 15)))


def test_summarize_without_weights_is_nanquantile():
    rng = np.random.default_rng(1)
    v = _table(rng)
    q = (0.16, 0.5, 0.84)
    s = derived.summarize(v, q)
    ok = ~np.isnan(v).any(axis=1)
    assert s["n_used"] == int(ok.sum()) and np.array_equal(s["q"], q)
    want = np.nanquantile(v, q, axis=0)
    for k, name in enumerate(derived.NAMES):
        assert np.array_equal(s[name], want[:, k]), name
    none = derived.summarize(np.full((5, 16), np.nan))
    assert none["n_used"] == 0 and all(np.all(np.isnan(none[n])) for n in derived.NAMES)
    for bad in ((), (1.5,), (np.nan,)):
        with pytest.raises(ValueError, match="quantile"):
            derived.summarize(v, bad)
    with pytest.raises(ValueError, match="2-D"):
        derived.summarize(np.zeros(16))


def _cdf_loop(x, w, q):
    """the least x of positive weight whose cumulative weight in sorted order reaches q of the total: a plain loop, the weights
    added one by one in sorted order"""
    order = [i for i in sorted(range(len(x)), key=lambda i: x[i]) if w[i] > 0.0]
    total = 0.0
    for i in order:
        total = total + float(w[i])
    acc = 0.0
    for i in order:
        acc = acc + float(w[i])
        if acc >= q * total:
            return x[i]
    return x[order[-1]]


def test_summarize_with_weights_is_the_sorted_cdf():
    rng = np.random.default_rng(2)
    v = _table(rng)
    w = rng.random(v.shape[0]) ** 4                           # a few heavy rows, as nested-sampling weights are
    w[5] = 0.0
    for k in range(16):                                        # a row of weight 0 below every other value of a column: never an answer
        v[5, k] = np.nanmin(v[:, k]) - 1.0
    q = (0.0, 0.025, 0.16, 0.5, 0.84, 0.975, 1.0)
    s = derived.summarize(v, q, weights=w)
    ok = ~np.isnan(v).any(axis=1)
    assert s["n_used"] == int(ok.sum())
    for k, name in enumerate(derived.NAMES):
        for j, qq in enumerate(q):
            assert s[name][j] == _cdf_loop(v[ok, k], w[ok], qq), (name, qq)
        assert s[name][0] > v[5, k], name                      # q = 0: the least value that carries weight
    # equal weights: every quantile lies in the bracket of order statistics np.nanquantile interpolates between
    e = derived.summarize(v, (0.16, 0.5, 0.84), weights=np.ones(v.shape[0]))
    lo = np.nanquantile(v[ok], (0.16, 0.5, 0.84), axis=0, method="lower")
    hi = np.nanquantile(v[ok], (0.16, 0.5, 0.84), axis=0, method="higher")
    for k, name in enumerate(derived.NAMES):
        assert np.all((lo[:, k] <= e[name]) & (e[name] <= hi[:, k])), name
    # a single row carrying all the weight is every quantile
    one = np.zeros(v.shape[0])
    one[1] = 2.0
    assert all(np.all(derived.summarize(v, q, weights=one)[n] == v[1, k]) for k, n in enumerate(derived.NAMES))
    zero = derived.summarize(v, q, weights=np.zeros(v.shape[0]))
    assert all(np.all(np.isnan(zero[n])) for n in derived.NAMES)
    for bad in (np.ones(3), -np.ones(v.shape[0]), np.full(v.shape[0], np.nan)):
        with pytest.raises(ValueError, match="weights"):
            derived.summarize(v, q, weights=bad)


def test_spin_period_and_rotational_energy_on_hand_values():
    assert derived.spin_period_ms(2.0 * np.pi * 1000.0) == pytest.approx(1.0, rel=1e-15)
    assert np.allclose(derived.spin_period_ms([2.0 * np.pi * 200.0, 2.0 * np.pi * 100.0]), [5.0, 10.0], rtol=1e-15)
    # a 1.4 Msol star of 10 km at 1 ms: I = f M R^2 = f x 2.786e45 g cm^2, E = 0.5 I (2 pi 1e3)^2
    omega = 2.0 * np.pi * 1.0e3
    for cfg, f in ((_capi.ModelCfg(inertia_factor=0.35), 0.35), (_capi.ModelCfg(inertia_factor=0.8), 0.8)):
        want = 0.5 * f * 1.4 * 1.99e33 * 1.0e12 * omega ** 2 / 1.0e50
        assert derived.rotational_energy(omega, cfg) == pytest.approx(want, rel=1e-14)
    assert derived.rotational_energy(omega, _capi.ModelCfg(inertia_factor=0.35)) == pytest.approx(192.5, rel=1e-3)   # 1.9e52 erg
    assert derived.rotational_energy(np.array([0.0, omega]), _capi.ModelCfg(inertia_factor=0.8)).shape == (2,)


def test_entry_point_refuses_bad_arguments_without_a_device():
    L = _capi.lib()
    assert "mp_model_derived" in _capi.EXPORTS and hasattr(L, "mp_model_derived")
    dp = ctypes.POINTER(ctypes.c_double)
    p, out = np.zeros((4, 6)), np.empty((4, 16))
    pp, po = p.ctypes.data_as(dp), out.ctypes.data_as(dp)
    assert L.mp_model_derived(None, pp, 4, 6, 0, po, None, None) == _capi.MP_EINVAL
    assert "mp_model_derived" in _capi.last_error() and "NULL" in _capi.last_error()
    assert L.mp_model_derived(None, pp, 0, 6, 0, po, None, None) == _capi.MP_EINVAL
    assert "n must be" in _capi.last_error()
    assert L.mp_model_derived(None, pp, 4, 5, 0, po, None, None) == _capi.MP_EINVAL
    assert "ndim" in _capi.last_error() and "5" in _capi.last_error()
    assert L.mp_model_derived(None, pp, 4, 10, 1, po, None, None) == _capi.MP_EINVAL


def test_product_code_imports_no_test_or_oracle_module():
    pkg = os.path.join(ROOT, "magprop_amd")
    for name in ("derived.py", "synth.py", "mcmc_eqns.py", "ensemble.py", "nested.py", "_capi.py"):
        src = open(os.path.join(pkg, name)).read()
        assert not re.search(r"^\s*(from|import)\s+(oracle|tests|derive_restated|derive_cases)\b", src, flags=re.M), name


def test_reference_fixture_shape_and_agreement_of_its_two_runs():
    g = np.load(os.path.join(GOLDEN, "golden_derived.npz"))
    n = g["pars"].shape[0]
    assert g["pars"].shape == (n, 6) and n >= 5
    assert g["ref"].shape == g["tight"].shape == (n, 7)
    assert g["tight_peak_idx"].shape == (n, 2) and g["tight_peak_nbr"].shape[:2] == (n, 2)
    assert g["tight_peak_nbr"].shape[2] % 2 == 1
    ok = np.isfinite(g["ref"]).all(axis=1) & np.isfinite(g["tight"]).all(axis=1)
    assert ok.sum() >= 4
    d = np.abs(g["ref"][ok, :3] - g["tight"][ok, :3])
    assert np.all(d <= LC_REF_RTOL * np.abs(g["tight"][ok, :3])), np.max(d / np.abs(g["tight"][ok, :3]))
