"""CPU checks of parallel tempering: the ladder rule, the thermodynamic-integration estimator and the new ABI names."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from magprop_amd import _capi, tempering


@pytest.mark.parametrize("betas", [
    [1.0],                                  # one temperature is no ladder
    [],
    [0.9, 0.5],                             # beta_0 must be 1
    [1.0, 1.0, 0.5],                        # strictly decreasing
    [1.0, 0.25, 0.5],
    [1.0, 0.5, 0.0],                        # beta = 0: 0 x -inf is NaN
    [1.0, 0.5, -0.1],
    [1.0, np.nan],
    [1.0, np.inf],
    [[1.0, 0.5], [1.0, 0.5]],               # not 1-D
])
def test_bad_ladders_are_refused(betas):
    with pytest.raises(ValueError):
        tempering.check_ladder(betas)


def test_good_ladders_pass_unchanged():
    for b in ([1.0, 0.5], [1.0, 0.5, 0.25, 0.125], [1.0, 1e-300]):
        out = tempering.check_ladder(b)
        assert out.dtype == np.float64 and np.array_equal(out, np.array(b))
    g = tempering.geometric_ladder(7, 1e-3)
    assert g[0] == 1.0 and g.size == 7 and np.all(np.diff(g) < 0) and np.isclose(g[-1], 1e-3, rtol=1e-12)
    with pytest.raises(ValueError):
        tempering.geometric_ladder(1, 0.5)
    with pytest.raises(ValueError):
        tempering.geometric_ladder(4, 0.0)


def _gauss_means(betas, d):
    """<ln L>_beta of a d-dimensional unit Gaussian likelihood under a flat prior: -d / (2 beta)."""
    return -d / (2.0 * np.asarray(betas))


def _explicit_trapezoid(betas, means):
    """Independent restatement: segment by segment, the beta = 0 segment carrying the hottest mean."""
    total = 0.0
    for t in range(len(betas) - 1):
        total += (betas[t] - betas[t + 1]) * (means[t] + means[t + 1]) / 2.0
    total += (betas[-1] - 0.0) * (means[-1] + means[-1]) / 2.0
    return total


@pytest.mark.parametrize("d", [1, 3, 6])
@pytest.mark.parametrize("n_temps,beta_min", [(2, 0.5), (4, 0.125), (9, 1e-2), (30, 1e-4)])
def test_trapezoid_equals_the_explicit_sum(d, n_temps, beta_min):
    b = np.geomspace(1.0, beta_min, n_temps)
    b[0] = 1.0
    m = _gauss_means(b, d)
    ti = tempering.thermodynamic_integral(b, m)
    ref = _explicit_trapezoid(list(b), list(m))
    assert abs(ti - ref) <= 1e-12 * max(1.0, abs(ref))
    # the beta = 0 segment alone contributes beta_min x (-d / (2 beta_min)) = -d / 2
    assert np.isclose(beta_min * m[-1], -d / 2.0, rtol=1e-14)
    # and the one-temperature-pair case by hand
    two = tempering.thermodynamic_integral([1.0, 0.5], [-1.0, -3.0])
    assert two == 0.5 * (-1.0 + -3.0) / 2.0 + 0.5 * -3.0


@pytest.mark.parametrize("d", [2, 6])
def test_dense_ladder_matches_the_closed_form(d):
    """integral_{beta_min}^1 -d/(2 beta) + beta_min x (-d/(2 beta_min)) = (d/2) ln beta_min - d/2."""
    beta_min = 1e-4
    b = tempering.geometric_ladder(200, beta_min)
    ti, dti = tempering.ti_log_evidence(b, _gauss_means(b, d))
    exact = 0.5 * d * np.log(beta_min) - 0.5 * d
    assert abs(ti / exact - 1.0) < 1e-3
    assert dti < 1e-2 * abs(exact)


def test_every_other_error_shrinks_as_the_ladder_is_refined():
    d, beta_min = 6, 1e-3
    errs, devs = [], []
    exact = 0.5 * d * np.log(beta_min) - 0.5 * d
    for n in (5, 9, 17, 33, 65):
        b = tempering.geometric_ladder(n, beta_min)
        ti, dti = tempering.ti_log_evidence(b, _gauss_means(b, d))
        errs.append(dti)
        devs.append(abs(ti - exact))
    assert all(e2 < e1 for e1, e2 in zip(errs, errs[1:])), errs
    # it bounds the true discretisation error of the fine ladder (trapezoid, error ~ h^2: the coarse one is ~4x worse)
    assert all(dv <= e for dv, e in zip(devs, errs)), (devs, errs)
    # both ends kept: an even number of temperatures still ends the coarse ladder at the hottest one
    assert list(tempering.every_other(4)) == [0, 2, 3] and list(tempering.every_other(5)) == [0, 2, 4]


def test_estimator_input_checks():
    with pytest.raises(ValueError):
        tempering.thermodynamic_integral([1.0, 0.5], [-1.0])
    with pytest.raises(ValueError):
        tempering.thermodynamic_integral([1.0, 0.5], [-1.0, -np.inf])
    lnf, dlnf = tempering.validity_term(750, 1000)
    assert np.isclose(lnf, np.log(0.75)) and np.isclose(dlnf, np.sqrt(0.25 / 750.0))
    assert tempering.validity_term(10, 10) == (0.0, 0.0)
    with pytest.raises(ValueError):
        tempering.validity_term(0, 1000)


def test_new_names_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "magprop_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("mp_sampler_set_temperatures", "mp_sampler_get_swaps"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in _capi.EXPORTS
        assert hasattr(_capi.lib(), name)
    assert _capi.ABI_VERSION == 5


def test_ladder_rule_of_the_library_without_a_device():
    """NULL sampler and NULL ladder are refused before anything touches a device."""
    import ctypes as C
    L = _capi.lib()
    b = np.array([1.0, 0.5])
    assert L.mp_sampler_set_temperatures(None, 2, b.ctypes.data_as(C.POINTER(C.c_double))) == _capi.MP_EINVAL
    assert L.mp_sampler_get_swaps(None, None) == _capi.MP_EINVAL
