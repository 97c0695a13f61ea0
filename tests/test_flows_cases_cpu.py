"""CPU checks of the radii, mass flows and torques (mp_model_flows): the numpy restatement (tests/flows_restated.py) against the
reference's own recorded arrays, against the recorded right-hand sides and against a long-double definition; the cases of
tests/flows_cases.py; the names of magprop_amd/flows.py against the header; the host helpers; the entry points' argument checks
without a device."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from magprop_amd import _capi, derived, flows

import derive_restated as dr
import flows_cases as fc
import flows_restated as fr

EPS = fr.EPS
RECOVERED = {"Rm": fr.RM, "Rc": fr.RC, "Rlc": fr.RLC, "w": fr.FASTNESS, "Ndip": fr.N_DIP, "Mdotprop": fr.MDOT_PROP,
             "Mdotacc": fr.MDOT_ACC, "Nacc": fr.N_ACC}


def test_names_follow_the_header_indices():
    hdr = open(os.path.join(ROOT, "include", "magprop_amd.h")).read()
    curves = dict((k, int(v)) for k, v in re.findall(r"#define\s+MP_FLOW_CURVE_([A-Z0-9_]+)\s+([0-9]+)\b", hdr))
    cols = dict((k, int(v)) for k, v in re.findall(r"#define\s+MP_FLOW_(?!CURVE_)([A-Z0-9_]+)\s+([0-9]+)\b", hdr))
    assert cols.pop("NCURVES") == len(flows.CURVES) == _capi.FLOW_NCURVES == fr.NCURVES == len(curves) == 10
    assert cols.pop("N") == len(flows.NAMES) == _capi.FLOW_N == fr.N == 16
    assert [k.lower() for k, _ in sorted(cols.items(), key=lambda kv: kv[1])] == [n.lower() for n in flows.NAMES]
    assert [k.lower() for k, _ in sorted(curves.items(), key=lambda kv: kv[1])] == [n.lower() for n in flows.CURVES]
    assert tuple(flows.CURVES) == fr.CURVE_NAMES
    for k, v in cols.items():
        assert getattr(fr, k) == v, k
    for k, v in curves.items():
        assert getattr(fr, k) == v, k
    assert re.search(r"#define\s+MP_ABI_VERSION\s+5\b", hdr)
    assert _capi.flow_curve_args(("N_dip", "Rm")) == (1 | 1 << 8, ("Rm", "N_dip"))
    with pytest.raises(ValueError, match="branch"):
        _capi.flow_curve_args(("Rm", "branch"), band=True)
    with pytest.raises(ValueError, match="non-empty"):
        _capi.flow_curve_args((), band=True)
    with pytest.raises(ValueError, match="selection"):
        _capi.flow_curve_args(("Rm", "Rm"))


@pytest.mark.parametrize("model, torque", [("po", 0), ("b", 1)])
def test_restated_cells_against_the_reference_script(model, torque):
    """tests/golden/golden_flows.npz (make_flows_golden.py: code/figure_3.py run up to its plotting section): the script's own
    (Mdisc, omega) through the restated cells, every one of its recovered arrays under flows_restated.cell_bounds(...,
    against_reference=True).

    The bound is derived there, not measured: per curve a count of roundings (RM 32, RC 8, RLC 8, FASTNESS 58, MDOT_FB 50, N_DIP
    14 or 112 units of 2^-52 relative), and for the quantities behind the switch the propagation of the fastness's error
    through tanh(n (w - 1)): x = n (w - 1) carries dx = n w E_W, e = exp(-2 |x|) the relative 2 dx, and so does the SMALLER of
    eta1 = e / (1 + e) and eta2 -- the relative 2 n w E_W of the issue -- while the larger carries only e times that next to
    its dozen roundings.  N_ACC crosses zero at w = 1 and takes the switch absolutely, (sech^2 x / 2) (2 dx + ...) sqrt(GM max(Rm,
    R)) Mdisc / tvisc, which vanishes where the switch is saturated.  Against the reference two more terms enter, because the
    script forms eta1 as 1 - eta2: 2 x 2^-52 Mdisc / tvisc on either rate, twice that times the arm on N_ACC."""
    g = np.load(os.path.join(GOLDEN, "golden_flows.npz"))
    n, alpha, cs7, k, inertia_factor = g["consts"]
    assert g["idx"][0] == 0 and g["idx"][-1] == 10000 and g["idx"].size == 401 and np.all(np.diff(g["idx"]) == 25)
    cfg = fc.Cfg("fig3", n_ode=n, alpha=alpha, cs7=cs7, k=k, inertia_factor=inertia_factor, dipole_torque=torque)
    c, aux = fr.cells(cfg, g["pars"], g["tarr"], g[model + "_Mdisc"], g[model + "_omega"])
    exact = fr.cells(cfg, g["pars"], g["tarr"], g[model + "_Mdisc"], g[model + "_omega"], literal_rc=True)[0]
    assert np.array_equal(exact[fr.RC], g[model + "_Rc"]) and np.array_equal(exact[fr.FASTNESS], g[model + "_w"])   # the script's own lines
    b = fr.cell_bounds(cfg, c, aux, against_reference=True)
    for name, curve in RECOVERED.items():
        ref = g[f"{model}_{name}"]
        d = np.abs(c[curve] - ref)
        print(model, name, "largest |d| / bound", np.max(d / np.maximum(b[curve], 1e-300)))
        assert np.all(d <= b[curve]), (name, int(np.argmax(d / np.maximum(b[curve], 1e-300))))
    # (the figure's parameters are a propeller throughout that ends under the cap; the other side of the switch, the other
    # branches and the break-up limit are among the recorded right-hand sides below)
    assert c[fr.FASTNESS].min() > 1.0 and set(np.unique(c[fr.BRANCH])) == {2.0, 3.0}


@pytest.mark.parametrize("name", ["synth", "lib"])
def test_restated_cells_against_the_recorded_right_hand_sides(grhs, name):
    """At the 1 500 states of golden_rhs.npz per variant (all branches; other k and alpha): MDOT_FB - MDOT_PROP - MDOT_ACC is the
    recorded dMdisc/dt and (N_ACC + N_DIP) / I the recorded domega/dt.  Bound: both sides evaluate the same few terms, each
    to at most 16 roundings (the fallback rate's power carries the most: flows_restated.E_FB / 2 on a side), so the sums agree
    to 32 * 2^-52 times the sum of the absolute TERMS -- MDOT_FB, MDOT_PROP, MDOT_ACC; arm * MDOT_ACC, arm * MDOT_PROP, N_DIP.
    (The corotation radius as the reference writes it, literal_rc: next to w = 1 with n = 10 the four units of the last place
    between fl(1/3) and the cube root are 75 of them in tanh.)"""
    P, t, y, ref = grhs[name + "_pars"], grhs[name + "_t"], grhs[name + "_y"], grhs[name + "_dydt"]
    cfg = fc.Cfg(name)
    c, aux = fr.cells(cfg, P.T, t, y[:, 0], y[:, 1], k=grhs[name + "_k"], alpha=grhs[name + "_alpha"], literal_rc=True)
    # the split itself against libm's tanh, the form the reference writes: eta2 = (1 + tanh x) / 2 to 2 units of the last place of 1
    eta2 = 0.5 * (1.0 + np.tanh(aux["x"]))
    assert np.all(np.abs(c[fr.MDOT_PROP] - eta2 * aux["mdot"]) <= 2.0 * EPS * aux["mdot"])
    assert np.all(np.abs(c[fr.MDOT_ACC] - (1.0 - eta2) * aux["mdot"]) <= 2.0 * EPS * aux["mdot"])
    assert np.count_nonzero(eta2 > 0.5) > 100 and np.count_nonzero(eta2 < 0.5) > 100
    dm = c[fr.MDOT_FB] - c[fr.MDOT_PROP] - c[fr.MDOT_ACC]
    terms = np.abs(c[fr.MDOT_FB]) + np.abs(c[fr.MDOT_PROP]) + np.abs(c[fr.MDOT_ACC])
    print(name, "dMdisc/dt: largest |d| / (eps * terms)", np.max(np.abs(dm - ref[:, 0]) / (EPS * terms)))
    assert np.all(np.abs(dm - ref[:, 0]) <= 32.0 * EPS * terms)
    inertia = fr.inertia(cfg)
    do = (c[fr.N_ACC] + c[fr.N_DIP]) / inertia
    live = aux["rot"] <= 0.27
    terms = (np.where(live, np.abs(aux["arm_mdot"]), 0.0) + np.abs(c[fr.N_DIP])) / inertia
    print(name, "domega/dt: largest |d| / (eps * terms)", np.max(np.abs(do - ref[:, 1]) / (EPS * terms)))
    assert np.all(np.abs(do - ref[:, 1]) <= 32.0 * EPS * terms)
    assert np.count_nonzero(~live) > 10 and len(np.unique(c[fr.BRANCH])) == 4            # every branch is among the states


def independent_row(c, t):
    """the integer- and index-valued columns of one row by plain loops"""
    G = t.size
    w, rm, br = c[fr.FASTNESS], c[fr.RM], c[fr.BRANCH]
    out = {}
    iw = ir = 0
    for i in range(1, G):
        if w[i] > w[iw]:
            iw = i
        if rm[i] < rm[ir]:
            ir = i
    hits = [i for i in range(G) if w[i] >= 1.0]
    out[fr.W_MAX], out[fr.T_W_MAX], out[fr.W_END] = w[iw], t[iw], w[G - 1]
    out[fr.RM_MIN], out[fr.T_RM_MIN] = rm[ir], t[ir]
    out[fr.N_PROP] = float(len(hits))
    out[fr.T_PROP_FIRST] = t[hits[0]] if hits else np.nan
    out[fr.T_PROP_LAST] = t[hits[-1]] if hits else np.nan
    out[fr.N_SWITCH] = float(sum((w[i] >= 1.0) != (w[i + 1] >= 1.0) for i in range(G - 1)))
    out[fr.N_CAPPED] = float(sum(int(b) & 1 for b in br))
    out[fr.N_INSIDE] = float(sum(1 - (int(b) >> 1 & 1) for b in br))
    return out


def same(a, b):
    a, b = np.atleast_1d(a), np.atleast_1d(b)
    return np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a), np.signbit(b))


@pytest.mark.parametrize("name", fc.reduce_names())
def test_reduction_restated_against_an_independent_definition(name):
    """The sums against np.longdouble sums in plain index order: a sum of G - 1 terms in any order is within (G - 1) eps of
    the exact one relative to the sum of the absolute terms, and every term carries three roundings -- 4 G eps sum |term|.
    Counts, indices and extrema against plain loops, exactly."""
    _, t, c, status = fc.reduce_case(name)
    G = t.size
    got = fr.reduce(c, status, t)
    for r in range(c.shape[1]):
        if status[r] != 0:
            assert np.all(np.isnan(got[r]))
            continue
        ld = fr.reduce_longdouble(c[:, r], t)
        for col, curve in fr.SUMS:
            scale = float((0.5 * (t[1:] - t[:-1]) * (np.abs(c[curve, r, :-1]) + np.abs(c[curve, r, 1:]))).sum())
            assert abs(float(np.longdouble(got[r, col]) - ld[col])) <= 4.0 * G * EPS * scale, (name, r, col)
        for col, v in independent_row(c[:, r], t).items():
            assert same(got[r, col], v), (name, r, col, got[r, col], v)


def test_the_cases_cover_what_they_are_named_for():
    col = lambda name, r=0: fr.reduce_row(fc.reduce_case(name)[2][:, r], fc.reduce_case(name)[1])   # noqa: E731
    G = 1000
    t = fc.reduce_case("alternating")[1]
    assert col("never_propeller")[fr.N_PROP] == 0 and np.isnan(col("never_propeller")[fr.T_PROP_FIRST])
    assert col("always_propeller")[fr.N_PROP] == G and col("always_propeller")[fr.N_SWITCH] == 0
    assert col("exactly_one")[fr.N_PROP] == G
    o = col("propeller_first_point_only")
    assert (o[fr.N_PROP], o[fr.T_PROP_FIRST], o[fr.T_PROP_LAST], o[fr.N_SWITCH]) == (1, t[0], t[0], 1)
    o = col("propeller_last_point_only")
    assert (o[fr.N_PROP], o[fr.T_PROP_FIRST], o[fr.T_PROP_LAST], o[fr.N_SWITCH]) == (1, t[-1], t[-1], 1)
    assert col("alternating")[fr.N_SWITCH] == G - 1
    assert dr.seg_len(G) == 4 and col("switch_on_segment_boundary")[fr.T_PROP_FIRST] == t[28]
    assert col("switch_before_segment_boundary")[fr.T_PROP_LAST] == t[26]
    tw = fc.reduce_case("switch_on_window_boundary")[1]
    assert dr.seg_len(tw.size) == 29 and col("switch_on_window_boundary")[fr.T_PROP_FIRST] == tw[5 * 29 + 14]
    o = col("ties")
    assert o[fr.T_W_MAX] == t[100] and o[fr.T_RM_MIN] == t[500]
    o = col("ties", 1)
    assert o[fr.T_W_MAX] == t[0] and o[fr.T_RM_MIN] == t[0]
    o = col("ties", 2)
    assert o[fr.T_W_MAX] == t[255] and o[fr.T_RM_MIN] == t[256]
    assert col("huge")[fr.M_FB] > 1e290 and 0 < col("tiny")[fr.M_FB] < 1e-290
    assert same(col("negative_zero")[fr.M_FB], 0.0) and same(col("negative_zero")[fr.RM_MIN], -0.0)
    names = fc.reduce_names()
    assert len(set(names)) == len(names) and all(f"grid_{G}" in names for G in fc.REDUCE_GRID_SIZES + fc.REDUCE_WINDOW_GRID_SIZES)
    # the cell cases: the constructed states sit where their names say
    names = fc.cell_names()
    assert len(set(names)) == len(names)
    for case in fc.cell_cases():
        cfg = fc.cfg_of(case)
        for r in range(case["pars"].shape[0]):
            c, aux = fr.cells(cfg, case["pars"][r], case["t"][r], case["mdisc"][r], case["omega"][r])
            if case["name"].startswith("cap_tie"):
                A, tvisc = fc.rmu_constants(cfg, case["pars"][r])
                rmu = A * np.power(cfg.rm_massflow_factor * case["mdisc"][r] / tvisc, -2.0 / 7.0)
                assert np.allclose(rmu, cfg.k * fr.C_LIGHT / case["omega"][r], rtol=1e-14, atol=0.0) and np.all(case["either"] == 1)
                assert np.all(c[fr.BRANCH].astype(int) & 2)                    # (the bit that is not tied)
            if case["name"].startswith("rm_equals_r"):
                assert np.allclose(c[fr.RM], fr.R_STAR, rtol=1e-14, atol=0.0) and np.all(case["either"] == 2)
                assert not np.any(c[fr.BRANCH].astype(int) & 1)
            if case["name"].startswith("w_equals_1"):
                assert np.allclose(c[fr.FASTNESS], 1.0, rtol=0.0, atol=3e-9) and not np.any(c[fr.BRANCH] % 2)
            if case["name"].startswith("breakup"):
                assert np.array_equal(aux["rot"] > 0.27, [False, True, False, True]) and np.allclose(aux["rot"], 0.27, rtol=1e-8)
                assert list(c[fr.BRANCH] % 2) == [0, 0, 1, 1]
            if case["name"] == "saturated_waves":
                x = aux["x"]
                W = fc.WAVE_POINTS
                if r < 3:
                    assert np.all(np.abs(x) > 19.5) and (r != 2 or (x.min() < 0 < x.max()))
                else:
                    assert np.all(np.abs(x[:W]) > 19.5) and np.any(np.abs(x[W:2 * W]) < 19.5) and np.count_nonzero(np.abs(x[2 * W:]) < 19.5) == 1


def test_host_helpers():
    rng = np.random.default_rng(5)
    v = np.abs(rng.standard_normal((50, 16))) + 0.1
    v[::7] = np.nan                                            # rows that did not finish
    v[1, 9:11] = np.nan                                        # a finished row that never propels
    s = flows.summarize(v, (0.25, 0.5))
    ok = ~np.isnan(v[:, 0])
    assert s["n_used"] == int(ok.sum()) and np.array_equal(s["q"], [0.25, 0.5])
    assert np.array_equal(s["M_fb"], np.quantile(v[ok, 0], [0.25, 0.5]))
    assert np.array_equal(s["t_prop_first"], np.nanquantile(v[ok, 9], [0.25, 0.5]))
    w = rng.uniform(0.0, 1.0, 50)
    sw = flows.summarize(v, (0.25, 0.5), w)
    assert np.array_equal(sw["J_dip"], derived.weighted_quantile(v[ok, 4], np.array([0.25, 0.5]), w[ok]))
    assert np.all(np.isnan(flows.summarize(np.full((3, 16), np.nan))["w_max"]))
    with pytest.raises(ValueError, match="16"):
        flows.summarize(np.zeros((3, 15)))
    with pytest.raises(ValueError, match="quantile"):
        flows.summarize(v, (1.5,))
    with pytest.raises(ValueError, match="weights"):
        flows.summarize(v, (0.5,), np.ones(3))
    assert np.array_equal(flows.ejected_fraction(v)[ok], v[ok, 1] / (v[ok, 1] + v[ok, 2]))
    assert np.array_equal(flows.propeller_fraction(v, 10001)[ok], v[ok, 8] / 10001.0)
    # budgets on numbers that close by construction
    cfg = _capi.ModelCfg(inertia_factor=0.8)
    inertia = 0.8 * derived.M_STAR * derived.R_STAR ** 2
    pars = np.array([[1.0, 5.0, 1.0e-3, 1000.0, 0.1, 1.0]])
    tab, dtab = np.zeros((1, 16)), np.zeros((1, 16))
    tab[0, :5] = [3.0e30, 1.0e30, 1.5e30, 4.0e47, -1.0e47]
    dtab[0, derived.NAMES.index("Mdisc_end")] = 1.0e-3 * flows.M_SOL + 0.5e30
    dtab[0, derived.NAMES.index("omega_end")] = 2.0 * np.pi / 5.0e-3 + 3.0e47 / inertia
    b = flows.budgets(tab, dtab, pars, cfg)
    assert b["mass"][0] < 1e-15 and b["momentum"][0] < 1e-14
    tab[0, 0] *= 1.1
    assert flows.budgets(tab, dtab, pars, cfg)["mass"][0] == pytest.approx(0.3e30 / 5.8e30, rel=1e-12)


def test_entry_points_refuse_bad_arguments_without_a_device():
    L = _capi.lib()
    dp = ctypes.POINTER(ctypes.c_double)
    p, out, q, band = np.zeros((4, 6)), np.empty((4, 16)), np.array([0.5]), np.empty(8)
    pp, po, pq, pb = (a.ctypes.data_as(dp) for a in (p, out, q, band))
    u32 = ctypes.c_uint32
    assert L.mp_model_flows(None, pp, 4, 6, 0, po, u32(0), None, None, None) == _capi.MP_EINVAL
    assert "mp_model_flows" in _capi.last_error() and "NULL" in _capi.last_error()
    assert L.mp_model_flows(None, pp, 0, 6, 0, po, u32(0), None, None, None) == _capi.MP_EINVAL
    assert "n must be" in _capi.last_error()
    for ndim in (5, 10):
        assert L.mp_model_flows(None, pp, 4, ndim, 0, po, u32(0), None, None, None) == _capi.MP_EINVAL
        assert "ndim" in _capi.last_error()
    assert L.mp_model_flows(None, pp, 4, 6, 0, po, u32(1 << 10), pb, None, None) == _capi.MP_EINVAL
    assert "curve_mask" in _capi.last_error()
    assert L.mp_model_flow_band(None, pp, 4, 6, 0, None, pq, 1, u32(1), pb, None, None) == _capi.MP_EINVAL
    assert "mp_model_flow_band" in _capi.last_error() and "NULL" in _capi.last_error()


def test_product_code_imports_no_test_or_oracle_module():
    pkg = os.path.join(ROOT, "magprop_amd")
    for name in ("flows.py", "figure_3.py", "synth.py", "mcmc_eqns.py", "ensemble.py", "nested.py", "_capi.py"):
        src = open(os.path.join(pkg, name)).read()
        assert not re.search(r"^\s*(from|import)\s+(oracle|tests|flows_restated|flows_cases)\b", src, flags=re.M), name
