"""The two kernels behind mp_model_flows on their own (magprop_amd/csrc/mp_flows.hip flow_cells_kernel, flow_reduce_kernel) on the
cases of tests/flows_cases.py, reached through the probe library libmp_probe_flows.so (csrc/mp_probe_flows.hip), which is test
infrastructure, no part of the product's ABI, and linked from the product's own kernel object.

Cells: against the numpy restatement (tests/flows_restated.py) under the bound its cell_bounds() derives -- a count of roundings
per curve with every device primitive at its tested 2 ulp, the inexact exponents of the restated powers, and the propagation of
the fastness's error through tanh(n (w - 1)), a relative 2 n w times that error on the smaller of eta1 and eta2 -- on states
exactly on and one ulp to either side of the cap and of Rm == R, at w == 1, with the switch saturated on both sides, in a
wavefront that is uniformly saturated next to one that is mixed, just below and above break-up, at both ends of the grid, for
the presets, both torque laws, ndim 6 to 9, failed rows between finished ones, row counts around a wavefront and grid sizes
around a workgroup's 512 points.  BRANCH agrees exactly away from the constructed ties ("either" in a case); at a tie the tied
bit may fall on either side and the other bit agrees exactly.  The reference's own states (tests/golden/golden_flows.npz) go through the kernel and are held to the same
bound against the reference's recorded arrays.

Reduce: against the restatement bit for bit on every column (NaNs by position, signs of zero included).
tests/test_flows_cases_cpu.py checks the cases and the restatement themselves."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN

import flows_cases as fc
import flows_probe
import flows_restated as fr

pytestmark = pytest.mark.gpu

_dp, _ip, _i = flows_probe._dp, flows_probe._ip, flows_probe._i
ALL = flows_probe.ALL
Probe = flows_probe.Probe


@pytest.fixture(scope="module")
def probe():
    return Probe()


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a), np.signbit(b))


def test_probe_shares_the_restatement_constants(probe):
    import derive_cases as dc
    import derive_restated as dr
    L = probe.L
    assert L.mpf_threads() == dr.SEGMENTS and L.mpf_columns() == fr.N and L.mpf_curves() == fr.NCURVES
    assert L.mpf_window() == dc.WINDOW and L.mpf_reduce_mask() == fr.REDUCE_MASK
    assert L.mpf_lane() * 64 == fc.WAVE_POINTS
    for G in fc.REDUCE_GRID_SIZES + fc.REDUCE_WINDOW_GRID_SIZES:
        assert L.mpf_seg(G) == dr.seg_len(G)
    t = np.arange(1.0, 4.0)
    z = np.zeros((10, 1, 3))
    st = np.zeros(1, dtype=np.int32)
    out = np.empty((1, 16))
    a = lambda x, p: x.ctypes.data_as(p)                   # noqa: E731
    assert L.mpf_reduce(None, a(st, _ip), a(t, _dp), 1, 3, a(out, _dp)) == -1
    assert L.mpf_reduce(a(z, _dp), a(st, _ip), a(t, _dp), 0, 3, a(out, _dp)) == -1
    assert L.mpf_reduce(a(z, _dp), a(st, _ip), a(t, _dp), 1, 1, a(out, _dp)) == -1
    cfg = probe.cfg("synth")
    p = np.ones((1, 6))
    assert L.mpf_cells(C.byref(cfg), a(t, _dp), a(t, _dp), a(t, _dp), a(p, _dp), a(st, _ip), 1, 3, 6, 0, a(z, _dp)) == -1
    assert L.mpf_cells(C.byref(cfg), a(t, _dp), a(t, _dp), a(t, _dp), a(p, _dp), a(st, _ip), 1, 3, 5, 1, a(z, _dp)) == -1
    assert L.mpf_cells(C.byref(cfg), a(t, _dp), a(t, _dp), a(t, _dp), a(p, _dp), a(st, _ip), 1, 3, 6, 1 << 10, a(z, _dp)) == -1


def check_cells(got, cfg, case, against_reference=None):
    """got (10, rows, G) of a case against the restatement (or, against_reference: (10, rows, G) recorded arrays with NaN where
    nothing is recorded) under cell_bounds; returns the largest |d| / bound seen"""
    worst = 0.0
    for r in range(case["pars"].shape[0]):
        if case["status"][r] != 0:
            assert np.all(np.isnan(got[:, r])), (case["name"], r)
            continue
        want, aux = fr.cells(cfg, case["pars"][r], case["t"][r], case["mdisc"][r], case["omega"][r])
        bound = fr.cell_bounds(cfg, want, aux, against_reference is not None)
        ref = want if against_reference is None else against_reference[:, r]
        assert not np.any(np.isnan(got[:, r])), (case["name"], r)
        for c in range(fr.NCURVES):
            have = ~np.isnan(ref[c])
            if c == fr.BRANCH:
                # away from a constructed tie exactly; at one, the tied bit may fall on either side and the other bit is as restated
                free = case["either"][r][have].astype(np.int64)
                g, w = got[c, r][have], ref[c][have]
                assert np.all(np.isin(g, (0.0, 1.0, 2.0, 3.0))), (case["name"], r, "BRANCH")
                assert np.array_equal(g.astype(np.int64) & ~free, w.astype(np.int64) & ~free), (case["name"], r, "BRANCH")
                continue
            d = np.abs(got[c, r] - ref[c])[have]
            ratio = d / np.maximum(bound[c][have], 1e-300)
            worst = max(worst, float(ratio.max()) if ratio.size else 0.0)
            assert np.all(d <= bound[c][have]), (case["name"], r, fr.CURVE_NAMES[c], int(np.argmax(ratio)), float(ratio.max()))
    return worst


@pytest.mark.parametrize("name", fc.cell_names())
def test_cells_against_the_restatement(probe, name):
    case = fc.cell_case(name)
    cfg = probe.cfg(case["preset"], **case["over"])
    got = probe.cells(cfg, case["pars"], case["t"], case["mdisc"], case["omega"], case["status"])
    print(name, "largest |d| / bound", check_cells(got, fc.cfg_of(case), case))


def test_saturated_wavefronts_take_the_smaller_rate_for_zero_and_mixed_ones_do_not(probe):
    """What the vote inside flow_state does, so that the floor in the bound is there for a reason: a uniformly saturated
    wavefront gives exactly 0 for the smaller rate, a mixed one its tiny value."""
    case = fc.cell_case("saturated_waves")
    cfg = probe.cfg(case["preset"], **case["over"])
    got = probe.cells(cfg, case["pars"], case["t"], case["mdisc"], case["omega"], case["status"])
    W = fc.WAVE_POINTS
    assert np.all(got[fr.MDOT_PROP, 0] == 0.0) and np.all(got[fr.MDOT_ACC, 1] == 0.0)
    assert np.all(got[fr.MDOT_PROP, 3, :W] == 0.0) and np.all(got[fr.MDOT_PROP, 3, W:] > 0.0)


def test_a_mask_writes_its_curves_only(probe):
    case = fc.cell_case("grid_513")
    cfg = probe.cfg(case["preset"], **case["over"])
    whole = probe.cells(cfg, case["pars"], case["t"], case["mdisc"], case["omega"], case["status"])
    mask = 1 << fr.RC | 1 << fr.MDOT_FB | 1 << fr.BRANCH
    part = probe.cells(cfg, case["pars"], case["t"], case["mdisc"], case["omega"], case["status"], mask=mask)
    assert part.shape[0] == 3 and same(part, whole[[fr.RC, fr.MDOT_FB, fr.BRANCH]])


@pytest.mark.parametrize("model, torque", [("po", 0), ("b", 1)])
def test_reference_states_through_the_cells_kernel(probe, model, torque):
    """The script's own (Mdisc, omega) at its recorded grid points through the kernel, against the script's recovered arrays."""
    g = np.load(os.path.join(GOLDEN, "golden_flows.npz"))
    n, alpha, cs7, k, inertia_factor = g["consts"]
    over = dict(n_ode=float(n), alpha=float(alpha), cs7=float(cs7), k=float(k), inertia_factor=float(inertia_factor), dipole_torque=torque)
    case = dict(name="golden_" + model, pars=g["pars"][None, :], t=g["tarr"][None, :], mdisc=g[model + "_Mdisc"][None, :],
                omega=g[model + "_omega"][None, :], status=np.zeros(1, dtype=np.int32), either=np.zeros((1, g["tarr"].size), np.int64))
    got = probe.cells(probe.cfg("fig3", **over), case["pars"], case["t"], case["mdisc"], case["omega"])
    ref = np.full((fr.NCURVES, 1, g["tarr"].size), np.nan)
    for name, curve in (("Rm", fr.RM), ("Rc", fr.RC), ("Rlc", fr.RLC), ("w", fr.FASTNESS), ("Ndip", fr.N_DIP), ("Mdotprop", fr.MDOT_PROP),
                        ("Mdotacc", fr.MDOT_ACC), ("Nacc", fr.N_ACC)):
        ref[curve, 0] = g[f"{model}_{name}"]
    print(model, "largest |d| / bound", check_cells(got, fc.Cfg("fig3", **over), case, against_reference=ref))


def test_a_row_of_cells_does_not_depend_on_its_place_in_the_batch(probe):
    case = fc.cell_case("rows_257")
    cfg = probe.cfg(case["preset"], **case["over"])
    args = lambda s: (case["pars"][s], case["t"][s], case["mdisc"][s], case["omega"][s], case["status"][s])   # noqa: E731
    whole = probe.cells(cfg, *args(slice(None)))
    for r in (0, 63, 64, 256):
        assert same(probe.cells(cfg, *args(slice(r, r + 1)))[:, 0], whole[:, r]), r
    perm = np.random.default_rng(3).permutation(257)
    assert same(probe.cells(cfg, *args(perm)), whole[:, perm])


@pytest.mark.parametrize("name", fc.reduce_names())
def test_reduce_equals_the_restatement_bit_for_bit(probe, name):
    _, t, cells, status = fc.reduce_case(name)
    got = probe.reduce(t, cells, status)
    want = fr.reduce(cells, status, t)
    assert np.all(np.isnan(got[status != 0]))
    bad = [(r, c) for r in range(got.shape[0]) for c in range(fr.N) if not same(got[r, c:c + 1], want[r, c:c + 1])]
    assert not bad, (name, bad[:5], [(got[r, c], want[r, c]) for r, c in bad[:5]])


def test_a_reduced_row_does_not_depend_on_its_place_in_the_batch(probe):
    _, t, cells, status = fc.reduce_case("rows_257")
    whole = probe.reduce(t, cells, status)
    for r in (0, 63, 64, 256):
        alone = probe.reduce(t, cells[:, r:r + 1], status[r:r + 1])
        assert same(alone[0], whole[r]), r
    perm = np.random.default_rng(3).permutation(257)
    assert same(probe.reduce(t, cells[:, perm], status[perm]), whole[perm])
