"""GPU tests of the radii, mass flows and torques through the ABI (mp_model_flows, mp_model_flow_band; run with -m gpu on an
MI355X): the device table and cell curves against the probe's two kernels (libmp_probe_flows.so: the product's own compiled
kernels behind host buffers) applied to what mp_model_lc returns in traj for the same rows one by one, bit for bit; independence
of the batch size across the chunk boundary; statuses; every refused argument; the band against np.nanquantile and the weighted
restatement of the returned curves; the closure of the mass and angular-momentum budgets; the front ends.

As in tests/test_gpu_derived.py the bit-for-bit comparison with mp_model_lc runs on a handle whose prior box is in physical
units with no log mask (`phys`): mp_model_lc takes physical parameters, and the device's 10^x and numpy's need not agree to the
bit."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN, TRUTHS

import flows_restated as fr
import wband_restated as wr
from flows_probe import Probe

pytestmark = pytest.mark.gpu

PHYS_LOWER = np.array([1.0e-3, 0.69, 1.0e-6, 50.0, 1.0e-2, 1.0e-1])
PHYS_UPPER = np.array([10.0, 10.0, 1.0e-2, 2000.0, 1.0e2, 1.0e3])
# the four canonical parameter sets (code/synthetic_datasets/generate_data.py:10-15), physical
GRB_PARS = {"Humped": [1.0, 5.0, 1.0e-3, 100.0, 0.1, 1.0], "Classic": [1.0, 5.0, 1.0e-3, 1000.0, 0.1, 1.0],
            "Sloped": [1.0, 1.0, 1.0e-3, 100.0, 10.0, 10.0], "Stuttering": [1.0, 5.0, 1.0e-5, 100.0, 0.1, 100.0]}
FLAGS = [1.8171068, 3.68147895, -2.61786801, 1.99840102, -0.33083576, 2.95613803]       # sampler coordinates: reaches break-up
Q3 = np.array([0.16, 0.5, 0.84])
ALL_CURVES = fr.CURVE_NAMES
# Closure of the budgets: the trapezoid's quadrature error on the 10 001-point grid, measured on the CPU with flows_restated
# applied to trajectories of the serial oracle in fixed-step mode (oracle/c_oracle.py trajectory, synthetic configuration) on
# the four canonical sets -- mass residual: Humped 7.079e-08, Classic 7.656e-08, Sloped 1.036e-08, Stuttering 7.551e-08;
# angular-momentum residual: 2.415e-07, 2.489e-07, 3.058e-07, 2.460e-07.  The device is held to 4 times the largest: the margin
# covers the product's stride-adaptive trajectory, which differs from the oracle's by at most 5.7e-8.
CLOSURE_MASS, CLOSURE_MOMENTUM = 4.0 * 7.656e-08, 4.0 * 3.058e-07
# figure_3.recover against the golden, measured the same way (the oracle's trajectory of the script's parameters through
# flows_restated against the recorded arrays, largest relative difference over both models): Mdisc 8.35e-08, omega 3.27e-08,
# Rm 3.27e-08, Rc 2.18e-08, Rlc 3.27e-08, w 4.46e-08, Ndip 9.82e-08, Mdotprop 8.35e-08, Nacc 7.16e-08 -- this is the reference's
# own default-tolerance LSODA noise; Mdotacc, which the script forms as (1 - eta2) Mdisc / tvisc and which is below 1e-10 of
# Mdisc / tvisc throughout, 1.86e-10 of Mdisc / tvisc.  Times 4:
RECOVER_REL, RECOVER_MDOTACC = 4.0 * 9.82e-08, 4.0 * 1.86e-10


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a), np.signbit(b))


@pytest.fixture(scope="module")
def probe():
    return Probe()


@pytest.fixture(scope="module")
def phys(tarr):
    from magprop_amd import _capi
    h = _capi.Handle(_capi.cfg_synth(), tarr)
    h.set_prior(PHYS_LOWER, PHYS_UPPER, 0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def humped(tarr, gsynth):
    from magprop_amd import _capi, synth
    h = _capi.Handle(_capi.cfg_synth(), tarr)
    h.set_dataset(0, gsynth["Humped_x"], gsynth["Humped_y"], gsynth["Humped_yerr"])
    h.set_prior(synth.PRIOR_LOWER, synth.PRIOR_UPPER, synth.LOG_MASK)
    yield h
    h.close()


def _six_rows():
    flag = np.array(FLAGS)
    flag[2:] = 10.0 ** flag[2:]
    outside = np.array(GRB_PARS["Humped"])
    outside[0] = 50.0                                          # B above the box
    return np.array([GRB_PARS["Humped"], flag, GRB_PARS["Classic"], outside, GRB_PARS["Sloped"], GRB_PARS["Stuttering"]])


@pytest.fixture(scope="module")
def six(phys, probe):
    """(rows, table, cells (n, 10, G), status) by the host path: mp_model_lc row by row, then the probe's two kernels"""
    from magprop_amd import _capi
    P = _six_rows()
    t = phys.tgrid
    cfg = _capi.cfg_synth()
    table = np.full((len(P), fr.N), np.nan)
    cells = np.full((len(P), fr.NCURVES, t.size), np.nan)
    st = np.full(len(P), 3, dtype=np.int32)
    for i, p in enumerate(P):
        if not np.all((p >= PHYS_LOWER) & (p <= PHYS_UPPER)):
            continue
        s, _, traj = phys.model_lc(p, want_traj=True)
        st[i] = s
        c = probe.cells(cfg, p, t, traj[0], traj[1], status=[s])
        table[i] = probe.reduce(t, c, [s])[0]
        cells[i] = c[:, 0]
    return P, table, cells, st


def test_table_and_curves_equal_the_kernels_on_model_lc_trajectories(phys, six):
    P, want, want_cells, st_want = six
    assert list(st_want) == [0, 1, 0, 3, 0, 0]
    got, cells, st, used = phys.model_flows(P, curves=ALL_CURVES)
    assert np.array_equal(st, st_want) and used == 4
    assert np.all(np.isnan(got[st != 0])) and np.all(np.isnan(cells[st != 0]))
    assert not np.any(np.isnan(cells[st == 0])) and not np.any(np.isnan(got[st == 0][:, :9]))
    for i in range(len(P)):
        assert _same(got[i], want[i]), (i, got[i], want[i])
        for c in range(fr.NCURVES):
            assert _same(cells[i, c], want_cells[i, c]), (i, fr.CURVE_NAMES[c])
    # physical rows are the same numbers on this handle
    again, cells2, st2, used2 = phys.model_flows(P, curves=ALL_CURVES, physical=True)
    ok = st == 0
    assert _same(again[ok], got[ok]) and _same(cells2[ok], cells[ok]) and np.all(st2[ok] == 0)
    # a selection of curves comes back in the order of the bits, and no curve at all is allowed
    part, pc, _, _ = phys.model_flows(P, curves=("N_dip", "Rc"))
    assert _same(part, got) and pc.shape[1] == 2 and _same(pc[:, 0], cells[:, fr.RC]) and _same(pc[:, 1], cells[:, fr.N_DIP])
    none, nc, _, _ = phys.model_flows(P)
    assert nc is None and _same(none, got)


def test_rows_do_not_depend_on_the_batch_size(phys):
    """n = mp_n_simd + 1 crosses a chunk: the first and the last row are what n = 1 gives (the summary only)."""
    n = phys.n_simd + 1
    rng = np.random.default_rng(21)
    P = np.array(GRB_PARS["Humped"]) * (1.0 + 0.01 * rng.standard_normal((n, 6)))
    P[5] = _six_rows()[1]                                      # a row that flags inside the first chunk
    got, _, st, used = phys.model_flows(P)
    assert st[5] == 1 and used == n - 1 and np.all(np.isnan(got[5]))
    for r in (0, n - 2, n - 1):
        alone, _, st1, _ = phys.model_flows(P[r:r + 1])
        assert st1[0] == 0 and _same(alone[0], got[r]), r


def test_statuses_are_lnprob_batch(humped):
    from magprop_amd import _capi
    rng = np.random.default_rng(22)
    S = np.array(TRUTHS["Humped"]) + 0.02 * rng.standard_normal((40, 6))
    S[3] = FLAGS
    S[7, 0] = 50.0
    S[11, 5] = 3.5
    _, st_ref = humped.lnprob_batch(S, ds_id=0, want_status=True)
    got, _, st, used = humped.model_flows(S)
    assert np.array_equal(st, st_ref) and st[3] == _capi.STATUS_FLAG and st[7] == st[11] == _capi.STATUS_PRIOR
    assert used == int(np.sum(st_ref == 0)) == 37 and np.array_equal(np.isnan(got[:, 0]), st != 0)


def test_refused_arguments(phys):
    from magprop_amd import _capi
    L, h = _capi.lib(), phys._h
    dp = C.POINTER(C.c_double)
    G = phys.tgrid.size
    p, out, cur, q, band = np.tile(GRB_PARS["Humped"], (2, 1)), np.empty((2, 16)), np.empty((2, 1, G)), Q3.copy(), np.empty((1, 3, G))
    pp, po, pc, pq, pb = (a.ctypes.data_as(dp) for a in (p, out, cur, q, band))
    u32 = C.c_uint32
    E = _capi.MP_EINVAL
    assert L.mp_model_flows(h, None, 2, 6, 1, po, u32(0), None, None, None) == E
    assert L.mp_model_flows(h, pp, 2, 6, 1, None, u32(0), None, None, None) == E
    assert L.mp_model_flows(h, pp, 0, 6, 1, po, u32(0), None, None, None) == E and "n must be" in _capi.last_error()
    assert L.mp_model_flows(h, pp, 2, 5, 1, po, u32(0), None, None, None) == E and "ndim" in _capi.last_error()
    assert L.mp_model_flows(h, pp, 2, 10, 1, po, u32(0), None, None, None) == E
    assert L.mp_model_flows(h, pp, 2, 6, 1, po, u32(1 << 10), pc, None, None) == E and "curve_mask" in _capi.last_error()
    assert L.mp_model_flows(h, pp, 2, 6, 1, po, u32(1), None, None, None) == E and "NULL" in _capi.last_error()
    assert L.mp_model_flows(h, pp, 2, 6, 1, po, u32(1), pc, None, None) == _capi.MP_OK
    B = L.mp_model_flow_band
    assert B(h, None, 2, 6, 1, None, pq, 3, u32(1), pb, None, None) == E
    assert B(h, pp, 2, 6, 1, None, None, 3, u32(1), pb, None, None) == E
    assert B(h, pp, 2, 6, 1, None, pq, 3, u32(1), None, None, None) == E and "NULL" in _capi.last_error()
    assert B(h, pp, 0, 6, 1, None, pq, 3, u32(1), pb, None, None) == E
    assert B(h, pp, _capi.BAND_MAX_SAMPLES + 1, 6, 1, None, pq, 3, u32(1), pb, None, None) == E and "MP_BAND_MAX_SAMPLES" in _capi.last_error()
    assert B(h, pp, 2, 5, 1, None, pq, 3, u32(1), pb, None, None) == E
    assert B(h, pp, 2, 6, 1, None, pq, 0, u32(1), pb, None, None) == E
    assert B(h, pp, 2, 6, 1, None, pq, _capi.BAND_MAX_Q + 1, u32(1), pb, None, None) == E and "MP_BAND_MAX_Q" in _capi.last_error()
    bad_q = np.array([0.1, 1.5, 0.2])
    assert B(h, pp, 2, 6, 1, None, bad_q.ctypes.data_as(dp), 3, u32(1), pb, None, None) == E and "q[1]" in _capi.last_error()
    assert B(h, pp, 2, 6, 1, None, pq, 3, u32(0), pb, None, None) == E
    assert B(h, pp, 2, 6, 1, None, pq, 3, u32(1 << 10), pb, None, None) == E
    assert B(h, pp, 2, 6, 1, None, pq, 3, u32(1 | 1 << fr.BRANCH), pb, None, None) == E and "BRANCH" in _capi.last_error()
    w = np.array([1.0, -1.0])
    assert B(h, pp, 2, 6, 1, w.ctypes.data_as(dp), pq, 3, u32(1), pb, None, None) == E and "weights" in _capi.last_error()
    assert B(h, pp, 2, 6, 1, None, pq, 3, u32(1), pb, None, None) == _capi.MP_OK
    with pytest.raises(ValueError, match="branch"):
        phys.model_flow_band(p, Q3, ("branch",))


@pytest.fixture(scope="module")
def rows33(humped):
    """33 rows in sampler coordinates, a flagged one and one outside the prior among them, and their curves"""
    rng = np.random.default_rng(23)
    S = np.array(TRUTHS["Humped"]) + 0.05 * rng.standard_normal((33, 6))
    S[4] = FLAGS
    S[9, 0] = 50.0
    _, cells, st, used = humped.model_flows(S, curves=ALL_CURVES[:-1])
    assert used == 31 and st[4] == 1 and st[9] == 3
    return S, cells, st


def test_band_is_nanquantile_of_the_returned_curves(humped, rows33):
    S, cells, st = rows33
    names = ("Rm", "fastness", "Mdot_acc", "N_dip")
    band, bst, used = humped.model_flow_band(S, Q3, names)
    assert np.array_equal(bst, st) and used == 31 and band.shape == (4, 3, humped.tgrid.size)
    for k, name in enumerate(names):
        want = np.nanquantile(cells[:, fr.CURVE_NAMES.index(name)], Q3, axis=0)
        assert _same(band[k], want), name
    one, _, _ = humped.model_flow_band(S, Q3, "fastness")
    assert _same(one[0], band[1])


def test_weighted_band_is_the_restatement_on_the_returned_curves(humped, rows33):
    from magprop_amd import _capi
    S, cells, st = rows33
    w = np.exp(np.random.default_rng(24).standard_normal(33))
    w[2] = 0.0
    names = ("Rc", "Mdot_prop", "N_acc")
    band, bst, used = humped.model_flow_band(S, Q3, names, weights=w)
    units = _capi.band_weight_units(w)
    assert np.array_equal(units, wr.weight_units(w)) and np.array_equal(bst, st) and used == 31
    for k, name in enumerate(names):
        assert _same(band[k], wr.weighted_band(cells[:, fr.CURVE_NAMES.index(name)].T, units, Q3)), name


def test_band_across_a_chunk_boundary(phys):
    """n = mp_n_simd + 1 rows, two curves, with and without weights: the cells of the second chunk land at their row offset of
    the n x n_grid matrices and the transpose and select run once behind the last chunk.  Against the curves mp_model_flows
    returns for the same rows; a second call (the matrices of a band of two curves are freed in between) repeats it."""
    from magprop_amd import _capi
    n = phys.n_simd + 1
    rng = np.random.default_rng(25)
    P = np.array(GRB_PARS["Humped"]) * (1.0 + 0.01 * rng.standard_normal((n, 6)))
    P[7] = _six_rows()[1]                                      # flags, in the first chunk
    P[n - 1, 0] = 50.0                                         # outside the prior: the only row of the second chunk is left out ...
    P[n - 2] = GRB_PARS["Classic"]                             # ... and the last row of the first is unlike the others
    names = ("fastness", "Mdot_fb")
    _, cells, st, used = phys.model_flows(P, curves=names)
    assert used == n - 2 and st[7] == 1 and st[n - 1] == 3
    band, bst, bused = phys.model_flow_band(P, Q3, names)
    assert np.array_equal(bst, st) and bused == used
    for k in range(2):
        assert _same(band[k], np.nanquantile(cells[:, k], Q3, axis=0)), names[k]
    again, _, _ = phys.model_flow_band(P, Q3, names)
    assert _same(again, band)
    # the second chunk's row decides: swapped with a finished row, the band of the permuted rows is the same band
    perm = np.arange(n)
    perm[[0, n - 1]] = [n - 1, 0]
    swapped, sst, _ = phys.model_flow_band(P[perm], Q3, names)
    assert np.array_equal(sst, st[perm]) and _same(swapped, band)
    w = np.exp(rng.standard_normal(n))
    wb, _, _ = phys.model_flow_band(P[perm], Q3, "Mdot_fb", weights=w)
    assert _same(wb[0], wr.weighted_band(cells[perm, 1].T, _capi.band_weight_units(w), Q3))


def test_budgets_close(phys):
    """The mass and angular-momentum budgets of the four canonical sets (all finish: no row may be left out) close to the
    trapezoid's quadrature error:
      mass      |(MDISC_END - Mdisc_0) - (M_FB - M_PROP - M_ACC)| / (M_FB + M_PROP + M_ACC)
      momentum  |I (OMEGA_END - omega_0) - (J_ACC + J_DIP)| / (|J_ACC| + |J_DIP|)
    Measured on the CPU (flows_restated on the serial oracle's fixed-step trajectories): mass 7.079e-08 / 7.656e-08 / 1.036e-08 /
    7.551e-08, momentum 2.415e-07 / 2.489e-07 / 3.058e-07 / 2.460e-07 for Humped / Classic / Sloped / Stuttering.  Bound: 4
    times the largest, 3.062e-07 and 1.223e-06; the margin covers the product's stride-adaptive trajectory (5.7e-8 from the
    oracle's)."""
    from magprop_amd import _capi, flows
    P = np.array([GRB_PARS[k] for k in ("Humped", "Classic", "Sloped", "Stuttering")])
    table, _, st, used = phys.model_flows(P, physical=True)
    dtable, dst, _ = phys.model_derived(P, physical=True)
    assert used == 4 and np.all(st == 0) and np.all(dst == 0)
    b = flows.budgets(table, dtable, P, _capi.cfg_synth())
    print("mass residuals", b["mass"], "momentum residuals", b["momentum"])
    assert np.all(b["mass"] <= CLOSURE_MASS) and np.all(b["momentum"] <= CLOSURE_MOMENTUM)
    # what the model exists to answer: Humped spends its first 8 060 grid points as a propeller and then accretes (and so
    # ejects the smallest share of its mass), the others never stop propelling
    f = flows.as_dict(table)
    assert list(f["n_switch"]) == [1, 0, 0, 0] and list(f["n_prop"][1:]) == [10001] * 3 and 7000 < f["n_prop"][0] < 9000
    ej = flows.ejected_fraction(table)
    assert np.all((ej > 0.0) & (ej <= 1.0)) and np.argmin(ej) == 0 and np.all(flows.propeller_fraction(table, 10001) <= 1.0)


@pytest.mark.parametrize("model, prefix", [("piroott", "po"), ("bucciantini", "b")])
def test_figure_3_recover_against_the_reference_script(model, prefix):
    """figure_3.recover at the script's parameters against what the script leaves behind (tests/golden/golden_flows.npz), held to
    RECOVER_REL = 4 x 9.82e-08 relative (Mdotacc: RECOVER_MDOTACC = 4 x 1.86e-10 of Mdisc / tvisc), measured on the CPU as stated
    at the top of this file."""
    from magprop_amd import figure_3
    g = np.load(os.path.join(GOLDEN, "golden_flows.npz"))
    rec = figure_3.recover(model, *g["pars"])
    assert isinstance(rec, dict) and np.array_equal(rec["tarr"][g["idx"]], g["tarr"])
    tvisc = g["pars"][3] * 1.0e5 / (g["consts"][1] * g["consts"][2] * 1.0e7)
    for name in ("Mdisc", "omega", "Rm", "Rc", "Rlc", "w", "Ndip", "Mdotprop", "Mdotacc", "Nacc"):
        got, ref = rec[name][g["idx"]], g[f"{prefix}_{name}"]
        bound = RECOVER_MDOTACC * g[prefix + "_Mdisc"] / tvisc if name == "Mdotacc" else RECOVER_REL * np.abs(ref)
        print(model, name, "largest |d| / bound", np.max(np.abs(got - ref) / bound))
        assert np.all(np.abs(got - ref) <= bound), name


def test_sampler_and_module_wiring(gsynth):
    from magprop_amd import EnsembleSampler, flows, synth
    x, y, yerr = gsynth["Humped_x"], gsynth["Humped_y"], gsynth["Humped_yerr"]
    rng = np.random.default_rng(4)
    p0 = np.array(TRUTHS["Humped"]) + 1e-3 * rng.standard_normal((32, 6))
    s = EnsembleSampler(32, 6, x, y, yerr, seed=5)
    s.run_mcmc(p0, 6, store=True)
    rows = s.get_chain()[2::2].reshape(-1, 6)
    got = s.get_flows(q=Q3, discard=2, thin=2, curves=("fastness",))
    want = synth.model_flows(rows, curves=("fastness",), q=Q3)
    assert got["n_used"] == want["n_used"] == rows.shape[0] and _same(got["values"], want["values"])
    assert _same(got["fastness"], want["fastness"]) and np.array_equal(got["t"], want["t"])
    assert list(got["summary"]) == ["q", "n_used"] + list(flows.NAMES) and _same(got["summary"]["M_acc"], want["summary"]["M_acc"])
    gb = s.get_flow_band(q=Q3, curves=("Mdot_prop", "Rm"), discard=2, thin=2)
    wb = synth.model_flow_band(rows, q=Q3, curves=("Mdot_prop", "Rm"))
    assert set(gb) == {"t", "Rm", "Mdot_prop", "n_used"} and _same(gb["Rm"], wb["Rm"]) and _same(gb["Mdot_prop"], wb["Mdot_prop"])
    assert _same(gb["Rm"], np.nanquantile(s.get_flows(discard=2, thin=2, curves=("Rm",))["Rm"], Q3, axis=0))
    s.close()
    from magprop_amd import mcmc_eqns
    S = np.array(TRUTHS["Humped"]) + 0.01 * np.abs(rng.standard_normal((8, 6)))
    lib = mcmc_eqns.model_flows(S, "L", curves=("N_acc",))
    assert lib["n_used"] >= 1 and lib["values"].shape == (8, 16) and lib["N_acc"].shape == (8, 10001)
