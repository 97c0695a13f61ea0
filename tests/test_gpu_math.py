"""The device math primitives (magprop_amd/csrc/mp_math.hpp), one at a time, against multiprecision expectations
(tests/golden/golden_math.npz, written by tests/golden/make_math_golden.py) and against numpy restatements
(tests/math_restated.py).  The kernels are reached through the probe library libmp_probe.so (csrc/mp_probe.hip), which is
test infrastructure and no part of the product's ABI.  numpy only; every assertion is on every element.

Where the root functions are applied (mp_eval.hpp), and the ranges those quantities span over the prior boxes:
  rcbrt_fast     u = (t + tfb) / tfb in mdot_fb / mdot_fb_d: t <= 1e6 s, tfb = epsilon tvisc >= 0.05 s, so 1 <= u <= 2e7.
  pow_m1_7_fast  the field B in 1e15 G (walker_setup): 1e-3 .. 10; and the accretion rate Mdisc / tvisc in g/s (disc_point):
                 Mdisc <= (1 + delta) MdiscI Msol ~ 2e34 g, tvisc >= 5 s, so up to ~4e33 g/s.  From below: dMdisc/dt =
                 Mdotfb - Mdisc / tvisc with a falling Mdotfb gives Mdisc / tvisc >= min(MdiscI Msol / tvisc, Mdotfb(t)), and
                 Mdotfb(t) = M0 tfb^(2/3) / (t + tfb)^(5/3) >= 2e25 g x (0.05 s)^(2/3) / (1e6 s)^(5/3) ~ 3e14 g/s
                 (M0 = delta MdiscI Msol >= 2e25 g in either box, tfb >= 0.05 s, t <= 1e6 s): the argument stays above 1e14.
                 2^100 = 1.3e30 does not cover the upper end, so the tested domain is every normal float, 2^-126 .. 2^127,
                 which is the domain the source states ("positive normal x within float range") and holds [1e14, 4e33].

The maxima measured on an MI355X are in DESIGN.md section 5 (printed by these tests as lines `MATH-MAX ...`)."""
import ctypes as C
import os

import numpy as np
import pytest

import math_restated as mr
import probe_lib
from math_restated import EPS, err_rel, err_ulps, same_bits

pytestmark = pytest.mark.gpu

_dp, _i, _d = C.POINTER(C.c_double), C.c_int, C.c_double


def _p(a):
    return a.ctypes.data_as(_dp)


def _in(a):
    return np.ascontiguousarray(a, np.float64).ravel()


class Probe:
    """libmp_probe.so behind numpy arrays; every call raises unless the probe returns 0."""

    def __init__(self):
        from magprop_amd import _capi
        _capi.lib()                                        # first, so that one HIP runtime is shared
        self.L = probe_lib.load()
        for name in mr.PROBE_EXPORTS:
            getattr(self.L, name).restype = _i
        self.L.mpp_lane_prev.argtypes = [_dp, _d, _dp, _i]

    def _ok(self, rc, what):
        assert rc == 0, f"{what} returned {rc}"

    def unary(self, func, N, x):
        x = _in(x)
        y = np.full(x.size, np.nan)
        self._ok(self.L.mpp_unary(func, N, _p(x), _p(y), x.size), "mpp_unary")
        return y

    def exp10(self, x):
        x = _in(x)
        y = np.full(x.size, np.nan)
        self._ok(self.L.mpp_exp10(_p(x), _p(y), x.size), "mpp_exp10")
        return y

    def phi(self, N, z):
        z = _in(z)
        out = np.full((z.size, 7), np.nan)
        self._ok(self.L.mpp_phi(N, _p(z), _p(out), z.size), "mpp_phi")
        return out

    def phi6(self, N, z, p5):
        z, p5 = _in(z), _in(p5)
        out = np.full(z.size, np.nan)
        self._ok(self.L.mpp_phi6(N, _p(z), _p(p5), _p(out), z.size), "mpp_phi6")
        return out

    def node_weights(self, N, pipelined, kind, wtab, z):
        z, wtab = _in(z), _in(wtab)
        out = np.full((z.size, 5), np.nan)
        self._ok(self.L.mpp_node_weights(N, int(pipelined), kind, _p(wtab), wtab.size, _p(z), _p(out), z.size), "mpp_node_weights")
        return out

    def two(self, name, a, b):
        a, b = _in(a), _in(b)
        x, y = np.full(a.size, np.nan), np.full(a.size, np.nan)
        self._ok(getattr(self.L, name)(_p(a), _p(b), _p(x), _p(y), a.size), name)
        return x, y

    def one(self, name, v, *args):
        v = _in(v)
        out = np.full(v.size, np.nan)
        self._ok(getattr(self.L, name)(_p(v), *args, _p(out), v.size), name)
        return out

    def lane_ext(self, func, N, v):
        v = _in(v)
        out = np.full(v.size // N, np.nan)
        self._ok(self.L.mpp_lane_ext(func, N, _p(v), _p(out), v.size), "mpp_lane_ext")
        return out

    def unfused(self, a, b, c):
        a, b, c = _in(a), _in(b), _in(c)
        x, y = np.full(a.size, np.nan), np.full(a.size, np.nan)
        self._ok(self.L.mpp_unfused(_p(a), _p(b), _p(c), _p(x), _p(y), a.size), "mpp_unfused")
        return x, y

    def lse(self, K, terms):
        t = _in(terms)
        m, s = np.full(t.size // K, np.nan), np.full(t.size // K, np.nan)
        self._ok(self.L.mpp_lse(K, _p(t), _p(m), _p(s), t.size), "mpp_lse")
        return m, s

    def pick(self, u, m, c0, c1):
        u, m, c0, c1 = _in(u), _in(m), _in(c0), _in(c1)
        out = np.full((u.size, 3), np.nan)
        self._ok(self.L.mpp_pick(_p(u), _p(m), _p(c0), _p(c1), _p(out), u.size), "mpp_pick")
        return out

    def lse_merge(self, m, s, mo, so):
        m, s, mo, so = _in(m), _in(s), _in(mo), _in(so)
        om, os_ = np.full(m.size, np.nan), np.full(m.size, np.nan)
        self._ok(self.L.mpp_lse_merge(_p(m), _p(s), _p(mo), _p(so), _p(om), _p(os_), m.size), "mpp_lse_merge")
        return om, os_


@pytest.fixture(scope="module")
def probe():
    return Probe()


@pytest.fixture(scope="module")
def g():
    return np.load(mr.GOLDEN)


def report(name, value):
    print(f"MATH-MAX {name} {value:.3e}")


# ---------------------------------------------------------------- argument checks of the probe itself
def test_probe_refuses_bad_sizes(probe):
    x = np.ones(256)
    y = np.zeros(256)
    for n in (0, -64, 63, 65, 128 + 1, (1 << 20) + 64):
        assert probe.L.mpp_unary(0, 1, _p(x), _p(y), n) == -1
    assert probe.L.mpp_unary(0, 4, _p(x), _p(y), 128) == -1            # not a multiple of 64 * 4
    assert probe.L.mpp_unary(0, 3, _p(x), _p(y), 192) == -1            # N outside 1, 2, 4
    assert probe.L.mpp_unary(9, 1, _p(x), _p(y), 64) == -1
    assert probe.L.mpp_lane_bcast(_p(x), 64, _p(y), 64) == -1
    assert probe.L.mpp_lane_ext(0, 6, _p(x), _p(y), 384) == -1
    assert probe.L.mpp_lse(65, _p(x), _p(y), _p(y), 64 * 65) == -1
    assert probe.L.mpp_node_weights(1, 0, 5, _p(x), mr.WTAB_SIZE, _p(x), _p(y), 64) == -1
    assert probe.L.mpp_node_weights(1, 0, 0, _p(x), 256, _p(x), _p(y), 64) == -1
    assert np.all(y == 0.0)
    assert probe.L.mpp_wtab_size() == mr.WTAB_SIZE and probe.L.mpp_wtab_stride() == mr.WTAB_STRIDE


# ---------------------------------------------------------------- seed plus one correction step
SEED_STEP = {"rcp_fast": (0, "recip_x", "rcp"), "rsqrt_fast": (1, "recip_x", "rsqrt"),
             "rcbrt_fast": (3, "root_x", "rcbrt"), "pow_m1_7_fast": (4, "root_x", "pow17")}


@pytest.mark.parametrize("name", list(SEED_STEP))
def test_seed_step_functions(probe, g, name):
    """At most 2 ulp everywhere in the domain (the source's claim: the last operation is one FMA that adds a correction of
    at most 1e-5 of the result, and the neglected term of the step is below 1e-18); the same bits at 1, 2 and 4 per lane."""
    func, xkey, key = SEED_STEP[name]
    x, hi, lo = g[xkey], g[key + "_hi"], g[key + "_lo"]
    got = {N: probe.unary(func, N, x) for N in (1, 2, 4)}
    e = err_ulps(got[1], hi, lo)
    report(f"{name} ulp", e.max())
    assert np.all(e <= 2.0), f"{name}: {e.max():.3f} ulp at x = {x[np.argmax(e)]!r}"
    assert same_bits(got[1], got[2]) and same_bits(got[1], got[4])


# ---------------------------------------------------------------- exp_fast, exp10_fast
# largest error of the restatement mr.exp_fast, in ulp, over k ln2 / 2 for every odd k inside [-750, 700] with both
# neighbours (mr.exp_worst_inputs(), 6276 inputs; normal results) and over the fixture: 2.2502 at x = -298.39986123105643.
# Produced by
#   python -m pytest tests/test_math_cpu.py -k exp_restatement -s        (prints `MATH-MAX exp_fast restated ...`)
# which measures it with mpmath and holds this constant to it.
EXP_MAX_ULPS = 2.26


def test_exp_fast(probe, g):
    """Bit for bit the numpy restatement (every operation is an IEEE one), hence the LDS-table build (2 per lane) bit for
    bit the literal builds: on the fixture's inputs and on k ln2 / 2 for every odd k with both neighbours.  The
    restatement's own error on all of these (tests/test_math_cpu.py) is the accuracy bound; subnormal results
    (x in [-750, -708]) within one unit of 2^-1074."""
    x, hi, lo = g["exp_x"], g["exp_hi"], g["exp_lo"]
    for xs in (x, mr.exp_worst_inputs()):
        want = mr.exp_fast(xs)
        for N in (1, 2, 4):
            assert same_bits(probe.unary(2, N, xs), want), f"exp_fast<{N}> differs from its restatement"
    got = probe.unary(2, 2, x)
    e = err_ulps(got, hi, lo)
    sub = np.abs(hi) < 2.0 ** -1022
    assert sub.sum() >= 64
    report("exp_fast ulp", e[~sub].max())
    report("exp_fast subnormal units", e[sub].max())
    assert np.all(e[~sub] <= EXP_MAX_ULPS)
    assert np.all(e[sub] <= 1.0)


def test_exp10_fast(probe, g):
    """At most 2 ulp (the source's claim) at every bound of the prior boxes with its neighbours, the integers, a dense sample
    of the span of the boxes and a sample of [-300, 300].  No bit equality is asserted with the restatement
    (tests/test_math_cpu.py holds that one to 2 ulp on 20 000 more inputs); how far the two agree is printed."""
    x = g["exp10_x"]
    got = probe.exp10(x)
    e = err_ulps(got, g["exp10_hi"], g["exp10_lo"])
    report("exp10_fast ulp", e.max())
    report("exp10_fast elements unlike the restatement", float((got != mr.exp10_fast(x)).sum()))
    assert np.all(e <= 2.0), f"{e.max():.3f} ulp at x = {x[np.argmax(e)]!r}"


# ---------------------------------------------------------------- phi functions
def phi_bounds_check(got, z, path, g, label):
    """Per output and |z| range: the plain-fp64 formulas on the same inputs within their caps (1.5 x the table), the device
    within 4 x their figure + 4 eps (exp_fast and rcp_fast are allowed 2 ulp each where libm's exp and true division give
    1 at most, and each of the up to six recurrence stages carries that forward once)."""
    hi, lo = g["phi_hi"], g["phi_lo"]
    plain = mr.phi_errors(mr.phi_plain(z, path), z, path, hi, lo)
    dev = mr.phi_errors(got, z, path, hi, lo)
    bad = []
    for r, rng in enumerate(mr.PHI_RANGES):
        if np.isnan(plain[r, 0]):
            continue
        for c in range(7):
            report(f"phi {label} {rng} col{c}", dev[r, c])
            if plain[r, c] > mr.phi_cap(rng, c):
                bad.append(f"plain {rng} col {c}: {plain[r, c]:.2e} > {mr.phi_cap(rng, c):.2e}")
            if not dev[r, c] <= 4.0 * plain[r, c] + 4.0 * EPS:
                bad.append(f"device {rng} col {c}: {dev[r, c]:.2e} > 4 x {plain[r, c]:.2e} + 4 eps")
    assert not bad, "\n".join(bad)
    # e^z where it is subnormal or underflows (z < -708): units of 2^-1074
    sub = np.abs(hi[:, 0]) < 2.0 ** -1022
    assert sub.any()
    assert np.all(err_ulps(got[sub, 0], hi[sub, 0], lo[sub, 0]) <= 1.0)
    assert not np.isnan(got).any()


@pytest.mark.parametrize("N", [1, 2, 4])
def test_phi_accuracy(probe, g, N):
    z = g["phi_z"]
    path = mr.wave_paths(z, N)
    # every branch runs, by construction of the fixture's blocks: waves of each single kind and both mixed ones
    kinds = {tuple(np.unique(w)) for w in path.reshape(-1, 64 * N)}
    assert {(0,), (1,), (2,), (1, 2)} <= kinds
    phi_bounds_check(probe.phi(N, z), z, path, g, f"N{N}")


@pytest.mark.parametrize("N", [1, 2, 4])
def test_phi_all_big_path_equals_mixed_path(probe, g, N):
    """The same z once in waves that are all in the stiff range and once with one tiny lane among them: the big lanes agree
    bit for bit (at 4 per lane the first run takes the recurrence-only path, at 2 per lane it skips the series)."""
    z = g["phi_z"][512:1024].copy()                         # blocks 2 and 3: every |z| >= 1/2
    assert np.all(np.abs(z) >= 0.5)
    a = probe.phi(N, z)
    zm = z.copy()
    holes = np.arange(7, z.size, 64 * N)                    # one element of every wavefront
    zm[holes] = 1.0e-3
    b = probe.phi(N, zm)
    keep = np.ones(z.size, bool)
    keep[holes] = False
    assert same_bits(a[keep], b[keep])


@pytest.mark.parametrize("N", [1, 2, 4])
@pytest.mark.parametrize("block", [0, 1, 2, 3, 4, 5])
def test_phi_nan_lane(probe, g, N, block):
    """A NaN z gives NaN in all seven outputs of that element and leaves every other element as it is in the same wave with
    a finite z of the same range in its place."""
    z = g["phi_z"][256 * block: 256 * block + 256].copy()
    spots = np.arange(9, 256, 64 * N)                      # one element of every wavefront, never the odd one of blocks 4, 5
    ref = probe.phi(N, z)
    zn = z.copy()
    zn[spots] = np.nan
    got = probe.phi(N, zn)
    keep = np.ones(256, bool)
    keep[spots] = False
    assert np.all(np.isnan(got[spots])), got[spots]
    assert same_bits(got[keep], ref[keep])
    if N > 1:                                              # a lane whose z are all NaN
        zn = z.copy()
        lane0 = (spots // N) * N
        for j in range(N):
            zn[lane0 + j] = np.nan
        got = probe.phi(N, zn)
        keep = ~np.isnan(zn)
        assert np.all(np.isnan(got[~keep]))
        assert same_bits(got[keep], ref[keep])


@pytest.mark.parametrize("N", [1, 2, 4])
def test_phi6_series_ignores_phi5(probe, g, N):
    """phi6 below |z| = 1/2 is the series alone, whatever the Phi5 passed in; elsewhere it is the recurrence from it."""
    z = g["phi_z"]
    small = np.abs(z) < 0.5
    ref = probe.phi(N, z)
    for junk in (np.nan, np.inf, -1.0e300, 0.0):
        p5 = np.where(small, junk, ref[:, 5])
        assert same_bits(probe.phi6(N, z, p5), ref[:, 6])


# ---------------------------------------------------------------- node weights
@pytest.mark.parametrize("N", [1, 2, 4])
def test_node_weights(probe, g, N):
    """eam5_node_weights and its pipelined form agree bit for bit, and both are sum_m W[k][m] phi_{m+1} of the fixture's
    phi values: within the phi bound of the range scaled by sum_m |W[k][m] phi_{m+1}| / |c_k| (plus 5 eps for the five
    roundings of the sum itself), for the tables of both product grids and every tile kind."""
    L = np.longdouble
    z, hi, lo = g["phi_z"], g["phi_hi"], g["phi_lo"]
    path = mr.wave_paths(z, N)
    ridx = mr.phi_range_index(z, path)
    plain = mr.phi_errors(mr.phi_plain(z, path), z, path, hi, lo)
    bound_phi = 4.0 * plain[ridx, 1:6].max(axis=1) + 4.0 * EPS          # per element: the largest of phi_1 .. phi_5 of its range
    phi = hi[:, 1:6].astype(L) + lo[:, 1:6].astype(L)
    worst = 0.0
    for lnq in (mr.LNQ_GRID, mr.LNQ_GRID_S):
        T = mr.wtab(lnq)
        for kind in range(mr.KINDS):
            W = T[kind * mr.WTAB_STRIDE: kind * mr.WTAB_STRIDE + 30].reshape(5, 6)[:, :5]
            plain_w = probe.node_weights(N, False, kind, T, z)
            piped = probe.node_weights(N, True, kind, T, z)
            assert same_bits(plain_w, piped)
            terms = W.astype(L)[None, :, :] * phi[:, None, :]            # [element][k][m]
            want = terms.sum(axis=2)
            amp = np.abs(terms).sum(axis=2) / np.abs(want)
            err = np.abs(plain_w.astype(L) - want) / np.abs(want)
            lim = (bound_phi[:, None] + 5.0 * EPS) * amp
            ratio = (err / lim).astype(float)
            worst = max(worst, ratio.max())
            assert np.all(err <= lim), f"grid {lnq:.3e} kind {kind}: {ratio.max():.2f} x the bound"
    report(f"node_weights N{N} worst/bound", worst)


# ---------------------------------------------------------------- wavefront primitives
def scan_inputs():
    rng = np.random.default_rng(5)
    a = rng.uniform(-2.0, 2.0, (8, 64))
    b = 10.0 ** rng.uniform(-200.0, 200.0, (8, 64)) * rng.choice([-1.0, 1.0], (8, 64))
    a[1, ::5] = 0.0
    a[2, 3::7] = -0.0
    b[3, ::4] = 0.0
    a[4], b[4] = 1.0, 0.0
    a[5] = -1.0
    a[6] = rng.uniform(0.9, 1.0, 64)
    b[7] = -0.0
    return a, b


def test_scan_affine_bitwise(probe):
    a, b = scan_inputs()
    wa, wb = mr.scan_affine(a, b)
    ga, gb = probe.two("mpp_scan_affine", a, b)
    assert same_bits(ga, wa.ravel()) and same_bits(gb, wb.ravel())


def test_scan_affine_accuracy(probe, g):
    """Positive a <= 1 and positive b (nothing cancels): within 128 eps of the exact serial composition (64 maps, two
    roundings each)."""
    ga, gb = probe.two("mpp_scan_affine", g["scan_a"], g["scan_b"])
    ea = err_rel(ga, g["scan_a_hi"], g["scan_a_lo"])
    eb = err_rel(gb, g["scan_b_hi"], g["scan_b_lo"])
    report("scan_affine a rel", ea.max())
    report("scan_affine b rel", eb.max())
    assert np.all(ea <= 128 * EPS) and np.all(eb <= 128 * EPS)


def special_values(n, seed):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(n) * 10.0 ** rng.integers(-300, 300, n)
    v[::11] = -0.0
    v[5::13] = 0.0
    v[3::17] = np.inf
    v[7::19] = -np.inf
    v[2::23] = np.nan
    v[4::29] = 5e-324
    return v


def test_lane_moves(probe):
    """lane_prev, lane_prev_map, lane_bcast from every source lane, uniform: exact."""
    v, w = special_values(256, 1).reshape(4, 64), special_values(256, 2).reshape(4, 64)
    first = -123.456
    want = np.concatenate([np.full((4, 1), first), v[:, :-1]], axis=1)
    assert same_bits(probe.one("mpp_lane_prev", v, first), want.ravel())
    pa, pb = probe.two("mpp_lane_prev_map", v, w)
    assert same_bits(pa, np.concatenate([np.full((4, 1), 1.0), v[:, :-1]], axis=1).ravel())
    assert same_bits(pb, np.concatenate([np.full((4, 1), 0.0), w[:, :-1]], axis=1).ravel())
    for src in range(64):
        assert same_bits(probe.one("mpp_lane_bcast", v, src), np.repeat(v[:, src], 64)), src
    assert same_bits(probe.one("mpp_uniform", v), np.repeat(v[:, 0], 64))


def test_wave_sum(probe):
    rng = np.random.default_rng(3)
    v = rng.standard_normal((6, 64)) * 10.0 ** rng.integers(-8, 8, (6, 64))
    v[4] = 10.0 ** rng.uniform(-300, 300, 64)
    v[5, ::9] = -0.0
    assert same_bits(probe.one("mpp_wave_sum", v), mr.wave_sum(v).ravel())


@pytest.mark.parametrize("N", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("func", [0, 1, 2, 3], ids=["maxabs", "minabs", "max", "min"])
def test_lane_extrema(probe, func, N):
    """Exact, -0.0 included; a NaN operand of max_raw / min_raw is dropped (a lane of NaNs alone gives NaN)."""
    v = special_values(128 * N, 10 + N).reshape(-1, N)
    v[5] = np.nan
    v[6] = -0.0
    v[7, 0], v[7, 1:] = 0.0, -0.0
    assert same_bits(probe.lane_ext(func, N, v), mr.lane_ext(func, v))


# ---------------------------------------------------------------- unfused arithmetic
def test_unfused_arithmetic(probe):
    """10 000 triples with fma(a, b, c) != (a b) + c in fp64 (checked here): the device returns the separately rounded value,
    for add_rn(mul_rn(a, b), c) and for sub_rn(a, mul_rn(b, c))."""
    rng = np.random.default_rng(7)
    a, b = rng.uniform(1.0, 2.0, 40000), rng.uniform(1.0, 2.0, 40000)
    c = -(a * b) * (1.0 + rng.uniform(-1e-3, 1e-3, 40000))            # cancels most of the product: its rounding error shows
    differ = mr.fma(a, b, c) != a * b + c
    idx = np.nonzero(differ)[0][:10000]
    assert idx.size == 10000
    a, b, c = a[idx], b[idx], c[idx]
    pad = (-a.size) % 64
    a, b, c = (np.concatenate([v, np.ones(pad)]) for v in (a, b, c))
    addmul, _ = probe.unfused(a, b, c)
    assert same_bits(addmul, a * b + c)
    # the other composition on triples of its own: a - b c with a next to b c
    b2, c2 = rng.uniform(1.0, 2.0, 40000), rng.uniform(1.0, 2.0, 40000)
    a2 = (b2 * c2) * (1.0 + rng.uniform(-1e-3, 1e-3, 40000))
    idx2 = np.nonzero(mr.fma(-b2, c2, a2) != a2 - b2 * c2)[0][:10000]
    assert idx2.size == 10000
    a2, b2, c2 = (np.concatenate([v[idx2], np.ones(pad)]) for v in (a2, b2, c2))
    _, submul = probe.unfused(a2, b2, c2)
    assert same_bits(submul, a2 - b2 * c2)


# ---------------------------------------------------------------- log-sum-exp
LSE_K = 4
# Bound on |ln(s) + m - ln sum e^v|, ln(s) + m formed in long double, i.e. on the relative error of the sum e^m s.  Every
# term passes LSE_K folds at most and 6 merge levels; each costs 2 eps (one product, one sum) and one exp, 1 ulp (the
# accuracy the HIP math API documents for exp in double precision).  The rounding of an exponent v - m changes its term by
# |v - m| eps / 2 of itself, e^-(|v - m|) of the sum: over n terms at most (1 + ln n) eps / 2 in all.  2^-63 |L|: the long double sum.
def lse_bound(K, want):
    return (K + 6) * 3.0 * EPS + 0.5 * EPS * (1.0 + np.log(64.0 * K)) + 2.0 ** -63 * np.abs(want)


def test_wave_lse(probe, g):
    L = np.longdouble
    terms = g["lse_terms"].reshape(8, 64 * LSE_K)
    m, s = probe.lse(LSE_K, terms)
    m, s = m.reshape(8, 64), s.reshape(8, 64)
    for w in range(8):                                      # every lane ends with the same pair
        assert same_bits(m[w], np.repeat(m[w, :1], 64)) and same_bits(s[w], np.repeat(s[w, :1], 64)), w
    assert m[0, 0] == -np.inf and s[0, 0] == 0.0 and not np.signbit(s[0, 0])       # the empty sum
    assert g["lse_hi"][0] == -np.inf
    assert m[1, 0] == -12.25 and s[1, 0] == 1.0                                     # one finite term among -inf
    assert m[2, 0] == terms[2].max() and s[2, 0] == 1.0                             # one term 700 above the rest
    assert m[3, 0] == 1.7 and s[3, 0] == 256.0                                      # equal terms
    worst = 0.0
    for w in range(1, 8):
        want = L(g["lse_hi"][w]) + L(g["lse_lo"][w])
        got = np.log(L(s[w, 0])) + L(m[w, 0])
        err = float(abs(got - want))
        worst = max(worst, err / lse_bound(LSE_K, float(want)))
        assert err <= lse_bound(LSE_K, float(want)), (w, err)
    report("wave_lse worst/bound", worst)


def test_lse_merge(probe, g):
    L = np.longdouble
    m, s, mo, so = g["merge_m"], g["merge_s"], g["merge_mo"], g["merge_so"]
    om, os_ = probe.lse_merge(m, s, mo, so)
    hi, lo = g["merge_hi"], g["merge_lo"]
    empty = hi == -np.inf
    assert empty.sum() == 2
    assert np.all(om[empty] == -np.inf) and np.all(os_[empty] == 0.0)
    assert np.all(om[~empty] == np.maximum(np.where(s != 0, m, -np.inf), np.where(so != 0, mo, -np.inf))[~empty])
    one = (~empty) & ((s == 0) | (so == 0))                 # an empty operand leaves the other pair as it is
    assert one.sum() == 6
    assert same_bits(os_[one], np.where(s == 0, so, s)[one])
    got = np.log(os_[~empty].astype(L)) + om[~empty].astype(L)
    want = hi[~empty].astype(L) + lo[~empty].astype(L)
    err = np.abs(got - want).astype(float)
    # one level: 2 eps and one exp of 1 ulp; the exponent's rounding, d e^-d eps / 2 <= eps / (2 e), is below another eps
    lim = 4.0 * EPS + 2.0 ** -63 * np.abs(hi[~empty])
    report("lse_merge abs", err.max())
    assert np.all(err <= lim), err.max()
    # a sum that is empty under a finite maximum (s = 0 on both sides) is the empty pair (-inf, 0), not (max, 0)
    stale = np.linspace(-700.0, 700.0, 64)
    zero = np.zeros(64)
    em, es = probe.lse_merge(stale, zero, stale[::-1], zero)
    assert np.all(em == -np.inf) and np.all(es == 0.0)
    em, es = probe.lse_merge(stale, zero, np.full(64, -np.inf), zero)
    assert np.all(em == -np.inf) and np.all(es == 0.0)
    # symmetric in its operands
    bm, bs = probe.lse_merge(mo, so, m, s)
    assert same_bits(bm, om) and same_bits(bs, os_)


# ---------------------------------------------------------------- index draws of the DE and snooker moves
def test_index_draws_equal_the_restatement(probe):
    """pick, pick_skip and pick_skip2 (mp_math.hpp) on the cases of tests/commit_cases.py: m = 1 .. 70, u at the double below, at
    and above every j / m' of the reduced ranges, 0 and 1 - 2^-53, every c0 != c1 for m <= 12 and seeded pairs above; equal to
    moves_restated.pick* on every element (-1 where m is below the draw's smallest size), which tests/test_commit_cases_cpu.py
    holds in range and distinct from c0 and c1.  One launch."""
    import commit_cases as cc
    u, m, c0, c1 = cc.pick_cases()
    got = probe.pick(u, m, c0, c1)
    assert np.array_equal(got, cc.pick_expected())
    one = np.ones(64)
    zero, out = np.zeros(64), np.full((64, 3), np.nan)
    for bad in ((one, one, zero, zero), (-one, one, zero, zero), (zero, zero, zero, zero), (zero, 2 * one, 2 * one, zero),
                (zero, 3 * one, one, one), (zero, 3 * one, -one, zero), (zero, 2.5 * one, zero, one), (np.full(64, np.nan), one, zero, zero)):
        assert probe.L.mpp_pick(*(_p(_in(a)) for a in bad), _p(out), 64) == -1 and np.all(np.isnan(out)), bad
