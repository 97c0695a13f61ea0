"""GPU tests of observation scoring on its own (run with -m gpu on an MI355X): every route by which walker_eval
(magprop_amd/csrc/mp_eval.hpp) turns a digested light curve into chi^2, on the crafted light curves of tests/scoring_cases.py,
against exact interpolation of the curve the device itself returns.

Two handles in sampler coordinates under the prior box: `short` holds only the cases of up to 64 points (the builds without the
long path, the on-knots route), `long` holds every case (the LONG builds, which then score the short cases too).  Both fill all
MP_MAX_DATASETS slots, so that obs_off and tile_off are non-zero for all but the first; the long handle has four cases more
than slots, which replace its first four slots in a second pass (another length: the arena is rebuilt), and every row of a slot
that was not replaced must then come back with the same bits.  Each pass is one mode-A and one mode-B launch per build, the
build chosen by the launch size: up to n_simd / 4 rows a team with a SIMD per wavefront, up to n_simd / 2 a team two
wavefronts per SIMD, up to n_simd four steps per lane, beyond two steps per lane (at a size where the curve kernel takes two as
well).  Rows: slot r mod 64, and pass r div 64 picks the walker, the even passes one of the three walkers around the truth the
case was drawn from (tests/test_scoring_cases_cpu.py states the sensitivity of a case for those).

Link 1, mode B against its own curve: z = pointwise_restated.cells(Ltot row, restated digest), lnp_ref = -sum z^2 / 2 in long
double, |lnp_B - lnp_ref| <= sum 8 eps (|z| |mod| / yerr + z^2): the bound tests/test_gpu_pointwise.py derives for these two
paths (only the division by 1e50 and the FMA round differently).
Link 2, every mode-A build against mode B of the same tile length and the same rows: B(delta) = sum delta |z| |mod| / yerr + the
sum above, delta = 1e-12 for the one-wavefront builds against the curve kernel of the same steps per lane (what
test_mode_b_batched_light_curves asserts), 1e-11 for the team builds against the 4-steps-per-lane curve kernel (what
test_batch_size_does_not_change_a_walker asserts across these builds).  Statuses are equal.

Each test prints its worst error / bound per build and link (SCORING-MAX) and its wall time."""
import time

import numpy as np
import pytest

import pointwise_restated as pr
import scoring_cases as sc
from test_pointwise_cases_cpu import same

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
L = np.longdouble
SLOTS = 64
DELTA_SAME, DELTA_TEAM = 1.0e-12, 1.0e-11
_DIG = {}


def digest(c):
    if c.name not in _DIG:
        _DIG[c.name] = sc.digested(c)
    return _DIG[c.name]


@pytest.fixture(scope="module")
def walkers():
    P, lower, upper = sc.walkers()
    assert P.shape == (24, 6) and np.all(P > lower) and np.all(P < upper)
    return P, lower, upper


def make_handle(walkers, tarr, slot_case, strict):
    from magprop_amd import _capi
    assert _capi.MAX_DATASETS == SLOTS == len(slot_case)
    kw = dict(sweep_tol=_capi.SWEEP_TOL_STRICT, max_stride=1) if strict else {}
    h = _capi.Handle(_capi.cfg_synth(**kw), tarr)
    h.set_prior(walkers[1], walkers[2], sc.LOG_MASK)
    for s, c in enumerate(slot_case):
        h.set_dataset(s, c.x, c.y, c.yerr)
    return h


def sizes(h):
    """[(rows, build, delta)] of the four builds, by the rule of mp_device.h (walker_variant, kernel_spl_curves)"""
    from magprop_amd import _capi
    ns = h.n_simd
    n2 = next(n for n in range(ns + ns // 8, 2 * ns) if _capi.curve_steps_per_lane(n, ns) == 2)
    assert ns % 256 == 0 and n2 <= ns + ns // 2
    return [(ns // 4, "team, a SIMD per wavefront", DELTA_TEAM), (ns // 2, "team, two wavefronts per SIMD", DELTA_TEAM),
            (ns, "four steps per lane", DELTA_SAME), (n2, "two steps per lane", DELTA_SAME)]


def layout(n, slot_case):
    """(ds_id[n], walker[n]): slot r mod 64; the even passes over the slots take a walker around the case's own truth, the odd ones
    another by the pass and the length of the case (cases that are one set in another order get the same walkers)"""
    r = np.arange(n)
    slot, p = r % SLOTS, r // SLOTS
    w = np.empty(n, dtype=np.int64)
    for i in range(n):
        c = slot_case[slot[i]]
        w[i] = sc.own_walkers(c)[(p[i] // 2) % 3] if p[i] % 2 == 0 else (11 * p[i] + c.x.size) % 24
    return slot.astype(np.int32), w


def check_launch(h, P, slot_case, n, delta, worst):
    """one mode-A and one mode-B launch of n rows; both links, the one-hot sets and the degenerate values per slot.  Returns
    (ids, lnp_A, lnp_B, status) and updates worst = [link 1, link 2, one-hot] error / bound."""
    from magprop_amd import _capi
    ids, w = layout(n, slot_case)
    rows_P = P[w]
    lnp_a, st_a = h.lnprob_batch(rows_P, ds_id=ids, want_status=True)
    lnp_b, st_b, lt = h.lnprob_batch(rows_P, ds_id=ids, want_status=True, want_ltot=True)
    assert np.array_equal(st_a, st_b), np.nonzero(st_a != st_b)[0][:8]
    assert np.all(lnp_a[st_a != 0] == -np.inf) and np.all(lnp_b[st_b != 0] == -np.inf)
    # (a row whose model did not finish is NaN; one whose chi^2 is not finite keeps its curve)
    assert np.all(np.isnan(lt[(st_b != 0) & (st_b != _capi.STATUS_NONFINITE)]))
    for s, c in enumerate(slot_case):
        rows = np.nonzero(ids == s)[0]
        g, dx, idt, y, yerr, _ = digest(c)
        kind, at = c.reach.get("degenerate", (None, None))
        if kind in ("yerr0", "ynan"):
            # chi^2 is inf or NaN for every walker inside the prior: -inf, MP_STATUS_NONFINITE, on every build and in mode B
            assert np.all(st_a[rows] == _capi.STATUS_NONFINITE), (c.name, st_a[rows])
            continue
        ok = st_b[rows] == 0
        own = np.isin(w[rows], sc.own_walkers(c))
        assert np.all(ok[own]) and ok.sum() >= 0.75 * rows.size, (c.name, st_b[rows])
        rows = rows[ok]
        aerr = np.abs(yerr)                                                   # (a negative yerr scores as its absolute value)
        z = pr.cells(lt[rows], st_b[rows], g, dx, idt, y, aerr)               # [n_obs][rows]; yerr = inf: exactly 0
        assert np.all(np.isfinite(z))
        with np.errstate(invalid="ignore"):
            mod = y[:, None] - z * aerr[:, None]
        ref = -0.5 * np.sum(z.astype(L) ** 2, axis=0)
        b1, b2 = sc.bound(z, mod, aerr, 0.0), sc.bound(z, mod, aerr, delta)
        e1 = np.abs(lnp_b[rows].astype(L) - ref).astype(np.float64)
        e2 = np.abs(lnp_a[rows] - lnp_b[rows])
        assert np.all(e1 <= b1), (c.name, "link 1", n, w[rows][e1 > b1], (e1 / b1).max())
        assert np.all(e2 <= b2), (c.name, "link 2", n, w[rows][e2 > b2], (e2 / b2).max())
        pos = b1 > 0.0
        if np.any(pos):
            worst[0] = max(worst[0], float(np.max(e1[pos] / b1[pos])))
            worst[1] = max(worst[1], float(np.max(e2[pos] / b2[pos])))
        if "hot" in c.reach:                                                  # lnprob = -z_k^2 / 2 within the bound of that one cell
            k = c.reach["hot"]
            refk = -0.5 * z[k].astype(L) ** 2
            for lnp, d in ((lnp_a, delta), (lnp_b, 0.0)):
                bk = sc.bound(z[k:k + 1], mod[k:k + 1], aerr[k:k + 1], d)
                ek = np.abs(lnp[rows].astype(L) - refk).astype(np.float64)
                assert np.all(ek <= bk), (c.name, "one-hot", n, d, ek / bk)
                worst[2] = max(worst[2], float(np.max(ek / bk)))
    # one set in another order: the same bits (no times tie)
    names = [c.name for c in slot_case]
    if "order_asc" in names:
        a = ids == names.index("order_asc")
        for other in ("order_rev", "order_shuf"):
            o = ids == names.index(other)
            assert np.array_equal(w[a], w[o]) and same(lnp_a[a], lnp_a[o]) and same(lnp_b[a], lnp_b[o]), other
    return ids, lnp_a, lnp_b, st_a


@pytest.mark.parametrize("policy", ["default", "strict"])
@pytest.mark.parametrize("which", ["short", "long"])
def test_every_build_against_exact_interpolation_of_the_device_curve(walkers, tarr, which, policy):
    t0 = time.time()
    P = walkers[0]
    if which == "short":
        cs = sc.short_cases()
        assert all(c.x.size <= 64 for c in cs) and 20 <= len(cs) <= SLOTS
        slot_case = [cs[s % len(cs)] for s in range(SLOTS)]
        # (one slot replaced by a case of another length: the on-knots set by the 64 observations of one interval)
        late = {slot_case.index(sc.case("knots_interior")): sc.case("one_g5003_n64")}
    else:
        cs = sc.cases()
        assert SLOTS < len(cs) <= SLOTS + 8 and max(c.x.size for c in cs) == 1944
        slot_case = cs[:SLOTS]
        late = {s: c for s, c in enumerate(cs[SLOTS:])}
        assert all(slot_case[s].x.size != c.x.size for s, c in late.items())
    h = make_handle(walkers, tarr, slot_case, policy == "strict")
    try:
        first = {}
        for n, build, delta in sizes(h):
            worst = [0.0, 0.0, 0.0]
            first[n] = check_launch(h, P, slot_case, n, delta, worst)
            print(f"SCORING-MAX {which} {policy} rows {n} ({build}): link 1 {worst[0]:.3f}, link 2 at {delta:g} {worst[1]:.3f}, one-hot {worst[2]:.3f}")
        # the second pass: slots replaced (the arena is rebuilt), every other slot's rows come back with the same bits
        again = list(slot_case)
        for s, c in late.items():
            h.set_dataset(s, c.x, c.y, c.yerr)
            again[s] = c
        for n, build, delta in sizes(h) if which == "long" else sizes(h)[::3]:
            worst = [0.0, 0.0, 0.0]
            ids, lnp_a, lnp_b, st = check_launch(h, P, again, n, delta, worst)
            keep = ~np.isin(ids, list(late))
            ids0, a0, b0, st0 = first[n]
            # (the walker of a row goes by the length of its slot's case: the kept slots' rows are the same rows)
            assert np.array_equal(ids, ids0) and np.array_equal(st[keep], st0[keep])
            assert same(lnp_a[keep], a0[keep]) and same(lnp_b[keep], b0[keep])
            print(f"SCORING-MAX {which} {policy} rows {n} ({build}), slots replaced: link 1 {worst[0]:.3f}, link 2 at {delta:g} {worst[1]:.3f}")
    finally:
        h.close()
    print(f"SCORING-TIME {which} {policy}: {time.time() - t0:.2f} s")


def test_pointwise_cells_of_the_crafted_cases(walkers, tarr):
    """mp_model_pointwise(cells=True) reads the same digested arrays: its cells equal the restated cells of mp_model_lc's row bit
    for bit, on a handle in physical units as in tests/test_gpu_pointwise.py (the device's 10^x and numpy's need not agree to the
    bit), for the 65-, 129- and 312-point cases, the one-hot sets and the degenerate values (yerr = 0: +-inf, y = NaN: NaN,
    yerr = inf: 0, a negative yerr: the sign of z turned)."""
    from magprop_amd import _capi
    from test_gpu_derived import PHYS_LOWER, PHYS_UPPER
    t0 = time.time()
    names = ["size_65", "size_129", "bucket_boundaries"] + [f"one_hot_{k}" for k in sc.ONE_HOT] + \
            [f"deg_{kind}_{n}" for n in (50, 65) for kind in ("yerr0", "yerrinf", "ynan", "yerrneg")]
    P = np.clip(sc.unlog(walkers[0]), PHYS_LOWER, PHYS_UPPER)
    h = _capi.Handle(_capi.cfg_synth(), tarr)
    try:
        h.set_prior(PHYS_LOWER, PHYS_UPPER, 0)
        for s, name in enumerate(names):
            c = sc.case(name)
            h.set_dataset(s, c.x, c.y, c.yerr)
        rows = [h.model_lc(p) for p in P]
        st_lc = np.array([r[0] for r in rows], dtype=np.int32)
        lt = np.array([r[1][1] for r in rows])
        assert np.sum(st_lc == 0) >= 20
        for s, name in enumerate(names):
            c = sc.case(name)
            g, dx, idt, y, yerr, _ = digest(c)
            obs, tail, st, used, z = h.model_pointwise(P, ds_id=s, cells=True)
            assert np.array_equal(st, st_lc) and used == int(np.sum(st == 0)) and z.shape == (c.x.size, len(P))
            want = pr.cells(lt, st_lc, g, dx, idt, y, yerr)
            assert same(z, want), (name, np.argwhere(~((z == want) | (np.isnan(z) & np.isnan(want))))[:5])
            kind, at = c.reach.get("degenerate", (None, None))
            fin = st == 0
            if kind == "yerr0":
                assert np.all(np.isinf(z[at, fin]))
            elif kind == "ynan":
                assert np.all(np.isnan(z[at])) and np.all(np.isfinite(np.delete(z, at, axis=0)[:, fin]))
            elif kind == "yerrinf":
                assert np.all(z[at, fin] == 0.0)
            elif kind == "yerrneg":
                twin = pr.cells(lt, st_lc, g, dx, idt, y, np.abs(yerr))
                assert same(z[at], -twin[at]) and same(np.delete(z, at, axis=0), np.delete(twin, at, axis=0))
    finally:
        h.close()
    print(f"SCORING-TIME pointwise cells: {time.time() - t0:.2f} s")
