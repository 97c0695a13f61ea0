"""CPU tests of the Nelder-Mead simplex search: the numpy restatement of the device scheme (tests/nm_restated.py) against
scipy.optimize.minimize(method="Nelder-Mead") bit for bit, its independence of how a run is split, the Python front end
(magprop_amd.optimize.nelder_mead, differential_evolution(polish=)) checking its arguments before it touches a device, and the
raw ABI's names."""
import ctypes as C
import os
import re
import warnings

import numpy as np
import pytest
from scipy.optimize import minimize

import nm_restated as nm
from conftest import ROOT


def rosenbrock(P):
    P = np.asarray(P)
    f = np.sum(100.0 * (P[:, 1:] - P[:, :-1] ** 2) ** 2 + (1.0 - P[:, :-1]) ** 2, axis=1)
    return -f, np.zeros(len(P), dtype=np.int32)


TARGETS = {"gaussian": nm.gaussian, "terraced": nm.terraced, "rosenbrock": rosenbrock}
# boxes: "wide" never binds; "binding" cuts the optimum off (the Gaussians' at 0, Rosenbrock's at 1), so that the search ends on faces
BOXES = {"wide": (-50.0, 50.0), "binding": (0.3, 0.9)}


def _case(target, N, box, seed, outside=False):
    """(lower, upper, initial simplex): a random simplex inside the box; outside: partly beyond both bounds, for scipy's
    reflect-then-clip rule."""
    rng = np.random.default_rng(seed)
    lo, hi = np.full(N, BOXES[box][0]), np.full(N, BOXES[box][1])
    if box == "wide":
        sim = rng.uniform(-2.0, 2.0, (N + 1, N))
    else:
        sim = rng.uniform(lo - 0.3 * outside, hi + 0.3 * outside, (N + 1, N))
        if outside:
            sim[0, 0], sim[1, N - 1], sim[N, 0] = hi[0] + 0.2, lo[0] - 0.2, hi[0] + 0.7      # (the last reflects to below lower)
    return lo, hi, sim


def _both(target, N, adaptive, lo, hi, sim0, maxiter, xatol=1e-6, fatol=1e-6):
    fn = TARGETS[target]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")            # (scipy warns when x0 lies outside the bounds)
        ref = minimize(lambda x: -fn(x[None, :])[0][0], sim0[0], method="Nelder-Mead", bounds=list(zip(lo, hi)),
                       options={"initial_simplex": sim0, "xatol": xatol, "fatol": fatol, "adaptive": adaptive, "maxiter": maxiter})
    s = nm.run(sim0[None], maxiter - 1, fn, *nm.coefficients(N, adaptive), lower=lo, upper=hi, xatol=xatol, fatol=fatol)
    return ref, s


CASES = [(t, N, a, b, False) for t in TARGETS for N in (2, 6, 9) for a in (False, True) for b in BOXES] + \
        [(t, N, a, "binding", True) for t in TARGETS for N in (2, 6) for a in (False, True)]
_seen = np.zeros(5, dtype=np.int64)


@pytest.mark.parametrize("target, N, adaptive, box, outside", CASES)
def test_restatement_equals_scipy_bit_for_bit(target, N, adaptive, box, outside):
    """final_simplex (vertices and values), nit and nfev of scipy's serial loop, for an iteration budget scipy exhausts in some
    cases and not in others."""
    lo, hi, sim0 = _case(target, N, box, 100 * N + 7 * adaptive + len(target), outside)
    if outside:
        assert np.any(sim0 > hi) and np.any(sim0 < lo)
    maxiter = 60 * N
    ref, s = _both(target, N, adaptive, lo, hi, sim0, maxiter)
    assert np.array_equal(ref.final_simplex[0], s.sim[0])
    assert np.array_equal(ref.final_simplex[1], -s.lnp[0])
    assert ref.nit == s.nit[0] and ref.nfev == s.nfev[0]
    assert ref.success == bool(s.stopped[0] and s.nit[0] < maxiter)
    assert s.outcomes[0].sum() == s.nit[0] - 1
    assert np.all((s.sim >= lo) & (s.sim <= hi))
    _seen[:] += s.outcomes[0]


def test_every_outcome_occurred_in_the_cases_above():
    """A condition on the cases, from the restatement that scipy has just confirmed: reflections, expansions, both contractions
    and shrinks all occur (run after the comparisons: pytest keeps the file's order)."""
    if _seen.sum() == 0:                 # this test selected alone: run the cases
        for c in CASES:
            test_restatement_equals_scipy_bit_for_bit(*c)
    assert np.all(_seen > 0), dict(zip(("reflect", "expand", "outside", "inside", "shrink"), _seen))


def test_ties_and_shrinks_on_the_terraced_target_follow_scipy():
    """The terraces make equal values: a simplex on one plateau, two vertices tied, against scipy (stable order of equal
    values, the replaced vertex last)."""
    N = 2
    lo, hi = np.full(N, -5.0), np.full(N, 5.0)
    sim0 = np.array([[0.5, 0.5], [0.5, -0.5], [0.51, 0.5]])
    assert nm.terraced(sim0)[0][0] == nm.terraced(sim0)[0][1]
    ref, s = _both("terraced", N, False, lo, hi, sim0, 80)
    assert np.array_equal(ref.final_simplex[0], s.sim[0]) and np.array_equal(ref.final_simplex[1], -s.lnp[0])
    assert ref.nit == s.nit[0] and ref.nfev == s.nfev[0]
    assert s.outcomes[0, nm.SHRINK] > 0


def test_a_run_in_pieces_equals_one_run():
    """Three simplexes of different fates (one stops early), 5 + 7 + 30 iterations against 42."""
    N = 3
    lo, hi = np.full(N, -4.0), np.full(N, 4.0)
    rng = np.random.default_rng(3)
    sim0 = rng.uniform(-2.0, 2.0, (3, N + 1, N))
    sim0[1] = 0.2 + 1e-3 * rng.random((N + 1, N))
    kw = dict(lower=lo, upper=hi, xatol=1e-2, fatol=1e-2)
    co = nm.coefficients(N)
    one = nm.run(sim0, 42, nm.terraced, *co, **kw)
    s = nm.run(sim0, 5, nm.terraced, *co, **kw)
    assert not np.all(s.stopped)
    s = nm.run(None, 7, nm.terraced, *co, **kw, state=s)
    s = nm.run(None, 30, nm.terraced, *co, **kw, state=s)
    for key in ("sim", "lnp", "status", "nit", "stopped", "nfev", "outcomes"):
        assert np.array_equal(getattr(one, key), getattr(s, key)), key
    assert len(set(one.nit)) > 1 and np.any(one.stopped)


def test_stop_rule_takes_nan_differences_as_not_stopped():
    sim = np.zeros((3, 2))
    assert nm.stop_rule(sim, np.array([-1.0, -1.0, -1.0]), 0.0, 0.0)
    assert not nm.stop_rule(sim, np.array([-1.0, -np.inf, -np.inf]), 1.0, 1.0)
    assert not nm.stop_rule(sim, np.array([-np.inf, -np.inf, -np.inf]), 1.0, 1.0)     # inf - inf
    assert not nm.stop_rule(sim + [[0, 0], [0, 0], [0, 2e-4]], np.array([-1.0, -1.0, -1.0]), 1e-4, 1e-4)


def test_front_end_builds_scipys_default_simplex_and_coefficients():
    from magprop_amd import optimize
    x0 = np.array([1.0, 0.0, -2.0])
    sim = optimize.default_simplex(x0)
    assert np.array_equal(sim, nm.default_simplex(x0))
    assert sim[1, 0] == 1.05 * 1.0 and sim[2, 1] == 0.00025 and sim[3, 2] == 1.05 * -2.0
    for N in (2, 6, 9):
        assert optimize.nm_coefficients(N, True) == nm.coefficients(N, True)
        assert optimize.nm_coefficients(N, False) == nm.coefficients(N, False) == (1.0, 2.0, 0.5, 0.5)


def _no_device(monkeypatch):
    from magprop_amd import _capi

    def no_device(*a, **k):
        raise AssertionError("the device was touched")

    for name in ("lib", "Handle", "Driver", "cfg_synth", "cfg_lib"):
        monkeypatch.setattr(_capi, name, no_device)


@pytest.mark.parametrize("kw, match", [
    ({"x0": np.zeros((2, 3, 6))}, "x0 must have shape"),
    ({"x0": np.zeros(5)}, "6 parameters"),
    ({"x0": np.full(6, np.nan)}, "x0 must be finite"),
    ({"x0": np.zeros((3, 6))}, "one start per simplex"),
    ({"bounds": [(0.0, 1.0)] * 5}, "one .* pair per coordinate"),
    ({"bounds": [(1.0, 0.0)] * 6}, "lower < upper"),
    ({"bounds": [(0.0, np.inf)] * 6}, "finite"),
    ({"variant": "lib", "x0": np.zeros(10)}, "6 to 9"),
    ({"variant": "other"}, "variant"),
    ({"xatol": -1.0}, "xatol"),
    ({"fatol": np.nan}, "fatol"),
    ({"maxiter": 0}, "maxiter"),
    ({"maxiter": 2.5}, "maxiter"),
    ({"n_starts": 0}, "n_starts"),
    ({"n_starts": 1025}, "at most"),
    ({"initial_simplex": np.zeros((6, 6))}, "initial_simplex must have shape"),
    ({"initial_simplex": np.full((7, 6), np.inf)}, "initial_simplex must be finite"),
])
def test_nelder_mead_checks_its_arguments_before_any_device_is_touched(monkeypatch, kw, match):
    from magprop_amd import optimize
    _no_device(monkeypatch)
    x = np.linspace(1.0, 10.0, 5)
    kw = dict({"x0": np.zeros(6)}, **kw)
    with pytest.raises(ValueError, match=match):
        optimize.nelder_mead(kw.pop("x0"), x, x, x, **kw)
    with pytest.raises(ValueError, match="dataset"):
        optimize.nelder_mead(np.zeros(6))


def test_polish_needs_enough_members_and_raises_before_any_device_is_touched(monkeypatch):
    from magprop_amd import optimize
    _no_device(monkeypatch)
    x = np.linspace(1.0, 10.0, 5)
    with pytest.raises(ValueError, match="too few"):
        optimize.differential_evolution(x, x, x, popsize=1, polish=True)


class _Stub:
    """Stands in for the library, the handle and the drivers: records what the front end passes down."""

    def __init__(self, members, ndim):
        self.members, self.ndim, self.drivers, self.calls = members, ndim, [], []

    def driver(self, name, handle, *args):
        self.drivers.append((name, args))
        return self

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def __getattr__(self, name):
        if not name.startswith("mp_"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append((name, args))
            return 0
        return call

    def opt_state(self, L, o, n_pops, members, ndim):
        rng = np.random.default_rng(0)
        lnp = -rng.random((n_pops, members))
        return {"pop": rng.random((n_pops, members, ndim)), "lnprob": lnp, "status": np.zeros((n_pops, members), dtype=np.int32),
                "best": np.argmax(lnp, axis=1).astype(np.int32), "nit": np.full(n_pops, 3, dtype=np.int32),
                "converged": np.ones(n_pops, dtype=np.int32), "nfev": np.full(n_pops, 4 * members, dtype=np.int64)}

    def simplex_state(self, L, s, n, ndim):
        sim0 = np.ctypeslib.as_array(self.calls[-2][1][1], shape=(n, ndim + 1, ndim)).copy()   # what set_vertices was handed
        self.sim0 = sim0
        lnp = np.tile(-np.arange(ndim + 1, dtype=np.float64), (n, 1))
        lnp[0] += 5.0                                   # simplex 0 improves on its population, the others do not
        lnp[1:] -= 5.0
        return {"sim": sim0 + 1.0, "lnprob": lnp, "status": np.zeros((n, ndim + 1), dtype=np.int32),
                "nit": np.full(n, 11, dtype=np.int32), "stopped": np.ones(n, dtype=np.int32),
                "nfev": np.full(n, 17, dtype=np.int64), "outcomes": np.ones((n, 5), dtype=np.int64)}


def _stubbed(monkeypatch, **kw):
    from magprop_amd import _capi, engine, optimize
    stub = _Stub(90, 6)
    monkeypatch.setattr(_capi, "lib", lambda: stub)
    monkeypatch.setattr(_capi, "Driver", stub.driver)
    monkeypatch.setattr(engine, "open_handle", lambda *a, **k: stub)
    monkeypatch.setattr(optimize, "get_state", stub.opt_state)
    monkeypatch.setattr(optimize, "get_simplex_state", stub.simplex_state)
    x = np.linspace(1.0, 10.0, 5)
    res = optimize.differential_evolution(datasets=[(x, x, x), (x, x, x)], seed=4, maxiter=7, **kw)
    return stub, res


def test_polish_false_passes_what_it_passes_today(monkeypatch):
    """The keyword exists, is off by default, and off means the optimizer's driver alone, with today's arguments and results."""
    from magprop_amd import _capi, synth
    for kw in ({}, {"polish": False}):
        stub, res = _stubbed(monkeypatch, **kw)
        assert [d[0] for d in stub.drivers] == ["mp_optimizer"]
        a = stub.drivers[0][1]
        assert a[:3] == (90, 2, 6) and a[4:11] == (4, _capi.DE_BEST1BIN, 0.5, 1.0, 0.7, 0.01, 0.0) and a[13] == 0
        assert np.array_equal(np.ctypeslib.as_array(a[3], shape=(2,)), [0, 1])
        assert np.array_equal(np.ctypeslib.as_array(a[11], shape=(6,)), synth.PRIOR_LOWER)
        assert [c[0] for c in stub.calls] == ["mp_optimizer_set_population", "mp_optimizer_run"]
        assert stub.calls[1][1][1:] == (7, None)
        st = stub.opt_state(None, None, 2, 90, 6)
        for p, r in enumerate(res):
            assert "polish" not in r and r.nfev == 360 and r.lnprob == st["lnprob"][p].max()
            assert np.array_equal(r.x, st["pop"][p, st["best"][p]])


def test_polish_true_starts_from_the_best_members_and_keeps_the_better_point(monkeypatch):
    stub, res = _stubbed(monkeypatch, polish=True)
    assert [d[0] for d in stub.drivers] == ["mp_optimizer", "mp_simplex"]
    a = stub.drivers[1][1]
    assert a[:2] == (2, 6) and a[3:9] == (1.0, 2.0, 0.5, 0.5, 1e-4, 1e-4) and a[11] == 0
    assert np.array_equal(np.ctypeslib.as_array(a[2], shape=(2,)), [0, 1])
    assert [c[0] for c in stub.calls][2:] == ["mp_simplex_set_vertices", "mp_simplex_run"]
    assert stub.calls[3][1][1:] == (200 * 6 - 1, None)
    st = stub.opt_state(None, None, 2, 90, 6)
    for p, r in enumerate(res):
        order = sorted(range(90), key=lambda i: (-st["lnprob"][p, i], i))[:7]
        assert np.array_equal(stub.sim0[p], st["pop"][p, order])
        assert r.nfev == 360 + 17 and r.polish.nit == 11 and r.polish.success
        assert r.polish.outcomes == dict(reflect=1, expand=1, outside=1, inside=1, shrink=1)
    # simplex 0 found a better point (lnprob 5 > every member's), simplex 1 did not (-5): scipy's rule keeps the better one
    assert res[0].lnprob == 5.0 == res[0].polish.lnprob and np.array_equal(res[0].x, res[0].polish.x) and res[0].fun == -5.0
    assert res[1].lnprob == st["lnprob"][1].max() > res[1].polish.lnprob == -5.0
    assert np.array_equal(res[1].x, st["pop"][1, st["best"][1]])


def test_raw_abi_names_and_null_arguments():
    """The header, the binding table and the library export the same five names; NULL arguments give MP_EINVAL."""
    from magprop_amd import _capi
    names = ["mp_simplex_create", "mp_simplex_set_vertices", "mp_simplex_run", "mp_simplex_get_state", "mp_simplex_destroy"]
    hdr = open(os.path.join(ROOT, "include", "magprop_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(set(re.findall(r"\b(mp_simplex_[a-z_]+)\s*\(", hdr))) == sorted(names)
    assert [n for n in _capi.EXPORTS if n.startswith("mp_simplex_")] == names
    L = _capi.lib()
    for n in names:
        assert hasattr(L, n)
    box = np.zeros(6)
    dp = C.POINTER(C.c_double)
    assert not L.mp_simplex_create(None, 1, 6, None, 1.0, 2.0, 0.5, 0.5, 1e-4, 1e-4, box.ctypes.data_as(dp), box.ctypes.data_as(dp), 0)
    assert "mp_simplex_create: NULL argument" in _capi.last_error()
    assert L.mp_simplex_set_vertices(None, None) == _capi.MP_EINVAL
    assert L.mp_simplex_run(None, 1, None) == _capi.MP_EINVAL
    assert L.mp_simplex_get_state(None, None, None, None, None, None, None, None) == _capi.MP_EINVAL
    assert L.mp_simplex_destroy(None) == _capi.MP_OK
