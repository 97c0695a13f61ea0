"""What the four resident drivers besides the ensemble sampler share (mp_host.h: Resident, resident_destroy, the entry macros,
run_chunked, groups_running, check_inside), asserted once for all of them through the raw C ABI: mp_optimizer_*, mp_nested_*,
mp_simplex_* and mp_smc_* on the unit Gaussian (target 1: no model is evaluated) in the box [-5, 5]^2, each at the smallest size
its create function takes, two groups each.  Every comparison of states is bit for bit."""
import ctypes as C

import numpy as np
import pytest

from raw_abi import dp, synth_handle

pytestmark = pytest.mark.gpu

NDIM, GROUPS, SEED, LARGE = 2, 2, 20261020, 100000
LO, HI = np.full(NDIM, -5.0), np.full(NDIM, 5.0)
F8, I4, I8 = np.float64, np.int32, np.int64
G = GROUPS

# per driver: the prefix of its functions, its set function, the rows of a group that the set function takes, the arguments of
# create between the handle and the box (after it for the SMC sampler), and get_state's outputs in argument order
DRIVERS = {
    "optimizer": dict(prefix="mp_optimizer", set="set_population", rows=5,
                      create=lambda L, h: L.mp_optimizer_create(h, 5, G, NDIM, None, SEED, 0, 0.5, 1.0, 0.7, 0.01, 1e-3, dp(LO), dp(HI), 1),
                      state=[("pop", (G, 5, NDIM), F8), ("lnprob", (G, 5), F8), ("status", (G, 5), I4), ("best", G, I4),
                             ("nit", G, I4), ("converged", G, I4), ("nfev", G, I8)]),
    "nested": dict(prefix="mp_nested", set="set_live", rows=16,
                   create=lambda L, h: L.mp_nested_create(h, 16, 1, G, NDIM, None, SEED, 5, 0.0, 0.1, 0.01, dp(LO), dp(HI), 1),
                   state=[("live", (G, 16, NDIM), F8), ("lnl", (G, 16), F8), ("status", (G, 16), I4), ("acc", (G, 16), I4),
                          ("nit", G, I4), ("stopped", G, I4), ("lnx", G, F8), ("lnz", G, F8), ("ncall", G, I8), ("nacc", G, I8),
                          ("nzero", G, I8)]),
    "simplex": dict(prefix="mp_simplex", set="set_vertices", rows=NDIM + 1,
                    create=lambda L, h: L.mp_simplex_create(h, G, NDIM, None, 1.0, 2.0, 0.5, 0.5, 1e-4, 1e-4, dp(LO), dp(HI), 1),
                    state=[("sim", (G, NDIM + 1, NDIM), F8), ("lnprob", (G, NDIM + 1), F8), ("status", (G, NDIM + 1), I4),
                           ("nit", G, I4), ("stopped", G, I4), ("nfev", G, I8), ("outcomes", (G, 5), I8)]),
    "smc": dict(prefix="mp_smc", set="set_particles", rows=16,
                create=lambda L, h: L.mp_smc_create(h, 16, G, NDIM, None, SEED, dp(LO), dp(HI), 0.5, 4, 0.0, 0.1, 1),
                state=[("x", (G, 16, NDIM), F8), ("lnl", (G, 16), F8), ("status", (G, 16), I4), ("acc", (G, 16), I4),
                       ("beta", G, F8), ("lnz", G, F8), ("nstage", G, I4), ("run_status", G, I4), ("ncall", G, I8),
                       ("nacc", G, I8), ("nfail", G, I8)]),
}
FLAG = {"optimizer": "converged", "nested": "stopped", "simplex": "stopped", "smc": "run_status"}


class Raw:
    """One driver object of DRIVERS[kind] on handle h; run() returns (code, n_running)."""

    def __init__(self, kind, h):
        from magprop_amd import _capi
        self.cap, self.L, self.d = _capi, _capi.lib(), DRIVERS[kind]
        self.obj = self.d["create"](self.L, h._h)
        assert self.obj, _capi.last_error()

    def fn(self, name):
        return getattr(self.L, f"{self.d['prefix']}_{name}")

    def set(self, points):
        return self.fn(self.d["set"])(self.obj, dp(np.ascontiguousarray(points, dtype=np.float64)))

    def run(self, limit):
        n = C.c_int32(-1)
        return self.fn("run")(self.obj, limit, C.byref(n)), n.value

    def state(self):
        st = self.cap.read_back(self.fn("get_state"), self.obj, self.d["state"])
        if self.d["prefix"] == "mp_nested":                       # the dead rows, which mp_nested_run files per chunk
            from magprop_amd import nested
            for r in range(GROUPS):
                st[f"dead{r}"] = np.concatenate([a.ravel().astype(F8) for a in nested.get_dead(self.L, self.obj, r, NDIM)])
        return st

    def close(self):
        assert self.fn("destroy")(self.obj) == self.cap.MP_OK


def same(a, b):
    return a.keys() == b.keys() and all(a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes() for k in a)


class Case:
    """A driver kind on a handle of its own: start(), a fresh driver set to the case's starting points, and whole, the state behind
    one run of it with a large limit (made once)."""

    def __init__(self, kind):
        self.kind, self.h, self._whole = kind, synth_handle(), None
        rows = DRIVERS[kind]["rows"]
        self.points = LO + (HI - LO) * np.random.default_rng(SEED).random((GROUPS * rows, NDIM))

    def start(self):
        r = Raw(self.kind, self.h)
        assert r.set(self.points) == r.cap.MP_OK, r.cap.last_error()
        return r

    @property
    def whole(self):
        if self._whole is None:
            r = self.start()
            code, running = r.run(LARGE)
            assert code == r.cap.MP_OK and running == 0, (code, running, r.cap.last_error())
            self._whole = r.state()
            r.close()
        return self._whole


@pytest.fixture(scope="module", params=list(DRIVERS))
def case(request):
    c = Case(request.param)
    yield c
    c.h.close()


def test_entry_refusals(case):
    """destroy(NULL) is MP_OK; run and get_state before the set call are MP_ESTATE and name it; the two setters that check the box
    refuse a point one ulp outside it with MP_EINVAL and leave the driver without a state."""
    r = Raw(case.kind, case.h)
    ok, estate, einval = r.cap.MP_OK, r.cap.MP_ESTATE, r.cap.MP_EINVAL
    set_fn = f"{r.d['prefix']}_{r.d['set']}"
    try:
        assert r.fn("destroy")(None) == ok
        assert r.run(1)[0] == estate and set_fn in r.cap.last_error()
        assert r.fn("get_state")(r.obj, *[None] * len(r.d["state"])) == estate and set_fn in r.cap.last_error()
        if case.kind in ("nested", "smc"):
            for edge, bound in ((np.nextafter(5.0, np.inf), 1), (np.nextafter(-5.0, -np.inf), 0)):
                bad = case.points.copy()
                bad[-1, bound] = edge
                assert r.set(bad) == einval and "outside the box" in r.cap.last_error()
                assert r.run(1)[0] == estate
            on_edge = case.points.copy()
            on_edge[-1] = [-5.0, 5.0]
            assert r.set(on_edge) == ok, r.cap.last_error()
    finally:
        r.close()


def test_run_limits(case):
    """run(0) changes nothing and reports every group running; a run with a large limit ends with none running (Case.whole), every
    group's flag non-zero; a further run reports 0 and changes nothing."""
    r = case.start()
    try:
        before = r.state()
        assert r.run(0) == (r.cap.MP_OK, GROUPS) and same(r.state(), before)
        assert r.run(LARGE) == (r.cap.MP_OK, 0)
        after = r.state()
        assert same(after, case.whole) and not same(after, before) and np.all(after[FLAG[case.kind]] != 0)
        for limit in (0, 1, LARGE):
            assert r.run(limit) == (r.cap.MP_OK, 0) and same(r.state(), after)
    finally:
        r.close()


def test_a_split_run_equals_one_run(case):
    """Limits of 1, then 3, then the rest, from the same start: the state of the one run."""
    whole = case.whole
    r = case.start()
    try:
        counts = [r.run(limit) for limit in (1, 3, LARGE)]
        assert all(code == r.cap.MP_OK for code, _ in counts) and counts[-1][1] == 0
        assert all(0 <= n <= GROUPS for _, n in counts)
        assert same(r.state(), whole)
    finally:
        r.close()
