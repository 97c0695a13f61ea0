"""The path from samples to results of the model summaries (band, derived, flows, flow band, pointwise), held fixed: what every
front end of synth, mcmc_eqns and NestedSampler hands to the engine and to the Handle, and the dict it returns, against a recording
stand-in for the Handle.  No device and no library call.  (EnsembleSampler opens its device when constructed: its five front ends
are held by the GPU wiring tests.)"""
import warnings

import numpy as np
import pytest

from magprop_amd import _capi, derived, engine, flows, mcmc_eqns, nested, pointwise, synth

N_GRID, N_OBS, SLOT = 7, 3, 5
Q2 = (0.9, 0.1)


def _copy(a):
    return None if a is None else np.array(a, dtype=np.float64)


class RecordingHandle:
    """Handle's summary methods: every call recorded (copies of rows and weights), fixed seeded arrays of the right shapes
    returned and kept in .ret; the status vector mixes STATUS_OK with failures."""

    def __init__(self):
        self.tgrid = np.logspace(0.0, 1.0, N_GRID)
        self.calls, self.ret = [], None

    def dataset_size(self, ds_id):
        return N_OBS

    def _out(self, name, rows, seed, **rec):
        n = np.asarray(rows).shape[0]
        st = np.zeros(n, dtype=np.int32)
        st[1::3], st[2::5] = _capi.STATUS_FLAG, _capi.STATUS_PRIOR
        self.calls.append(dict(rec, name=name, rows=_copy(rows)))
        return np.random.default_rng(seed), st, int(np.sum(st == _capi.STATUS_OK))

    def model_band(self, pars, q, components=("Ltot",), physical=False, weights=None):
        rng, st, used = self._out("model_band", pars, 1, q=_copy(q), names=tuple(components), physical=physical, weights=_copy(weights))
        self.ret = (rng.standard_normal((len(components), len(q), N_GRID)), st, used)
        return self.ret

    def model_derived(self, pars, physical=False):
        rng, st, used = self._out("model_derived", pars, 2, physical=physical)
        v = rng.standard_normal((len(st), _capi.DERIVED_N))
        v[st != 0] = np.nan
        self.ret = (v, st, used)
        return self.ret

    def model_flows(self, pars, curves=(), physical=False):
        rng, st, used = self._out("model_flows", pars, 3, names=curves, physical=physical)
        v = rng.standard_normal((len(st), _capi.FLOW_N))
        v[st != 0] = np.nan
        _, names = _capi.flow_curve_args(curves)
        self.ret = (v, rng.standard_normal((len(st), len(names), N_GRID)) if names else None, st, used)
        return self.ret

    def model_flow_band(self, pars, q, curves=("fastness",), physical=False, weights=None):
        rng, st, used = self._out("model_flow_band", pars, 4, q=_copy(q), names=tuple(curves), physical=physical, weights=_copy(weights))
        self.ret = (rng.standard_normal((len(curves), len(q), N_GRID)), st, used)
        return self.ret

    def model_pointwise(self, pars, ds_id=0, physical=False, cells=False):
        rng, st, used = self._out("model_pointwise", pars, 5, ds_id=ds_id, physical=physical, cells=cells)
        m = pointwise.tail_len(len(st)) - 1
        assert used > m >= pointwise.MIN_TAIL
        tail = np.sort(rng.standard_normal((N_OBS, m + 1)), axis=1) + 3.0
        obs = np.abs(rng.standard_normal((N_OBS, _capi.POINTWISE_N))) + 0.5
        obs[:, pointwise.N_USED], obs[:, pointwise.NONTAIL_COUNT] = used, used - m
        obs[:, pointwise.CUT], obs[:, pointwise.R_MAX], obs[:, pointwise.NONTAIL_M] = tail[:, 0], tail[:, -1], tail[:, 0]
        self.ret = (obs, tail, st, used) + ((rng.standard_normal((N_OBS, len(st))),) if cells else ())
        return self.ret


class RecordingEngine:
    def __init__(self):
        self.handle, self.log = RecordingHandle(), []

    def set_prior(self, lower, upper, log_mask):
        self.log.append(("set_prior", _copy(lower), _copy(upper), log_mask))

    def dataset_slot(self, x, y, yerr):
        self.log.append(("dataset_slot", _copy(x), _copy(y), _copy(yerr)))
        return SLOT


@pytest.fixture
def eng(monkeypatch):
    """engine.acquire / release answered by one RecordingEngine (.acquired: (variant, GRBtype, device) per call; .released: calls);
    the two model configurations built without the library, marked 1 (synth) and 2 (lib) in their reserved field."""
    e = RecordingEngine()
    e.acquired, e.released = [], 0

    def acquire(cfg, GRBtype=None, device=-1):
        e.acquired.append((cfg.reserved, GRBtype, device))
        return e

    def release(got):
        assert got is e
        e.released += 1

    monkeypatch.setattr(engine, "acquire", acquire)
    monkeypatch.setattr(engine, "release", release)
    monkeypatch.setattr(_capi, "cfg_synth", lambda **kw: _capi.ModelCfg(reserved=1))
    monkeypatch.setattr(_capi, "cfg_lib", lambda **kw: _capi.ModelCfg(reserved=2))
    monkeypatch.setattr(synth, "_cfg_cache", {})
    return e


def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if a is None or b is None:
        return a is b
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _rows(n, ndim, seed=0):
    return np.random.default_rng(seed).standard_normal((n, ndim))


def _weights(n, seed=0):
    return np.exp(np.random.default_rng(100 + seed).standard_normal(n))


def _call(h):
    assert len(h.calls) == 1
    return h.calls.pop()


# ---------------------------------------------------------------- what each summary must return for what the Handle gave
def _want_band(h, names, weights=None, **extra):
    band, st, used = h.ret
    out = {"t": h.tgrid, **{c: band[k] for k, c in enumerate(names)}, "n_used": used}
    if weights is not None:
        out["n_eff"] = _capi.kish_n_eff(weights, st)
    return dict(out, **extra)


def _want_table(h, module, q, weights, names=()):
    values, status, used = h.ret[0], h.ret[-2], h.ret[-1]
    out = {"values": values, "status": status, "n_used": used, "summary": module.summarize(values, q, weights)}
    if names:
        out["t"] = h.tgrid
        out.update({c: h.ret[1][:, k] for k, c in enumerate(names)})
    return out


def _want_pointwise(h, x, cells):
    obs, tail, st, used = h.ret[:4]
    back = np.empty(N_OBS, dtype=int)
    back[np.argsort(x, kind="stable")] = np.arange(N_OBS)
    obs, tail = obs[back], tail[back]
    loo, w = pointwise.psis_loo(obs, tail), pointwise.waic(obs)
    out = {"obs": obs, "tail": tail, "status": st, "n_used": used, "loo": loo, "waic": w, "summary": pointwise.summarize({**w, **loo})}
    if cells:
        out["z"] = h.ret[4][back]
    return out


X, Y, YERR = np.array([30.0, 10.0, 20.0]), np.array([1.0, 2.0, 3.0]), np.array([0.1, 0.2, 0.3])   # (x not sorted)


def _check_engine(e, variant, GRBtype, device, prior, dataset=None):
    """One acquire of that engine, released once; the dataset (when one is given) registered before the prior is set."""
    assert e.acquired == [(variant, GRBtype, device)] and e.released == 1
    want = ([("dataset_slot",) + dataset] if dataset else []) + [("set_prior",) + prior]
    assert len(e.log) == len(want)
    for got, w in zip(e.log, want):
        assert got[0] == w[0] and all(_same(g, v) for g, v in zip(got[1:], w[1:]))
    e.acquired.clear()
    e.log.clear()
    e.released = 0


# ---------------------------------------------------------------- synth
SYNTH_PRIOR = (synth.PRIOR_LOWER, synth.PRIOR_UPPER, synth.LOG_MASK)


@pytest.mark.parametrize("weighted", [False, True])
def test_synth_bands(eng, weighted):
    h, p = eng.handle, _rows(5, 6)
    w = _weights(5) if weighted else None
    got = synth.model_band(p, weights=w)                                         # defaults
    c = _call(h)
    assert _same(c["rows"], p) and _same(c["q"], (0.025, 0.5, 0.975)) and c["names"] == ("Ltot",) and c["physical"] is False
    assert _same(c["weights"], w)
    assert _same(got, _want_band(h, ("Ltot",), w))
    assert list(got) == ["t", "Ltot", "n_used"] + (["n_eff"] if weighted else [])
    if weighted:
        assert got["n_eff"] == _capi.kish_n_eff(w, h.ret[1]) and 0.0 < got["n_eff"] < 5.0    # (over the rows that finished only)
    _check_engine(eng, 1, None, -1, SYNTH_PRIOR)
    got = synth.model_band(p.tolist(), q=Q2, components=("Ldip", "Ltot"), device=3, weights=w)
    c = _call(h)
    assert _same(c["rows"], p) and _same(c["q"], Q2) and c["names"] == ("Ltot", "Ldip") and _same(c["weights"], w)
    assert _same(got, _want_band(h, ("Ltot", "Ldip"), w)) and list(got)[:3] == ["t", "Ltot", "Ldip"]
    _check_engine(eng, 1, None, 3, SYNTH_PRIOR)

    got = synth.model_flow_band(p, weights=w)                                    # defaults
    c = _call(h)
    assert c["name"] == "model_flow_band" and _same(c["rows"], p) and _same(c["q"], (0.025, 0.5, 0.975))
    assert c["names"] == ("fastness",) and c["physical"] is False and _same(c["weights"], w)
    assert _same(got, _want_band(h, ("fastness",), w))
    _check_engine(eng, 1, None, -1, SYNTH_PRIOR)
    got = synth.model_flow_band(p, q=Q2, curves=("N_dip", "Rm", "Mdot_acc"), device=1, weights=w)
    c = _call(h)
    assert _same(c["q"], Q2) and c["names"] == ("Rm", "Mdot_acc", "N_dip") and _same(c["weights"], w)
    assert _same(got, _want_band(h, ("Rm", "Mdot_acc", "N_dip"), w))
    assert list(got) == ["t", "Rm", "Mdot_acc", "N_dip", "n_used"] + (["n_eff"] if weighted else [])
    _check_engine(eng, 1, None, 1, SYNTH_PRIOR)


@pytest.mark.parametrize("weighted", [False, True])
def test_synth_tables(eng, weighted):
    h, p = eng.handle, _rows(70, 6)
    w = _weights(70) if weighted else None
    got = synth.model_derived(p, weights=w)
    c = _call(h)
    assert c["name"] == "model_derived" and _same(c["rows"], p) and c["physical"] is False
    assert _same(got, _want_table(h, derived, (0.16, 0.5, 0.84), w)) and 0 < got["n_used"] < 70
    _check_engine(eng, 1, None, -1, SYNTH_PRIOR)
    assert _same(synth.model_derived(p, q=Q2, weights=w, device=2), _want_table(h, derived, Q2, w))
    _call(h)
    _check_engine(eng, 1, None, 2, SYNTH_PRIOR)

    got = synth.model_flows(p, weights=w)
    c = _call(h)
    assert c["name"] == "model_flows" and _same(c["rows"], p) and tuple(c["names"]) == () and c["physical"] is False
    assert _same(got, _want_table(h, flows, (0.16, 0.5, 0.84), w)) and list(got) == ["values", "status", "n_used", "summary"]
    _check_engine(eng, 1, None, -1, SYNTH_PRIOR)
    got = synth.model_flows(p, curves=("branch", "Rc", "fastness"), q=Q2, weights=w, device=2)
    c = _call(h)
    assert tuple(c["names"]) == ("branch", "Rc", "fastness")
    assert _same(got, _want_table(h, flows, Q2, w, ("Rc", "fastness", "branch")))
    assert list(got) == ["values", "status", "n_used", "summary", "t", "Rc", "fastness", "branch"]
    _check_engine(eng, 1, None, 2, SYNTH_PRIOR)


@pytest.mark.parametrize("cells", [False, True])
def test_synth_pointwise(eng, cells):
    h, p = eng.handle, _rows(70, 6)
    got = synth.model_pointwise(p, X, Y, YERR, device=1, cells=cells)
    c = _call(h)
    assert c["name"] == "model_pointwise" and _same(c["rows"], p) and c["ds_id"] == SLOT and c["physical"] is False
    assert bool(c["cells"]) is cells
    assert _same(got, _want_pointwise(h, X, cells))
    assert list(got) == ["obs", "tail", "status", "n_used", "loo", "waic", "summary"] + (["z"] if cells else [])
    assert not _same(got["obs"], h.ret[0])                               # (in the caller's order of x, not the library's)
    _check_engine(eng, 1, None, 1, SYNTH_PRIOR, (X, Y, YERR))


# ---------------------------------------------------------------- mcmc_eqns
DATA = {"t": X, "Lum50": Y, "Lum50err": YERR}


@pytest.mark.parametrize("ndim,GRBtype", [(6, "L"), (9, "S")])
def test_mcmc_eqns_front_ends(eng, ndim, GRBtype):
    h = eng.handle
    prior = (*mcmc_eqns._bounds(ndim), mcmc_eqns.LIB_LOG_MASK)
    assert prior[0].shape == (ndim,)
    p, big = _rows(5, ndim), _rows(70, ndim)
    for w in (None, _weights(5)):
        got = mcmc_eqns.model_band(p, GRBtype, weights=w)
        c = _call(h)
        assert _same(c["rows"], p) and _same(c["q"], (0.025, 0.5, 0.975)) and c["names"] == ("Ltot",) and c["physical"] is False
        assert _same(c["weights"], w) and _same(got, _want_band(h, ("Ltot",), w))
        _check_engine(eng, 2, GRBtype, -1, prior)
        got = mcmc_eqns.model_band(p, GRBtype, q=Q2, components=("Lprop", "Ltot"), weights=w, device=2)
        c = _call(h)
        assert _same(c["q"], Q2) and c["names"] == ("Ltot", "Lprop") and _same(got, _want_band(h, ("Ltot", "Lprop"), w))
        assert list(got) == ["t", "Ltot", "Lprop", "n_used"] + ([] if w is None else ["n_eff"])
        _check_engine(eng, 2, GRBtype, 2, prior)
    for w in (None, _weights(70)):
        got = mcmc_eqns.model_derived(big, GRBtype, q=Q2, weights=w)
        c = _call(h)
        assert c["name"] == "model_derived" and _same(c["rows"], big) and c["physical"] is False
        assert _same(got, _want_table(h, derived, Q2, w))
        _check_engine(eng, 2, GRBtype, -1, prior)
        got = mcmc_eqns.model_flows(big, GRBtype, curves=("Mdot_fb", "Rm"), weights=w, device=1)
        c = _call(h)
        assert c["name"] == "model_flows" and _same(c["rows"], big) and tuple(c["names"]) == ("Mdot_fb", "Rm")
        assert _same(got, _want_table(h, flows, (0.16, 0.5, 0.84), w, ("Rm", "Mdot_fb")))
        _check_engine(eng, 2, GRBtype, 1, prior)
        assert list(mcmc_eqns.model_flows(big, GRBtype, weights=w)) == ["values", "status", "n_used", "summary"]
        _call(h)
        _check_engine(eng, 2, GRBtype, -1, prior)
    for cells in (False, True):
        got = mcmc_eqns.model_pointwise(big, DATA, GRBtype, cells=cells)
        c = _call(h)
        assert c["name"] == "model_pointwise" and _same(c["rows"], big) and c["ds_id"] == SLOT and bool(c["cells"]) is cells
        assert _same(got, _want_pointwise(h, X, cells)) and ("z" in got) is cells
        _check_engine(eng, 2, GRBtype, -1, prior, (X, Y, YERR))


# ---------------------------------------------------------------- requests refused before any device is touched
def test_bad_requests_raise_before_the_engine_is_acquired(eng):
    p6, p9 = _rows(5, 6), _rows(5, 9)
    bad = [lambda: synth.model_band(p6, q=[1.5]), lambda: synth.model_band(p6, q=[]), lambda: synth.model_band(p6, components=("L",)),
           lambda: synth.model_band(p6[0]), lambda: synth.model_band(p6[:, :5]), lambda: synth.model_band(p6[:0]),
           lambda: synth.model_band(p6, weights=np.ones(4)), lambda: synth.model_band(p6, weights=[1, 1, np.nan, 1, 1]),
           lambda: synth.model_derived(p6[0]), lambda: synth.model_derived(p9),
           lambda: synth.model_flows(p6[0]), lambda: synth.model_flows(p9),
           lambda: synth.model_flow_band(p6, q=[-0.1]), lambda: synth.model_flow_band(p6[0]), lambda: synth.model_flow_band(p9),
           lambda: synth.model_flow_band(p6, weights=np.zeros(5)),
           lambda: synth.model_pointwise(p6[0], X, Y, YERR), lambda: synth.model_pointwise(p6[:, :5], X, Y, YERR),
           lambda: mcmc_eqns.model_band(p9, "L", q=[np.nan]), lambda: mcmc_eqns.model_band(p9[0], "L"),
           lambda: mcmc_eqns.model_band(p9[:, :5], "L"), lambda: mcmc_eqns.model_band(_rows(5, 10), "L"),
           lambda: mcmc_eqns.model_band(p9, "L", weights=np.ones((5, 1))),
           lambda: mcmc_eqns.model_derived(p9[0], "L"), lambda: mcmc_eqns.model_derived(_rows(5, 10), "L"),
           lambda: mcmc_eqns.model_flows(p9[0], "L"), lambda: mcmc_eqns.model_flows(p9[:, :5], "L"),
           lambda: mcmc_eqns.model_pointwise(p9[0], DATA, "L"), lambda: mcmc_eqns.model_pointwise(_rows(5, 10), DATA, "L")]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
        assert eng.acquired == [] and eng.handle.calls == [], k
    with pytest.raises(ValueError, match="2-D"):
        synth.model_derived(p6[0])
    with pytest.raises(ValueError, match="samples must be 2-D"):
        synth.model_pointwise(p6[:, :5], X, Y, YERR)
    with pytest.raises(ValueError, match="16384"):
        synth.model_band(np.zeros((16385, 6)))
    assert eng.acquired == []


def test_the_engine_is_released_when_the_handle_raises(eng, monkeypatch):
    def boom(*a, **kw):
        raise _capi.MagpropAmdError("boom")
    for name in ("model_band", "model_derived", "model_flows", "model_flow_band", "model_pointwise"):
        monkeypatch.setattr(eng.handle, name, boom)
    p = _rows(5, 6)
    calls = [lambda: synth.model_band(p), lambda: synth.model_derived(p), lambda: synth.model_flows(p), lambda: synth.model_flow_band(p),
             lambda: synth.model_pointwise(p, X, Y, YERR), lambda: mcmc_eqns.model_band(p, "L"), lambda: mcmc_eqns.model_derived(p, "L"),
             lambda: mcmc_eqns.model_flows(p, "L"), lambda: mcmc_eqns.model_pointwise(p, DATA, "L")]
    for k, call in enumerate(calls):
        with pytest.raises(_capi.MagpropAmdError, match="boom"):
            call()
        assert len(eng.acquired) == eng.released == k + 1


# ---------------------------------------------------------------- NestedSampler: its handle and results are public attributes
def _nested(n, n_runs=1, seed=0):
    s = nested.NestedSampler(X, Y, YERR, nlive=64, n_runs=n_runs, seed=7)
    s.handle = RecordingHandle()
    runs = [nested.Results(samples=_rows(n, 6, seed + r), logwt=np.random.default_rng(50 + seed + r).standard_normal(n))
            for r in range(n_runs)]
    s.results = runs[0] if n_runs == 1 else runs
    return s, runs


def test_nested_bands():
    s, (r,) = _nested(5)
    h = s.handle
    eq = nested.resample_equal(r.samples, r.logwt, 7)
    rows, w, dropped = nested.band_exact_selection(r.samples, r.logwt)
    assert rows.shape == (5, 6) and dropped == 0.0
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = s.get_model_band()                                                 # weights="resample"
        c = _call(h)
        assert c["name"] == "model_band" and _same(c["rows"], eq) and c["weights"] is None and c["physical"] is False
        assert _same(c["q"], (0.025, 0.5, 0.975)) and c["names"] == ("Ltot",)
        assert _same(got, _want_band(h, ("Ltot",))) and list(got) == ["t", "Ltot", "n_used"]
        got = s.get_model_band(q=Q2, components=("Ldip", "Lprop"), weights="exact")
        c = _call(h)
        assert _same(c["rows"], rows) and _same(c["weights"], w) and _same(c["q"], Q2) and c["names"] == ("Lprop", "Ldip")
        assert _same(got, _want_band(h, ("Lprop", "Ldip"), w, weight_dropped=0.0))
        assert list(got) == ["t", "Lprop", "Ldip", "n_used", "n_eff", "weight_dropped"]

        got = s.get_flow_band()                                                  # weights="exact"
        c = _call(h)
        assert c["name"] == "model_flow_band" and _same(c["rows"], rows) and _same(c["weights"], w) and c["names"] == ("fastness",)
        assert _same(c["q"], (0.025, 0.5, 0.975)) and c["physical"] is False
        assert _same(got, _want_band(h, ("fastness",), w, weight_dropped=0.0))
        assert list(got) == ["t", "fastness", "n_used", "n_eff", "weight_dropped"]
        got = s.get_flow_band(q=Q2, curves=("N_acc", "Rlc"), weights="resample")
        c = _call(h)
        assert _same(c["rows"], eq) and c["weights"] is None and _same(c["q"], Q2) and c["names"] == ("Rlc", "N_acc")
        assert _same(got, _want_band(h, ("Rlc", "N_acc"))) and list(got) == ["t", "Rlc", "N_acc", "n_used"]


def test_nested_bands_cut_at_the_cap(monkeypatch):
    """More samples than a band takes: weights="exact" keeps the heaviest, reports weight_dropped and warns; "resample" thins."""
    s, (r,) = _nested(9)
    h = s.handle
    monkeypatch.setattr(_capi, "BAND_MAX_SAMPLES", 4)
    rows, w, dropped = nested.band_exact_selection(r.samples, r.logwt, cap=4)
    assert rows.shape == (4, 6) and dropped > 1.0e-3
    eq = nested.resample_equal(r.samples, r.logwt, 7)[np.linspace(0, 8, 4).astype(int)]
    for front, name, default in ((s.get_model_band, "Ltot", {}), (s.get_flow_band, "fastness", {})):
        with pytest.warns(RuntimeWarning, match="4 heaviest samples leave"):
            got = front(weights="exact")
        c = _call(h)
        assert _same(c["rows"], rows) and _same(c["weights"], w)
        assert _same(got, _want_band(h, (name,), w, weight_dropped=dropped)) and got["weight_dropped"] == dropped
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            got = front(weights="resample")
        c = _call(h)
        assert _same(c["rows"], eq) and c["weights"] is None and _same(got, _want_band(h, (name,)))


def test_nested_tables_take_every_sample_under_its_weight():
    s, runs = _nested(70, n_runs=2)
    h = s.handle
    for run, r in enumerate(runs):
        w = np.exp(r.logwt - np.max(r.logwt))
        got = s.get_derived(run=run)
        c = _call(h)
        assert c["name"] == "model_derived" and _same(c["rows"], r.samples) and c["physical"] is False
        assert _same(got, _want_table(h, derived, (0.16, 0.5, 0.84), w))
        assert _same(s.get_derived(q=Q2, run=run), _want_table(h, derived, Q2, w))
        _call(h)
        got = s.get_flows(run=run)
        c = _call(h)
        assert c["name"] == "model_flows" and _same(c["rows"], r.samples) and tuple(c["names"]) == () and c["physical"] is False
        assert _same(got, _want_table(h, flows, (0.16, 0.5, 0.84), w))
        got = s.get_flows(q=Q2, run=run, curves=("N_dip", "Rm"))
        c = _call(h)
        assert tuple(c["names"]) == ("N_dip", "Rm") and _same(got, _want_table(h, flows, Q2, w, ("Rm", "N_dip")))
        assert list(got) == ["values", "status", "n_used", "summary", "t", "Rm", "N_dip"]
    assert not _same(runs[0].samples, runs[1].samples)


def test_nested_checks_fail_in_their_order():
    s = nested.NestedSampler(X, Y, YERR, nlive=64)
    s.handle = RecordingHandle()
    for front in (s.get_model_band, s.get_flow_band):
        with pytest.raises(ValueError, match="'resample' or 'exact'"):       # before "run_nested first"
            front(weights="nope")
        for weights in ("resample", "exact"):
            with pytest.raises(ValueError, match="run_nested first"):
                front(weights=weights)
    for front in (s.get_derived, s.get_flows):
        with pytest.raises(ValueError, match="run_nested first"):
            front()
    s.results = nested.Results(samples=_rows(5, 6), logwt=np.zeros(5))
    for front in (s.get_model_band, s.get_flow_band, s.get_derived, s.get_flows):
        with pytest.raises(ValueError, match="run must be 0 .. 0"):
            front(run=1)
    g = nested.NestedSampler(nlive=64, target="gaussian", bounds=[(-1.0, 1.0)] * 2)   # before either
    for front, what in ((g.get_model_band, "light curve"), (g.get_flow_band, "trajectory")):
        with pytest.raises(ValueError, match=f"{front.__name__} needs the posterior target: the gaussian target has no {what}"):
            front(weights="nope")
    for front, what in ((g.get_derived, "light curve"), (g.get_flows, "trajectory")):
        with pytest.raises(ValueError, match=f"{front.__name__} needs the posterior target: the gaussian target has no {what}"):
            front()
    assert s.handle.calls == []
