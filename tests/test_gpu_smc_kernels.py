"""The stage kernel of the SMC sampler (magprop_amd/csrc/mp_smc.hip smc_stage_kernel) on crafted lnl vectors, reached through
the probe library libmp_probe_smc.so (csrc/mp_probe_smc.hip), which is test infrastructure, no part of the product's ABI, and
linked from the product's own object, so that the kernel under test is the one libmagprop_amd.so runs.

Held: bit for bit.  The restatement (tests/smc_restated.py) forms its sums in the kernel's order (thread k its particles k,
k + 256, ... in order, then mp_wg.h's butterfly and wavefront order) and takes the device's exp (mpz_exp) and log (mpl_libm), so
d, ESS(d), ln Z, the units, their cumulative sums and the ancestors are the device's exactly; the bound 4 N 2^-52 of a sum in any
order is not needed."""
import ctypes as C

import numpy as np
import pytest

import probe_lib
import smc_restated as sm
from raw_abi import dp, ip, lp

pytestmark = pytest.mark.gpu

CANARY = -7
COLS = 4


def probe(name):
    """The probe library libmp_probe_<name>.so, behind the product's library so that one HIP runtime is shared."""
    from magprop_amd import _capi
    _capi.lib()
    return probe_lib.load(name)


def device_exp(x):
    """The device runtime's exp, element by element (mpz_exp)."""
    x = np.asarray(x, dtype=np.float64)
    if x.size == 0:
        return x.copy()
    buf, out = np.ascontiguousarray(x.ravel()), np.empty(x.size)
    assert probe("smc").mpz_exp(dp(buf), dp(out), C.c_int(buf.size)) == 0
    return out.reshape(x.shape)


def device_log(x):
    """The device runtime's log (mpl_libm), of a scalar or an array."""
    a = np.atleast_1d(np.asarray(x, dtype=np.float64))
    n = -(-a.size // 64) * 64
    buf, out = np.ones(n), np.empty(n)
    buf[:a.size] = a.ravel()
    assert probe("libm").mpl_libm(0, dp(buf), dp(out), C.c_int(n)) == 0
    out = out[:a.size].reshape(a.shape)
    return float(out[0]) if np.ndim(x) == 0 else out


def stage_launch(lnl, beta, lnz, status, nstage, ncall, nacc, seed, t, ess):
    """One mpz_stage call over lnl[n_runs, n]; every output starts as a canary.  Returns the buffers as the device left them."""
    L = probe("smc")
    n_runs, n = lnl.shape
    ms = L.mpz_max_stages()
    o = dict(anc=np.full((n_runs, n), CANARY, dtype=np.int32), units=np.full((n_runs, n), 0xDEADBEEF, dtype=np.uint32),
             cum=np.full((n_runs, n), 0xDEADBEEF, dtype=np.uint64), beta=np.array(beta, dtype=np.float64),
             lnz=np.array(lnz, dtype=np.float64), status=np.array(status, dtype=np.int32), nstage=np.array(nstage, dtype=np.int32),
             ncall=np.array(ncall, dtype=np.int64), nacc=np.array(nacc, dtype=np.int64),
             log=np.full((n_runs, ms, COLS), -123.0), log_cnt=np.full((n_runs, ms, 2), CANARY, dtype=np.int64))
    rc = L.mpz_stage(C.c_int(n), C.c_int(n_runs), C.c_uint64(seed), C.c_uint32(t), C.c_double(ess),
                     dp(np.ascontiguousarray(lnl, dtype=np.float64)), ip(o["anc"]), o["units"].ctypes.data_as(C.c_void_p),
                     o["cum"].ctypes.data_as(C.c_void_p), dp(o["beta"]), dp(o["lnz"]), ip(o["status"]), ip(o["nstage"]),
                     lp(o["ncall"]), lp(o["nacc"]), dp(o["log"]), lp(o["log_cnt"]))
    assert rc == 0, rc
    return o


def crafted(n, rng):
    """The runs of one launch: (name, lnl[n], beta, status, nstage)."""
    ulp = 1.0 - 2.0 ** -53
    dom = np.full(n, -1.0e300)
    dom[n // 2] = 0.0
    peak = -40.0 * rng.random(n)
    peak[n - 1] = 500.0
    ends = -20.0 * rng.random(n)
    ends[[0, n - 1]] = -np.inf
    return [("equal", np.full(n, -7.5), 0.0, 0, 0),
            ("dominant", dom, 0.0, 0, 5),
            ("peak", peak, 0.125, 0, 1),
            ("ties", -3.0 * np.floor(12.0 * rng.random(n)), 0.3, 0, 2),
            ("inf at both ends", ends, 0.0, 0, 0),
            ("all inf", np.full(n, -np.inf), 0.0, 0, 3),
            ("range 1e9", -1.0e9 * rng.random(n), 0.0, 0, 0),
            ("one ulp left", -100.0 * rng.random(n), ulp, 0, 40),
            ("stopped", -rng.random(n), 1.0, sm.DONE, 9),
            ("stage limit", -rng.random(n), 0.5, 0, sm.MAX_STAGES)]


@pytest.mark.parametrize("n", [4, 63, 64, 65, 255, 256, 257, 1025, 16384])
def test_stage_kernel_equals_the_restatement_bit_for_bit(n):
    rng = np.random.default_rng(1000 + n)
    runs = crafted(n, rng)
    seed, t, ess = 20261020 + n, 17, 0.5
    lnl = np.array([c[1] for c in runs])
    lnz = np.linspace(-3.0, 2.0, len(runs))
    ncall, nacc = 100 + np.arange(len(runs)), 7 + np.arange(len(runs))
    o = stage_launch(lnl, [c[2] for c in runs], lnz, [c[3] for c in runs], [c[4] for c in runs], ncall, nacc, seed, t, ess)
    for r, (name, v, beta, status, made) in enumerate(runs):
        untouched = True
        if status != sm.RUNNING:
            want = status
        elif made >= sm.MAX_STAGES:
            want = sm.STAGE_LIMIT
        else:
            ref = sm.stage(v, beta, lnz[r], ess, seed, t, r, exp=device_exp, log=device_log)
            want = sm.FAILED if ref is None else (sm.DONE if ref["beta"] >= 1.0 else sm.RUNNING)
            untouched = ref is None
        assert o["status"][r] == want, name
        if untouched:
            assert np.all(o["anc"][r] == CANARY) and np.all(o["units"][r] == 0xDEADBEEF) and np.all(o["log"][r] == -123.0), name
            assert o["beta"][r] == beta and o["lnz"][r] == lnz[r] and o["nstage"][r] == made, name
            continue
        assert np.array_equal(o["units"][r], ref["units"]), name
        assert np.array_equal(o["cum"][r], ref["cum"]), name
        assert np.array_equal(o["anc"][r], ref["anc"]), name
        row = o["log"][r, made]
        assert (o["beta"][r], o["lnz"][r], o["nstage"][r]) == (ref["beta"], ref["lnz"], made + 1), (name, o["beta"][r], ref["beta"])
        assert row.tolist() == [ref["beta"], ref["d"], ref["ess"], ref["lnz"]], (name, row, ref["d"], ref["ess"])
        assert o["log_cnt"][r, made].tolist() == [ncall[r], nacc[r]] and np.all(o["log"][r, made + 1:] == -123.0), name
        # the properties the cases are there for
        fin = np.isfinite(v)
        assert np.all(o["units"][r][~fin] == 0) and not np.any(np.isin(o["anc"][r], np.nonzero(o["units"][r] == 0)[0])), name
        assert np.all(np.diff(o["anc"][r]) >= 0) and o["units"][r].max() == 1 << 31, name
        if name == "equal":
            assert np.array_equal(o["anc"][r], np.arange(n)) and o["beta"][r] == 1.0 and row[2] == n
            assert row[3] == lnz[r] + (-7.5 + device_log(1.0))
        if name == "dominant":
            assert np.all(o["anc"][r] == n // 2) and row[1] == 2.0 ** -128
        if name == "inf at both ends":
            assert o["anc"][r].min() >= 1 and o["anc"][r].max() <= n - 2
        if name == "range 1e9" and n >= 63:
            assert 1e-11 < row[1] < 1e-7 and row[2] >= ess * n > row[2] - 1.0
        if name == "one ulp left":
            assert o["beta"][r] == 1.0 and row[1] == 2.0 ** -53


def test_the_probe_refuses_what_the_library_refuses():
    L = probe("smc")
    assert (L.mpz_min_particles(), L.mpz_max_particles(), L.mpz_max_stages()) == (4, 16384, sm.MAX_STAGES)
    n = 8
    bufs = dict(lnl=np.zeros(n), anc=np.zeros(n, dtype=np.int32), units=np.zeros(n, dtype=np.uint32), cum=np.zeros(n, dtype=np.uint64),
                beta=np.zeros(1), lnz=np.zeros(1), status=np.zeros(1, dtype=np.int32), nstage=np.zeros(1, dtype=np.int32),
                ncall=np.zeros(1, dtype=np.int64), nacc=np.zeros(1, dtype=np.int64), log=np.zeros((sm.MAX_STAGES, COLS)),
                log_cnt=np.zeros((sm.MAX_STAGES, 2), dtype=np.int64))

    def call(n_=n, n_runs=1, ess=0.5, **kw):
        b = {**bufs, **kw}
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        return L.mpz_stage(C.c_int(n_), C.c_int(n_runs), C.c_uint64(1), C.c_uint32(0), C.c_double(ess), *(vp(b[k]) for k in bufs))

    assert call() == 0
    for bad in (dict(n_=3), dict(n_=16385), dict(n_runs=0), dict(n_runs=65), dict(ess=0.0), dict(ess=1.0), dict(ess=float("nan")),
                dict(lnl=None), dict(anc=None), dict(log=None), dict(nstage=np.array([-1], dtype=np.int32)),
                dict(nstage=np.array([sm.MAX_STAGES + 1], dtype=np.int32))):
        assert call(**bad) == -1, bad
    x = np.array([0.0, 1.0, -700.0, 709.0])
    assert np.allclose(device_exp(x), np.exp(x), rtol=4e-16) and device_exp(np.array([0.0]))[0] == 1.0
    assert L.mpz_exp(None, None, C.c_int(4)) == -1 and L.mpz_exp(dp(x), dp(x), C.c_int(0)) == -1
