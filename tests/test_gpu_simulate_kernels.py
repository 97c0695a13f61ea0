"""The cells kernel of the simulated light curves alone, through the probe library libmp_probe_simulate.so
(csrc/mp_probe_simulate.hip: the product's compiled kernel behind its launcher), on every crafted case of tests/simulate_cases.py
against the restatement tests/simulate_restated.py.  model and yerr bit for bit on numpy alone; z and y bit for bit with the
restatement's log, cos, sin and sqrt taken from the device runtime (mpt_libm, mpl_libm), as tests/test_gpu_bridge_kernels.py
takes them.  The host's bracket rule (mpm_bracket: the code mp_set_dataset shares) bit for bit as well."""
import ctypes as C

import numpy as np
import pytest

import probe_lib
import simulate_cases as sc
import simulate_restated as sr
from raw_abi import dp, ip

pytestmark = pytest.mark.gpu


def _probe(name):
    from magprop_amd import _capi
    _capi.lib()                      # (first: one HIP runtime, the product's)
    return probe_lib.load(name)


def _device_fn(lib, entry, func):
    fn = getattr(_probe(lib), entry)

    def f(x):
        a = np.ascontiguousarray(np.asarray(x, dtype=np.float64))
        flat = np.ascontiguousarray(a.ravel())
        res = np.empty(flat.size)
        assert fn(func, dp(flat), dp(res), C.c_int(flat.size)) == 0
        return res.reshape(a.shape)
    return f


@pytest.fixture(scope="module")
def libm():
    """the device runtime's functions, element by element"""
    return sr.Libm(exp=None, log=_device_fn("ladder", "mpt_libm", 1), cos=_device_fn("libm", "mpl_libm", 1),
                   sin=_device_fn("libm", "mpl_libm", 2), sqrt=_device_fn("libm", "mpl_libm", 3))


def same(a, b):
    """bit for bit, NaN equal to NaN"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


def device_bracket(t, x):
    t, flat = np.ascontiguousarray(t), np.ascontiguousarray(np.asarray(x, dtype=np.float64).ravel())
    g, dx, idt = np.full(flat.size, -9, dtype=np.int32), np.full(flat.size, -9.0), np.full(flat.size, -9.0)
    rc = _probe("simulate").mpm_bracket(dp(t), t.size, dp(flat), C.c_int64(flat.size), ip(g), dp(dx), dp(idt))
    assert rc == 0, rc
    return g.reshape(np.shape(x)), dx.reshape(np.shape(x)), idt.reshape(np.shape(x))


def launch(case, g, dx, idt, lo=0, hi=None, want=("y", "yerr", "model", "z")):
    """rows [lo, hi) of the case in one launch: the outputs named in `want` (the others are not asked for) and the zero marks"""
    hi = case["ltot"].shape[0] if hi is None else hi
    cnt, per_row = hi - lo, case["x"].ndim == 2
    sl = (lambda a: np.ascontiguousarray(a[lo:hi])) if per_row else np.ascontiguousarray
    ltot, status = np.ascontiguousarray(case["ltot"][lo:hi]), np.ascontiguousarray(case["status"][lo:hi])
    n_obs = case["x"].shape[-1]
    out = {k: np.full((cnt, n_obs), -7.0) for k in want}
    zero = np.zeros(cnt, dtype=np.int32)
    tabs = [sl(g), sl(dx), sl(idt), None if case["yerr"] is None else sl(case["yerr"])]
    rc = _probe("simulate").mpm_cells(dp(ltot), ip(status), ip(tabs[0]), dp(tabs[1]), dp(tabs[2]), dp(tabs[3]), C.c_double(case["frac_err"]),
                                      C.c_uint64(case["seed"]), C.c_int64(case["row0"] + lo), cnt, n_obs, ltot.shape[1],
                                      cnt if per_row else 1, dp(out.get("y")), dp(out.get("yerr")), dp(out.get("model")), dp(out.get("z")),
                                      ip(zero))
    assert rc == 0, rc
    out["zero"] = zero
    return out


@pytest.mark.parametrize("name", list(sc.CASES))
def test_cells_kernel_alone(libm, name):
    case = sc.CASES[name]
    g, dx, idt = device_bracket(case["t"], case["x"])
    rg, rdx, ridt = sr.bracket(case["t"], case["x"])
    assert np.array_equal(g, rg) and same(dx, rdx) and same(idt, ridt)
    got = launch(case, g, dx, idt)
    plain = sr.cells(case["ltot"], case["status"], g, dx, idt, case["yerr"], case["frac_err"], case["seed"], case["row0"])
    assert same(got["model"], plain["model"]) and same(got["yerr"], plain["yerr"]) and np.array_equal(got["zero"], plain["zero"])
    want = sr.cells(case["ltot"], case["status"], g, dx, idt, case["yerr"], case["frac_err"], case["seed"], case["row0"], libm)
    assert same(got["z"], want["z"]) and same(got["y"], want["y"])
    # the same bits in launches of one row and of three, and with y alone asked for
    n = case["ltot"].shape[0]
    for step in (1, 3):
        if step >= n and step > 1:
            continue
        for lo in range(0, n, step):
            part = launch(case, g, dx, idt, lo, min(n, lo + step))
            for k in ("y", "yerr", "model", "z"):
                assert same(part[k], got[k][lo:lo + step]), (name, k, lo)
            assert np.array_equal(part["zero"], got["zero"][lo:lo + step])
    assert same(launch(case, g, dx, idt, want=("y",))["y"], got["y"])


def test_probe_refuses_bad_arguments():
    case = sc.CASES["n_obs_2"]
    p = _probe("simulate")
    t, x = np.ascontiguousarray(case["t"]), np.array([0.5])
    g, dx, idt = np.zeros(1, dtype=np.int32), np.zeros(1), np.zeros(1)
    assert p.mpm_bracket(dp(t), t.size, dp(x), C.c_int64(1), ip(g), dp(dx), dp(idt)) == -1            # a time below the grid
    assert p.mpm_bracket(dp(t[::-1].copy()), t.size, dp(np.array([5.0])), C.c_int64(1), ip(g), dp(dx), dp(idt)) == -1
    gg, ddx, iidt = sr.bracket(case["t"], case["x"])
    bad = gg.copy()
    bad[0] = case["t"].size                                                                         # a bracket past the curve
    ltot, status, y = np.ascontiguousarray(case["ltot"]), np.ascontiguousarray(case["status"]), np.empty((2, 2))
    assert p.mpm_cells(dp(ltot), ip(status), ip(bad), dp(ddx), dp(iidt), None, C.c_double(0.25), C.c_uint64(1), C.c_int64(0), 2, 2,
                       ltot.shape[1], 1, dp(y), None, None, None, None) == -1
    assert p.mpm_threads() == 256
    p.mpm_counter.restype = C.c_uint32
    assert p.mpm_counter() == sr.CTR
