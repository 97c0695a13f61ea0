"""The kernels of the bridge-sampling evidence (magprop_amd/csrc/mp_bridge.hip) on the crafted cases of tests/bridge_cases.py: the
fixed-point kernel alone and the moments kernels alone through the probe library libmp_probe_bridge.so (csrc/mp_probe_bridge.hip:
test infrastructure, no part of the product's ABI, linked from the product's own object), and whole calls of mp_bridge_logz on
the test targets with every optional output.

Held: bit for bit.  The restatement (tests/bridge_restated.py) forms every sum in the kernels' order and takes the device's exp,
log (mpt_libm) and cos, sin, sqrt (mpl_libm); the host's logs are the C library's on both sides."""
import ctypes as C

import numpy as np
import pytest

import bridge_cases as bc
import bridge_restated as br
import probe_lib
from raw_abi import dp, synth_handle

pytestmark = pytest.mark.gpu


def _probe(name):
    from magprop_amd import _capi
    _capi.lib()                      # (first: one HIP runtime, the product's)
    return probe_lib.load(name)


def _device_fn(lib, entry, func):
    fn = getattr(_probe(lib), entry)

    def f(x):
        a = np.ascontiguousarray(np.asarray(x, dtype=np.float64))
        out = np.empty(a.size)
        flat = a.ravel()
        for lo in range(0, flat.size, 1 << 20):
            part = np.ascontiguousarray(flat[lo:lo + (1 << 20)])
            res = np.empty(part.size)
            assert fn(func, dp(part), dp(res), C.c_int(part.size)) == 0
            out[lo:lo + part.size] = res
        return out.reshape(a.shape)
    return f


@pytest.fixture(scope="module")
def libm():
    """the device runtime's functions, element by element"""
    return br.Libm(exp=_device_fn("ladder", "mpt_libm", 0), log=_device_fn("ladder", "mpt_libm", 1),
                   cos=_device_fn("libm", "mpl_libm", 1), sin=_device_fn("libm", "mpl_libm", 2), sqrt=_device_fn("libm", "mpl_libm", 3))


@pytest.fixture(scope="module")
def handle():
    with synth_handle() as h:
        yield h


def same(a, b):
    """bit for bit, NaN equal to NaN"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


def fixed_launch(case, k):
    a, b = case["a"], np.ascontiguousarray(case["b"])
    out = np.full((b.shape[0], br.NOUT), -7.0)
    ln_s1, ln_s2, ln_n1, ln_n2, tau, lv = k
    rc = _probe("bridge").mpb_fixed(dp(a), C.c_int64(a.size), dp(b), C.c_int64(b.shape[1]), b.shape[0], C.c_double(ln_s1), C.c_double(ln_s2),
                                    C.c_double(ln_n1), C.c_double(ln_n2), C.c_double(tau), C.c_double(lv), case["max_iter"],
                                    C.c_double(case["tol"]), dp(out))
    assert rc == 0, rc
    return out


@pytest.mark.parametrize("name", list(bc.FIXED))
def test_fixed_point_kernel_alone(libm, name):
    case = bc.FIXED[name]
    want, k = bc.fixed_expected(case, libm)
    got = fixed_launch(case, k)
    assert np.all(got[:, br.STATUS] == case["expect"])
    assert same(got, want), (name, got, want)


# every size on ndim 6; ndim 1 and 9 on the sizes that differ in kind
MOMENT_SHAPES = [(n, 6) for n in bc.SIZES + (3 * br.BLOCK + 5,)] + [(n, d) for d in (1, 9) for n in (1, 257, br.BLOCK + 1, 3 * br.BLOCK + 5)]


@pytest.mark.parametrize("n,ndim", MOMENT_SHAPES)
def test_moments_kernels_alone(n, ndim):
    """The sums need no libm: against the restatement on numpy alone, and the same bits however the rows are cut into launches."""
    rng = np.random.default_rng(n + ndim)
    x = np.ascontiguousarray(rng.standard_normal((n, ndim)) * np.logspace(-3, 2, ndim) + rng.standard_normal(ndim))
    want = br.moments(x)
    for chunk_blocks in (1, 2, 1000):
        out = np.full(br.n_moments(ndim), -7.0)
        rc = _probe("bridge").mpb_moments(dp(x), C.c_int64(n), ndim, dp(np.ascontiguousarray(x[0])), C.c_int64(chunk_blocks), dp(out))
        assert rc == 0, rc
        assert same(out, want), (n, ndim, chunk_blocks)


def test_probe_refuses_bad_arguments():
    a = np.zeros(4)
    out = np.zeros(br.NOUT)
    p = _probe("bridge")
    assert p.mpb_fixed(None, C.c_int64(4), dp(a), C.c_int64(4), 1, C.c_double(0), C.c_double(0), C.c_double(0), C.c_double(0), C.c_double(1),
                       C.c_double(0), 10, C.c_double(0), dp(out)) == -1
    assert p.mpb_fixed(dp(a), C.c_int64(4), dp(a), C.c_int64(4), 65, C.c_double(0), C.c_double(0), C.c_double(0), C.c_double(0), C.c_double(1),
                       C.c_double(0), 10, C.c_double(0), dp(out)) == -1
    assert p.mpb_moments(dp(a), C.c_int64(4), 10, dp(a), C.c_int64(1), dp(out)) == -1


@pytest.mark.parametrize("name", list(bc.CALLS))
def test_whole_calls_on_the_test_targets(handle, libm, name):
    """moments, draws, draw_lnp, draw_lnq, est_lnq and every number of out, the update count included."""
    case = bc.CALLS[name]
    want = bc.call_expected(case, libm)
    got = handle.bridge_logz(case["x_fit"], case["x_est"], case["lnp_est"], case["lower"], case["upper"], n_draws=case["n_draws"],
                             n_rep=case["n_rep"], seed=case["seed"], neff=case["neff"], max_iter=case["max_iter"], tol=case["tol"],
                             target=case["target"], details=True)
    for key in ("moments", "draws", "draw_lnq", "draw_lnp", "est_lnq", "out"):
        assert same(got[key], want[key]), (name, key, got[key], want[key])


def test_constant_column_returns_erange(handle):
    from magprop_amd import _capi
    case = bc.ERANGE_CALL
    with pytest.raises(ValueError, match="dimension 1"):
        handle.bridge_logz(case["x_fit"], case["x_est"], case["lnp_est"], target=1, n_draws=case["n_draws"])
    out = np.zeros(br.NOUT)
    rc = _capi.lib().mp_bridge_logz(handle._h, dp(case["x_fit"]), 300, dp(case["x_est"]), dp(case["lnp_est"]), 300, 3, 0, None, None, 300, 1,
                                    C.c_uint64(1), C.c_double(300.0), 10, C.c_double(1e-9), 1, dp(out), None, None, None, None, None)
    assert rc == _capi.MP_ERANGE
