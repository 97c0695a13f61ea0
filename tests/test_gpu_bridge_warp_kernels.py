"""The kernels of the bridge-sampling evidence with a Student-t proposal and with Warp-III (magprop_amd/csrc/mp_bridge.hip:
bridge_draws_warp_kernel, bridge_est_warp_kernel, bridge_pair_kernel, bridge_count_kernel) through whole calls of
mp_bridge_logz_warp on the test targets 1 .. 4 with every optional output, on the crafted cases of tests/bridge_warp_cases.py,
and the parity of the new entry with mp_bridge_logz where both apply.

Held: bit for bit.  The restatement (tests/bridge_warp_restated.py) forms every sum in the kernels' order and takes the device's
exp, log (mpt_libm) and cos, sin, sqrt (mpl_libm); the host's sqrt, log and lgamma are the C library's on both sides."""
import ctypes as C

import numpy as np
import pytest

import bridge_cases as bc
import bridge_restated as br
import bridge_warp_cases as wc
import bridge_warp_restated as bw
from raw_abi import dp, synth_handle
from test_gpu_bridge_kernels import _device_fn, same

pytestmark = pytest.mark.gpu

DETAILS = ("moments", "draws", "draw_lnp", "draw_lnq", "est_lnq", "a", "b", "draw_mirrors", "est_mirror_lnp", "draw_mirror_lnp")


@pytest.fixture(scope="module")
def libm():
    """the device runtime's functions, element by element"""
    return br.Libm(exp=_device_fn("ladder", "mpt_libm", 0), log=_device_fn("ladder", "mpt_libm", 1),
                   cos=_device_fn("libm", "mpl_libm", 1), sin=_device_fn("libm", "mpl_libm", 2), sqrt=_device_fn("libm", "mpl_libm", 3))


@pytest.fixture(scope="module")
def handle():
    with synth_handle() as h:
        yield h


def raw_warp(handle, case, proposal, nu, warp, ds_id=0):
    """mp_bridge_logz_warp itself on a case of either cases file, every optional output asked for (the front end sends the
    defaults of proposal and warp to mp_bridge_logz)."""
    from magprop_amd import _capi
    xf, xe, le = (np.ascontiguousarray(case[k], dtype=np.float64) for k in ("x_fit", "x_est", "lnp_est"))
    nd, n_est, n_draws, n_rep = xf.shape[1], xe.shape[0], case["n_draws"], case["n_rep"]
    tot = n_rep * n_draws
    shapes = dict(moments=br.n_moments(nd), draws=(tot, nd), draw_lnp=tot, draw_lnq=tot, est_lnq=n_est, a=n_est, b=tot,
                  draw_mirrors=(tot, nd), est_mirror_lnp=n_est, draw_mirror_lnp=tot)
    res = {k: np.full(shapes[k], -7.0) for k in DETAILS}
    res["out"] = np.full((n_rep, _capi.BRIDGE_WARP_NOUT), -7.0)
    lo = None if case["lower"] is None else np.ascontiguousarray(case["lower"], dtype=np.float64)
    hi = None if case["upper"] is None else np.ascontiguousarray(case["upper"], dtype=np.float64)
    rc = _capi.lib().mp_bridge_logz_warp(handle._h, dp(xf), xf.shape[0], dp(xe), dp(le), n_est, nd, ds_id, dp(lo), dp(hi), n_draws, n_rep,
                                         C.c_uint64(case["seed"]), C.c_double(n_est if case["neff"] is None else case["neff"]),
                                         case["max_iter"], C.c_double(case["tol"]), case["target"], proposal, nu, int(warp), dp(res["out"]),
                                         *(dp(res[k]) for k in DETAILS))
    assert rc == _capi.MP_OK, _capi.last_error()
    return res


@pytest.mark.parametrize("name", list(wc.CALLS))
def test_whole_calls_on_the_test_targets(handle, libm, name):
    """moments, draws, both lnp arrays, draw_lnq, est_lnq, a, b, the mirrors and every number of out, the update count and the
    mirror counts included."""
    case = wc.CALLS[name]
    want = wc.call_expected(case, libm)
    got = handle.bridge_logz(case["x_fit"], case["x_est"], case["lnp_est"], case["lower"], case["upper"], n_draws=case["n_draws"],
                             n_rep=case["n_rep"], seed=case["seed"], neff=case["neff"], max_iter=case["max_iter"], tol=case["tol"],
                             target=case["target"], details=True, proposal=case["proposal"], nu=case["nu"], warp=case["warp"])
    keys = [k for k in DETAILS if case["warp"] or "mirror" not in k] + ["out"]
    assert set(got) == set(keys)
    for key in keys:
        assert same(got[key], want[key]), (name, key, got[key], want[key])
    if name == "no_draw_inside":
        assert np.all(got["out"][:, br.STATUS] == br.NO_OVERLAP)
    if name == "draw_and_mirror_both_outside":
        assert 0 < np.count_nonzero(np.isneginf(got["b"])) < got["b"].size


def test_the_mirror_outputs_are_left_alone_without_warp(handle):
    case = wc.CALLS["t_5_unwarped_three_reps"]
    got = raw_warp(handle, case, bw.STUDENT, 5, False)
    assert all(np.all(got[k] == -7.0) for k in ("draw_mirrors", "est_mirror_lnp", "draw_mirror_lnp"))
    assert np.all(got["out"][:, bw.EST_MIRRORS:] == 0.0) and np.all(got["b"] != -7.0)


@pytest.mark.parametrize("name", ["ndim_9", "box_cuts_the_draws", "terraces", "sizes_257", "sizes_4097"])
def test_parity_with_the_old_entry_on_the_test_targets(handle, name):
    """proposal = 0, warp = 0 through mp_bridge_logz_warp against mp_bridge_logz on the same arguments: the kernels of the new
    entry against the three the old one keeps."""
    case = bc.CALLS[name]
    old = handle.bridge_logz(case["x_fit"], case["x_est"], case["lnp_est"], case["lower"], case["upper"], n_draws=case["n_draws"],
                             n_rep=case["n_rep"], seed=case["seed"], neff=case["neff"], max_iter=case["max_iter"], tol=case["tol"],
                             target=case["target"], details=True)
    new = raw_warp(handle, case, bw.NORMAL, 0, False)
    for key in ("moments", "draws", "draw_lnp", "draw_lnq", "est_lnq"):
        assert same(new[key].ravel(), old[key].ravel()), (name, key)       # (raw_warp's arrays are flat over the repetitions)
    assert same(new["out"][:, :br.NOUT], old["out"]) and np.all(new["out"][:, br.NOUT:] == 0.0)
    assert same(new["a"], case["lnp_est"] - old["est_lnq"])
