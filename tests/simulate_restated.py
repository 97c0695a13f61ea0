"""numpy restatement of the simulated light curves (include/magprop_amd.h mp_simulate; magprop_amd/csrc/mp_simulate.hip,
mp_simulate.h): the host's bracket of an observed time, the model value, the error, the Philox / Box-Muller normal of every cell
and the noisy value.  Test infrastructure: the GPU tests compare the device's numbers with it bit for bit, the CPU tests hold its
model value against exact rational interpolation and its noise against the chunking.

Every product, sum and difference is a separately rounded float64 operation in the kernel's order.  The Philox rounds are the
oracle's, u01 and the Libm tuple (log, cos, sin, sqrt over arrays: numpy's on the CPU, the device's through the libm probes where
a device value is compared bit for bit) are tests/bridge_restated.py's."""
import numpy as np

from bridge_restated import NUMPY, TWO_PI, Libm, u01  # noqa: F401  (Libm, NUMPY: what the callers pass as libm)
from oracle.stretch_oracle import philox4x32_10

M32 = 0xFFFFFFFF
CTR = 0x53494D00                       # kSimCtr
STATUS_OK, STATUS_ZEROERR = 0, 5
MAX_ROWS, MAX_CELLS = 262144, 1 << 28  # MP_SIM_*


def bracket(t, x):
    """(g, dx, idt) of the times x on the grid t: g the largest index with t[g] <= x, dx = x - t[g], idt = 1 / (t[g + 1] - t[g]);
    the last grid point sits on its knot (g = G - 1, dx = 0, idt = 0).  ValueError for a time outside the grid or not finite."""
    t, x = np.asarray(t, dtype=np.float64), np.asarray(x, dtype=np.float64)
    if not np.all((x >= t[0]) & (x <= t[-1])):
        raise ValueError("a time is outside the grid")
    g = np.searchsorted(t, x, side="right") - 1
    last = g == t.size - 1
    gi = np.minimum(g, t.size - 2)
    dx = np.where(last, 0.0, x - t[gi])
    idt = np.where(last, 0.0, 1.0 / (t[gi + 1] - t[gi]))
    return g.astype(np.int32), dx, idt


def model_value(L, g, dx, idt):
    """mod of one curve L[G] at the brackets: L[g] where dx == 0, otherwise ((L[g + 1] - L[g]) * idt) * dx + L[g]"""
    L = np.asarray(L, dtype=np.float64)
    La = L[g]
    Lb = L[np.minimum(g + 1, L.size - 1)]
    with np.errstate(all="ignore"):
        d = Lb - La
        slope = d * idt
        rise = slope * dx
        mod = rise + La
    return np.where(dx == 0.0, La, mod)


def normals(seed, i, n_obs, libm=NUMPY):
    """z[n_obs] of row index i: pair p = j // 2 from Philox (seed; i, p, 0, CTR), even j its first normal, odd j its second"""
    seed, npairs = int(seed), (n_obs + 1) // 2
    p = np.arange(npairs, dtype=np.uint64)
    w = philox4x32_10(seed & M32, seed >> 32, np.full(npairs, int(i) & M32, dtype=np.uint64), p, np.zeros(npairs, dtype=np.uint64),
                      np.full(npairs, CTR, dtype=np.uint64))
    rad = libm.sqrt(-2.0 * libm.log(1.0 - u01(w[0], w[1])))
    ang = TWO_PI * u01(w[2], w[3])
    z = np.empty(2 * npairs)
    z[0::2], z[1::2] = rad * libm.cos(ang), rad * libm.sin(ang)
    return z[:n_obs]


def cells(ltot, status, g, dx, idt, yerr, frac_err, seed, row0, libm=NUMPY):
    """What one launch of the cells kernel writes for the curves ltot[cnt][G] with statuses status[cnt] and the tables g, dx, idt,
    yerr (None: frac_err) of shape [n_obs] (shared) or [cnt][n_obs]: {"y", "yerr", "model", "z": [cnt][n_obs], "zero": [cnt] the
    rows it marks for a zero error}.  Row s draws under index row0 + s."""
    ltot = np.atleast_2d(np.asarray(ltot, dtype=np.float64))
    cnt, n_obs = ltot.shape[0], np.shape(g)[-1]
    out = {k: np.full((cnt, n_obs), np.nan) for k in ("y", "yerr", "model", "z")}
    zero = np.zeros(cnt, dtype=np.int32)

    def row(a, s):
        a = np.asarray(a)
        return a if a.ndim == 1 else a[s]
    for s in range(cnt):
        if status[s] != STATUS_OK:
            continue
        mod = model_value(ltot[s], row(g, s).astype(np.int64), row(dx, s), row(idt, s))
        with np.errstate(all="ignore"):
            ye = np.asarray(row(yerr, s), dtype=np.float64) if yerr is not None else frac_err * np.abs(mod)
            z = normals(seed, row0 + s, n_obs, libm)
            noise = ye * z
            y = mod + noise
        zero[s] = int(np.any(ye == 0.0))
        out["model"][s], out["yerr"][s], out["z"][s], out["y"][s] = mod, ye, z, y
    out["zero"] = zero
    return out


def simulate(t, ltot, status, x, yerr=None, frac_err=0.25, seed=0, chunk=None, libm=NUMPY):
    """mp_simulate behind its curve pass, for curves ltot[n][G] that the caller supplies: the brackets of x ((n_obs,) or
    (n, n_obs)), the cells in chunks of `chunk` rows (None: all at once), then NaN cells and STATUS_ZEROERR for the rows with a
    zero error.  Returns {"y", "yerr", "model", "z", "status"}."""
    ltot = np.atleast_2d(np.asarray(ltot, dtype=np.float64))
    n = ltot.shape[0]
    x = np.asarray(x, dtype=np.float64)
    g, dx, idt = bracket(t, x)
    chunk = n if chunk is None else int(chunk)
    out = {k: np.empty((n, x.shape[-1])) for k in ("y", "yerr", "model", "z")}
    status = np.array(status, dtype=np.int32)
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        sl = (lambda a: a) if x.ndim == 1 else (lambda a: a[lo:hi])
        c = cells(ltot[lo:hi], status[lo:hi], sl(g), sl(dx), sl(idt), None if yerr is None else sl(np.asarray(yerr, dtype=np.float64)),
                  frac_err, seed, lo, libm)
        for k in out:
            out[k][lo:hi] = c[k]
        bad = (status[lo:hi] == STATUS_OK) & (c["zero"] != 0)
        status[lo:hi][bad] = STATUS_ZEROERR
        for k in out:
            out[k][lo:hi][bad] = np.nan
    out["status"] = status
    return out
