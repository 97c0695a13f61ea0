"""numpy restatement of mp_model_derived's definition (include/magprop_amd.h; the order of the sums is stated there and in
magprop_amd/csrc/mp_derive.h): what tests/test_gpu_derive_kernels.py and tests/test_gpu_derived.py hold the device against bit
for bit, and what tests/test_derive_cases_cpu.py holds against an independent definition.

The G - 1 trapezoid terms are padded with 0.0 to (256, seg), seg = ceil((G - 1) / 256); np.cumsum along a segment adds them in
increasing i, np.cumsum of the 256 totals adds those in segment order.  Both sums start from 0.0 on the device and from their
first term in np.cumsum: the two differ where a term is -0.0 only, and adding 0.0 to the running sums restores the device's +0.0
(x + 0.0 is x for every other x).  np.cumsum adds its elements one by one in order (no pairwise blocking, unlike np.sum)."""
import numpy as np

N = 16
SEGMENTS = 256
E_TOT, E_PROP, E_DIP, L_PEAK, T_PEAK, LPROP_PEAK, T_LPROP_PEAK, T10, T50, T90 = range(10)
OMEGA_END, OMEGA_MAX, T_OMEGA_MAX, MDISC_END, MDISC_MAX, T_MDISC_MAX = range(10, 16)
FRACTIONS = (0.1, 0.5, 0.9)


def seg_len(G):
    return -(-(G - 1) // SEGMENTS)


def running_sums(L, t):
    """(running sum inside its segment after every interval (256, seg), total of the segments before each (256,), total)."""
    L, t = np.asarray(L, dtype=np.float64), np.asarray(t, dtype=np.float64)
    G = t.size
    seg = seg_len(G)
    dt = t[1:] - t[:-1]
    terms = np.zeros(SEGMENTS * seg)
    terms[:G - 1] = (0.5 * dt) * (L[:-1] + L[1:])
    run = np.cumsum(terms.reshape(SEGMENTS, seg), axis=1) + 0.0
    incl = np.cumsum(run[:, -1]) + 0.0
    before = np.concatenate([[0.0], incl[:-1]])
    return run, before, incl[-1]


def peak(v):
    """(largest value, its index), the first of equal values"""
    i = int(np.argmax(v))
    return v[i], i


def derive_row(curves, t):
    """The 16 columns of one finished row: curves (5, G) = Ltot, Lprop, Ldip, Mdisc, omega on the grid t (G,)."""
    ltot, lprop, ldip, mdisc, omega = (np.asarray(c, dtype=np.float64) for c in curves)
    t = np.asarray(t, dtype=np.float64)
    G = t.size
    out = np.empty(N)
    run, before, e_tot = running_sums(ltot, t)
    out[E_TOT] = e_tot
    out[E_PROP] = running_sums(lprop, t)[2]
    out[E_DIP] = running_sums(ldip, t)[2]
    for col, v in ((L_PEAK, ltot), (LPROP_PEAK, lprop), (OMEGA_MAX, omega), (MDISC_MAX, mdisc)):
        out[col], i = peak(v)
        out[col + 1] = t[i]
    cum = (before[:, None] + run).reshape(-1)[:G - 1]        # cumulative energy up to t_{i+1}
    for col, f in zip((T10, T50, T90), FRACTIONS):
        hit = np.nonzero(cum >= f * e_tot)[0]
        i = 0 if e_tot == 0.0 else (int(hit[0]) if hit.size else G - 2)
        out[col] = t[i + 1]
    out[OMEGA_END] = omega[-1]
    out[MDISC_END] = mdisc[-1]
    return out


def derive(curves, status, t):
    """out (n, 16) of curves (5, n, G) and status (n,): rows whose status is not 0 are NaN."""
    curves = np.asarray(curves, dtype=np.float64)
    n = curves.shape[1]
    out = np.full((n, N), np.nan)
    for r in range(n):
        if status[r] == 0:
            out[r] = derive_row(curves[:, r], t)
    return out
