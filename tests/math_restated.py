"""numpy restatements of the device math primitives (magprop_amd/csrc/mp_math.hpp) and the error measures of their tests
(tests/test_gpu_math.py on the device, tests/test_math_cpu.py for the reference side).  numpy and libm only."""
import ctypes
import ctypes.util
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_math.npz")
EPS = 2.0 ** -52
TINY = 2.0 ** -1074

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fma.restype = ctypes.c_double
_libm.fma.argtypes = [ctypes.c_double] * 3
_fma = np.frompyfunc(_libm.fma, 3, 1)


def fma(a, b, c):
    """Correctly rounded a * b + c, element by element (libm: Python 3.10 has no math.fma)."""
    a, b, c = np.broadcast_arrays(np.asarray(a, float), np.asarray(b, float), np.asarray(c, float))
    return _fma(a, b, c).astype(np.float64).reshape(a.shape)


# every function libmp_probe.so exports (magprop_amd/csrc/mp_probe.hip); none of them belongs to libmagprop_amd.so
PROBE_EXPORTS = ("mpp_unary", "mpp_exp10", "mpp_phi", "mpp_phi6", "mpp_node_weights", "mpp_wtab_size", "mpp_wtab_stride",
                 "mpp_scan_affine", "mpp_lane_prev", "mpp_lane_prev_map", "mpp_lane_bcast", "mpp_uniform", "mpp_wave_sum",
                 "mpp_lane_ext", "mpp_unfused", "mpp_lse", "mpp_lse_merge", "mpp_pick")


# ---------------------------------------------------------------- error measures against a double-double expectation
def ulp(hi):
    """Spacing of the doubles at |hi| (2^-1074 at and below the subnormals)."""
    return np.maximum(np.spacing(np.abs(np.asarray(hi, float))), TINY)


def err_ulps(got, hi, lo):
    """|got - (hi + lo)| in units of ulp(hi), in long double (exact to ~2^-11 ulp)."""
    L = np.longdouble
    d = (np.asarray(got, L) - np.asarray(hi, L)) - np.asarray(lo, L)
    return np.abs(d / ulp(hi).astype(L)).astype(np.float64)


def err_rel(got, hi, lo):
    """|got - (hi + lo)| / |hi| in long double; 0 where both are 0, inf where only the expectation is."""
    L = np.longdouble
    d = np.abs((np.asarray(got, L) - np.asarray(hi, L)) - np.asarray(lo, L))
    h = np.abs(np.asarray(hi, L))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d == 0, L(0), d / h)
    return r.astype(np.float64)


def same_bits(a, b):
    """Equality of two double arrays bit for bit (NaN payloads and the sign of zero included)."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---------------------------------------------------------------- exp_fast
LOG2E, LN2_HI, LN2_LO = 1.4426950408889634074, -6.93147180369123816490e-01, -1.90821492927058770002e-10
_FACT = [float(math.factorial(k)) for k in range(18)]


def exp_fast(x):
    """exp_fast of mp_math.hpp, operation by operation: every one of them is an IEEE operation (rint, FMA, ldexp)."""
    x = np.asarray(x, float)
    k = np.rint(x * LOG2E)
    r = fma(k, LN2_HI, x)
    r = fma(k, LN2_LO, r)
    p = np.full_like(x, 1.0 / _FACT[12])
    for j in range(11, 1, -1):
        p = fma(p, r, 1.0 / _FACT[j])
    p = fma(p, r, 1.0)
    p = fma(p, r, 1.0)
    return np.ldexp(p, k.astype(np.int64).astype(np.int32))


def exp_worst_inputs():
    """Every k ln2 / 2 for odd k inside [-750, 700] with both neighbours: the ends of exp_fast's reduced range, where the
    polynomial is at its worst and the result sits next to a power of two.  Padded with 0 to a multiple of 256."""
    ks = np.arange(-2163, 2020, 2).astype(float)
    x = ks * (math.log(2.0) / 2.0)
    x = np.concatenate([np.nextafter(x, -np.inf), x, np.nextafter(x, np.inf)])
    x = x[(x >= -750.0) & (x <= 700.0)]
    return np.concatenate([x, np.zeros((-x.size) % 256)])


LN10, LN10_LO = 2.302585092994046, -2.1707562233822494e-16


def exp10_fast(x):
    """exp10_fast of mp_math.hpp, operation by operation (the source writes every multiply-add as an fma and leaves none to
    the compiler's contraction)."""
    x = np.asarray(x, float)
    hi = x * LN10
    lo = fma(x, LN10_LO, fma(x, LN10, -hi))
    a = np.minimum(np.maximum(hi, -750.0), 709.0)
    k = np.rint(a * LOG2E)
    r0 = fma(k, LN2_HI, a)
    d = fma(k, LN2_LO, lo)
    r = r0 + d
    t = (r0 - r) + d
    q = np.full_like(x, 1.0 / _FACT[14])
    for j in range(13, 1, -1):
        q = fma(q, r, 1.0 / _FACT[j])
    s = fma(r * r, q, fma(t, r, t))
    u = r + s
    return np.ldexp(1.0 + u, k.astype(np.int64).astype(np.int32))


# ---------------------------------------------------------------- phi functions
def wave_paths(z, N):
    """Which formula phi12345<N> / phi6<N> apply to every element of z, from what its wavefront holds (lane l of wave w
    owns the elements (w * 64 + l) * N ..): 0 the 7-term series (every |z| of the wave below 1/32), 1 the 13-term series
    (|z| < 1/2), 2 the recurrence from e^z."""
    z = np.asarray(z, float)
    a = np.abs(z).reshape(-1, 64 * N)
    all_tiny = np.all(a < 0.03125, axis=1, keepdims=True)
    path = np.where(a < 0.5, np.where(all_tiny, 0, 1), 2)
    return path.reshape(z.shape)


def phi_plain(z, path):
    """The documented formulas in plain fp64 (libm exp, true division, separately rounded Horner steps):
    columns e^z, phi_1 .. phi_6."""
    z = np.asarray(z, float)
    out = np.empty(z.shape + (7,))
    with np.errstate(all="ignore"):
        s7 = np.full_like(z, 1.0 / _FACT[11])
        for j in range(10, 4, -1):
            s7 = s7 * z + 1.0 / _FACT[j]
        s13 = np.full_like(z, 1.0 / _FACT[17])
        for j in range(16, 4, -1):
            s13 = s13 * z + 1.0 / _FACT[j]
        p5 = np.where(path == 0, s7, s13)
        p4 = z * p5 + 1.0 / 24.0
        p3 = z * p4 + 1.0 / 6.0
        p2 = z * p3 + 0.5
        p1 = z * p2 + 1.0
        e = z * p1 + 1.0
        p6 = np.full_like(z, 1.0 / _FACT[17])
        for j in range(16, 5, -1):
            p6 = p6 * z + 1.0 / _FACT[j]
        ce = np.exp(np.maximum(z, -750.0))
        zs = np.where(path == 2, z, 1.0)
        c1 = (ce - 1.0) / zs
        c2 = (c1 - 1.0) / zs
        c3 = (c2 - 0.5) / zs
        c4 = (c3 - 1.0 / 6.0) / zs
        c5 = (c4 - 1.0 / 24.0) / zs
        c6 = (c5 - 1.0 / 120.0) / zs
    big = path == 2
    for col, (s, c) in enumerate(((e, ce), (p1, c1), (p2, c2), (p3, c3), (p4, c4), (p5, c5), (p6, c6))):
        out[..., col] = np.where(big, c, s)
    return out


# |z| ranges of the accuracy table and the figures measured for the plain-fp64 formulas (400 log-uniform |z| per sign and
# range against mpmath); None: no figure was taken.  Columns e^z, phi_1 .. phi_6.
PHI_RANGES = ("series7", "series13", "rec[0.5,1)", "rec[1,4)", "rec[4,40)", "rec[40,750]-", "rec[40,700]+")
PHI_TABLE = {
    "series7": (None, None, None, None, None, 1.2e-16, None),
    "series13": (None, None, None, None, None, 1.2e-16, None),
    "rec[0.5,1)": (1.1e-16, 2.8e-16, 1.2e-15, 7.5e-15, 6.1e-14, 6.1e-13, 7.3e-12),
    "rec[1,4)": (1.1e-16, 2.5e-16, 5.9e-16, 2.0e-15, 8.2e-15, 4.2e-14, 2.5e-13),
    "rec[4,40)": (1.2e-16, 2.2e-16, 3.5e-16, 4.5e-16, 6.0e-16, 9.8e-16, 1.6e-15),
    "rec[40,750]-": (None, 1.1e-16, 2.2e-16, 1.9e-16, 2.8e-16, 2.9e-16, 2.1e-16),
}
# Where no figure was taken the plain formulas are held to bounds that follow from their construction:
#  - the series ranges: phi_j = z phi_{j+1} + 1/j! with |z| < 1/2 damps the error of phi_{j+1} by |z| phi_{j+1} / phi_j < 1/2
#    and adds the roundings of the constant and of the step, half an eps each: below 2 eps throughout (phi_6: the Horner
#    sum itself, the same);
#  - z >= 40: nothing cancels (e^z dominates every difference), so the figures of [4, 40) hold a fortiori;
#  - e^z for z <= -40: libm's exp, as in the rows above; subnormal results are judged in units of 2^-1074 instead.
PHI_SERIES_CAP = 2.0 * EPS
PHI_TABLE["rec[40,700]+"] = PHI_TABLE["rec[4,40)"]
PHI_TABLE["rec[40,750]-"] = (1.2e-16,) + PHI_TABLE["rec[40,750]-"][1:]


def phi_range_index(z, path):
    """Index into PHI_RANGES of every element."""
    a = np.abs(np.asarray(z, float))
    r = np.where(a < 1.0, 2, np.where(a < 4.0, 3, np.where(a < 40.0, 4, np.where(np.asarray(z) < 0, 5, 6))))
    return np.where(path == 2, r, path)


def phi_cap(rng, col):
    """Bound of the plain-fp64 formulas for one range and output: 1.5 x the table's figure, or the constructed bound."""
    t = PHI_TABLE[rng][col]
    return 1.5 * t if t is not None else PHI_SERIES_CAP


def phi_errors(got, z, path, hi, lo):
    """max relative error per (range, output) -> array [len(PHI_RANGES)][7] (NaN: range not present).  Subnormal and zero
    expectations of e^z are left out here (judged in units of 2^-1074 by the caller)."""
    rel = err_rel(got, hi, lo)
    rel[np.abs(hi) < 2.0 ** -1022] = 0.0
    idx = phi_range_index(z, path)
    out = np.full((len(PHI_RANGES), 7), np.nan)
    for r in range(len(PHI_RANGES)):
        m = idx == r
        if m.any():
            out[r] = rel[m].max(axis=0)
    return out


# ---------------------------------------------------------------- quadrature table (mp_capi.cpp quad_weights, mp_device.h)
KINDS, WTAB_STRIDE, WTAB_SIZE = 5, 40, 5 * 40 + 3 * 7 * 12


def quad_weights(Q, K=5):
    """W[k][m] = m! [theta^m] l_k(theta), l_k the Lagrange basis on the nodes 1, 0, -1/Q, -(1/Q + 1/Q^2), ... : the host's
    loop, statement by statement."""
    x = [1.0, 0.0]
    acc, f = 0.0, 1.0
    for _ in range(2, K):
        f /= Q
        acc -= f
        x.append(acc)
    W = np.zeros((K, K))
    for k in range(K):
        co = [1.0] + [0.0] * 7
        deg, denom = 0, 1.0
        for j in range(K):
            if j == k:
                continue
            for m in range(deg + 1, 0, -1):
                co[m] = co[m - 1] - x[j] * co[m]
            co[0] = -x[j] * co[0]
            deg += 1
            denom *= x[k] - x[j]
        fact = 1.0
        for m in range(K):
            if m > 1:
                fact *= float(m)
            W[k, m] = fact * co[m] / denom
    return W


def wtab(lnq):
    """The quadrature rows of the device table for a geometric grid of ratio e^lnq: per kind (steps over 1/8, 1, 2, 4, 8
    grid intervals) W5[k][m] at [40 kind + 6 k + m].  (The other entries of the table are not read by the node weights.)"""
    T = np.zeros(WTAB_SIZE)
    for kind in range(KINDS):
        lnQ = lnq / 8.0 if kind == 0 else lnq * float(1 << (kind - 1))
        W = quad_weights(math.exp(lnQ))
        for k in range(5):
            T[kind * WTAB_STRIDE + 6 * k: kind * WTAB_STRIDE + 6 * k + 5] = W[k]
    return T


LNQ_GRID = math.log(10.0) * 6.0 / 10000.0      # the synthetic sets' grid: logspace(0, 6, 10001)
LNQ_GRID_S = math.log(10.0) * 9.0 / 10000.0    # the "S" grid: logspace(-3, 6, 10001)


# ---------------------------------------------------------------- wavefront primitives
def scan_affine(a, b):
    """scan_affine of mp_math.hpp on rows of 64 lanes: the six DPP steps in their order, b = fma(a, pb, b) then a = a * pa,
    the identity (1, 0) where a lane has no source."""
    a = np.array(a, float).reshape(-1, 64)
    b = np.array(b, float).reshape(-1, 64)
    lane = np.arange(64)

    def step(src, valid):
        nonlocal a, b
        pa = np.where(valid, a[:, np.clip(src, 0, 63)], 1.0)
        pb = np.where(valid, b[:, np.clip(src, 0, 63)], 0.0)
        b = fma(a, pb, b)
        a = a * pa

    for s in (1, 2, 4, 8):                                   # row_shr:s inside every row of 16 lanes
        step(lane - s, (lane % 16) >= s)
    row = lane // 16
    step(row * 16 - 1, (row == 1) | (row == 3))              # row_bcast:15 into rows 1 and 3: lane 15 of the row before
    step(np.full(64, 31), row >= 2)                          # row_bcast:31 into rows 2 and 3: lane 31
    return a, b


def wave_sum(v):
    """wave_sum on rows of 64 lanes, in the butterfly's order: v += v[lane ^ d], d = 32, 16, .., 1."""
    v = np.array(v, float).reshape(-1, 64)
    lane = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lane ^ d]
    return v


def max_raw(a, b):
    """v_max_f64: IEEE maxNum (a quiet NaN operand is dropped) with -0 ordered below +0."""
    a, b = np.asarray(a, float), np.asarray(b, float)
    zeros = (a == 0) & (b == 0)
    return np.where(zeros, np.where(np.signbit(a) & np.signbit(b), -0.0, 0.0), np.fmax(a, b))


def min_raw(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    zeros = (a == 0) & (b == 0)
    return np.where(zeros, np.where(np.signbit(a) | np.signbit(b), -0.0, 0.0), np.fmin(a, b))


def lane_ext(func, v):
    """lane_maxabs / lane_minabs / lane_max / lane_min (func 0 .. 3) over the last axis, in the source's order."""
    v = np.asarray(v, float)
    N = v.shape[-1]
    if func >= 2:
        op = max_raw if func == 2 else min_raw
        m = v[..., 0]
        for i in range(1, N):
            m = op(m, v[..., i])
        return m
    op = max_raw if func == 0 else min_raw
    a = np.abs(v)
    m = op(a[..., 0], a[..., 1]) if N > 1 else a[..., 0]
    i = 2
    while i + 1 < N:
        m = op(m, op(a[..., i], a[..., i + 1]))
        i += 2
    if N > 2 and N & 1:
        m = op(m, a[..., N - 1])
    return m
