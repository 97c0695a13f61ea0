"""A plain restatement of the read-out of a kept tile (magprop_amd/csrc/mp_eval.hpp image_state with hermite, hermite5,
hermite_mdisc and dense_mdisc_qs under it) and of the host-built tables it indexes (mp_capi.cpp build_tables), for
tests/test_dense_cases_cpu.py (the reference side) and tests/test_gpu_dense_kernels.py (the device, through libmp_probe_dense.so).

The INDEX LOGIC (sh8, J, rem, i, l0, variant, the table base, the choice quintic / cubic / quasi-steady by z < 1 and keep < 3) is
restated in integers and in the three fp64 products that decide the branch (t1 = t_s E, h = t1 (1 - 1/Q), z = h / tvisc: lone
multiplications, which no compiler can contract, so they are the device's bit for bit).  The INTERPOLANTS are evaluated in
exact arithmetic (fractions.Fraction on the doubles given; the one irrational factor u^(-5/3) from decimal at 60 digits) and are
built from their defining conditions, not from the source's basis polynomials: the Hermite forms by solving the 4 or 6 end
conditions for the coefficients of the monomials, the Lagrange weights by solving the Vandermonde system, so that nothing here
shares a coefficient with the source.

ROUNDING BOUNDS.  U = 2^-53, every fp64 operation of the source one rounding |delta| <= U (an fma one, too: fp contraction of
the plain * and + of hermite only REMOVES roundings, so a count for the uncontracted form covers both).  With th in [0, 1],
A = |y0| + |y1|, B = h (|d0| + |d1|), C = h^2 (|e0| + |e1|), errors in units of U, magnitudes bounded by the triangle inequality:

  hermite:  D = y1 - y0: |D| <= A, err A.   c3 = h (d0 + d1) - 2 D: |c3| <= 2A + B, err (B + B) + 2A + (2A + B) = 4A + 3B.
            c2 = 3 D - h (2 d0 + d1): 3 D err 3A + 3A; h (2 d0 + d1) <= 2B, err 2B + 2B; |c2| <= 3A + 2B, err 6A + 4B + 3A + 2B = 9A + 6B.
            c2 + th c3: th c3 err (4A + 3B) + (2A + B); sum <= 5A + 3B, err 9A + 6B + 6A + 4B + 5A + 3B = 20A + 13B.
            h d0 + th (..): th (..) err 20A + 13B + 5A + 3B; h d0 err B; sum <= 5A + 4B, err 25A + 16B + B + 5A + 4B = 30A + 21B.
            y0 + th (..): th (..) err 30A + 21B + 5A + 4B; sum <= 6A + 4B: 35A + 25B + 6A + 4B = 41A + 29B  ->  HERMITE_C = 41 on A + B.
  hermite_d: 2 c2 err 18A + 12B; (th 3) c3 <= 6A + 3B, err 3 (4A + 3B) + 2 (6A + 3B) = 24A + 15B; sum <= 12A + 7B, err 54A + 34B;
            th (..) err 66A + 41B; + h d0 <= 12A + 8B, err 66A + 42B + 12A + 8B = 78A + 50B; / h one more: 90A + 58B
            ->  HERMITE_D_C = 90 on (A + B) / h.
  hermite5: t2 err 1, t3 err 2, both <= 1.  s = t3 (10 - 15 th + 6 th^2): the fma chain <= 15, err 15, then in [1, 10], err 15 + 10;
            s in [0, 1], err 10 * 2 + 25 + 1 = 46.  b1 = fma(t3, -6 + 8 th - 3 th^2, th): chain err 8, 8 + 6; |b1| <= 1, err 6 * 2 + 14 + 1 = 27.
            b4 = t3 (-4 + 7 th - 3 th^2): chain err 7, 7 + 4; err 4 * 2 + 11 + 1 = 20.  b2 = (t2 / 2) (1 - th)^3: chain err 3, 6, 7; <= 1/2,
            err 1/2 + 7/2 + 1/2 = 4.5.  b5 = (t3 / 2) (1 - th)^2: chain err 2, 3; err 1 + 3/2 + 1/2 = 3.
            fma(s, D, y0) is a convex combination of y0, y1: <= A, err 46A + A + A = 48A.
            h fma(b1, d0, b4 d1): b4 d1 err 21 |d1|; fma err 27 |d0| + 21 |d1| + |d0| + |d1| <= 28 B / h; times h: 29B.
            (h h) fma(b2, e0, b5 e1): b5 e1 err 3.5 |e1|; fma <= C / 2 h^2, err 4.5 |e0| + 3.5 |e1| + (|e0| + |e1|) / 2 <= 5 C / h^2;
            h h err 1: C / 2 + 5C + C / 2 = 6C.   Sums: 48A + 29B + (A + B) = 49A + 30B, then + 6C + (A + B + C / 2) = 50A + 31B + 6.5C
            ->  HERMITE5_C = 50 on A + B + C.
  fallback rate: u = fma(t, inv_tfb, 1) is ONE rounding of the exact value and the tests form the same double.  rcbrt_fast is
            held to 2 ulp (tests/test_gpu_math.py), relative rho = 4U.  mdot_fb: r2 = r r (2 rho + 1), r2 r2 (4 rho + 3), times r
            (5 rho + 4), times S_amp: 5 rho + 5 = 25.  mdot_fb_d: r3 = r2 r (3 rho + 2) = 14 = FALLBACK_IU_C against 1/u; r2 r3 (5 rho + 4),
            times S_amp: 25 = FALLBACK_S_C; dS = ((-5/3 rounded) inv_tfb) S r3: 2 + 25 + 1, + 14 + 1 = 43 = FALLBACK_DS_C against
            -(5/3) inv_tfb S_amp u^(-8/3).
  quasi-steady form: S_k = fma(M_k, 1/tvisc, D_k) one rounding of the exact value (1); rcp_fast 2 ulp (4); M_k iS_k (1): every ratio
            6; the fma chain from 0 adds 4 roundings of partial sums <= sum |w_k x_k|: r within 10 sum |w_k x_k|.  t = fma(th - 1, h, t1):
            th - 1 err 1 (times h), the fma |t|: |dt| <= h + |t| <= 1.02 |t| (h / t <= Q - 1 < 0.017); u = fma(t, inv_tfb, 1): within
            (1.02 + 1) U u of the exact u, which moves u^(-5/3) by 5/3 of that, < 5; with FALLBACK_S_C: Mdotfb within 30.  The product: 1.
            ->  |dMv| <= U (10 |S| sum |w_k x_k| + 31 |r S|).

Every count is first order in U; gamma(n) = n U / (1 - n U) carries the higher orders."""
import decimal
import functools
import math
from fractions import Fraction

import numpy as np

import math_restated as mr

U = 2.0 ** -53
KINDS, WTAB_STRIDE, WTAB_THETA = 5, 40, 32
WTAB_DENSE = KINDS * WTAB_STRIDE
WTAB_SIZE = WTAB_DENSE + 3 * 7 * 12
TTAB_N = 257
KTAB_N = 20
HERMITE_C, HERMITE_D_C, HERMITE5_C = 41, 90, 50
FALLBACK_S_C, FALLBACK_IU_C, FALLBACK_DS_C = 25, 14, 43
QS_SUM_C, QS_PROD_C = 10, 31

# every function libmp_probe_dense.so exports (magprop_amd/csrc/mp_probe_dense.hip); none of them belongs to libmagprop_amd.so
PROBE_EXPORTS = ("mpi_kinds", "mpi_wtab_size", "mpi_wtab_stride", "mpi_wtab_theta", "mpi_wtab_dense", "mpi_ttab_n", "mpi_ktab_n",
                 "mpi_max_n", "mpi_tables", "mpi_lds_tables", "mpi_hermite", "mpi_fallback", "mpi_image_state")
# kKtabInit of mp_math.hpp: 1/16! .. 1/3!, log2(e), -ln2_hi, -ln2_lo, pad, 1/17!, pad
KTAB = np.array([1.0 / math.factorial(16 - k) for k in range(14)] +
                [1.4426950408889634074, -6.93147180369123816490e-01, -1.90821492927058770002e-10, 0.0, 1.0 / math.factorial(17), 0.0])


def gamma(n):
    return n * U / (1.0 - n * U)


# ---------------------------------------------------------------- the host's tables, statement by statement in doubles
def ln_Q(lnq, kind):
    return lnq / 8.0 if kind == 0 else lnq * float(1 << (kind - 1))


def n_skip(kind):
    """Grid intervals per step (kind 0: an eighth of one, no grid point inside)."""
    return 1 if kind == 0 else 1 << (kind - 1)


def build_tables(lnq):
    """sk[5][3] (lnQ, 1/Q, 1 - 1/Q), wtab[WTAB_SIZE], ttab[4][257] as build_tables of mp_capi.cpp forms them (libm exp and expm1)."""
    sk = np.zeros((KINDS, 3))
    wtab = mr.wtab(lnq)                                   # the quadrature rows
    ttab = np.zeros((KINDS - 1, TTAB_N))
    for kind in range(KINDS):
        lnQ = ln_Q(lnq, kind)
        sk[kind] = lnQ, math.exp(-lnQ), -math.expm1(-lnQ)
        ns = n_skip(kind)
        T = kind * WTAB_STRIDE
        for i in range(8):
            wtab[T + WTAB_THETA + i] = math.expm1(lnq * float(i)) / math.expm1(lnQ) if (i < ns and ns > 1) else 0.0
        if kind >= 2:
            Q = math.exp(lnQ)
            nodes = ((0.0, 1.0, 1.0 + Q, 1.0 + Q + Q * Q), (-1.0 / Q, 0.0, 1.0, 1.0 + Q), (-1.0 / Q - 1.0 / (Q * Q), -1.0 / Q, 0.0, 1.0))
            for i in range(1, ns):
                th = wtab[T + WTAB_THETA + i]
                for v in range(3):
                    for k in range(4):
                        l = 1.0
                        for m in range(4):
                            if m != k:
                                l *= (th - nodes[v][m]) / (nodes[v][k] - nodes[v][m])
                        wtab[WTAB_DENSE + ((kind - 2) * 7 + (i - 1)) * 12 + v * 4 + k] = l
        if kind >= 1:
            for k in range(TTAB_N):
                ttab[kind - 1, k] = math.exp(float(k) * lnQ)
    return dict(sk=sk, wtab=wtab, ttab=ttab)


def used_wtab_mask():
    """Which entries of wtab the layout of mp_device.h uses."""
    used = np.zeros(WTAB_SIZE, dtype=bool)
    for kind in range(KINDS):
        for k in range(5):
            used[kind * WTAB_STRIDE + 6 * k: kind * WTAB_STRIDE + 6 * k + 5] = True
        for i in range(1, n_skip(kind)):
            used[kind * WTAB_STRIDE + WTAB_THETA + i] = True
            d = WTAB_DENSE + ((kind - 2) * 7 + (i - 1)) * 12
            used[d: d + 12] = True
    return used


# Relative bounds of the host's table entries against their exact values (functions of the double lnq), in units of U.  glibc's exp
# and expm1 are within 1 ulp, relative 2 U.
#   invq, omi  one call on an exact argument (lnQ is lnq times a power of two): 2.
#   theta      expm1(fl(lnq i)) / expm1(lnQ): the argument's rounding (1, times the condition x e^x / (e^x - 1) < 1.01 of expm1) and the
#              call (2); the denominator (2); the division (1): 6.01 -> 7.
#   ttab       exp(fl(k lnQ)): the argument's rounding moves the value by k lnQ U, the call 2: 2 + k lnQ.
#   dense      a product of three fl((th - n_m) / (n_k - n_m)).  th carries 7 (times th < 1), a node at most 8 in absolute terms
#              (Q: 2; 1 + Q + Q Q < 3.1: 2 Q + 2 Q^2 + Q^2 + 3.1 + 2.1 < 12.5 on a magnitude of 3, the worst; the others less);
#              |th - n_m| >= 0.117 (theta_1 of kind 4 on the "S" grid, the smallest distance to a node, 0), |n_k - n_m| >= 0.98:
#              a factor carries (7 + 12.5) / 0.117 + 1 + (12.5 + 12.5) / 0.98 + 1 + 1 < 196; three of them and two products: < 590 -> 600.
TABLE_C = {"invq": 2.0, "omi": 2.0, "theta": 7.0, "dense": 600.0}


def table_errors(T, g, name):
    """The tables T (sk, wtab, ttab: the product's, or build_tables' here) against the fixture g of grid `name`: a list of
    (label, worst |error| / bound, bound's count) with the bounds above; every ratio must be <= 1."""
    out = []
    lnq = float(g[f"lnq_{name}"][0])
    hi, lo = g[f"invq_{name}_hi"], g[f"invq_{name}_lo"]
    out.append(("invq", (mr.err_rel(T["sk"][:, 1], hi, lo) / gamma(TABLE_C["invq"])).max(), TABLE_C["invq"]))
    hi, lo = g[f"omi_{name}_hi"], g[f"omi_{name}_lo"]
    out.append(("omi", (mr.err_rel(T["sk"][:, 2], hi, lo) / gamma(TABLE_C["omi"])).max(), TABLE_C["omi"]))
    th = np.array([T["wtab"][k * WTAB_STRIDE + WTAB_THETA: k * WTAB_STRIDE + WTAB_THETA + 8] for k in range(KINDS)]).ravel()
    hi, lo = g[f"theta_{name}_hi"], g[f"theta_{name}_lo"]
    assert np.array_equal(th == 0.0, hi == 0.0)
    out.append(("theta", (mr.err_rel(th, hi, lo) / gamma(TABLE_C["theta"])).max(), TABLE_C["theta"]))
    hi, lo = g[f"dense_{name}_hi"], g[f"dense_{name}_lo"]
    dw = T["wtab"][WTAB_DENSE:]
    assert np.array_equal(dw == 0.0, hi == 0.0)
    out.append(("dense", (mr.err_rel(dw, hi, lo) / gamma(TABLE_C["dense"])).max(), TABLE_C["dense"]))
    hi, lo = g[f"ttab_{name}_hi"], g[f"ttab_{name}_lo"]
    c = np.array([[2.0 + k * ln_Q(lnq, kind) for k in range(TTAB_N)] for kind in range(1, KINDS)])
    out.append(("ttab", (mr.err_rel(T["ttab"].ravel(), hi, lo) / (c.ravel() * U / (1.0 - c.ravel() * U))).max(), float(c.max())))
    return out


def w5_errors(T, g, name):
    """|W5 of the tables T - exact| per entry, relative to the largest |W5| of its kind: array [5][25]."""
    hi, lo = g[f"w5_{name}_hi"].reshape(KINDS, 25), g[f"w5_{name}_lo"].reshape(KINDS, 25)
    W = np.array([[T["wtab"][kind * WTAB_STRIDE + 6 * k + m] for k in range(5) for m in range(5)] for kind in range(KINDS)])
    L = np.longdouble
    d = np.abs((W.astype(L) - hi.astype(L)) - lo.astype(L))
    return (d / np.abs(hi).max(axis=1, keepdims=True).astype(L)).astype(np.float64)


# ---------------------------------------------------------------- exact arithmetic
def solve(A, b):
    """x of A x = b over the rationals (Gauss-Jordan with the first non-zero pivot)."""
    n = len(A)
    M = [[Fraction(v) for v in row] + [Fraction(b[r])] for r, row in enumerate(A)]
    for c in range(n):
        p = next(r for r in range(c, n) if M[r][c] != 0)
        M[c], M[p] = M[p], M[c]
        M[c] = [v / M[c][c] for v in M[c]]
        for r in range(n):
            if r != c and M[r][c] != 0:
                M[r] = [a - M[r][c] * pv for a, pv in zip(M[r], M[c])]
    return [M[r][n] for r in range(n)]


@functools.lru_cache(maxsize=None)
def _hermite_system(m):
    """Rows of the 2 m end conditions of a polynomial sum a_j s^j on [0, 1]: its derivatives 0 .. m - 1 at s = 0, then at s = 1."""
    n = 2 * m
    return tuple(tuple(Fraction(math.perm(j, r)) * (Fraction(x) ** (j - r) if j > r else Fraction(int(j == r))) if j >= r else Fraction(0)
                       for j in range(n)) for x in (0, 1) for r in range(m))


def hermite_coeffs(h, left, right):
    """Coefficients a_j of the polynomial in s = (t - t_0) / h whose value and derivatives with respect to TIME at s = 0 are `left`
    and at s = 1 `right` (two entries each: the cubic; three: the quintic), from the end conditions themselves."""
    m = len(left)
    assert m == len(right) and m in (2, 3)
    h = Fraction(h)
    rhs = [Fraction(v) * h ** r for r, v in enumerate(left)] + [Fraction(v) * h ** r for r, v in enumerate(right)]
    return solve(_hermite_system(m), rhs)


def hermite_exact(th, h, left, right, deriv=False):
    """The Hermite interpolant (its time derivative) at the fraction th of a step of length h, exactly."""
    a, th = hermite_coeffs(h, left, right), Fraction(th)
    if deriv:
        return sum(j * a[j] * th ** (j - 1) for j in range(1, len(a))) / Fraction(h)
    return sum(a[j] * th ** j for j in range(len(a)))


def dense_nodes(Q, variant):
    """The four nodes around a step in units of the step, origin at its start, consecutive steps growing by Q; the step is the
    first (variant 0), middle (1) or last (2) of their three intervals."""
    Q = Fraction(Q)
    return ((0, 1, 1 + Q, 1 + Q + Q * Q), (-1 / Q, 0, 1, 1 + Q), (-1 / Q - 1 / (Q * Q), -1 / Q, 0, 1))[variant]


def lagrange_weights(th, nodes):
    """w_k with sum w_k p(x_k) = p(th) for every cubic p: the Vandermonde system."""
    return solve([[Fraction(x) ** j for x in nodes] for j in range(4)], [Fraction(th) ** j for j in range(4)])


def pow_m53(u, extra=0):
    """u^(-5/3 - extra) of a rational u > 0 to 60 digits."""
    with decimal.localcontext() as c:
        c.prec = 60
        d = decimal.Decimal(u.numerator) / decimal.Decimal(u.denominator)
        return Fraction((d.ln() * (decimal.Decimal(-5) / decimal.Decimal(3) - extra)).exp())


def fallback_exact(S_amp, inv_tfb, u):
    """S, dS / dt, 1 / u of the fallback rate at the rational u = 1 + t / tfb."""
    u = Fraction(u)
    S = Fraction(S_amp) * pow_m53(u)
    return S, Fraction(-5, 3) * Fraction(inv_tfb) * S / u, 1 / u


# ---------------------------------------------------------------- image_state
def index(kind, pos8, keep, p8):
    """The integers of image_state and dense_mdisc_qs for one query."""
    sh8 = 0 if kind == 0 else kind + 2
    rel = p8 - pos8
    J = rel >> sh8
    rem = rel - (J << sh8)
    i = (rem >> 3) & 7
    l0 = max(min(J - 1, keep - 3), 0)
    variant = J - l0
    base = WTAB_DENSE + ((kind - 2) * 7 + (i - 1)) * 12 + variant * 4
    return dict(sh8=sh8, J=J, rem=rem, i=i, l0=l0, variant=variant, base=base)


def legal(kind, pos8, keep, p8, G):
    sh8 = 0 if kind == 0 else kind + 2
    return 0 <= kind < KINDS and 1 <= keep <= 64 * G and pos8 <= p8 <= pos8 + (keep << sh8) and (kind == 0 or (p8 - pos8) % 8 == 0)


def read_out(T, walker, kind, pos8, keep, t_s, img, p8):
    """(Mv, Wv) of one legal query, exactly, on the doubles of the tables T (sk, wtab, ttab), the walker (inv_tau, S_amp, inv_tfb)
    and the image img[5][nodes] (W, F, M, D, D2), with the branch taken and the rounding bounds of the device's evaluation.
    Returns a dict: branch ("node", "quintic", "cubic", "qs"), J, i, variant, z, th, h, Mv, Wv (Fraction), bM, bW (float)."""
    inv_tau, S_amp, inv_tfb = (float(v) for v in walker)
    W, F, M, D, D2 = img
    ix = index(kind, pos8, keep, p8)
    J = ix["J"]
    out = dict(ix, branch="node", z=None, th=None, h=None, Mv=Fraction(float(M[J])), Wv=Fraction(float(W[J])), bM=0.0, bW=0.0)
    if ix["rem"] == 0:
        return out
    assert kind >= 2 and 1 <= ix["i"] < n_skip(kind) and J + 1 <= keep
    th = float(T["wtab"][kind * WTAB_STRIDE + WTAB_THETA + ix["i"]])
    t1 = float(np.float64(t_s) * np.float64(T["ttab"][kind - 1, J + 1]))
    h = float(np.float64(t1) * np.float64(T["sk"][kind, 2]))
    z = float(np.float64(h) * np.float64(inv_tau))
    out.update(z=z, th=th, h=h)
    y0, y1 = (float(M[J]), float(D[J]), float(D2[J])), (float(M[J + 1]), float(D[J + 1]), float(D2[J + 1]))
    A, B, C = abs(y0[0]) + abs(y1[0]), h * (abs(y0[1]) + abs(y1[1])), h * h * (abs(y0[2]) + abs(y1[2]))
    if z < 1.0:
        out.update(branch="quintic", Mv=hermite_exact(th, h, y0, y1), bM=gamma(HERMITE5_C) * (A + B + C))
    elif keep < 3:
        out.update(branch="cubic", Mv=hermite_exact(th, h, y0[:2], y1[:2]), bM=gamma(HERMITE_C) * (A + B))
    else:
        l0, v = ix["l0"], ix["variant"]
        assert 0 <= v <= 2 and l0 + 3 <= keep
        w = [Fraction(float(T["wtab"][ix["base"] + k])) for k in range(4)]
        x = [Fraction(float(M[l0 + k])) / (Fraction(float(M[l0 + k])) * Fraction(inv_tau) + Fraction(float(D[l0 + k]))) for k in range(4)]
        r = sum(wk * xk for wk, xk in zip(w, x))
        t = (Fraction(th) - 1) * Fraction(h) + Fraction(t1)
        S = fallback_exact(S_amp, inv_tfb, t * Fraction(inv_tfb) + 1)[0]
        out.update(branch="qs", Mv=r * S, bM=gamma(QS_SUM_C) * float(abs(S) * sum(abs(wk * xk) for wk, xk in zip(w, x))) +
                   gamma(QS_PROD_C) * float(abs(r * S)))
    w0, w1 = (float(W[J]), float(F[J])), (float(W[J + 1]), float(F[J + 1]))
    out.update(Wv=hermite_exact(th, h, w0, w1), bW=gamma(HERMITE_C) * (abs(w0[0]) + abs(w1[0]) + h * (abs(w0[1]) + abs(w1[1]))))
    return out


def err(got, exact):
    """|got - exact| of a double against a rational, as a double (rounded once)."""
    return float(abs(Fraction(float(got)) - exact))
