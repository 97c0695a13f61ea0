"""Writes tests/golden/golden_dense.npz: what the read-out of a kept tile (magprop_amd/csrc/mp_eval.hpp image_state and the
functions under it) and the host-built tables it indexes (mp_capi.cpp build_tables) are held to, from mpmath at 400 bits, values
as double-double pairs hi = float(v), lo = float(v - hi).

    python tests/golden/make_dense_golden.py          # rewrites the fixture and its entry in MANIFEST.json

For the synthetic grid "L" (logspace(0, 6, 10001)) and the "S" grid (logspace(-3, 6, 10001)):

  tables   as exact functions of the DOUBLE lnq the product forms (log(t[-1] / t[0]) / (n - 1)): per kind theta_i, exp(-lnQ),
           1 - exp(-lnQ), the 25 quadrature weights W5; the 3 x 7 x 12 dense-output Lagrange weights; exp(k lnQ), k = 0 .. 256, of
           kinds 1 .. 4.
  traj     tiles of the true solution of dM/dt = S_amp (1 + t inv_tfb)^(-5/3) - M inv_tau (by Gauss-Legendre quadrature of its
           variation-of-constants integral, grid interval by grid interval; one case is cross-checked against a Taylor-series
           solution of the ODE) and of omega(t) = W0 (1 + t inv_tsd)^(-1/2), sampled at the step ends t_s Q^k of a tile and at
           every skipped grid point, with D = dM/dt, D2 = d2M/dt2 and F = domega/dt there.  The regimes (CASES): the transition
           a few viscous times after the start where every step resolves the viscous time (quintic), a tile inside which
           z = h / tvisc crosses 1, quasi-steady tiles (z >= 1) of 8, 3, 2 and 1 kept steps, and a deep quasi-steady one.

numpy and mpmath only.  tables(grid) and traj_case(name) return the arrays of one part, so a test can regenerate a slice
(tests/test_dense_cases_cpu.py)."""
import json
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PREC = 400
KINDS, WTAB_STRIDE, WTAB_THETA, TTAB_N = 5, 40, 32, 257
GRIDS = {"L": (0.0, 6.0), "S": (-3.0, 6.0)}
N_GRID = 10001
META = ("grid", "kind", "g0", "keep", "inv_tau", "S_amp", "inv_tfb", "t_s", "M_init", "W0", "inv_tsd")
# regime -> (start time of the tile in seconds, kept steps, inv_tau or None: 1 / (length of step keep / 2), so that z crosses 1 there)
REGIMES = {"quintic": (100.0, 12, 0.05), "cross": (1000.0, 16, None), "qs": (1000.0, 8, 1.0), "qs3": (1000.0, 3, 1.0),
           "qs2": (1000.0, 2, 1.0), "qs1": (1000.0, 1, 1.0), "qsdeep": (1000.0, 8, 10.0)}
S_AMP, INV_TFB, M_INIT = 2.0e29, 0.01, 2.0e30          # g/s, 1/s, g: a disc of 1e-3 solar masses, tfb = 100 s
W0, INV_TSD = 6283.185307179586, 1.0 / 300.0            # a 1 ms spin period, spin-down time 300 s
CASES = tuple(f"{g}{k}_{r}" for g in GRIDS for k in (2, 3, 4) for r in REGIMES)


def _mp():
    import mpmath
    mpmath.mp.prec = PREC
    return mpmath


def dd(mp, values):
    """hi, lo arrays of a list of mpf."""
    hi = np.array([float(v) for v in values])
    lo = np.array([float(v - mp.mpf(h)) for v, h in zip(values, hi)])
    return hi, lo


def grid(name):
    """The grid and the double lnq that mp_create forms from it."""
    t = np.logspace(*GRIDS[name], num=N_GRID, base=10.0)
    return t, math.log(t[-1] / t[0]) / float(N_GRID - 1)


def ln_Q(lnq, kind):
    return lnq / 8.0 if kind == 0 else lnq * float(1 << (kind - 1))      # (exact: powers of two)


# ---------------------------------------------------------------- tables
def _w5(mp, Q):
    """W[k][m] = m! [theta^m] l_k(theta), l_k the Lagrange basis on the nodes 1, 0, -1/Q, -(1/Q + 1/Q^2), -(.. + 1/Q^3)."""
    x = [mp.mpf(1), mp.mpf(0), -1 / Q, -1 / Q - 1 / Q ** 2, -1 / Q - 1 / Q ** 2 - 1 / Q ** 3]
    W = []
    for k in range(5):
        co, den = [mp.mpf(1)], mp.mpf(1)
        for j in range(5):
            if j == k:
                continue
            co = [(co[m - 1] if m >= 1 else 0) - x[j] * (co[m] if m < len(co) else 0) for m in range(len(co) + 1)]
            den *= x[k] - x[j]
        W.append([mp.factorial(m) * co[m] / den for m in range(5)])
    return W


def dense_nodes(Q):
    """The four nodes around a step (times in units of the step, origin at its start; consecutive steps grow by Q), the step
    being the first / middle / last of their three intervals."""
    return ((0, 1, 1 + Q, 1 + Q + Q * Q), (-1 / Q, 0, 1, 1 + Q), (-1 / Q - 1 / (Q * Q), -1 / Q, 0, 1))


def tables(name):
    mp = _mp()
    _, lnq = grid(name)
    q = mp.mpf(lnq)
    theta, inv_q, omi, w5, dense, ttab = [], [], [], [], [mp.mpf(0)] * (3 * 7 * 12), []
    for kind in range(KINDS):
        lnQ = mp.mpf(ln_Q(lnq, kind))
        Q = mp.exp(lnQ)
        ns = 1 if kind == 0 else 1 << (kind - 1)
        th = [mp.expm1(q * i) / mp.expm1(lnQ) if (i < ns and ns > 1) else mp.mpf(0) for i in range(8)]
        theta += th
        inv_q.append(mp.exp(-lnQ))
        omi.append(-mp.expm1(-lnQ))
        w5 += [v for row in _w5(mp, Q) for v in row]
        if kind >= 2:
            for i in range(1, ns):
                for v, nodes in enumerate(dense_nodes(Q)):
                    for k in range(4):
                        l = mp.mpf(1)
                        for m in range(4):
                            if m != k:
                                l *= (th[i] - nodes[m]) / (nodes[k] - nodes[m])
                        dense[((kind - 2) * 7 + (i - 1)) * 12 + v * 4 + k] = l
        if kind >= 1:
            ttab += [mp.exp(lnQ * k) for k in range(TTAB_N)]
    out = {f"lnq_{name}": np.array([lnq])}
    for key, vals in (("theta", theta), ("invq", inv_q), ("omi", omi), ("w5", w5), ("dense", dense), ("ttab", ttab)):
        out[f"{key}_{name}_hi"], out[f"{key}_{name}_lo"] = dd(mp, vals)
    return out


# ---------------------------------------------------------------- trajectories
def case_meta(name):
    """The numbers of a case, all of them doubles (META)."""
    g, kind, regime = name[0], int(name[1]), name[3:]
    t, lnq = grid(g)
    t_start, keep, inv_tau = REGIMES[regime]
    g0 = int(round(math.log(t_start / t[0]) / lnq))
    t_s = float(t[g0])
    if inv_tau is None:
        lnQ = ln_Q(lnq, kind)
        inv_tau = 1.0 / (t_s * math.exp(lnQ * (keep // 2)) * -math.expm1(-lnQ))
    return dict(zip(META, (float("LS".index(g)), float(kind), float(g0), float(keep), inv_tau, S_AMP, INV_TFB, t_s, M_INIT, W0, INV_TSD)))


def _fallback(mp, m, t, n=0):
    """The n-th time derivative of S_amp (1 + t inv_tfb)^(-5/3)."""
    c = mp.mpf(1)
    for j in range(n):
        c *= -(mp.mpf(5) / 3 + j) * m["inv_tfb"]
    return m["S_amp"] * c * mp.power(1 + t * m["inv_tfb"], -(mp.mpf(5) / 3 + n))


def _advance(mp, m, t0, M0, t1):
    """M(t1) from M(t0): the variation-of-constants integral over pieces of at most four viscous times."""
    if t1 == t0:
        return M0
    pieces = max(1, int(mp.ceil((t1 - t0) * m["inv_tau"] / 4)))
    pts = [t0 + (t1 - t0) * j / pieces for j in range(pieces + 1)]
    val, err = mp.quad(lambda s: mp.exp(-(t1 - s) * m["inv_tau"]) * _fallback(mp, m, s), pts, method="gauss-legendre", error=True)
    assert err <= mp.mpf(10) ** -60 * abs(val), (err, val)
    return mp.exp(-(t1 - t0) * m["inv_tau"]) * M0 + val


def _start(mp, m, t):
    """M(t) of the solution with M(0) = M_init: what lies more than 300 viscous times back has decayed by e^-300."""
    lo = max(mp.mpf(0), t - 300 / m["inv_tau"])
    return _advance(mp, m, lo, m["M_init"] if lo == 0 else mp.mpf(0), t)


def _taylor(mp, m, t0, M0, t1):
    """The same step by the Taylor series of the solution about t0: M^(n+1) = S^(n) - M^(n) inv_tau."""
    d, term, total, Mn, n = t1 - t0, mp.mpf(1), mp.mpf(0), M0, 0
    while True:
        add = Mn * term
        total += add
        Mn = _fallback(mp, m, t0, n) - Mn * m["inv_tau"]
        n += 1
        term = term * d / n
        if n > 40 and abs(add) < abs(total) * mp.mpf(2) ** -(PREC - 10):
            return total


def traj_case(name, check=False):
    mp = _mp()
    md = case_meta(name)
    m = {k: mp.mpf(v) for k, v in md.items()}
    _, lnq = grid(name[0])
    kind, keep = int(md["kind"]), int(md["keep"])
    ns = 1 << (kind - 1)
    t = [m["t_s"] * mp.exp(mp.mpf(lnq) * p) for p in range(keep * ns + 1)]
    M = [_start(mp, m, t[0])]
    for p in range(1, len(t)):
        M.append(_advance(mp, m, t[p - 1], M[-1], t[p]))
        if check:
            ty = _taylor(mp, m, t[p - 1], M[-2], t[p])
            assert abs(ty - M[-1]) <= mp.mpf(10) ** -50 * abs(ty), (name, p)
    D = [_fallback(mp, m, tp) - Mp * m["inv_tau"] for tp, Mp in zip(t, M)]
    D2 = [_fallback(mp, m, tp, 1) - Dp * m["inv_tau"] for tp, Dp in zip(t, D)]
    W = [m["W0"] / mp.sqrt(1 + tp * m["inv_tsd"]) for tp in t]
    F = [-m["W0"] * m["inv_tsd"] / 2 * mp.power(1 + tp * m["inv_tsd"], mp.mpf(-3) / 2) for tp in t]
    out = {f"traj_{name}_meta": np.array([md[k] for k in META])}
    for key, vals in (("t", t), ("M", M), ("W", W)):
        out[f"traj_{name}_{key}_hi"], out[f"traj_{name}_{key}_lo"] = dd(mp, vals)
    for key, vals in (("D", D), ("D2", D2), ("F", F)):
        out[f"traj_{name}_{key}"] = np.array([float(v) for v in vals])
    return out


def main():
    mp = _mp()
    arrays = {}
    for g in GRIDS:
        arrays.update(tables(g))
    for i, name in enumerate(CASES):
        arrays.update(traj_case(name, check=name == "S4_cross"))
        print(name, flush=True)
    path = os.path.join(HERE, "golden_dense.npz")
    np.savez_compressed(path, **arrays)
    mpath = os.path.join(HERE, "MANIFEST.json")
    man = json.load(open(mpath))
    man["golden_dense.npz"] = {"generator": "tests/golden/make_dense_golden.py", "mpmath": mp.__version__,
                               "precision_bits": PREC, "numpy": np.__version__, "python": "%d.%d.%d" % sys.version_info[:3]}
    with open(mpath, "w") as f:
        json.dump(man, f, indent=1)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
