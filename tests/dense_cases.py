"""Crafted inputs of the tile read-out tests (tests/test_dense_cases_cpu.py on the restatement alone, tests/test_gpu_dense_kernels.py
on the device through libmp_probe_dense.so): tiles and queries for image_state, elements for the Hermite forms and the fallback
rate, the branch coverage the tiles must reach (judged on tests/dense_restated.py), and the trajectory cases of
tests/golden/golden_dense.npz as tiles.  numpy only; everything is built from SEED."""
import math
import os

import numpy as np

import dense_restated as dr
import math_restated as mr

SEED = 20261019
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_dense.npz")
GRIDS = {"L": (0.0, 6.0), "S": (-3.0, 6.0)}
N_GRID = 10001
LDS_INSTANCES = ((2, 64), (4, 64), (4, 128), (4, 256))      # (G, NT) of tables_init in the kernels
S_AMP, INV_TFB, W0, INV_TSD = 2.0e29, 0.01, 6283.185307179586, 1.0 / 300.0

# Method bounds of the read-out against the true solution, relative to |M| (|omega|), per (branch, kind): 2 x the largest error of the
# EXACT-arithmetic read-out (tests/dense_restated.py on the restated tables) over the trajectory cases of the fixture, measured by
# tests/test_dense_cases_cpu.py test_method_bounds_are_the_measured_ones, which fails when a figure here is not 2 x (to two digits,
# rounded up) what it measures.  DESIGN.md section 5 sets them against the source's own claims.
METHOD_MEASURED = {("cubic", 2): 4.1e-11, ("cubic", 3): 6.5e-10, ("cubic", 4): 1.1e-08, ("omega", 2): 1.9e-12, ("omega", 3): 3.2e-11, ("omega", 4): 5.7e-10,
                   ("qs", 2): 1.3e-12, ("qs", 3): 4.2e-11, ("qs", 4): 1.6e-09, ("quintic", 2): 2.4e-16, ("quintic", 3): 1.3e-14, ("quintic", 4): 8.6e-13}
METHOD_BOUNDS = {k: 2.0 * v for k, v in METHOD_MEASURED.items()}
# the source's claims (mp_eval.hpp, above hermite5 and hermite_mdisc): the cubic 2e-10 on the quasi-steady power law, 1e-9 off in
# the transition at stride 4 (kind 3) where the quintic is not
CLAIM_CUBIC_QS, CLAIM_CUBIC_TRANSITION = 2.0e-10, 1.0e-9


def grid(name):
    """The grid and the double lnq mp_create forms from it."""
    t = np.logspace(*GRIDS[name], num=N_GRID, base=10.0)
    return t, math.log(t[-1] / t[0]) / float(N_GRID - 1)


# ---------------------------------------------------------------- image_state
def _image(t, inv_tau, kN, keep):
    """A smooth image on the node times t[0 .. keep]: Mdisc = (S / inv_tau) (1 + a), a = cos(ln t) / 4, so that the fallback rate
    D + M inv_tau the quasi-steady form divides by is S itself; NaN at every node beyond keep."""
    img = np.full((5, kN), np.nan)
    u = 1.0 + t * INV_TFB
    S = S_AMP * u ** (-5.0 / 3.0)
    a = 0.25 * np.cos(np.log(t))
    M = S / inv_tau * (1.0 + a)
    D = -a * S
    img[0, :keep + 1] = W0 / np.sqrt(1.0 + t * INV_TSD)
    img[1, :keep + 1] = -0.5 * W0 * INV_TSD * (1.0 + t * INV_TSD) ** -1.5
    img[2, :keep + 1] = M
    img[3, :keep + 1] = D
    img[4, :keep + 1] = -(5.0 / 3.0) * INV_TFB * S / u - D * inv_tau
    return img


def _queries(kind, pos8, keep, steps):
    """Every node of the kept part, and every skipped grid point of the steps listed."""
    sh8 = 0 if kind == 0 else kind + 2
    p8 = [pos8 + (J << sh8) for J in range(keep + 1)]
    for J in sorted(set(steps)):
        assert 0 <= J < keep
        p8 += [pos8 + (J << sh8) + 8 * i for i in range(1, dr.n_skip(kind))]
    return np.array(p8, dtype=np.int32)


def tiles(gname, kind, G):
    """The tiles of one (grid, kind, G): dicts name, walker (inv_tau, S_amp, inv_tfb), kind, pos8, keep, t_s, img[5][64 G + 1], p8.
    Kinds 0 and 1 have nodes only; kinds 2 .. 4 a full tile (keep = 64 G) and partial ones of 37 and 3 kept steps where every
    step is longer than the viscous time, tiles of 1 and 2 kept steps there, one where every step resolves the viscous time,
    and one inside which z = h / tvisc crosses 1."""
    tg, lnq = grid(gname)
    kN, full = 64 * G + 1, 64 * G
    lnQ = dr.ln_Q(lnq, kind)
    omi = -math.expm1(-lnQ)
    out = []

    def add(name, g0_8, keep, z_at, z, steps):
        # a tile that starts at position g0_8 (eighths of a grid interval) and whose step z_at has h / tvisc = z
        t_s = float(tg[0] * math.exp(lnq / 8.0 * g0_8))
        t = t_s * np.exp(lnQ * np.arange(keep + 1))
        inv_tau = z / (t[z_at + 1] * omi)
        out.append(dict(name=name, walker=(inv_tau, S_AMP, INV_TFB), kind=kind, pos8=g0_8, keep=keep, t_s=t_s,
                        img=_image(t, inv_tau, kN, keep), p8=_queries(kind, g0_8, keep, steps)))

    if kind == 0:
        add("full", 8 * 3, full, 0, 3.0, [])
        add("keep37", 5, 37, 0, 0.2, [])
        return out
    g0 = 8 * (1200 if gname == "L" else 2400)
    if kind == 1:
        add("full", g0, full, 0, 3.0, [])
        add("keep37", g0 + 8, 37, 0, 0.2, [])
        return out
    add("qs_full", g0, full, 0, 1.5, [0, 1, 2, full // 2, full - 3, full - 2, full - 1])
    add("qs_keep37", g0 + 8 * 7, 37, 0, 3.0, [0, 1, 35, 36])
    add("qs_keep3", g0, 3, 0, 2.0, [0, 1, 2])
    add("cubic_keep2", g0, 2, 0, 2.0, [0, 1])
    add("cubic_keep1", g0 + 16, 1, 0, 40.0, [0])
    add("quintic", g0, 20, 19, 0.5, [0, 1, 10, 18, 19])
    add("quintic_keep2", g0, 2, 1, 0.9, [0, 1])
    add("cross", g0, 24, 12, 1.0, [0, 10, 11, 12, 13, 14, 22, 23])
    return out


def golden_tiles(g, G, only=None):
    """The trajectory cases of the fixture as tiles (images of the true solution rounded to doubles), each with the true values
    at its queries: extra keys truth_M, truth_W (hi, lo pairs by query) and regime."""
    out = []
    for key in g.files:
        if not key.endswith("_meta"):
            continue
        name = key[len("traj_"):-len("_meta")]
        if only is not None and name not in only:
            continue
        m = dict(zip(("grid", "kind", "g0", "keep", "inv_tau", "S_amp", "inv_tfb", "t_s", "M_init", "W0", "inv_tsd"), g[key]))
        kind, keep, g0 = int(m["kind"]), int(m["keep"]), int(m["g0"])
        ns = dr.n_skip(kind)
        img = np.full((5, 64 * G + 1), np.nan)
        node = np.arange(keep + 1) * ns
        for row, f in enumerate(("W_hi", "F", "M_hi", "D", "D2")):
            img[row, :keep + 1] = g[f"traj_{name}_{f}"][node]
        p = np.arange(keep * ns + 1)
        out.append(dict(name=name, regime=name[3:], walker=(m["inv_tau"], m["S_amp"], m["inv_tfb"]), kind=kind, pos8=8 * g0, keep=keep,
                        t_s=m["t_s"], img=img, p8=(8 * g0 + 8 * p).astype(np.int32),
                        truth_M=(g[f"traj_{name}_M_hi"], g[f"traj_{name}_M_lo"]), truth_W=(g[f"traj_{name}_W_hi"], g[f"traj_{name}_W_lo"])))
    return out


def restate(T, tile):
    """dense_restated.read_out of every query of a tile."""
    return [dr.read_out(T, tile["walker"], tile["kind"], tile["pos8"], tile["keep"], tile["t_s"], tile["img"], int(p)) for p in tile["p8"]]


def coverage(kind, G, tile, results):
    """What the queries of a tile reach, as tags, judged on the restatement's results."""
    keep, tags = tile["keep"], set()
    full = keep == 64 * G
    for r in results:
        J, b = r["J"], r["branch"]
        if b == "node":
            tags.add("node_first" if J == 0 else "node_last" if J == keep else "node_inner")
            if J == keep and full:
                tags.add("node_last_clamped")
            continue
        tags.add(f"{b}_i{r['i']}")
        tags.add(b)
        if b == "cubic":
            tags.add(f"cubic_keep{keep}")
        if b == "qs":
            tags.add(f"qs_v{r['variant']}")
            if keep == 3:
                tags.add(f"qs_keep3_v{r['variant']}")
            if full:
                tags.add(f"qs_full_v{r['variant']}")
            if J == 0:
                tags.add("qs_first_step")
            if J == keep - 1:
                tags.add("qs_last_step")
    if {"quintic", "qs"} <= tags:
        tags.add("z_crosses_1")
    return tags


def required(kind):
    """The tags the tiles of a kind must reach between them."""
    need = {"node_first", "node_inner", "node_last", "node_last_clamped"}
    if kind < 2:
        return need
    need |= {"quintic", "cubic_keep1", "cubic_keep2", "qs_first_step", "qs_last_step", "z_crosses_1"}
    need |= {f"{s}_v{v}" for s in ("qs", "qs_keep3", "qs_full") for v in range(3)}
    need |= {f"{b}_i{i}" for b in ("quintic", "cubic", "qs") for i in range(1, dr.n_skip(kind))}
    return need


# ---------------------------------------------------------------- Hermite forms
def hermite_cases(thetas):
    """Elements (th, h, z, y0, d0, e0, y1, d1, e1) in blocks, as a dict of name -> array [9][n]:
    th0 / th1: the ends; th1 also with h a power of two; poly: data of integer polynomials of degree <= 3 and <= 5 on integer
    nodes, exact in doubles; random: unit-scale data; physical: Mdisc ~ 1e30 g, h from 1e-3 to 1e4 s, every theta given (the
    product's table) and random ones; switch: z on both sides of 1."""
    rng = np.random.default_rng([SEED, 1])
    thetas = np.asarray(thetas, float)
    out = {}

    def rand(n, scale=1.0):
        return scale * rng.standard_normal(n)

    def block(th, h, z=None, scale=(1.0, 1.0, 1.0)):
        n = len(th)
        y, d, e = scale
        return np.array([th, h, np.full(n, 0.5) if z is None else z, rand(n, y), rand(n, d), rand(n, e), rand(n, y), rand(n, d), rand(n, e)])

    n = 64
    h = np.exp(rng.uniform(math.log(1e-3), math.log(1e4), n))
    out["th0"] = block(np.zeros(n), h)
    out["th0_pow2"] = block(np.zeros(n), np.ldexp(1.0, rng.integers(-10, 14, n)))
    out["th1"] = block(np.ones(n), h)
    # integer polynomials p of degree deg on [t0, t0 + h], t0 and h small integers: every datum is an integer below 2^53
    rows = []
    for deg in (0, 1, 2, 3, 4, 5):
        for _ in range(12):
            c = rng.integers(-9, 10, deg + 1)
            c[-1] = c[-1] or 1
            p = np.polynomial.Polynomial(c.astype(float))
            t0, hh = float(rng.integers(-3, 4)), float(rng.integers(1, 5))
            vals = [f(x) for x in (t0, t0 + hh) for f in (p, p.deriv(1), p.deriv(2))]
            rows.append([rng.uniform(0.0, 1.0), hh, 0.5] + vals + [float(deg), t0] + list(np.pad(c.astype(float), (0, 5 - deg))))
    rows = np.array(rows).T
    out["poly"] = rows[:9]
    out["poly_aux"] = rows[9:]                             # degree, t0, the six coefficients
    th = np.concatenate([thetas, rng.uniform(0.0, 1.0, 96 - len(thetas) % 96)])
    n = len(th)
    out["random"] = block(th, np.exp(rng.uniform(math.log(1e-3), math.log(1e4), n)))
    h = np.exp(rng.uniform(math.log(1e-3), math.log(1e4), n))
    tau = np.exp(rng.uniform(math.log(1e-2), math.log(1e3), n))
    out["physical"] = block(th, h, z=h / tau, scale=(1.0e30, 1.0e30 / tau.mean(), 1.0e30 / tau.mean() ** 2))
    n = 32
    z = np.concatenate([np.full(8, np.nextafter(1.0, 0.0)), np.full(8, 1.0), np.full(8, np.nextafter(1.0, 2.0)), [0.0, 0.5, 2.0, 1e3, 1e-300, np.inf, 0.999, 1.001]])
    out["switch"] = block(rng.uniform(0.05, 0.95, n), np.exp(rng.uniform(0.0, 3.0, n)), z=z)
    return out


# ---------------------------------------------------------------- fallback rate
def fallback_case(N):
    """192 threads of N times each: S_amp[nq], inv_tfb[nq], t[nq][N].  u = fma(t, inv_tfb, 1) covers [1, 2e7] log-uniformly with the N
    values of a thread far apart; thread 0 holds t = 0 (u = 1) in every slot, thread 1 (inv_tfb = 1) u = 2e7 exactly, thread 2 mixes
    both ends."""
    rng = np.random.default_rng([SEED, 2, N])
    nq = 192
    inv_tfb = np.exp(rng.uniform(math.log(1e-4), math.log(10.0), nq))
    S_amp = np.exp(rng.uniform(math.log(1e24), math.log(1e31), nq))
    u = np.exp(rng.uniform(0.0, math.log(2.0e7), (nq, N)))
    t = (u - 1.0) / inv_tfb[:, None]
    t[0] = 0.0
    inv_tfb[1:3] = 1.0
    t[1] = 2.0e7 - 1.0
    t[2] = np.where(np.arange(N) % 2 == 0, 0.0, 2.0e7 - 1.0)
    uu = mr.fma(t, inv_tfb[:, None], 1.0)
    assert uu.min() == 1.0 and uu.max() == 2.0e7
    return S_amp, inv_tfb, t
