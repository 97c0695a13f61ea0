"""Named cases for the derived-quantity kernel (magprop_amd/csrc/mp_derive.hip) and its numpy restatement
(tests/derive_restated.py): crafted curves on crafted grids.  A case is (name, t[G], curves[5][n][G], status[n]); the curves are
Ltot, Lprop, Ldip, Mdisc, omega in mp_model_derived's order.  cases() builds them once.

Segments: 256 of seg = ceil((G - 1) / 256) intervals.  G = 2, 3 and 256 leave most or one segment empty, 257 fills every
segment with one interval, 258 and 514 start the next length (the last segments empty), 513 fills two each, 10 001 is the
product's grid (40 each, six segments empty).  WINDOW_GRID_SIZES sit on the corners of the kernel's staging windows."""
import functools

import numpy as np

GRID_SIZES = (2, 3, 256, 257, 258, 513, 514, 10001)
# the corners of the kernel's LDS windows of WINDOW intervals per segment: seg = 14 (one full window), 15 (a second window of one
# interval), 29 (a third of one interval), and last segments that end at, one short of and one past a window boundary
WINDOW = 14
WINDOW_GRID_SIZES = (256 * 14 + 1, 256 * 14 + 2, 256 * 28 + 2, 255 * 15 + 14 + 1, 255 * 15 + 13 + 1, 255 * 15 + 15 + 1, 255 * 29 + 28 + 1)
ROW_COUNTS = (1, 63, 64, 65, 257)
# cases in which a cumulative energy equals f * E_tot exactly, so that a definition in another precision may cross one grid
# point later (tests/test_derive_cases_cpu.py: at most 2)
AT_THRESHOLD = ("exact_threshold",)


def log_grid(G, decades=6.0):
    return np.logspace(0.0, decades, G)


def smooth(rng, n, G):
    """n positive curves of G points with a hump somewhere inside"""
    x = np.linspace(0.0, 1.0, G)
    c, w, a = rng.uniform(0.1, 0.9, (n, 1)), rng.uniform(0.05, 0.4, (n, 1)), rng.uniform(0.5, 2.0, (n, 1))
    return a * np.exp(-0.5 * ((x - c) / w) ** 2) + rng.uniform(1e-3, 1e-2, (n, 1)) * (1.0 + rng.random((n, G)))


def five(rng, n, G):
    return np.stack([smooth(rng, n, G) for _ in range(5)])


def one_interval(G, i, a=3.0):
    """a curve whose trapezoid terms are all exactly zero but that of interval i: L_i = L_{i+1} = a, signs alternating away from them"""
    j = np.arange(G)
    return np.where(j <= i, a * (-1.0) ** (i - j), a * (-1.0) ** (j - i - 1))


def same_on_all(curve, n=1):
    c = np.asarray(curve, dtype=np.float64)
    return np.broadcast_to(c, (5, n, c.size)).copy()


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(20261)
    out = []

    def add(name, t, curves, status=None):
        curves = np.ascontiguousarray(curves, dtype=np.float64)
        assert curves.ndim == 3 and curves.shape[0] == 5 and curves.shape[2] == len(t)
        st = np.zeros(curves.shape[1], dtype=np.int32) if status is None else np.asarray(status, dtype=np.int32)
        out.append((name, np.ascontiguousarray(t, dtype=np.float64), curves, st))

    for G in GRID_SIZES:
        add(f"grid_{G}", log_grid(G), five(rng, 2 if G > 1000 else 3, G))
    wrng = np.random.default_rng(20262)                         # (its own stream: the cases behind keep their values)
    for G in WINDOW_GRID_SIZES:
        add(f"grid_{G}", log_grid(G), five(wrng, 2, G))
    G = 300
    t = log_grid(G)
    add("all_zero", t, np.zeros((5, 1, G)))
    add("negative_zero", t, np.full((5, 1, G), -0.0))
    add("constant", t, same_on_all(np.full(G, 0.7)))
    falling, rising = np.linspace(2.0, 1.0, G), np.linspace(1.0, 2.0, G)
    add("peak_first", t, same_on_all(falling))
    add("peak_last", t, same_on_all(rising))
    plateau = smooth(rng, 1, G)[0]
    plateau[100:140] = plateau.max() + 1.0                     # equal values: the first one is the peak
    add("peak_plateau", t, same_on_all(plateau))
    # all energy in one interval: G = 1 000 has seg = 4, so segment 7 holds intervals 28 .. 31
    G = 1000
    t = log_grid(G)
    for name, i in (("energy_segment_first", 28), ("energy_segment_last", 31), ("energy_row_first", 0), ("energy_row_last", G - 2)):
        add(name, t, same_on_all(one_interval(G, i)))
    # unit steps and a unit curve: the cumulative energy after interval i is i + 1 exactly, E_tot = 8, so 0.5 E_tot is met at t_4
    add("exact_threshold", np.arange(1.0, 10.0), same_on_all(np.ones(9)))
    G = 700
    t = log_grid(G)
    add("tiny_1e-300", t, 1e-300 * five(rng, 2, G))
    add("huge_1e+150", t, 1e150 * five(rng, 2, G))
    add("failed_rows_between", t, five(rng, 9, G), status=[0, 1, 0, 2, 3, 0, 0, 3, 0])
    for n in ROW_COUNTS:
        st = np.zeros(n, dtype=np.int32)
        st[3::7] = 1 + np.arange(len(st[3::7])) % 3
        add(f"rows_{n}", log_grid(130), five(rng, n, 130), st)
    return tuple(out)


def names():
    return [c[0] for c in cases()]


def case(name):
    return next(c for c in cases() if c[0] == name)
