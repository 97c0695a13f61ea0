"""The crafted inputs of the tune rule of the adaptive SMC moves (tests/smc_adapt_restated.py tune, magprop_amd/csrc/mp_smc.hip
smc_tune_kernel): the runs of one launch, each (name, start[n, ndim], now[n, ndim], acc[n], g).  Shared by the CPU test, which
holds the restatement to a long-double correlation, and the GPU test, which holds the kernel to the restatement bit for bit."""
import numpy as np

SIZES = [4, 255, 256, 257, 16384]       # below, at and above the workgroup's 256 threads; the largest run
NDIMS = [2, 6, 9]
WALKS = 3
G0 = 0.7


def exact_rho(name, ndim):
    """rho_d the rule gives exactly, for the cases built so that no sum rounds; None where it is a computed number."""
    if name in ("nothing moved", "pure shift"):
        return np.ones(ndim)
    if name == "one ancestor":
        return np.zeros(ndim)
    if name == "sign flip":
        return -np.ones(ndim)
    return None


def symmetric(n, ndim, rng):
    """Multiples of 1/8 up to 64 whose sum over the slots is exactly 0 in every dimension (every partial sum is exact too)."""
    half = rng.integers(1, 513, (n // 2, ndim)) / 8.0
    rows = np.concatenate([half, -half] + ([np.zeros((1, ndim))] if n % 2 else []))
    return np.stack([rows[rng.permutation(n), d] for d in range(ndim)], axis=1)


def runs(n, ndim, made, rng, g_min, g_max):
    """The runs of one launch behind the round that makes the stage's rounds `made`."""
    full, none = np.full(n, made * WALKS, dtype=np.int32), np.zeros(n, dtype=np.int32)
    some = rng.integers(0, made * WALKS + 1, n).astype(np.int32)
    a = rng.standard_normal((n, ndim))
    mixed = 0.6 * a + 0.8 * rng.standard_normal((n, ndim))
    loose = 0.1 * a + rng.standard_normal((n, ndim))
    sym = symmetric(n, ndim, rng)
    flat = mixed.copy()
    flat[:, 1] = -1.25
    return [("nothing moved", a, a.copy(), none, G0),                               # rho = 1
            ("one ancestor", np.repeat(a[:1], n, axis=0), mixed, some, G0),         # Saa = 0: rho = 0
            ("constant dimension", a, flat, some, G0),                              # Sbb = 0 in dimension 1: rho_1 = 1
            ("pure shift", sym, sym + 3.0, some, G0),                               # rho = 1 with Sbb > 0
            ("sign flip", a, -a, some, G0),                                         # rho = -1
            ("mixed", a + 1.5, mixed - 1.0, some, G0),
            ("loose", a, loose, some, G0),
            ("tiny", 1.0e-300 * a, 1.0e-300 * mixed, some, G0),
            ("huge", 1.0e150 * a, 1.0e150 * loose, some, G0),
            ("accept 0", a, loose, none, G0),
            ("accept 1", a, loose, full, G0),
            ("g at the upper clamp", a, loose, full, g_max),
            ("g at the lower clamp", a, loose, none, g_min)]
