"""Named cases for the kernels of the ladder adaptation and of the thermodynamic monitor (magprop_amd/csrc/mp_ladder.hip): the
launches that tests/test_ladder_cpu.py holds to the rule's properties on the restatement and tests/test_gpu_ladder_kernels.py
holds to the restatement bit for bit on the device.  Test infrastructure."""
from typing import NamedTuple

import numpy as np

from magprop_amd.tempering import adaptation_rate

N_TEMPS = (3, 4, 63, 64, 65, 256, 257)
N_GROUPS = (1, 2, 5)
DELTAS = ("zero", "full", "one zero", "alternating", "single")
N_ADAPT, LAG, TIME = 120, 20.0, 5.0
# the rate of the first update, of the last one, and one so small that exp returns 1
KAPPAS = (("first", adaptation_rate(0, LAG, TIME)), ("last", adaptation_rate(N_ADAPT - 1, LAG, TIME)), ("tiny", 1.0e-300))
LADDERS = (("1 .. 1e-14", 1.0e-14), ("1 .. 0.999", 0.999))


class AdaptCase(NamedTuple):
    name: str
    n_walkers: int
    kappa: float
    betas: np.ndarray      # (n_groups, T)
    gap: np.ndarray        # (n_groups, T - 1) None: the init launch's
    span: np.ndarray       # (n_groups,) None: the init launch's
    prev: np.ndarray       # (n_groups, T - 1)
    swaps: np.ndarray      # (n_groups, T - 1)
    drops: bool = False    # every group's update is dropped


def delta(kind, n_pairs, n_walkers):
    """The accepted swaps of one step of every pair."""
    d = np.zeros(n_pairs, dtype=np.int64)
    if kind == "full":
        d[:] = n_walkers
    elif kind == "one zero":
        d[:] = n_walkers
        d[n_pairs // 2] = 0
    elif kind == "alternating":
        d[::2] = n_walkers
    elif kind == "single":
        d[n_pairs - 1] = 1
    return d


def ladder(beta_min, n_temps):
    b = np.geomspace(1.0, beta_min, n_temps)
    b[0] = 1.0
    return b


def adapt_cases(n_temps):
    """Every ladder, rate and pattern of swaps at n_temps temperatures, the patterns dealt out over launches of 1, 2 and 5
    groups so that every pattern meets every ladder and rate."""
    out, k = [], 0
    rng = np.random.default_rng(n_temps)
    for lname, beta_min in LADDERS:
        for kname, kappa in KAPPAS:
            for first in range(len(DELTAS)):
                n_groups = N_GROUPS[k % 3]
                n_walkers = (16, 30, 64)[k % 3]
                k += 1
                kinds = [DELTAS[(first + g) % len(DELTAS)] for g in range(n_groups)]
                prev = rng.integers(0, 1 << 40, size=(n_groups, n_temps - 1))
                swaps = prev + np.array([delta(kind, n_temps - 1, n_walkers) for kind in kinds])
                betas = np.array([ladder(beta_min, n_temps)] * n_groups)
                out.append(AdaptCase(f"T={n_temps} {lname} kappa {kname} {kinds}", n_walkers, kappa, betas, None, None, prev, swaps))
    return out


def dropped_cases():
    """Updates that are not taken: a gap so small that the new ladder ties in double (exp(-1e-17) = 1 = beta_0), and a rate at
    which exp overflows (h = inf, G = inf, c = 0, g' = NaN).  The swap counts move, so prev advances."""
    tie_b = np.array([[1.0, np.nextafter(1.0, 0.0), np.exp(-1.0), np.exp(-2.0)]])
    tie_g = np.array([[1.0e-17, 1.0, 1.0]])
    prev = np.array([[5, 6, 7]], dtype=np.int64)
    b = np.array([ladder(1.0e-3, 5)] * 2)
    g = np.log(b[:, :-1]) - np.log(b[:, 1:])
    prev2 = np.zeros((2, 4), dtype=np.int64)
    return [AdaptCase("tie in double", 16, 0.2, tie_b, tie_g, np.array([2.0]), prev, prev + 16, True),
            AdaptCase("exp overflows", 16, 1.0e4, b, g, -np.log(b[:, -1]), prev2, prev2 + np.array([16, 0, 16, 0]), True)]


THERMO_WALKERS = (1, 2, 63, 64, 65, 255, 256, 257, 513)


def thermo_rows(n_walkers, n_ensembles=3, n_rows=6):
    """lnp[n_rows, n_ensembles, n_walkers] of one sign (a Gaussian target's), with -inf and NaN cells, a row of one ensemble
    without a finite cell, and values of 1e-300 and 1e9 in size."""
    rng = np.random.default_rng(7000 + n_walkers)
    lnp = -np.abs(rng.normal(size=(n_rows, n_ensembles, n_walkers))) * 10.0 ** rng.integers(-3, 4, size=(n_rows, n_ensembles, 1))
    lnp[1, 0, 0] = -np.inf
    lnp[2, 1, n_walkers - 1] = np.nan
    lnp[3, 2, :] = -np.inf
    lnp[3, 2, ::2] = np.nan
    lnp[4, 0, n_walkers // 2] = -1.0e-300
    lnp[4, 1, n_walkers // 2] = -1.0e9
    lnp[5, 0, 0] = np.inf
    return lnp
