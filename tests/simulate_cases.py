"""Crafted cases of the simulated light curves (mp_simulate's cells kernel; tests/simulate_restated.py is the definition): small
synthetic grids and curves, named.  Each case is {"t": grid [G], "ltot": curves [n][G], "status": [n], "x": times [n_obs] (shared)
or [n][n_obs], "yerr": errors of x's shape or None, "frac_err", "seed", "row0": index of the first row}.  Shared by the CPU tests
(exact interpolation, knots, chunking) and the GPU test of the kernel alone."""
import numpy as np

G = 40


def _grid(g=G):
    """a geometric grid, as the product's: unequal intervals whose reciprocals do not round trip"""
    return np.logspace(0.0, 3.0, g)


def _curves(n, g=G, seed=1, scale=1.0):
    """n smooth positive curves with a hump, rising and falling parts"""
    rng = np.random.default_rng(seed)
    u = np.linspace(0.0, 1.0, g)
    a, b, c = rng.uniform(0.5, 2.0, (3, n, 1))
    return scale * (a * np.exp(-3.0 * u) + b * np.exp(-0.5 * ((u - 0.4) / (0.05 + 0.1 * c)) ** 2) + 1.0e-3)


def _case(x, n=1, yerr=None, frac_err=0.25, seed=7, row0=0, ltot=None, status=None, t=None):
    t = _grid() if t is None else np.asarray(t, dtype=np.float64)
    ltot = _curves(n, t.size) if ltot is None else np.atleast_2d(np.asarray(ltot, dtype=np.float64))
    n = ltot.shape[0]
    return {"t": t, "ltot": ltot, "status": np.zeros(n, dtype=np.int32) if status is None else np.asarray(status, dtype=np.int32),
            "x": np.asarray(x, dtype=np.float64), "yerr": None if yerr is None else np.asarray(yerr, dtype=np.float64),
            "frac_err": frac_err, "seed": seed, "row0": row0}


def _inside(t, n_obs, seed):
    """n_obs times spread over the whole grid, between the knots"""
    rng = np.random.default_rng(seed)
    return np.exp(rng.uniform(np.log(t[0]), np.log(t[-1]), n_obs))


def _build():
    t = _grid()
    up, down = np.nextafter(t, np.inf), np.nextafter(t, -np.inf)
    c = {}
    c["knots_first_inner_last"] = _case([t[0], t[17], t[-1]])
    c["every_knot"] = _case(t.copy(), n=3)
    c["one_ulp_above_knots"] = _case(up[[0, 1, 17, G - 2]])
    c["one_ulp_below_knots"] = _case(down[[1, 17, G - 2, G - 1]])
    c["inside_first_interval"] = _case([0.5 * (t[0] + t[1]), t[0] + 0.1 * (t[1] - t[0])])
    c["inside_last_interval"] = _case([0.5 * (t[-2] + t[-1]), t[-1] - 0.1 * (t[-1] - t[-2])])
    c["unsorted_and_repeated"] = _case([t[30], 5.0, t[3], 5.0, 700.0, t[30], 1.5, t[-1], t[0], 5.0], n=2)
    for n_obs in (1, 2, 63, 64, 65, 257):
        c[f"n_obs_{n_obs}"] = _case(_inside(t, n_obs, n_obs), n=2, seed=100 + n_obs)
    for n in (1, 63, 64, 65):
        c[f"rows_{n}"] = _case(_inside(t, 7, n), n=n, seed=200 + n, row0=3 * n)
    xr = np.stack([_inside(t, 9, 40 + i) for i in range(5)])
    xr[2, 4], xr[3, 0], xr[4, 8] = t[11], t[-1], t[0]
    c["per_row_times"] = _case(xr, n=5)
    c["given_errors_shared"] = _case(_inside(t, 12, 5), n=4, yerr=np.random.default_rng(6).uniform(0.01, 2.0, 12))
    c["given_errors_per_row"] = _case(xr, n=5, yerr=np.random.default_rng(8).uniform(0.01, 2.0, xr.shape))
    c["fractional_error_small"] = _case(_inside(t, 12, 9), n=2, frac_err=1.0e-3)
    flat = _curves(3)
    flat[1, 10:13] = 0.0                       # a curve value of 0: on knot 11 and inside [10, 12] the model and the error are 0
    c["curve_value_zero"] = _case([t[11], 0.5 * (t[10] + t[11]), t[20], 3.0], ltot=flat)
    c["falling_curve"] = _case(_inside(t, 33, 12), ltot=np.linspace(5.0, 0.25, G)[None, :] * np.ones((2, 1)))   # Lb - La < 0 throughout
    nan = _curves(4)
    nan[2] = np.nan
    c["failed_row"] = _case(_inside(t, 10, 13), ltot=nan, status=[0, 0, 1, 0])
    c["failed_row_per_row_times"] = _case(np.stack([_inside(t, 6, 50 + i) for i in range(4)]), ltot=nan, status=[0, 3, 2, 0])
    c["tiny_values"] = _case(_inside(t, 20, 14), ltot=_curves(2, scale=1.0e-280))   # (every intermediate stays a normal number)
    c["huge_values"] = _case(_inside(t, 20, 15), ltot=_curves(2, scale=1.0e300))
    c["subnormal_error"] = _case(_inside(t, 6, 16), ltot=_curves(1, scale=1.0e-310), frac_err=1.0e-20)   # frac_err * |mod| underflows to 0
    c["large_seed_and_index"] = _case(_inside(t, 5, 17), n=2, seed=0xFEDCBA9876543210, row0=262142)
    return c


CASES = _build()
