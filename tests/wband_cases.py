"""Named cases for the weighted select of the band (band_wselect_kernel, magprop_amd/csrc/mp_band.hip; wg_wradix_select,
mp_wg.h).  numpy only, seeded and deterministic.  A case is point-major columns cols[n_grid][n], the rows' integer units
units[n] and quantiles q; tests/test_wband_cpu.py runs every case through the restatement (tests/wband_restated.py) and checks
that it has the property its name claims, tests/test_gpu_wband_kernels.py runs the same list through the kernel
(libmp_probe_wselect.so), so that no case exists on one side only."""
import zlib
from collections import namedtuple

import numpy as np

import wband_restated as wr

BAND_MAX_SAMPLES, BAND_MAX_Q = 16384, 16            # MP_BAND_MAX_SAMPLES, MP_BAND_MAX_Q
FULL = np.uint32(1 << 31)                           # the units of the heaviest row
# dynamic LDS of band_wselect_kernel: a header of kWKeysOffset bytes (mp_band.hip) and 8 bytes per row; above 65 536 bytes the
# launcher has to raise the kernel's limit first
LDS_HEADER, LDS_PLAIN = 8240, 65536
N_LAST_PLAIN = (LDS_PLAIN - LDS_HEADER) // 8        # 7 162 rows: exactly 65 536 bytes, the last size of the plain branch
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1000)

Q7 = np.array([0.0, 0.025, 0.16, 0.5, 0.84, 0.975, 1.0])
Q16 = np.concatenate([Q7, [1.0 - 2.0 ** -53, 2.0 ** -1074, 0.25, 1.0 / 3.0, 0.999, 0.5 + 2.0 ** -53, 0.75, 2.0 ** -31, 0.1]])
Q3 = np.array([0.025, 0.5, 0.975])

WCase = namedtuple("WCase", "name cols units q")


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _units(rng, n, spread=3.0):
    """units of log-weights spread * N(0, 1)"""
    return wr.weight_units(np.exp(spread * rng.standard_normal(n)))


def _values(rng, n_grid, n):
    return rng.standard_normal((n_grid, n)) * 10.0 ** rng.integers(-3, 4, (n_grid, 1))


def _case(name, cols, units, q=Q7):
    cols = np.ascontiguousarray(np.atleast_2d(np.asarray(cols, dtype=np.float64)))
    units = np.ascontiguousarray(units, dtype=np.uint32)
    q = np.ascontiguousarray(q, dtype=np.float64)
    assert cols.shape[1] == units.size and 1 <= units.size <= BAND_MAX_SAMPLES and 1 <= q.size <= BAND_MAX_Q and cols.shape[0] <= 5
    return WCase(name, cols, units, q)


def _build():
    cases = []
    for k, n in enumerate(SIZES):
        name = f"random-n{n}"
        rng = _rng(name)
        cases.append(_case(name, _values(rng, 1 + k % 5, n), _units(rng, n), Q16 if k % 2 == 0 else Q7))
        # all weight on one row: every quantile of a column is that row's value
        name = f"one-row-n{n}"
        rng = _rng(name)
        u = np.zeros(n, dtype=np.uint32)
        u[rng.integers(n)] = FULL
        cases.append(_case(name, _values(rng, 2, n), u))
        # rows of zero units, the least and the largest value of every column among them
        if n >= 3:
            name = f"zero-ends-n{n}"
            rng = _rng(name)
            cols, u = _values(rng, 3, n), _units(rng, n)
            u[rng.random(n) < 0.3] = 0
            u[0] = u[1] = 0
            u[2] = FULL
            for c in cols:
                c[0], c[1] = c.min() - 1.0, c.max() + 1.0
            cases.append(_case(name, cols, u))
        # NaNs on the heaviest rows (a different set in every column)
        if n >= 2:
            name = f"nan-heaviest-n{n}"
            rng = _rng(name)
            cols, u = _values(rng, 4, n), _units(rng, n)
            heavy = np.argsort(u)[::-1]
            for g, c in enumerate(cols):
                c[heavy[:max(1, min(n - 1, (g + 1) * n // 8))]] = np.nan
            cases.append(_case(name, cols, u, Q16))

    name = "all-nan-column"
    rng = _rng(name)
    cols = _values(rng, 3, 130)
    cols[1] = np.nan
    cases.append(_case(name, cols, _units(rng, 130)))

    # the weight sits on rows that are NaN in column 0: its used rows carry no unit
    name = "used-rows-without-units"
    rng = _rng(name)
    cols, u = _values(rng, 2, 200), np.zeros(200, dtype=np.uint32)
    heavy = rng.choice(200, 40, replace=False)
    u[heavy] = _units(rng, 40)
    u[heavy[0]] = FULL
    cols[0, heavy] = np.nan
    cases.append(_case(name, cols, u))

    for n in (64, 257, 1000):
        name = f"ties-n{n}"
        rng = _rng(name)
        cols = rng.integers(-3, 4, (3, n)).astype(float) * 0.5
        cases.append(_case(name, cols, _units(rng, n), Q16))

    name = "signed-zeros"
    rng = _rng(name)
    cols = rng.choice([0.0, -0.0, 1.5, -2.0], (4, 300))
    cols[3] = rng.choice([0.0, -0.0], 300)
    cases.append(_case(name, cols, _units(rng, 300, 1.0), Q16))

    name = "infinities"
    rng = _rng(name)
    cols = rng.choice([np.inf, -np.inf, 0.0, 1.0e308, -1.0e308, 5e-324], (3, 257))
    cols[2, rng.random(257) < 0.2] = np.nan
    cases.append(_case(name, cols, _units(rng, 257, 1.0), Q16))

    # three rows of 2^31 units: their sum does not fit 32 bits
    cases.append(_case("overflow-n3", [[3.0, 1.0, 2.0], [-1.0, -1.0, 5.0]], [FULL] * 3, Q16))
    name = "overflow-n300"
    rng = _rng(name)
    cases.append(_case(name, _values(rng, 2, 300), np.full(300, FULL), Q16))

    # W = 2^33 and q = 0.5: the target 2^32 is the cumulative sum behind the second value; with one unit less on the first row
    # W = 2^33 - 1, the target stays 2^32 and lies one unit beyond that sum
    cases.append(_case("boundary-on", [[4.0, 1.0, 3.0, 2.0]], [FULL] * 4, [0.5]))
    cases.append(_case("boundary-beyond", [[4.0, 1.0, 3.0, 2.0]], [FULL, FULL - np.uint32(1), FULL, FULL], [0.5]))

    # keys that differ in one byte only: every byte position, every value of the byte that is no NaN
    base = wr.band_key(np.array([1.5]))[0]
    for byte in range(8):
        name = f"one-key-byte-{byte}"
        rng = _rng(name)
        keys = (base & ~(np.uint64(255) << np.uint64(8 * byte))) | (np.arange(256, dtype=np.uint64) << np.uint64(8 * byte))
        vals = np.where(keys >> np.uint64(63) != 0, keys & ~np.uint64(1 << 63), ~keys).view(np.float64)
        vals = rng.permutation(vals[~np.isnan(vals)])
        cases.append(_case(name, [vals, vals[::-1]], _units(rng, vals.size, 1.0), Q16))

    # dynamic LDS: the last size of the plain branch, the first above it, 8 188 rows (65 504 bytes of keys: with the header just
    # above the 65 536 bytes) and the cap
    for n, n_grid in ((N_LAST_PLAIN, 1), (N_LAST_PLAIN + 1, 1), (8188, 2), (BAND_MAX_SAMPLES, 3)):
        name = f"lds-n{n}"
        rng = _rng(name)
        cols = 10.0 ** rng.uniform(-5, 3, (n_grid, n))
        cols[rng.random((n_grid, n)) < 0.02] = np.nan
        cases.append(_case(name, cols, _units(rng, n), Q3))
    return cases


CASES = _build()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
