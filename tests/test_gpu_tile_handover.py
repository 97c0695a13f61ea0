"""The hand-over between a walker's tiles in the one-wavefront, 4-steps-per-lane kernel (run with -m gpu on an MI355X).

That kernel carries the end of a kept tile to the next one through lanes and keeps out of the tile's image in LDS what nothing
reads back; the team of four wavefronts per walker goes through the image as before.  Both share tiles, policy and the order of
the arithmetic, so the same walkers through both must give equal statuses, equal tile and sweep counts, tile logs that are
equal word for word, and values within TEAM_RTOL -- the bound tests/test_gpu_parity.py holds between these two kernels
(test_batch_size_does_not_change_a_walker), taken from there and not from the code under test.

The kernel goes by the launch size (mp_kernels.hip launch_lnprob): n_simd / 2 + 1 ... n_simd rows run one wavefront per
walker with four steps per lane, up to n_simd / 4 rows the team of four with a SIMD for every wavefront.  The walkers are
launched once padded with repeats into the first range and once as they are.

Every run of the module is made once (fixture `runs`); the tests read it.  The serial oracle reports tile counts, not the
tiles themselves, so the classes of tiles the sample has to contain are asserted from the kernels' own logs
(test_every_class_of_tile_occurs): a sample that stops covering a class fails there.
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN, TRUTHS, TYPES

pytestmark = pytest.mark.gpu

TEAM_RTOL = 1e-11       # tests/test_gpu_parity.py: team kernels against the 4-steps-per-lane kernel
LOG_MASK = 0b111100
FLAG_WALKER = [1.8171068, 3.68147895, -2.61786801, 1.99840102, -0.33083576, 2.95613803]
GRID_SIZES = [2, 3, 9, 33, 34, 100, 257, 1000, 4097, 20001]   # test_unusual_grid_sizes_through_the_c_abi; (n - 1) mod 4 takes 1, 2, 0, 0, 1, 3, 0, 3, 0, 0
DATASETS = ["knots50", "off8", "ends", "long112"]


def _walkers(lo, hi):
    """32 near each truth, 64 prior-wide (fixed seed), the flag walker, one NaN, one outside the prior: 195 rows."""
    rng = np.random.default_rng(20240)
    P = [np.array(TRUTHS[n]) + 1.0e-3 * rng.standard_normal((32, 6)) for n in TYPES]
    P.append(lo + (hi - lo) * rng.random((64, 6)))
    P = np.clip(np.concatenate(P), lo, hi)
    nan = np.array(TRUTHS["Humped"], dtype=float)
    nan[0] = np.nan
    return np.concatenate([P, [FLAG_WALKER], [nan], [hi + 0.5]])


def _both_kernels(h, P):
    """P through the one-wavefront 4-steps-per-lane kernel (padded with repeats) and through the team of four."""
    ns, n = h.n_simd, len(P)
    assert n <= ns // 4, "the sample must fit the team of four with a SIMD per wavefront"
    n_one = ns // 2 + 1 + (ns // 2 - 1) // 3            # inside n_simd / 2 + 1 ... n_simd
    assert ns // 2 < n_one <= ns and n_one >= 2 * n
    res = []
    for rows in (np.resize(np.arange(n), n_one), np.arange(n)):
        out, st = h.lnprob_batch(P[rows], want_status=True)
        res.append({"lnprob": out[:n], "status": st[:n], "tiles": h.last_tiles(n), "sweeps": h.last_sweeps(n),
                    "log": [h.last_tile_log(w) for w in range(n)]})
        if len(rows) > n:   # a repeat is the same walker: the same bits wherever it sits in the launch
            assert np.array_equal(out[n:2 * n], out[:n]) and np.array_equal(st[n:2 * n], st[:n])
    return res


def _handle(tg, lo, hi, x, y, yerr):
    from magprop_amd import _capi
    h = _capi.Handle(_capi.cfg_synth(), tg)
    h.set_prior(lo, hi, LOG_MASK)
    h.set_dataset(0, x, y, yerr)
    h.tile_log(True)
    return h


@pytest.fixture(scope="module")
def runs(gsynth, tarr):
    lo, hi = gsynth["prior_lower"], gsynth["prior_upper"]
    P = _walkers(lo, hi)
    rng = np.random.default_rng(77)
    sets = {"knots50": (gsynth["Humped_x"], gsynth["Humped_y"], gsynth["Humped_yerr"])}
    # eight times strictly inside grid intervals: both bracketing states of every observation are read
    k8 = np.array([3, 40, 700, 2500, 4100, 6000, 8200, 9900])
    x8 = np.sqrt(tarr[k8] * tarr[k8 + 1])
    sets["off8"] = (x8, 10.0 ** rng.uniform(-2, 2, 8), None)
    # the first grid point, the last one, and the last node of the sub-stepped first tile (grid point 32: kept whole, that
    # tile ends there), with two times further in for good measure
    ke = np.array([0, 32, 5000, 9999, 10000])
    sets["ends"] = (tarr[ke], 10.0 ** rng.uniform(-2, 2, 5), None)
    g = np.load(os.path.join(GOLDEN, "golden_longlc.npz"))
    sets["long112"] = tuple(g["synth112_ds"])
    out = {}
    for name in DATASETS:
        x, y, yerr = sets[name]
        yerr = 0.3 * y if yerr is None else yerr
        h = _handle(tarr, lo, hi, x, y, yerr)
        out[name] = _both_kernels(h, P)
        h.close()
    for n_grid in GRID_SIZES:   # the data of test_unusual_grid_sizes_through_the_c_abi on each grid
        r = np.random.default_rng(n_grid)
        tg = np.logspace(0.0, 6.0 * min(1.0, (n_grid - 1) / 10000.0), n_grid)
        n_obs = min(50, max(1, n_grid))
        x = np.sort(np.exp(r.uniform(np.log(tg[0]), np.log(tg[-1]), n_obs)))
        x[0], x[-1] = tg[0], tg[-1]
        y = 10.0 ** r.uniform(-2, 2, n_obs)
        h = _handle(tg, lo, hi, x, y, 0.3 * y)
        out[n_grid] = _both_kernels(h, P)
        h.close()
    return out


@pytest.mark.parametrize("case", DATASETS + GRID_SIZES)
def test_one_wavefront_kernel_against_the_team_of_four(runs, case):
    one, team = runs[case]
    assert np.array_equal(one["status"], team["status"]), np.nonzero(one["status"] != team["status"])[0][:5]
    assert np.array_equal(one["tiles"], team["tiles"]) and np.array_equal(one["sweeps"], team["sweeps"])
    assert one["log"] == team["log"]
    n = len(one["status"])
    assert one["status"][n - 1] == 3 and one["lnprob"][n - 2] == -np.inf and np.isneginf(one["lnprob"][n - 1])
    if case in DATASETS:
        assert one["status"][n - 3] == 1                       # the flag walker flags on the reference's grid
    fin = np.isfinite(team["lnprob"])
    assert np.array_equal(fin, np.isfinite(one["lnprob"])) and np.array_equal(fin, team["status"] == 0)
    assert fin.sum() > 0
    diff, ref = np.abs(one["lnprob"][fin] - team["lnprob"][fin]), np.abs(team["lnprob"][fin])
    print(case, "finite", int(fin.sum()), "largest |difference| / |value|", float(np.max(diff / np.maximum(ref, 1e-300))))
    assert np.all(diff <= TEAM_RTOL * ref)
    assert np.all(one["lnprob"][~fin] == -np.inf) and np.all(team["lnprob"][~fin] == -np.inf)


def test_a_short_grid_is_at_most_two_tiles(runs):
    """99 grid intervals: the sub-stepped start (32 of them) and one tile over the other 67."""
    one, _ = runs[100]
    ok = one["status"] == 0
    assert ok.sum() > 0 and one["tiles"][ok].min() <= 2


def test_every_class_of_tile_occurs(runs):
    """(kind, sweeps, lanes kept, why) per tile solved; why & 64: given up during the sweeps; 0 lanes: redone."""
    seen = dict.fromkeys(("cut coarse", "redone", "given up", "stride rising", "stride falling", "short final tile"), 0)
    for case, (one, _) in runs.items():
        for w in np.nonzero(one["status"] == 0)[0]:
            log = one["log"][w]
            if len(log) < one["tiles"][w]:
                continue                                        # more tiles than the log holds: the walker's end is not in it
            kept = []
            for kind, _sweeps, lanes, why in log:
                if why & 64:
                    seen["given up"] += 1
                elif lanes == 0:
                    seen["redone"] += 1
                else:
                    kept.append(kind)
                    if kind >= 2 and lanes <= 63:
                        seen["cut coarse"] += 1
            seen["stride rising"] += sum(b > a for a, b in zip(kept, kept[1:]))
            seen["stride falling"] += sum(b < a for a, b in zip(kept, kept[1:]))
            # a finished walker on a grid whose intervals behind the sub-stepped start (32) are fewer than a tile's 256 steps,
            # or that is shorter than the start itself (fewer than 256 sub-steps), ends on a tile of fewer than 256 steps
            if not isinstance(case, str) and case - 1 != 32 and case - 1 - 32 < 256 and kept:
                seen["short final tile"] += 1
    print(seen)
    assert all(v > 0 for v in seen.values()), seen
