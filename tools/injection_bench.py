"""Timing of the simulated light curves (mp_simulate) and of whole injection-recovery studies on one GPU.

1. mp_simulate against mp_model_pointwise on the same rows and the same 50 observed times: synchronised calls after warm-up,
   alternated in the same process (both see the same machine state; the first round is warm-up), medians over --reps rounds, at
   1 024, 16 384 and 131 072 rows.  mp_model_pointwise is code this feature does not touch, so its figure is the parent
   commit's; both calls run the same curve launches (Ltot only) plus light kernels, and mp_simulate copies four n x n_obs
   matrices to the host where mp_model_pointwise copies a table.  The ratio is reported, nothing is fixed by it.
   Rows: the Humped truth with a 0.02 spread in sampler coordinates.
2. calibration.injection_study at 16, 32 and 64 datasets (one batch each: 64 is MP_MAX_DATASETS): the reference's recipe, truths
   uniform in the narrow box of tests/test_gpu_injection.py, 32 walkers, the default moves, through the monitors (store=False);
   wall time of the whole study, the steps to convergence, and the calibration summary.  The 16-dataset study with seed 29 is the
   one tests/test_gpu_injection.py asserts on.

    python tools/injection_bench.py --out-simulate profiles/r29_simulate_bench.json --out-study profiles/r29_injection_study.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from magprop_amd import _capi, calibration, engine, synth  # noqa: E402

TRUTH = np.array([1.0, 5.0, -3.0, 2.0, -1.0, 0.0])
SPREAD = (0.3, 0.5, 0.3, 0.15, 0.3, 0.3)
ROWS = (1024, 16384, 131072)


def write(path, obj):
    line = json.dumps(obj)
    print(line)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(line + "\n")


def simulate_bench(reps):
    g = np.load(os.path.join(ROOT, "tests", "golden", "golden_synth.npz"))
    x, y, yerr = g["Humped_x"], g["Humped_y"], g["Humped_yerr"]
    h = _capi.Handle(_capi.cfg_synth(), engine.grid(None), 0)
    h.set_prior(synth.PRIOR_LOWER, synth.PRIOR_UPPER, synth.LOG_MASK)
    h.set_dataset(0, x, y, yerr)
    res = {"what": "mp_simulate against mp_model_pointwise", "rows": "Humped truth + 0.02 N(0,1)", "n_obs": int(x.size),
           "n_grid": int(h.tgrid.size), "n_simd": int(h.n_simd), "reps": reps,
           "pointwise_note": "mp_model_pointwise is not touched by this feature: its time here is the parent commit's", "calls": []}
    rng = np.random.default_rng(0)
    for n in ROWS:
        P = TRUTH + 0.02 * rng.standard_normal((n, 6))
        h.simulate(P[:2048], x, seed=1)                      # warm-up (code objects; the timed calls grow the workspaces once more)
        h.model_pointwise(P[:2048], ds_id=0)
        sim, pw = [], []
        for rep in range(reps + 1):
            t0 = time.perf_counter()
            out = h.simulate(P, x, seed=1)
            t1 = time.perf_counter()
            h.model_pointwise(P, ds_id=0)
            t2 = time.perf_counter()
            if rep:
                sim.append(t1 - t0), pw.append(t2 - t1)
        s, p = float(np.median(sim)), float(np.median(pw))
        res["calls"].append({"n": n, "n_ok": out["n_ok"], "simulate_ms_median": s * 1e3, "simulate_ms_min": float(np.min(sim)) * 1e3,
                             "simulate_us_per_row": s / n * 1e6, "pointwise_ms_median": p * 1e3, "simulate_over_pointwise": s / p})
    h.close()
    return res


def study_bench(sizes):
    res = {"what": "calibration.injection_study, store=False", "recipe": "50 grid points, yerr = 0.25 |model|", "centre": TRUTH.tolist(),
           "spread": list(SPREAD), "nwalkers": 32, "moves": "[(KDEMove(), 0.8), (DEMove(), 0.2)]", "studies": []}
    for nds in sizes:
        t0 = time.perf_counter()
        r = calibration.injection_study(n_datasets=nds, centre=TRUTH, spread=SPREAD, n_obs=50, frac_err=0.25, nwalkers=32,
                                        max_steps=20000, check_every=200, seed=29)
        wall = time.perf_counter() - t0
        s = r.summarize()
        res["studies"].append({
            "n_datasets": nds, "seed": 29, "wall_s": wall, "steps": int(r.steps.max()), "discard": r.discard,
            "converged": bool(np.all(r.converged)), "left_out": r.left_out, "redrawn": r.redrawn,
            "pit_values": int(r.pit.size), "pit_inside_0.005_0.995": int(np.sum((r.pit >= 0.005) & (r.pit <= 0.995))),
            "max_abs_zscore": float(np.nanmax(np.abs(r.zscore))), "tau_max": float(np.nanmax(r.tau)),
            "acceptance_mean": float(np.nanmean(r.acceptance)), "pit_resolution_max": float(np.nanmax(r.pit_resolution)),
            "ks": s["ks"].tolist(), "ks_critical_0.001": s["ks_critical"].tolist(), "calibrated": s["calibrated"].tolist(),
            "coverage": [{"level": c["level"], "observed": c["observed"].tolist()} for c in s["coverage"]],
            "contraction_median": s["contraction_median"].tolist(), "z_mean": s["z_mean"].tolist(), "z_sd": s["z_sd"].tolist()})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="*", default=[16, 32, 64])
    ap.add_argument("--out-simulate", default=None)
    ap.add_argument("--out-study", default=None)
    args = ap.parse_args()
    write(args.out_simulate, simulate_bench(args.reps))
    write(args.out_study, study_bench(args.sizes))


if __name__ == "__main__":
    main()
