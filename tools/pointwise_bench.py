"""Timing of the pointwise scores (mp_model_pointwise) on one GPU.

Synchronised calls after warm-up (the entry returns when the table and the tail rows are in host memory) at 1 024, 16 384 and
131 072 rows on the 50-point Humped light curve and at 16 384 rows on the 1 944-point one (tests/golden/golden_longlc.npz), each
alternated in the same process with
  * mp_model_derived on the same rows: the same chunks with all five curves and its reduction, code this feature does not touch
    (so the figure is the parent commit's) -- the yardstick for what the new kernels cost on top of the curve launches;
  * the host path on a subsample: mp_model_lc row by row, the numpy restatement of the cells and of the reductions
    (tests/pointwise_restated.py), EXTRAPOLATED to the call's rows by the row count and labelled so;
  * the host scores (PSIS-LOO, WAIC) computed from the device's table.
Rows: the Humped truth with a 0.02 spread in sampler coordinates (a burnt-in chain's rows).  Then, in a `rocprofv3
--kernel-trace --stats` run of its own (a fresh child process, tracing only), the times of the three pointwise kernels next to
the curve launch that feeds them, at one chunk of mp_n_simd rows on both light curves; if that child fails or leaves no stats
file the script exits non-zero before it touches the GPU itself.  Prints one JSON line; --out also writes it to a file.

    python tools/pointwise_bench.py --out profiles/r15_pointwise_bench.json
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pointwise_restated as pr  # noqa: E402
from magprop_amd import _capi, engine, pointwise, synth  # noqa: E402

TRUTH = np.array([1.0, 5.0, -3.0, 2.0, -1.0, 0.0])
CASES = (("humped50", 1024), ("humped50", 16384), ("humped50", 131072), ("synth1944", 16384))


def datasets():
    g = np.load(os.path.join(ROOT, "tests", "golden", "golden_synth.npz"))
    long = np.load(os.path.join(ROOT, "tests", "golden", "golden_longlc.npz"))["synth1944_ds"]
    return {"humped50": (g["Humped_x"], g["Humped_y"], g["Humped_yerr"]), "synth1944": tuple(long)}


def handle(data):
    h = _capi.Handle(_capi.cfg_synth(), engine.grid(None), 0)
    h.set_prior(synth.PRIOR_LOWER, synth.PRIOR_UPPER, synth.LOG_MASK)
    for k, name in enumerate(data):
        h.set_dataset(k, *data[name])
    return h


def host_path(h, Pphys, x, y, yerr):
    order = np.argsort(x, kind="stable")
    g, dx, idt = pr.digest(h.tgrid, x[order])
    z = np.full((x.size, len(Pphys)), np.nan)
    for i, p in enumerate(Pphys):
        s, lc = h.model_lc(p)
        if s == 0:
            z[:, i] = pr.cells(lc[1][None, :], np.zeros(1, dtype=np.int32), g, dx, idt, y[order], yerr[order])[:, 0]
    return pr.pointwise(z)


def trace_child(calls):
    """what the traced process runs: `calls` calls of one chunk on each light curve"""
    data = datasets()
    h = handle(data)
    P = TRUTH + 0.02 * np.random.default_rng(0).standard_normal((h.n_simd, 6))
    for _ in range(calls):
        for k in range(len(data)):
            h.model_pointwise(P, ds_id=k)
    h.close()


def trace(calls, limit=300):
    """{kernel name: {"calls", "mean_us", ...}} of the curve and the pointwise kernels from a rocprofv3 run of a child process
    under its own time limit.  A child that fails or leaves no stats file ends the script: nothing more is started on the GPU."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["timeout", "-k", "10", str(limit), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d,
               "-o", "pointwise", "--", sys.executable, os.path.abspath(__file__), "--trace-child", str(calls)]
        rc = subprocess.call(cmd)
        if rc:
            print(f"traced child failed (exit {rc}): {' '.join(cmd)}", file=sys.stderr)
            sys.exit(rc)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            print("the traced child left no *kernel_stats.csv", file=sys.stderr)
            sys.exit(1)
        out = {}
        for row in csv.DictReader(open(files[0])):
            name = row.get("Name", "")
            if "pointwise_" in name or "lnprob_kernel" in name:
                out[name[:96]] = {"calls": int(row["Calls"]), "mean_us": float(row["AverageNs"]) * 1e-3,
                                  "min_us": float(row["MinNs"]) * 1e-3, "max_us": float(row["MaxNs"]) * 1e-3}
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-rows", type=int, default=128)
    ap.add_argument("--trace-calls", type=int, default=4)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-child", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.trace_child:
        trace_child(args.trace_child)
        return
    res = {"what": "mp_model_pointwise", "rows": "Humped truth + 0.02 N(0,1)",
           "derived_note": "mp_model_derived is not touched by the pointwise feature: its time here is the parent commit's",
           "host_note": "host path measured on host_rows rows and EXTRAPOLATED to n by the row count"}
    if not args.no_trace:                                   # first: no GPU is open in this process yet; exits if the child fails
        res["kernel_trace"] = trace(args.trace_calls)
    data = datasets()
    h = handle(data)
    res.update({"n_grid": int(h.tgrid.size), "n_simd": int(h.n_simd), "calls": []})
    rng = np.random.default_rng(0)
    for name, n in CASES:
        ds_id = list(data).index(name)
        x, y, yerr = data[name]
        P = TRUTH + 0.02 * rng.standard_normal((n, 6))
        Pphys = P[:args.host_rows].copy()
        Pphys[:, 2:] = 10.0 ** Pphys[:, 2:]
        h.model_pointwise(P[:2048], ds_id=ds_id)             # warm-up (code objects; the timed calls grow the workspace once more)
        h.model_derived(P[:2048])
        host_path(h, Pphys[:4], x, y, yerr)
        dev, der, host, score = [], [], [], []
        for rep in range(args.reps + 1):                    # alternated: all see the same machine state; the first round is warm-up
            t0 = time.perf_counter()
            obs, tail, _, used = h.model_pointwise(P, ds_id=ds_id)
            t1 = time.perf_counter()
            h.model_derived(P)
            t2 = time.perf_counter()
            host_path(h, Pphys, x, y, yerr)
            t3 = time.perf_counter()
            loo = pointwise.psis_loo(obs, tail)
            pointwise.waic(obs)
            t4 = time.perf_counter()
            if rep:
                dev.append(t1 - t0), der.append(t2 - t1), host.append(t3 - t2), score.append(t4 - t3)
        d, de, ho = float(np.median(dev)), float(np.median(der)), float(np.median(host))
        res["calls"].append({"dataset": name, "n_obs": int(x.size), "n": n, "n_used": used, "ms_median": d * 1e3,
                             "ms_min": float(np.min(dev)) * 1e3, "us_per_row": d / n * 1e6,
                             "derived_ms_median": de * 1e3, "over_derived": d / de,
                             "host_rows": len(Pphys), "host_ms_measured": ho * 1e3,
                             "host_ms_extrapolated": ho / len(Pphys) * n * 1e3, "speedup_over_host_extrapolated": (ho / len(Pphys) * n) / d,
                             "host_scores_ms": float(np.median(score)) * 1e3, "khat_max": float(np.nanmax(loo["khat"])),
                             "elpd_loo": float(np.sum(loo["elpd_loo"]))})
    h.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
