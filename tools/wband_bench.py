"""Timing of the weighted band (mp_model_band_weighted) against the band (mp_model_band) on one GPU.

Synchronised calls after warm-up (each entry returns when its result is in host memory) at S = 1 024, 4 096, 16 384 rows,
component Ltot, three quantiles, the two entries alternated call by call in one process on the same rows.  Rows: the Humped
truth with a 0.02 spread in sampler coordinates (a burnt-in chain's rows); weights: exp(3 N(0, 1)), a nested run's spread.  Both
calls make the same curve pass and the same transpose, so their difference is the select's.  Then, in a `rocprofv3
--kernel-trace --stats` run of its own (a fresh child process, tracing only), band_wselect_kernel next to band_select_kernel at
every size; if that child fails or leaves no stats file the script exits non-zero before it touches the GPU itself.  Prints one
JSON line; --out also writes it to a file.

    python tools/wband_bench.py --reps 7 --out profiles/r17_wband_bench.json
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

from magprop_amd import _capi, engine, synth  # noqa: E402

TRUTH = np.array([1.0, 5.0, -3.0, 2.0, -1.0, 0.0])
Q = (0.025, 0.5, 0.975)
KERNELS = ("band_wselect_kernel", "band_select_kernel", "band_transpose_kernel")


def handle():
    h = _capi.Handle(_capi.cfg_synth(), engine.grid(None), 0)
    h.set_prior(synth.PRIOR_LOWER, synth.PRIOR_UPPER, synth.LOG_MASK)
    return h


def inputs(sizes):
    rng = np.random.default_rng(0)
    return [(S, TRUTH + 0.02 * rng.standard_normal((S, 6)), np.exp(3.0 * rng.standard_normal(S))) for S in sizes]


def trace_child(sizes, calls):
    """what the traced process runs: `calls` calls of either entry at every size, the sizes in turn (a size is told from the
    trace by its launch order)"""
    h = handle()
    for _, P, w in inputs(sizes):
        for _ in range(calls):
            h.model_band(P, Q)
            h.model_band(P, Q, weights=w)
    h.close()


def trace(sizes, calls, limit=300):
    """per size {kernel: {"calls", "mean_us", "min_us", "max_us"}} of the band kernels from a rocprofv3 run of a child process
    under its own time limit, from the per-launch trace (the stats file sums over the sizes; it has to be there all the same).  A
    child that fails or leaves no trace ends the script: nothing more is started on the GPU."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["timeout", "-k", "10", str(limit), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d,
               "-o", "wband", "--", sys.executable, os.path.abspath(__file__), "--trace-child", str(calls),
               "--sizes", ",".join(str(s) for s in sizes)]
        rc = subprocess.call(cmd)
        if rc:
            print(f"traced child failed (exit {rc}): {' '.join(cmd)}", file=sys.stderr)
            sys.exit(rc)
        stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        launches = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if not stats or not launches:
            print("the traced child left no *kernel_stats.csv / *kernel_trace.csv", file=sys.stderr)
            sys.exit(1)
        rows = list(csv.DictReader(open(launches[0])))
        if not rows or not {"Kernel_Name", "Start_Timestamp", "End_Timestamp"} <= set(rows[0]):
            # (a trace file of another layout: the stats file's means over all sizes are what is left)
            return {"all sizes": {r["Name"][:96]: {"calls": int(r["Calls"]), "mean_us": float(r["AverageNs"]) * 1e-3}
                                  for r in csv.DictReader(open(stats[0])) if any(k in r.get("Name", "") for k in KERNELS)}}
        rows.sort(key=lambda r: int(r["Start_Timestamp"]))
        out = {}
        for kernel in KERNELS:
            mine = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3 for r in rows if kernel in r["Kernel_Name"]]
            per = len(mine) // len(sizes)                    # launches of this kernel per size, in launch order
            for k, S in enumerate(sizes):
                us = mine[k * per:(k + 1) * per][1:]         # (the first launch of a size loads code or grows the LDS limit)
                if us:
                    out.setdefault(f"S={S}", {})[kernel] = {"calls": len(us), "mean_us": float(np.mean(us)),
                                                            "min_us": float(np.min(us)), "max_us": float(np.max(us))}
        for per_size in out.values():
            if "band_wselect_kernel" in per_size and "band_select_kernel" in per_size:
                per_size["wselect_over_select"] = per_size["band_wselect_kernel"]["mean_us"] / per_size["band_select_kernel"]["mean_us"]
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", default="1024,4096,16384")
    ap.add_argument("--trace-calls", type=int, default=4)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-child", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sizes = [int(s) for s in args.sizes.split(",")]
    if args.trace_child:
        trace_child(sizes, args.trace_child)
        return
    res = {"what": "mp_model_band_weighted against mp_model_band", "q": list(Q), "components": ["Ltot"],
           "rows": "Humped truth + 0.02 N(0,1)", "weights": "exp(3 N(0,1))"}
    if not args.no_trace:                                   # first: no GPU is open in this process yet; exits if the child fails
        res["kernel_trace"] = trace(sizes, args.trace_calls)
    h = handle()
    res.update({"n_grid": int(h.tgrid.size), "calls": []})
    for S, P, w in inputs(sizes):
        h.model_band(P, Q)                                  # warm-up (workspace growth, code objects)
        h.model_band(P, Q, weights=w)
        plain, weighted = [], []
        for _ in range(args.reps):                          # alternated: both see the same machine state
            t0 = time.perf_counter()
            _, _, used = h.model_band(P, Q)
            plain.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            h.model_band(P, Q, weights=w)
            weighted.append(time.perf_counter() - t0)
        p, wt = float(np.median(plain)), float(np.median(weighted))
        res["calls"].append({"S": S, "n_used": used, "band_ms_median": p * 1e3, "band_ms_min": float(np.min(plain)) * 1e3,
                             "weighted_ms_median": wt * 1e3, "weighted_ms_min": float(np.min(weighted)) * 1e3,
                             "weighted_over_band": wt / p})
    h.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
