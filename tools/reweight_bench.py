"""Timing of the importance reweighting (mp_model_reweight) on one GPU.

Synchronised calls after warm-up (the entry returns when the log weights, the table and the tail rows are in host memory) at
n_alt = 1, 8 and 64 alternatives (Gaussians and Student-t's in turn, every one with a jitter) and 1 024, 16 384 and 131 072 rows,
on the 50-point Humped light curve and on the 1 944-point one (tests/golden/golden_longlc.npz), each alternated in the same process
with mp_model_pointwise on the same rows: the same chunks and curve launches with its own cells kernel and reductions -- the
yardstick for what the row kernel's log and log1p cost on top of the curve launches.  (The feature leaves that entry alone apart
from its select kernel, whose body moved into the template of mp_tail.h that both selects use: its time here is this build's.)
Rows: the Humped truth with a 0.02 spread in sampler coordinates (a burnt-in chain's rows).  Then, in a `rocprofv3 --kernel-trace
--stats` run of its own (a fresh child process, tracing only), the times of the three reweight kernels next to the curve launch
that feeds them, at one chunk of mp_n_simd rows per n_alt on both light curves; if that child fails or leaves no stats file the
script exits non-zero before it touches the GPU itself.  Prints one JSON line; --out also writes it.

    python tools/reweight_bench.py --out profiles/r31_reweight_bench.json
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

from magprop_amd import _capi, engine, reweight, synth  # noqa: E402

TRUTH = np.array([1.0, 5.0, -3.0, 2.0, -1.0, 0.0])
DATASETS, ROWS, N_ALT = ("humped50", "synth1944"), (1024, 16384, 131072), (1, 8, 64)


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


def alternatives(n_alt):
    """Gaussians and Student-t's in turn, scales 1 .. 2, every one with a jitter: no term is cheaper than the general one"""
    return [reweight.gaussian(1.0 + k / 64.0, 0.05) if k % 2 == 0 else reweight.student_t(3.0 + k, 1.0 + k / 64.0, 0.05) for k in range(n_alt)]


def trace_child(calls):
    """what the traced process runs: `calls` calls of one chunk per n_alt on each light curve"""
    data = datasets()
    h = handle(data)
    P = TRUTH + 0.02 * np.random.default_rng(0).standard_normal((h.n_simd, 6))
    for _ in range(calls):
        for k, name in enumerate(data):
            for n_alt in N_ALT:
                h.model_reweight(P, *reweight.pack(alternatives(n_alt), data[name][0].size), ds_id=k)
    h.close()


def trace(calls, limit=300):
    """{kernel name: {"calls", "mean_us", ...}} of the curve and the reweight kernels from a rocprofv3 run of a child process
    under its own time limit (the calls of every n_alt and both light curves pooled per kernel).  A child that fails or leaves no
    stats file ends the script: nothing more is started on the GPU."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["timeout", "-k", "10", str(limit), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d,
               "-o", "reweight", "--", sys.executable, os.path.abspath(__file__), "--trace-child", str(calls)]
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
            if "reweight_" in name or "lnprob_kernel" in name:
                out[name[:96]] = {"calls": int(row["Calls"]), "mean_us": float(row["AverageNs"]) * 1e-3,
                                  "min_us": float(row["MinNs"]) * 1e-3, "max_us": float(row["MaxNs"]) * 1e-3}
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--trace-calls", type=int, default=4)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-child", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.trace_child:
        trace_child(args.trace_child)
        return
    res = {"what": "mp_model_reweight", "rows": "Humped truth + 0.02 N(0,1)",
           "pointwise_note": "mp_model_pointwise as this build runs it: the reweight feature moved the body of its select kernel into a template both "
                             "selects share (mp_tail.h) and touches nothing else of it"}
    if not args.no_trace:                                   # first: no GPU is open in this process yet; exits if the child fails
        res["kernel_trace"] = trace(args.trace_calls)
    data = datasets()
    h = handle(data)
    res.update({"n_grid": int(h.tgrid.size), "n_simd": int(h.n_simd), "calls": []})
    rng = np.random.default_rng(0)
    for ds_id, name in enumerate(DATASETS):
        n_obs = data[name][0].size
        packed = {n_alt: reweight.pack(alternatives(n_alt), n_obs) for n_alt in N_ALT}
        for n in ROWS:
            P = TRUTH + 0.02 * rng.standard_normal((n, 6))
            h.model_pointwise(P[:2048], ds_id=ds_id)         # warm-up (code objects; the timed calls grow the workspaces once more)
            for n_alt in N_ALT:
                h.model_reweight(P[:2048], *packed[n_alt], ds_id=ds_id)
            pw, rw = [], {n_alt: [] for n_alt in N_ALT}
            for rep in range(args.reps + 1):                # alternated: all see the same machine state; the first round is warm-up
                t0 = time.perf_counter()
                h.model_pointwise(P, ds_id=ds_id)
                t = [time.perf_counter()]
                for n_alt in N_ALT:
                    table, used = h.model_reweight(P, *packed[n_alt], ds_id=ds_id)[1::3]
                    t.append(time.perf_counter())
                if rep:
                    pw.append(t[0] - t0)
                    for k, n_alt in enumerate(N_ALT):
                        rw[n_alt].append(t[k + 1] - t[k])
            p = float(np.median(pw))
            for n_alt in N_ALT:
                d = float(np.median(rw[n_alt]))
                res["calls"].append({"dataset": name, "n_obs": int(n_obs), "n": n, "n_alt": n_alt, "n_used": used, "ms_median": d * 1e3,
                                     "ms_min": float(np.min(rw[n_alt])) * 1e3, "us_per_row": d / n * 1e6,
                                     "ns_per_term_over_pointwise": max(d - p, 0.0) / (n * float(n_obs) * n_alt) * 1e9,
                                     "pointwise_ms_median": p * 1e3, "over_pointwise": d / p})
    h.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
