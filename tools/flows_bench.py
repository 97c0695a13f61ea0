"""Timing of the radii, mass flows and torques (mp_model_flows, mp_model_flow_band) on one GPU.

Synchronised calls after warm-up (an entry returns when its results are in host memory), alternated in the same process with
the neighbour that runs the same curve launches: mp_model_flows (the summary only) against mp_model_derived at n = 1 024,
16 384 and 131 072 rows, the same call with three cell curves returned against the summary only at n = 1 024 and 4 096, and
mp_model_flow_band (one curve, three quantiles) against mp_model_band (Ltot) at n = 1 024, 4 096
and 16 384 rows.  Rows: the Humped truth with a 0.02 spread in sampler coordinates (a burnt-in chain's rows).  Then, in a
`rocprofv3 --kernel-trace --stats` run of its own (a fresh child process, tracing only), the times of flow_cells_kernel and
flow_reduce_kernel next to the curve launch that feeds them, at one chunk of mp_n_simd rows; if that child fails or leaves no
stats file the script exits non-zero before it touches the GPU itself.  Prints one JSON line; --out also writes it to a file.

    python tools/flows_bench.py --reps 5 --out profiles/r18_flows_bench.json
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
Q3 = (0.16, 0.5, 0.84)


def handle():
    h = _capi.Handle(_capi.cfg_synth(), engine.grid(None), 0)
    h.set_prior(synth.PRIOR_LOWER, synth.PRIOR_UPPER, synth.LOG_MASK)
    return h


def trace_child(calls):
    """what the traced process runs: `calls` calls of one chunk"""
    h = handle()
    P = TRUTH + 0.02 * np.random.default_rng(0).standard_normal((h.n_simd, 6))
    for _ in range(calls):
        h.model_flows(P)
    h.close()


def trace(calls, limit=200):
    """{kernel name: {"calls", "mean_us", ...}} of the curve, cells and reduce kernels from a rocprofv3 run of a child process
    under its own time limit.  A child that fails or leaves no stats file ends the script: nothing more is started on the GPU."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["timeout", "-k", "10", str(limit), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d,
               "-o", "flows", "--", sys.executable, os.path.abspath(__file__), "--trace-child", str(calls)]
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
            if "flow_cells_kernel" in name or "flow_reduce_kernel" in name or "lnprob_kernel" in name:
                out[name[:96]] = {"calls": int(row["Calls"]), "mean_us": float(row["AverageNs"]) * 1e-3,
                                  "min_us": float(row["MinNs"]) * 1e-3, "max_us": float(row["MaxNs"]) * 1e-3}
        return out


def alternate(reps, a, b):
    """medians and minima (s) of a() and b(), called in turn so that both see the same machine state"""
    ta, tb = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        a()
        ta.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        b()
        tb.append(time.perf_counter() - t0)
    return float(np.median(ta)), float(np.min(ta)), float(np.median(tb)), float(np.min(tb))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="1024,16384,131072")
    ap.add_argument("--band-sizes", default="1024,4096,16384")
    ap.add_argument("--trace-calls", type=int, default=6)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-child", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.trace_child:
        trace_child(args.trace_child)
        return
    res = {"what": "mp_model_flows, mp_model_flow_band", "rows": "Humped truth + 0.02 N(0,1)"}
    if not args.no_trace:                                   # first: no GPU is open in this process yet; exits if the child fails
        res["kernel_trace"] = trace(args.trace_calls)
    h = handle()
    res.update({"n_grid": int(h.tgrid.size), "n_simd": int(h.n_simd), "flows": [], "curves": [], "band": []})
    rng = np.random.default_rng(0)
    for n in (int(s) for s in args.sizes.split(",")):
        P = TRUTH + 0.02 * rng.standard_normal((n, 6))
        used = h.model_flows(P)[3]                          # warm-up (workspace growth, code objects)
        h.model_derived(P)
        f, fmin, d, dmin = alternate(args.reps, lambda: h.model_flows(P), lambda: h.model_derived(P))
        res["flows"].append({"n": n, "n_used": used, "ms_median": f * 1e3, "ms_min": fmin * 1e3, "us_per_row": f / n * 1e6,
                             "derived_ms_median": d * 1e3, "derived_ms_min": dmin * 1e3, "ratio_to_derived": f / d})
    # with cell curves returned: one strided device-to-host copy per curve and chunk into the caller's (pageable) buffer
    three = ("fastness", "Mdot_prop", "Mdot_acc")
    for n in (1024, 4096):
        P = TRUTH + 0.02 * rng.standard_normal((n, 6))
        h.model_flows(P, curves=three)
        f, fmin, d, dmin = alternate(args.reps, lambda: h.model_flows(P, curves=three), lambda: h.model_flows(P))
        res["curves"].append({"n": n, "curves": len(three), "mb_returned": n * len(three) * h.tgrid.size * 8 / 1e6, "ms_median": f * 1e3,
                              "ms_min": fmin * 1e3, "summary_only_ms_median": d * 1e3, "ratio_to_summary_only": f / d})
    for n in (int(s) for s in args.band_sizes.split(",")):
        P = TRUTH + 0.02 * rng.standard_normal((n, 6))
        used = h.model_flow_band(P, Q3, ("fastness",))[2]
        h.model_band(P, Q3, ("Ltot",))
        f, fmin, b, bmin = alternate(args.reps, lambda: h.model_flow_band(P, Q3, ("fastness",)), lambda: h.model_band(P, Q3, ("Ltot",)))
        res["band"].append({"n": n, "n_used": used, "ms_median": f * 1e3, "ms_min": fmin * 1e3, "band_ms_median": b * 1e3,
                            "band_ms_min": bmin * 1e3, "ratio_to_band": f / b})
    h.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
