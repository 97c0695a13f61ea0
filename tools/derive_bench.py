"""Timing of the derived quantities (mp_model_derived) on one GPU.

Synchronised calls after warm-up (the entry returns when the table is in host memory) at n = 1 024, 4 096, 16 384 rows,
alternated in the same process with the host path on a 256-row subsample: mp_model_lc row by row and the numpy restatement
of the definition (tests/derive_restated.py).  Rows: the Humped truth with a 0.02 spread in sampler coordinates (a burnt-in
chain's rows).  Then, in a `rocprofv3 --kernel-trace --stats` run of its own (a fresh child process, tracing only), the time
of derive_kernel next to the curve launch that feeds it, at one chunk of mp_n_simd rows; if that child fails or leaves no
stats file the script exits non-zero before it touches the GPU itself.  Prints one JSON line; --out also
writes it to a file.

    python tools/derive_bench.py --reps 5 --out profiles/r14_derive_bench.json
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

import derive_restated as dr  # noqa: E402
from magprop_amd import _capi, engine, synth  # noqa: E402

TRUTH = np.array([1.0, 5.0, -3.0, 2.0, -1.0, 0.0])


def handle():
    h = _capi.Handle(_capi.cfg_synth(), engine.grid(None), 0)
    h.set_prior(synth.PRIOR_LOWER, synth.PRIOR_UPPER, synth.LOG_MASK)
    return h


def host_path(h, P):
    out = np.full((len(P), dr.N), np.nan)
    for i, p in enumerate(P):
        s, lc, traj = h.model_lc(p, want_traj=True)
        if s == 0:
            out[i] = dr.derive_row(np.stack([lc[1], lc[2], lc[3], traj[0], traj[1]]), lc[0])
    return out


def trace_child(calls):
    """what the traced process runs: `calls` calls of one chunk"""
    h = handle()
    P = TRUTH + 0.02 * np.random.default_rng(0).standard_normal((h.n_simd, 6))
    for _ in range(calls):
        h.model_derived(P)
    h.close()


def trace(calls, limit=200):
    """{kernel name: {"calls", "mean_us", ...}} of the curve and the derive kernel from a rocprofv3 run of a child process under
    its own time limit.  A child that fails or leaves no stats file ends the script: nothing more is started on the GPU."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["timeout", "-k", "10", str(limit), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d,
               "-o", "derive", "--", sys.executable, os.path.abspath(__file__), "--trace-child", str(calls)]
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
            if "derive_kernel" in name or "lnprob_kernel" in name:
                out[name[:96]] = {"calls": int(row["Calls"]), "mean_us": float(row["AverageNs"]) * 1e-3,
                                  "min_us": float(row["MinNs"]) * 1e-3, "max_us": float(row["MaxNs"]) * 1e-3}
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="1024,4096,16384")
    ap.add_argument("--host-rows", type=int, default=256)
    ap.add_argument("--trace-calls", type=int, default=6)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-child", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.trace_child:
        trace_child(args.trace_child)
        return
    res = {"what": "mp_model_derived", "rows": "Humped truth + 0.02 N(0,1)"}
    if not args.no_trace:                                   # first: no GPU is open in this process yet; exits if the child fails
        res["kernel_trace"] = trace(args.trace_calls)
    h = handle()
    res.update({"n_grid": int(h.tgrid.size), "n_simd": int(h.n_simd), "calls": []})
    rng = np.random.default_rng(0)
    for n in (int(s) for s in args.sizes.split(",")):
        P = TRUTH + 0.02 * rng.standard_normal((n, 6))
        Pphys = P[:args.host_rows].copy()
        Pphys[:, 2:] = 10.0 ** Pphys[:, 2:]
        h.model_derived(P)                                  # warm-up (workspace growth, code objects)
        host_path(h, Pphys[:4])
        dev, host = [], []
        for _ in range(args.reps):                          # alternated: both see the same machine state
            t0 = time.perf_counter()
            _, _, used = h.model_derived(P)
            dev.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            host_path(h, Pphys)
            host.append(time.perf_counter() - t0)
        d, ho = float(np.median(dev)), float(np.median(host))
        res["calls"].append({"n": n, "n_used": used, "ms_median": d * 1e3, "ms_min": float(np.min(dev)) * 1e3,
                             "us_per_row": d / n * 1e6, "host_rows": len(Pphys), "host_ms_median": ho * 1e3,
                             "host_us_per_row": ho / len(Pphys) * 1e6, "speedup_per_row": (ho / len(Pphys)) / (d / n)})
    h.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
