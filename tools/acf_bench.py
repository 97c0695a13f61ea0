"""Cost of the sampler's device autocorrelation monitor (EnsembleSampler.monitor_autocorr) on Humped, one GPU.

    python tools/acf_bench.py rate [--sizes 64,512,1024,4096] [--lags 256,1024,4096]   steps/s with the monitor off and on
    python tools/acf_bench.py estimate                   one get_autocorr_time(device=True) against the host path, same stored chain
    python tools/acf_bench.py profile --walkers 1024     a short monitored run to profile (rocprofv3 --kernel-trace --stats -- ...)
    python tools/acf_bench.py all --dir DIR              the three above, each a child process under its own `timeout`; stops at
                                                         the first failure; writes DIR/r12_acf_{rate,estimate}.json and
                                                         DIR/r12_acf_kernel_stats.csv

Rate: per size one sampler per setting (monitor off, on with every --lags), all started at the Humped truth (1e-4 ball) and
warmed --warm steps; then --rounds rounds in which every setting runs --steps unstored steps in turn (alternated in one process
on one box); a setting's rate is its best round.  on_over_off = steps/s with the monitor on over off.
Estimate: chains of 6 000 x 512 x 6 and 10 000 x 1 024 x 6 stored with the monitor on (max_lag 1 024); the device figure is the
mean of 5 calls, the host figure one call of the FFT estimator on the stored chain; device_K4096_s is the device figure of the
same run under max_lag 4 096.
Prints one JSON line; --out also writes it to a file.
"""
import argparse
import glob
import json
import os
import shutil
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from magprop_amd import EnsembleSampler  # noqa: E402

TRUTH = [1.0, 5.0, -3.0, 2.0, -1.0, 0.0]     # Humped, sampler coordinates


def data():
    g = np.load(os.path.join(ROOT, "tests", "golden", "golden_synth.npz"))
    return g["Humped_x"], g["Humped_y"], g["Humped_yerr"]


def _start(nwalk, seed):
    return np.array(TRUTH) + 1.0e-4 * np.random.default_rng(seed).standard_normal((nwalk, 6))


def rate(args):
    x, y, yerr = data()
    lags = [int(v) for v in args.lags.split(",")]
    out = {"what": "sampler steps/s on Humped with the autocorrelation monitor off and on, settings alternated in one process",
           "warm": args.warm, "steps": args.steps, "rounds": args.rounds, "sizes": {}}
    for nwalk in (int(v) for v in args.sizes.split(",")):
        samplers = {}
        for k in [0] + lags:
            s = EnsembleSampler(nwalk, 6, x, y, yerr, seed=1)
            if k:
                s.monitor_autocorr(max_lag=k)
            s.run_mcmc(_start(nwalk, 0), args.warm, store=False)
            samplers[k] = s
        best = {k: np.inf for k in samplers}
        for _ in range(args.rounds):
            for k, s in samplers.items():
                t0 = time.perf_counter()
                s.run_mcmc(None, args.steps, store=False)
                best[k] = min(best[k], time.perf_counter() - t0)
        row = {"off_steps_per_s": args.steps / best[0], "off_walker_steps_per_s": args.steps * nwalk / best[0]}
        for k in lags:
            row[f"K{k}_steps_per_s"] = args.steps / best[k]
            row[f"K{k}_on_over_off"] = best[0] / best[k]
        out["sizes"][str(nwalk)] = row
        for s in samplers.values():
            s.close()
    return out


def estimate(args):
    x, y, yerr = data()
    out = {"what": "one tau estimate: get_autocorr_time(device=True) against the host FFT path on the same stored chain", "chains": {}}
    for steps, nwalk in ((6000, 512), (10000, 1024)):
        s = EnsembleSampler(nwalk, 6, x, y, yerr, seed=1)
        s.monitor_autocorr(max_lag=1024)
        s.run_mcmc(_start(nwalk, 0), steps)
        s.get_autocorr_time(device=True, quiet=True)
        t0 = time.perf_counter()
        for _ in range(5):
            dev = s.get_autocorr_time(device=True, quiet=True)
        t_dev = (time.perf_counter() - t0) / 5
        t0 = time.perf_counter()
        host = s.get_autocorr_time(quiet=True)
        t_host = time.perf_counter() - t0
        s.close()
        # the same run (same seed, no host chain) under the largest monitor: the estimate reads max_lag^2 / 32 ring rows per series
        s = EnsembleSampler(nwalk, 6, x, y, yerr, seed=1)
        s.monitor_autocorr(max_lag=4096)
        s.run_mcmc(_start(nwalk, 0), steps, store=False)
        dev4 = s.get_autocorr_time(device=True, quiet=True)
        t0 = time.perf_counter()
        for _ in range(5):
            s.get_autocorr_time(device=True, quiet=True)
        t_dev4 = (time.perf_counter() - t0) / 5
        s.close()
        out["chains"][f"{steps}x{nwalk}x6"] = {"device_s": t_dev, "device_K4096_s": t_dev4, "host_s": t_host,
                                               "host_over_device": t_host / t_dev,
                                               "tau_device": [float(v) for v in dev], "tau_host": [float(v) for v in host],
                                               "max_rel_diff": float(np.nanmax(np.abs(dev / host - 1.0))),
                                               "K4096_equals_K1024": bool(np.array_equal(dev, dev4))}
    return out


def profile(args):
    x, y, yerr = data()
    s = EnsembleSampler(args.walkers, 6, x, y, yerr, seed=1)
    for k in (1024, 4096):
        s.monitor_autocorr(max_lag=k)
        s.set_positions(_start(args.walkers, 0))
        for _ in range(3):
            s.run_mcmc(None, 100, store=False)
            s.get_autocorr_time(device=True, quiet=True)
    s.close()
    return {"what": "profiling run (monitor on, max_lag 1024 then 4096: 3 x 100 steps and an estimate each)", "walkers": args.walkers}


def run_all(args):
    """Every GPU step a child process under its own time limit; the first failure ends the script."""
    os.makedirs(args.dir, exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__)]
    trace = os.path.join(args.dir, "r12_acf_trace")
    steps = [
        (600, me + ["rate", "--out", os.path.join(args.dir, "r12_acf_rate.json")]),
        (900, me + ["estimate", "--out", os.path.join(args.dir, "r12_acf_estimate.json")]),
        (300, ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", trace, "--"] + me + ["profile", "--walkers", "1024"]),
    ]
    for limit, cmd in steps:
        rc = subprocess.call(["timeout", "-k", "10", str(limit)] + cmd)
        if rc:
            print(f"step failed (exit {rc}): {' '.join(cmd)}", file=sys.stderr)
            return rc
    stats = glob.glob(os.path.join(trace, "**", "*kernel_stats.csv"), recursive=True)
    if not stats:
        print(f"the profiling step left no *kernel_stats.csv under {trace}", file=sys.stderr)
        return 1
    shutil.copy(stats[0], os.path.join(args.dir, "r12_acf_kernel_stats.csv"))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=("rate", "estimate", "profile", "all"))
    ap.add_argument("--sizes", default="64,512,1024,4096")
    ap.add_argument("--lags", default="256,1024,4096")
    ap.add_argument("--walkers", type=int, default=1024)
    ap.add_argument("--warm", type=int, default=200)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--dir", default="profiles")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.mode == "all":
        sys.exit(run_all(args))
    res = {"rate": rate, "estimate": estimate, "profile": profile}[args.mode](args)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
