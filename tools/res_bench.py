"""Cost of the sampler's device sample reservoir (EnsembleSampler.monitor_samples) on Humped, one GPU.

    python tools/res_bench.py rate [--shapes 64,1024,4096,8x64]   ms per step with the monitor off, on at K = 4 096, on at
                                                              K = 65 536, and with the posterior monitor on instead
    python tools/res_bench.py unset --walkers 1024            ms per step of a sampler whose monitor was never set (the A/B leg:
                                                              alternate it with a process on the parent commit's tree)
    python tools/res_bench.py profile --walkers 1024          a short monitored run to profile, the filling chunks and the steady
                                                              state in two processes (--phase fill | steady):
                                                              rocprofv3 --kernel-trace --stats -- python tools/res_bench.py ...
    python tools/res_bench.py all --dir DIR                   rate and the two profiling runs, each a child process under its own
                                                              `timeout`; stops at the first failure; writes
                                                              DIR/r26_reservoir_rate.json and DIR/r26_reservoir_kernels_{fill,steady}.csv

Rate: per shape (walkers, or TxW for T temperatures of W walkers) one sampler per setting, all started at the Humped truth (1e-4
ball) and warmed --warm steps; then --rounds rounds in which the settings run --steps unstored steps in turn (alternated in one
process on one box).  Reported per setting: the median of the rounds' ms per step with their least and largest.  The posterior
monitor forces the same slab writes as the reservoir, so the difference of those two settings is the monitors' own cost.
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

TRUTH = [1.0, 5.0, -3.0, 2.0, -1.0, 0.0]     # Humped, sampler coordinates
SETTINGS = (("off", None), ("reservoir K=4096", 4096), ("reservoir K=65536", 65536), ("posterior monitor", "post"))


def data():
    g = np.load(os.path.join(ROOT, "tests", "golden", "golden_synth.npz"))
    return g["Humped_x"], g["Humped_y"], g["Humped_yerr"]


def make(shape, setting):
    from magprop_amd import EnsembleSampler, tempering
    x, y, yerr = data()
    n_temps, nwalk = (int(v) for v in shape.split("x")) if "x" in shape else (1, int(shape))
    betas = tempering.geometric_ladder(n_temps, 1.0e-3) if n_temps > 1 else None
    s = EnsembleSampler(nwalk, 6, x, y, yerr, seed=1, betas=betas)
    if setting == "post":
        s.monitor_posterior(256, 64)
    elif setting is not None:
        s.monitor_samples(size=setting)
    s.set_positions(np.array(TRUTH) + 1.0e-4 * np.random.default_rng(0).standard_normal((s.ntotal, 6)))
    return s


def summarise(times, steps):
    ms = np.array(times) / steps * 1e3
    return {"ms_per_step_median": float(np.median(ms)), "ms_per_step_min": float(ms.min()), "ms_per_step_max": float(ms.max())}


def rate(args):
    out = {"what": "ms per step on Humped with the sample reservoir off and on, and with the posterior monitor on instead; settings alternated in one process",
           "warm": args.warm, "steps": args.steps, "rounds": args.rounds, "shapes": {}}
    for shape in args.shapes.split(","):
        samplers = {name: make(shape, setting) for name, setting in SETTINGS}
        for s in samplers.values():
            s.run_mcmc(None, args.warm, store=False)
        times = {name: [] for name in samplers}
        for _ in range(args.rounds):
            for name, s in samplers.items():
                t0 = time.perf_counter()
                s.run_mcmc(None, args.steps, store=False)
                times[name].append(time.perf_counter() - t0)
        row = {name: summarise(times[name], args.steps) for name in samplers}
        for name, setting in SETTINGS:
            if isinstance(setting, int):
                got = samplers[name].get_samples()
                row[name]["rows_held"], row[name]["n_seen"] = int(len(got["step"])), got["n_seen"]
        for s in samplers.values():
            s.close()
        out["shapes"][shape] = row
    return out


def unset(args):
    s = make(str(args.walkers), None)
    s.run_mcmc(None, args.warm, store=False)
    times = []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        s.run_mcmc(None, args.steps, store=False)
        times.append(time.perf_counter() - t0)
    s.close()
    from magprop_amd import _capi
    return dict(summarise(times, args.steps), what="monitor never set", walkers=args.walkers, lib=_capi.LIB_PATH)


def profile(args):
    """fill: K = 65 536 and 60 steps of 1 024 walkers, so that the reservoir is still filling at the end (every sample a
    candidate in every slice).  steady: K = 4 096 over 400 steps; the reservoir is full after the first 4 of them, so all but
    the first of the 50 slices of 8 steps run against a threshold."""
    size, steps = (65536, 60) if args.phase == "fill" else (4096, 400)
    s = make(str(args.walkers), size)
    s.run_mcmc(None, steps, store=False)
    got = s.get_samples()
    s.close()
    return {"what": f"profiling run ({args.phase}: K = {size}, {steps} steps)", "walkers": args.walkers, "rows_held": int(len(got["step"])),
            "n_seen": got["n_seen"]}


def run_all(args):
    """Every GPU step a child process under its own time limit; the first failure ends the script."""
    os.makedirs(args.dir, exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__)]
    steps = [(500, me +["rate", "--out", os.path.join(args.dir, "r26_reservoir_rate.json")], None)]
    for phase in ("fill", "steady"):
        trace = os.path.join(args.dir, "r26_reservoir_trace_" + phase)
        steps.append((200, ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", trace, "--"] + me +
                      ["profile", "--walkers", "1024", "--phase", phase], (trace, phase)))
    for limit, cmd, trace in steps:
        rc = subprocess.call(["timeout", "-k", "10", str(limit)] + cmd)
        if rc:
            print(f"step failed (exit {rc}): {' '.join(cmd)}", file=sys.stderr)
            return rc
        if trace:
            stats = glob.glob(os.path.join(trace[0], "**", "*kernel_stats.csv"), recursive=True)
            if not stats:
                print(f"the profiling step left no *kernel_stats.csv under {trace[0]}", file=sys.stderr)
                return 1
            shutil.copy(stats[0], os.path.join(args.dir, f"r26_reservoir_kernels_{trace[1]}.csv"))
            shutil.rmtree(trace[0], ignore_errors=True)
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=("rate", "unset", "profile", "all"))
    ap.add_argument("--shapes", default="64,1024,4096,8x64")
    ap.add_argument("--walkers", type=int, default=1024)
    ap.add_argument("--phase", choices=("fill", "steady"), default="steady")
    ap.add_argument("--warm", type=int, default=100)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--dir", default="profiles")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.mode == "all":
        sys.exit(run_all(args))
    res = {"rate": rate, "unset": unset, "profile": profile}[args.mode](args)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
