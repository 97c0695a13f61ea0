"""Cost of the sampler's device posterior monitor (EnsembleSampler.monitor_posterior) on Humped, one GPU.

    python tools/post_bench.py rate [--sizes 64,1024,4096]   walker-steps/s with the monitor off and on (256 / 64 bins)
    python tools/post_bench.py summary                   one get_posterior against numpy doing the same on the stored chain
    python tools/post_bench.py profile --walkers 1024    a short monitored run to profile (rocprofv3 --kernel-trace --stats -- ...)
    python tools/post_bench.py all --dir DIR             the three above, each a child process under its own `timeout`; stops at
                                                         the first failure; writes DIR/r13_post_{rate,summary}.json and
                                                         DIR/r13_post_kernel_stats.csv

Rate: per size one sampler with the monitor off and one with it on (range = the prior box), both started at the Humped truth
(1e-4 ball) and warmed --warm steps; then --rounds rounds in which the two run --steps unstored steps in turn (alternated in one
process on one box); a setting's rate is its best round.  on_over_off = steps/s with the monitor on over off.
Summary: a chain of --summary-steps x 1 024 x 6 stored with the monitor on; the device figure is the mean of 5 get_posterior
calls, the host figure one pass of numpy over the stored chain for the same numbers (np.histogram per dimension, np.histogram2d
per pair, mean, covariance and argmax).
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
BINS, BINS2 = 256, 64


def data():
    g = np.load(os.path.join(ROOT, "tests", "golden", "golden_synth.npz"))
    return g["Humped_x"], g["Humped_y"], g["Humped_yerr"]


def _start(nwalk, seed):
    return np.array(TRUTH) + 1.0e-4 * np.random.default_rng(seed).standard_normal((nwalk, 6))


def rate(args):
    x, y, yerr = data()
    out = {"what": "sampler rate on Humped with the posterior monitor off and on (256 / 64 bins over the prior box), settings alternated in one process",
           "warm": args.warm, "steps": args.steps, "rounds": args.rounds, "sizes": {}}
    for nwalk in (int(v) for v in args.sizes.split(",")):
        samplers = {}
        for on in (False, True):
            s = EnsembleSampler(nwalk, 6, x, y, yerr, seed=1)
            if on:
                s.monitor_posterior(BINS, BINS2)
            s.run_mcmc(_start(nwalk, 0), args.warm, store=False)
            samplers[on] = s
        best = {k: np.inf for k in samplers}
        for _ in range(args.rounds):
            for k, s in samplers.items():
                t0 = time.perf_counter()
                s.run_mcmc(None, args.steps, store=False)
                best[k] = min(best[k], time.perf_counter() - t0)
        out["sizes"][str(nwalk)] = {"off_walker_steps_per_s": args.steps * nwalk / best[False],
                                    "on_walker_steps_per_s": args.steps * nwalk / best[True],
                                    "on_over_off": best[False] / best[True]}
        for s in samplers.values():
            s.close()
    return out


def _numpy_summary(chain, lnp, lo, hi):
    flat = chain.reshape(-1, chain.shape[-1])
    nd = flat.shape[1]
    h1 = [np.histogram(flat[:, d], bins=BINS, range=(lo[d], hi[d]))[0] for d in range(nd)]
    h2 = [np.histogram2d(flat[:, a], flat[:, b], bins=BINS2, range=[(lo[a], hi[a]), (lo[b], hi[b])])[0]
          for a in range(nd) for b in range(a + 1, nd)]
    return h1, h2, flat.mean(axis=0), np.cov(flat.T), flat[int(np.argmax(lnp.ravel()))]


def summary(args):
    x, y, yerr = data()
    nwalk, steps = 1024, args.summary_steps
    s = EnsembleSampler(nwalk, 6, x, y, yerr, seed=1)
    s.run_mcmc(_start(nwalk, 0), 200, store=False)
    s.monitor_posterior(BINS, BINS2, range="ensemble")
    s.run_mcmc(None, steps)
    s.get_posterior()
    t0 = time.perf_counter()
    for _ in range(5):
        got = s.get_posterior()
    t_dev = (time.perf_counter() - t0) / 5
    _, _, lo, hi = s._post
    chain, lnp = s.get_chain(), s.get_log_prob()
    t0 = time.perf_counter()
    h1, h2, mean, cov, best = _numpy_summary(chain, lnp, lo, hi)
    t_host = time.perf_counter() - t0
    s.close()
    return {"what": "one get_posterior against numpy over the stored chain (histograms, mean, covariance, argmax)",
            "chain": f"{steps}x{nwalk}x6", "device_s": t_dev, "host_s": t_host, "host_over_device": t_host / t_dev,
            "hist1_cells_that_differ": int(sum(np.count_nonzero(a != b) for a, b in zip(h1, got["hist1"]))),
            "hist2_cells_that_differ": int(sum(np.count_nonzero(a != b) for a, b in zip(h2, got["hist2"]))),
            "mean_max_abs_diff": float(np.max(np.abs(mean - got["mean"]))), "cov_max_rel_diff": float(np.max(np.abs(got["cov"] / cov - 1.0))),
            "best_equal": bool(np.array_equal(best, got["best_x"]))}


def profile(args):
    x, y, yerr = data()
    s = EnsembleSampler(args.walkers, 6, x, y, yerr, seed=1)
    s.monitor_posterior(BINS, BINS2)
    s.set_positions(_start(args.walkers, 0))
    for _ in range(3):
        s.run_mcmc(None, 100, store=False)
        s.get_posterior()
    s.close()
    return {"what": "profiling run (monitor on, 256 / 64 bins: 3 x 100 steps and a get_posterior each)", "walkers": args.walkers}


def run_all(args):
    """Every GPU step a child process under its own time limit; the first failure ends the script."""
    os.makedirs(args.dir, exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__)]
    trace = os.path.join(args.dir, "r13_post_trace")
    steps = [
        (400, me + ["rate", "--out", os.path.join(args.dir, "r13_post_rate.json")]),
        (300, me + ["summary", "--out", os.path.join(args.dir, "r13_post_summary.json")]),
        (200, ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", trace, "--"] + me + ["profile", "--walkers", "1024"]),
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
    shutil.copy(stats[0], os.path.join(args.dir, "r13_post_kernel_stats.csv"))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=("rate", "summary", "profile", "all"))
    ap.add_argument("--sizes", default="64,1024,4096")
    ap.add_argument("--walkers", type=int, default=1024)
    ap.add_argument("--warm", type=int, default=200)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--summary-steps", type=int, default=2000)
    ap.add_argument("--dir", default="profiles")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.mode == "all":
        sys.exit(run_all(args))
    res = {"rate": rate, "summary": summary, "profile": profile}[args.mode](args)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
