"""Cost and accuracy of the bridge-sampling evidence (mp_bridge_logz, EnsembleSampler.log_evidence(method="bridge")), one GPU.

    python tools/bridge_bench.py time [--sizes 4096,65536,1048576]   ms per call at N1 = N2 = n_fit = N: the unit-Gaussian test
                                                                  target in 6-D (the estimator's own cost: no model), the
                                                                  posterior of Humped (N model evaluations on top), and the
                                                                  numpy restatement of the fixed point on the same a and b
    python tools/bridge_bench.py evidence [--seeds 8]              ln Z, dlnz and the scatter over sampler seeds on Humped with
                                                                  yerr x 10 (the brute-force case) and on Humped as it is
    python tools/bridge_bench.py profile --n 1048576 [--target 0]  one warmed call to profile:
                                                                  rocprofv3 --kernel-trace --stats -- python tools/bridge_bench.py ...
    python tools/bridge_bench.py all --dir DIR                     the three, each a child process under its own `timeout`; stops
                                                                  at the first failure; writes DIR/r28_bridge_bench.json

Times are a host clock around whole calls (a call ends in a stream synchronise), the median of --rounds calls after one
warm-up call per shape, with their least and largest.  The kernel split comes from the profiler's run of its own, never from
the timed calls.  Prints one JSON line per mode; --out also writes it to a file.
"""
import argparse
import csv
import glob
import json
import math
import os
import shutil
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TRUTH = np.array([1.0, 5.0, -3.0, 2.0, -1.0, 0.0])     # Humped, sampler coordinates
# what the other routes recorded on the two cases (README: nested sampler, SMC sampler; tests/test_gpu_tempering.py: brute force)
RECORDED = {"humped_yerr_x10": {"brute_force": -5.5046, "brute_force_ess": 160641, "nested": "-5.430 +- 0.053", "smc": "-5.510, sd 0.084 over 8 runs"},
            "humped": {"nested": -46.57, "smc": -46.52}}


def data(inflate=1.0):
    g = np.load(os.path.join(ROOT, "tests", "golden", "golden_synth.npz"))
    return g["Humped_x"], g["Humped_y"], g["Humped_yerr"] * inflate


def spread(times):
    ms = np.array(times) * 1e3
    return {"ms_median": float(np.median(ms)), "ms_min": float(ms.min()), "ms_max": float(ms.max()), "calls": len(times)}


def gaussian_inputs(n, rng):
    x = rng.standard_normal((2 * n, 6))
    return x[:n], x[n:], -0.5 * np.sum(x[n:] * x[n:], axis=1)


def posterior_inputs(n, seed):
    """n fit rows and n estimator rows with their lnprob from a KDE-move run on Humped with yerr x 10, and the sampler (its
    handle evaluates the draws)"""
    from magprop_amd import EnsembleSampler, KDEMove, LogProb, synth
    x, y, yerr = data(10.0)
    lo, hi = synth.PRIOR_LOWER, synth.PRIOR_UPPER
    rng = np.random.default_rng(seed)
    start = lo + (hi - lo) * rng.random((4096, 6))
    start = start[np.isfinite(LogProb(x, y, yerr)(start))][:512]
    s = EnsembleSampler(512, 6, x, y, yerr, seed=seed, moves=KDEMove())
    s.run_mcmc(start, 100, store=False)
    steps = -(-2 * n // 512)
    s.run_mcmc(None, steps)
    rows, lnp = s.get_chain().reshape(-1, 6), s.get_log_prob().reshape(-1)
    return s, rows[:n], rows[-n:], lnp[-n:], (lo, hi)


def timed(fn, rounds):
    fn()                                                  # warm-up: code objects, buffers of this shape
    times = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return spread(times)


def time_mode(args):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import bridge_restated as br
    from raw_abi import synth_handle
    out = {"what": "ms per call of mp_bridge_logz at N1 = N2 = n_fit = N, one repetition, tol 1e-10; numpy: the restated fixed point on the call's own a and b",
           "rounds": args.rounds, "sizes": {}}
    h = synth_handle()
    for n in (int(v) for v in args.sizes.split(",")):
        row = {}
        fit, est, lnp = gaussian_inputs(n, np.random.default_rng(n))
        call = lambda details=False: h.bridge_logz(fit, est, lnp, target=1, seed=1, details=details)
        row["gaussian_6d"] = timed(call, args.rounds)
        res = call(True)
        o = res["out"][0]
        row["gaussian_6d"].update(lnz=float(o[0]), truth=3.0 * math.log(2.0 * math.pi), dlnz=float(o[3]), updates=int(o[4]), status=int(o[5]))
        if n <= args.numpy_max:
            a = lnp - res["est_lnq"]
            b = res["draw_lnp"][0] - res["draw_lnq"][0]
            k = br.constants(n, n, n)
            t0 = time.perf_counter()
            ref = br.fixed_point(a, b, *k, 1000, 1.0e-10)
            row["numpy_fixed_point"] = {"ms": (time.perf_counter() - t0) * 1e3, "updates": int(ref[br.NITER]), "lambda": float(ref[br.LAMBDA])}
            t0 = time.perf_counter()
            with np.errstate(all="ignore"):          # the same updates as plain vectorised numpy, sums in numpy's own order
                lam, c = float(ref[br.LAMBDA0]), 0
                while c < 1000:
                    c2 = k[1] + lam
                    num = np.logaddexp.reduce(b - np.logaddexp(k[0] + b, c2)) - k[3]
                    den = np.logaddexp.reduce(-np.logaddexp(k[0] + a, c2)) - k[2]
                    c, step, lam = c + 1, abs((num - den) - lam), num - den
                    if step <= 1.0e-10:
                        break
            row["numpy_plain_fixed_point"] = {"ms": (time.perf_counter() - t0) * 1e3, "updates": c, "lambda": float(lam)}
        s, pfit, pest, plnp, (lo, hi) = posterior_inputs(n, 7)
        pcall = lambda: s.handle.bridge_logz(pfit, pest, plnp, lo, hi, seed=1, neff=n / 8.0)
        row["humped_yerr_x10"] = timed(pcall, args.rounds)
        o = pcall()["out"][0]
        row["humped_yerr_x10"].update(lnz=float(o[0]), dlnz=float(o[3]), updates=int(o[4]), status=int(o[5]), finite_draws=int(o[6]))
        batch = lambda: s.handle.lnprob_batch(pest)
        row["lnprob_batch_of_n_rows"] = timed(batch, args.rounds)
        s.close()
        out["sizes"][str(n)] = row
    h.close()
    return out


def wide_importance_sampling(s, discard, lo, hi, rng, n=1 << 22):
    """A yardstick that needs no fixed point and no half of the chain as estimator: plain importance sampling from the Gaussian
    fitted to the chain with its scale inflated by 1.5 and by 2 (tails heavier than the posterior's in every direction the
    fit sees), n draws each, evaluated by lnprob_batch: ln Z and the effective sample size (sum w)^2 / sum w^2."""
    rows = s.get_chain()[discard:].reshape(-1, 6)
    m, L = rows.mean(axis=0), np.linalg.cholesky(np.cov(rows.T))
    ln_v = float(np.sum(np.log(hi - lo)))
    out = {}
    for scale in (1.5, 2.0):
        z = rng.standard_normal((n, 6))
        x = m + scale * (z @ L.T)
        lnq = -0.5 * np.sum(z * z, axis=1) - np.sum(np.log(scale * np.diag(L))) - 3.0 * math.log(2.0 * math.pi)
        inside = np.all((x >= lo) & (x <= hi), axis=1)
        lnp = np.full(n, -np.inf)
        lnp[inside] = np.concatenate([s.handle.lnprob_batch(c) for c in np.array_split(x[inside], 16)])
        lw = np.where(np.isfinite(lnp), lnp - lnq, -np.inf)
        w = np.exp(lw - lw.max())
        out[f"scale_{scale}"] = {"lnz": float(lw.max() + math.log(w.sum() / n) - ln_v), "ess": float(w.sum() ** 2 / np.sum(w * w)), "draws": n,
                                 "relative_error": float(math.sqrt(np.sum(w * w)) / w.sum())}
    return out


def wide_first(rows):
    return next((r.pop("wide") for r in rows if r.get("wide")), None)


def evidence_mode(args):
    from magprop_amd import DEMove, EnsembleSampler, KDEMove, LogProb, synth
    lo, hi = synth.PRIOR_LOWER, synth.PRIOR_UPPER
    out = {"what": f"log_evidence(method='bridge') over {args.seeds} sampler seeds, 512 walkers; recorded: what the other routes gave", "cases": {}}
    for case, inflate in (("humped_yerr_x10", 10.0), ("humped", 1.0)):
        x, y, yerr = data(inflate)
        lp = LogProb(x, y, yerr)
        rows = []
        for seed in range(args.seeds):
            rng = np.random.default_rng(2000 + seed)
            if inflate > 1.0:           # the posterior fills a sizeable part of the box: start from box draws, the KDE move alone
                start = lo + (hi - lo) * rng.random((4096, 6))
                start = start[np.isfinite(lp(start))][:512]
                moves, steps, discard = KDEMove(), 400, 100
            else:                       # the narrow posterior: from the truth, KDE + DE as tests/test_gpu_moves_kde.py runs it
                start = TRUTH + 1.0e-4 * rng.standard_normal((512, 6))
                moves, steps, discard = [(KDEMove(), 0.8), (DEMove(), 0.2)], 1500, 500
            s = EnsembleSampler(512, 6, x, y, yerr, seed=1000 + seed, moves=moves)
            s.run_mcmc(start, steps)
            t0 = time.perf_counter()
            r = s.log_evidence(method="bridge", discard=discard, repetitions=4)
            dt = time.perf_counter() - t0
            tau = s.get_autocorr_time(quiet=True)
            wide = wide_importance_sampling(s, discard, lo, hi, rng) if seed == 0 else None
            s.close()
            rows.append({"seed": 1000 + seed, "lnz": r.lnz, "dlnz": r.dlnz, "dlnz_reps": r.dlnz_reps, "lnz_is": float(np.median(r.lnz_is)),
                         "updates": r.niter.tolist(), "status": r.status.tolist(), "neff": r.neff, "n_est": r.n_est,
                         "finite_draw_fraction": float(np.mean(r.n_finite) / r.n_draws), "tau_max": float(np.max(tau)), "seconds": dt, "wide": wide})
        lnz = np.array([r["lnz"] for r in rows])
        out["cases"][case] = {"wide_importance_sampling": wide_first(rows), "steps": steps, "discard": discard, "mean_lnz": float(lnz.mean()), "sd_over_seeds": float(lnz.std(ddof=1)),
                              "mean_dlnz": float(np.mean([r["dlnz"] for r in rows])), "mean_importance_sampling": float(np.mean([r["lnz_is"] for r in rows])),
                              "recorded": RECORDED[case], "runs": rows}
    return out


def profile_mode(args):
    from raw_abi import synth_handle
    n = args.n
    if args.target == 0:
        s, fit, est, lnp, (lo, hi) = posterior_inputs(n, 7)
        call = lambda: s.handle.bridge_logz(fit, est, lnp, lo, hi, seed=1, neff=n / 8.0)
    else:
        h = synth_handle()
        fit, est, lnp = gaussian_inputs(n, np.random.default_rng(n))
        call = lambda: h.bridge_logz(fit, est, lnp, target=1, seed=1)
    call()
    o = call()["out"][0]
    return {"what": f"profiling run: two calls at N = {n}, target {args.target}", "lnz": float(o[0]), "updates": int(o[4])}


def kernel_rows(path):
    """[{name, calls, total_ns, percent}] of a rocprofv3 kernel_stats.csv, largest first"""
    with open(path) as f:
        rows = list(csv.DictReader(f))
    pick = lambda r, *keys: next((r[k] for k in keys if k in r), None)
    out = [{"name": pick(r, "Name", "KernelName"), "calls": int(float(pick(r, "Calls", "Count") or 0)),
            "total_ns": float(pick(r, "TotalDurationNs", "TotalDuration(ns)", "TotalDuration") or 0.0),
            "percent": float(pick(r, "Percentage", "Percent") or 0.0)} for r in rows]
    return sorted(out, key=lambda r: -r["total_ns"])


def run_all(args):
    """Every GPU step a child process under its own time limit; the first failure ends the script."""
    os.makedirs(args.dir, exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__)]
    parts = {k: os.path.join(args.dir, f"r28_bridge_{k}.json") for k in ("time", "evidence")}
    steps = [(560, me + ["time", "--out", parts["time"]], None), (400, me + ["evidence", "--out", parts["evidence"]], None)]
    for target in (1, 0):
        trace = os.path.join(args.dir, f"r28_bridge_trace_target{target}")
        steps.append((300, ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", trace, "--"] + me +
                      ["profile", "--n", str(1 << 20 if target else 65536), "--target", str(target)], (trace, target)))
    kernels = {}
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
            kernels["gaussian_6d_n1048576" if trace[1] else "humped_yerr_x10_n65536"] = kernel_rows(stats[0])[:12]
            shutil.rmtree(trace[0], ignore_errors=True)
    out = {k: json.load(open(p)) for k, p in parts.items()}
    out["kernels"] = {"what": "rocprofv3 --kernel-trace --stats of a run of its own (two calls and, for the posterior, the sampler run that made the rows)",
                      **kernels}
    with open(os.path.join(args.dir, "r28_bridge_bench.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for p in parts.values():
        os.remove(p)
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=("time", "evidence", "profile", "all"))
    ap.add_argument("--sizes", default="4096,65536,1048576")
    ap.add_argument("--numpy-max", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--seeds", type=int, default=8)
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--target", type=int, default=1)
    ap.add_argument("--dir", default="profiles")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "tests"))      # raw_abi.synth_handle, bridge_restated
    if args.mode == "all":
        sys.exit(run_all(args))
    res = {"time": time_mode, "evidence": evidence_mode, "profile": profile_mode}[args.mode](args)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
