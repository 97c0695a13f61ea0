"""Cost and accuracy of the bridge-sampling evidence under the Student-t proposal and Warp-III (mp_bridge_logz_warp,
EnsembleSampler.log_evidence(method="bridge", proposal=, nu=, warp=)), one GPU.  The rows, the timing and the sampler runs are
tools/bridge_bench.py's, so that the figures stand next to that file's.

    python tools/bridge_warp_bench.py time [--sizes 4096,65536,1048576]   ms per call at N1 = N2 = n_fit = N on the posterior of
                                                                       Humped with yerr x 10: plain mp_bridge_logz and the four
                                                                       variants of mp_bridge_logz_warp in the same process
    python tools/bridge_warp_bench.py evidence [--seeds 8]              ln Z of Humped as it is (1 500 steps, KDE + DE) under the
                                                                       four variants, from the same chain per sampler seed
    python tools/bridge_warp_bench.py all --dir DIR                     the two, each a child process under its own `timeout`;
                                                                       stops at the first failure; writes
                                                                       DIR/r30_bridge_warp_bench.json

Prints one JSON line per mode; --out also writes it to a file.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bridge_bench as bb  # noqa: E402

VARIANTS = {"plain": dict(proposal="normal", warp=False), "warped": dict(proposal="normal", warp=True),
            "t5": dict(proposal="t", nu=5, warp=False), "warped_t5": dict(proposal="t", nu=5, warp=True)}
RECORDED = {"humped_plain_r28": "-46.424 +- 0.004 (sd over 8 seeds), 4 repetitions", "ms_per_call_r28": {"4096": 0.60, "65536": 4.1, "1048576": 61.0}}


def plain_through_the_new_entry(handle, fit, est, lnp, lo, hi, n):
    """mp_bridge_logz_warp with proposal 0 and warp 0 on the arguments of the timed calls"""
    from magprop_amd import _capi
    out = np.zeros((1, _capi.BRIDGE_WARP_NOUT))
    dp = _capi._dptr
    _capi.check(_capi.lib().mp_bridge_logz_warp(handle._h, dp(fit), n, dp(est), dp(lnp), n, 6, 0, dp(lo), dp(hi), n, 1, 1, n / 8.0, 1000, 1.0e-10,
                                                0, _capi.BRIDGE_NORMAL, 0, 0, dp(out), *([None] * 10)), "mp_bridge_logz_warp")
    return {"out": out}


def time_mode(args):
    out = {"what": "ms per call at N1 = N2 = n_fit = N on Humped with yerr x 10, one repetition, neff = N / 8: mp_bridge_logz, then "
                   "mp_bridge_logz_warp under each variant (plain: proposal 0, warp 0 through the new entry), same process, same rows",
           "rounds": args.rounds, "recorded": RECORDED["ms_per_call_r28"], "sizes": {}}
    for n in (int(v) for v in args.sizes.split(",")):
        s, *rows = bb.posterior_inputs(n, 7)
        fit, est, lnp, lo, hi = (np.ascontiguousarray(v, dtype=np.float64) for v in (*rows[:3], *rows[3]))
        row = {}
        old = lambda: s.handle.bridge_logz(fit, est, lnp, lo, hi, seed=1, neff=n / 8.0)
        row["mp_bridge_logz"] = bb.timed(old, args.rounds)
        o = old()["out"][0]
        row["mp_bridge_logz"].update(lnz=float(o[0]), dlnz=float(o[3]), updates=int(o[4]), status=int(o[5]), finite_draws=int(o[6]))
        for name, kw in VARIANTS.items():
            if name == "plain":                     # the front end sends the defaults to mp_bridge_logz: the new entry by hand
                call = lambda: plain_through_the_new_entry(s.handle, fit, est, lnp, lo, hi, n)
            else:
                call = lambda kw=kw: s.handle.bridge_logz(fit, est, lnp, lo, hi, seed=1, neff=n / 8.0, **kw)
            row[name] = bb.timed(call, args.rounds)
            o = call()["out"][0]
            row[name].update(lnz=float(o[0]), dlnz=float(o[3]), updates=int(o[4]), status=int(o[5]), finite_draws=int(o[6]),
                             est_mirrors=int(o[12]), draw_mirrors=int(o[13]))
        row["lnprob_batch_of_n_rows"] = bb.timed(lambda: s.handle.lnprob_batch(est), args.rounds)
        s.close()
        out["sizes"][str(n)] = row
    return out


def evidence_mode(args):
    from magprop_amd import DEMove, EnsembleSampler, KDEMove
    x, y, yerr = bb.data(1.0)
    runs = {v: [] for v in VARIANTS}
    for seed in range(args.seeds):
        rng = np.random.default_rng(2000 + seed)
        s = EnsembleSampler(512, 6, x, y, yerr, seed=1000 + seed, moves=[(KDEMove(), 0.8), (DEMove(), 0.2)])
        s.run_mcmc(bb.TRUTH + 1.0e-4 * rng.standard_normal((512, 6)), 1500)
        neff = None
        for v, kw in VARIANTS.items():
            t0 = time.perf_counter()
            r = s.log_evidence(method="bridge", discard=500, repetitions=4, neff=neff, **kw)
            dt = time.perf_counter() - t0
            neff = r.neff                           # the chain's own, found once
            runs[v].append({"seed": 1000 + seed, "lnz": r.lnz, "dlnz": r.dlnz, "dlnz_reps": r.dlnz_reps, "lnz_is": float(np.median(r.lnz_is)),
                            "updates": r.niter.tolist(), "status": r.status.tolist(), "neff": r.neff, "n_est": r.n_est,
                            "finite_draw_fraction": float(np.mean(r.n_finite) / r.n_draws), "est_mirrors": r.est_mirrors,
                            "draw_mirrors": r.draw_mirrors.tolist(), "seconds": dt})
        s.close()
    out = {"what": f"log_evidence(method='bridge') of Humped as it is over {args.seeds} sampler seeds, 512 walkers, 1 500 steps of KDE + DE, "
                   "500 discarded, 4 repetitions; every variant from the same chain", "recorded": RECORDED["humped_plain_r28"], "variants": {}}
    for v, rows in runs.items():
        lnz = np.array([r["lnz"] for r in rows])
        out["variants"][v] = {"mean_lnz": float(lnz.mean()), "sd_over_seeds": float(lnz.std(ddof=1)), "mean_dlnz": float(np.mean([r["dlnz"] for r in rows])),
                              "mean_dlnz_reps": float(np.mean([r["dlnz_reps"] for r in rows])),
                              "mean_importance_sampling": float(np.mean([r["lnz_is"] for r in rows])), "runs": rows}
    return out


def run_all(args):
    """Every GPU step a child process under its own time limit; the first failure ends the script."""
    os.makedirs(args.dir, exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__)]
    parts = {k: os.path.join(args.dir, f"r30_bridge_warp_{k}.json") for k in ("time", "evidence")}
    for limit, mode in ((300, "time"), (400, "evidence")):
        cmd = me + [mode, "--out", parts[mode], "--sizes", args.sizes, "--rounds", str(args.rounds), "--seeds", str(args.seeds)]
        rc = subprocess.call(["timeout", "-k", "10", str(limit)] + cmd)
        if rc:
            print(f"step failed (exit {rc}): {' '.join(cmd)}", file=sys.stderr)
            return rc
    out = {k: json.load(open(p)) for k, p in parts.items()}
    with open(os.path.join(args.dir, "r30_bridge_warp_bench.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for p in parts.values():
        os.remove(p)
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=("time", "evidence", "all"))
    ap.add_argument("--sizes", default="4096,65536,1048576")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--seeds", type=int, default=8)
    ap.add_argument("--dir", default="profiles")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.mode == "all":
        sys.exit(run_all(args))
    res = {"time": time_mode, "evidence": evidence_mode}[args.mode](args)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
