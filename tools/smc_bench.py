"""Time to beta = 1 and scatter of ln Z of the tempered SMC sampler (magprop_amd.smc), next to the nested sampler on the same
case in the same call, one GPU.

    python tools/smc_bench.py scatter   8 runs in one launch per stage at N = 1 024 and 4 096: wall time to beta = 1, stages,
                                        evaluations per stage, mean and std of ln Z; then NestedSampler (nlive 1 024, nbatch 256,
                                        25 steps, dlogz 0.01), 8 runs in one launch per iteration: wall time, ncall, mean and std
                                        of ln Z and its own mean logzerr
    python tools/smc_bench.py sweep     the adaptive moves (SMCSampler(adapt=...)) over corr in 0.5, 0.3, 0.2, 0.1 and rounds of 2, 5
                                        and 10 steps, next to 10 and 40 steps per move without adaptation and to the nested
                                        sampler, on both cases at both sizes in this one call: the rows the defaults of
                                        magprop_amd.smc.ADAPT_DEFAULTS are chosen from
    python tools/smc_bench.py profile   a short run to profile (rocprofv3 --kernel-trace --stats -- python tools/smc_bench.py
                                        profile): smc_stage_kernel next to smc_move_kernel (and, with --adapt,
                                        smc_tune_kernel and the launches of rounds no run makes); --sizes and --runs choose
                                        the particle counts and the runs per launch

Cases: Humped (tests/golden) and Humped with yerr x 10 (the brute-force evidence case of tests/test_gpu_tempering.py, ln Z =
-5.5046).  --walks steps per move (default 10), ess = 0.5; --adapt runs scatter and profile adaptively (the shipped defaults,
--walks the length of a round).  Every timed run follows a run of two stages (library load, first launches).  Prints
one JSON line; --out also writes it to a file.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from magprop_amd import nested, smc  # noqa: E402

WALKS, ESS, RUNS = 10, 0.5, 8
SIZES = (1024, 4096)
CASES = ("Humped", "Humped_yerr10")
BRUTE_FORCE = {"Humped_yerr10": -5.5046}


def data(case):
    g = np.load(os.path.join(ROOT, "tests", "golden", "golden_synth.npz"))
    f = 10.0 if case.endswith("yerr10") else 1.0
    return g["Humped_x"], g["Humped_y"], f * g["Humped_yerr"]


SWEEP_CORR, SWEEP_ROUND, SWEEP_MAX_STEPS = (0.5, 0.3, 0.2, 0.1), (2, 5, 10), 160


def smc_row(case, n, walks=WALKS, seed=100, runs=RUNS, adapt=False):
    x, y, yerr = data(case)
    smc.SMCSampler(x, y, yerr, nparticles=n, walks=walks, ess=ESS, n_runs=runs, seed=seed, adapt=adapt).run(max_stages=2)
    s = smc.SMCSampler(x, y, yerr, nparticles=n, walks=walks, ess=ESS, n_runs=runs, seed=seed, adapt=adapt)
    t0 = time.perf_counter()
    res = s.run()
    dt = time.perf_counter() - t0
    s.close()
    res = res if isinstance(res, list) else [res]
    lnz = np.array([r.logz for r in res])
    stages = [r.nstages for r in res]
    row = {"case": case, "method": "smc", "nparticles": n, "walks": walks, "ess": ESS, "runs": runs, "seconds": round(dt, 3),
           "status": sorted({r.status for r in res}), "stages": stages,
           "evals_per_stage": round(float(np.mean([r.ncall_stage.mean() for r in res])), 1),
           "ncall": [r.ncall for r in res], "nfail": [r.nfail for r in res],
           "accept_first_last": [round(float(res[0].accept[0]), 3), round(float(res[0].accept[-1]), 3)],
           "logz": [round(float(v), 4) for v in lnz], "logz_mean": round(float(lnz.mean()), 4),
           "logz_std": round(float(lnz.std(ddof=1)), 4) if runs > 1 else None,
           "log_bias_std2_over_2": round(float(lnz.std(ddof=1)) ** 2 / 2.0, 5) if runs > 1 else None}
    row["ncall_mean"] = round(float(np.mean([r.ncall for r in res])), 1)
    if s.adapt is not None:
        rounds = np.concatenate([r.rounds for r in res])
        row.update(adapt=s.adapt, rounds_mean=round(float(rounds.mean()), 2), rounds_max=int(rounds.max()),
                   stages_at_max_rounds=int(np.sum(rounds == s.adapt["max_rounds"])), rounds_run0=res[0].rounds.tolist(),
                   scale_run0=[round(float(v), 4) for v in res[0].scale], rho_run0=[round(float(v), 3) for v in res[0].rho],
                   accept_run0=[round(float(v), 3) for v in res[0].accept])
    if case in BRUTE_FORCE:
        row["minus_brute_force"] = round(float(lnz.mean()) - BRUTE_FORCE[case], 4)
    return row


def nested_row(case, seed=100, runs=RUNS):
    x, y, yerr = data(case)
    kw = dict(nlive=1024, nbatch=256, walks=25, n_runs=runs, seed=seed)
    nested.NestedSampler(x, y, yerr, **kw).run_nested(maxiter=2)
    s = nested.NestedSampler(x, y, yerr, **kw)
    t0 = time.perf_counter()
    res = s.run_nested(dlogz=0.01)
    dt = time.perf_counter() - t0
    s.close()
    lnz = np.array([r.logz for r in res])
    row = {"case": case, "method": "nested", "nlive": 1024, "nbatch": 256, "walks": 25, "runs": runs, "seconds": round(dt, 3),
           "niter": [r.niter for r in res], "ncall": [r.ncall for r in res], "logz": [round(float(v), 4) for v in lnz],
           "logz_mean": round(float(lnz.mean()), 4), "logz_std": round(float(lnz.std(ddof=1)), 4),
           "logzerr_mean": round(float(np.mean([r.logzerr for r in res])), 4)}
    if case in BRUTE_FORCE:
        row["minus_brute_force"] = round(float(lnz.mean()) - BRUTE_FORCE[case], 4)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("scatter", "sweep", "profile"))
    ap.add_argument("--adapt", action="store_true", help="adaptive moves at the shipped defaults (scatter, profile)")
    ap.add_argument("--walks", type=int, help="Metropolis steps per move of the SMC runs (default 10; with --adapt the steps of a round, default 2)")
    ap.add_argument("--sizes", default=",".join(str(n) for n in SIZES), help="profile: the particle counts, comma separated")
    ap.add_argument("--runs", type=int, default=RUNS, help="profile: runs per launch")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.walks is None:
        args.walks = smc.WALKS_ADAPTIVE if args.adapt else WALKS
    if args.mode == "scatter":
        rows = []
        for c in CASES:
            rows += [smc_row(c, n, args.walks, adapt=args.adapt) for n in SIZES] + [nested_row(c)]
    elif args.mode == "sweep":
        rows = []
        for c in CASES:
            for n in SIZES:
                rows += [smc_row(c, n, 10), smc_row(c, n, 40)]
                rows += [smc_row(c, n, w, adapt=dict(corr=corr, max_rounds=SWEEP_MAX_STEPS // w)) for w in SWEEP_ROUND for corr in SWEEP_CORR]
            rows.append(nested_row(c))
    else:
        rows = [smc_row("Humped", int(n), args.walks, runs=args.runs, adapt=args.adapt) for n in args.sizes.split(",")]
    line = json.dumps({"mode": args.mode, "rows": rows})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
