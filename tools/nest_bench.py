"""Throughput and time to the stop rule of the nested sampler (magprop_amd.nested), one GPU.

    python tools/nest_bench.py rate       iterations/s and evaluations/s inside walks: a fixed number of iterations
    python tools/nest_bench.py converge   wall time to the stop rule (dlogz = 0.01), ln Z +- error, iterations, ncall
    python tools/nest_bench.py profile    a short run to profile (rocprofv3 --kernel-trace --stats -- python tools/nest_bench.py profile)
    python tools/nest_bench.py scatter    8 seeded runs of each case in one launch: the std of ln Z against the mean logzerr

--sample slice runs every mode with slice updates (NestedSampler(sample="slice"), its defaults: ndim slices per walk, mu = 1,
m = 8, 64 shrink points at most) instead of the random walk; --sample both alternates the two methods case by case.

Cases: Humped (tests/golden), Humped with yerr x 10 (the brute-force evidence case of tests/test_gpu_tempering.py) and the unit
Gaussian in an asymmetric 6-d box (target 1: the walk kernel without the model).  nlive = 1024, nbatch = 256, 25 steps per
walk.  Rate: the live set as NestedSampler draws it, 5 warm iterations, then --iters timed iterations with dlogz = 1e-300 (no run
stops); mp_nested_run returns when they are done.  Prints one JSON line; --out also writes it to a file.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from magprop_amd import _capi, nested  # noqa: E402

NLIVE, NBATCH, WALKS = 1024, 256, 25
G_LO = np.array([-2.0, -1.0, -4.0, -0.5, -3.0, -1.5])
G_HI = np.array([3.0, 2.5, 1.5, 4.0, 0.5, 1.0])
CASES = ("Humped", "Humped_yerr10", "gaussian6")


def sampler(case, seed=0, n_runs=1, sample="rwalk"):
    if case == "gaussian6":
        return nested.NestedSampler(nlive=NLIVE, nbatch=NBATCH, walks=WALKS, target="gaussian", bounds=np.stack([G_LO, G_HI], axis=1),
                                    seed=seed, n_runs=n_runs, sample=sample)
    g = np.load(os.path.join(ROOT, "tests", "golden", "golden_synth.npz"))
    f = 10.0 if case.endswith("yerr10") else 1.0
    return nested.NestedSampler(g["Humped_x"], g["Humped_y"], f * g["Humped_yerr"], nlive=NLIVE, nbatch=NBATCH, walks=WALKS,
                                seed=seed, n_runs=n_runs, sample=sample)


def _slice_fields(s, r, walks):
    """The slice counters of a result (random walk: none)."""
    if not s.slices:
        return {}
    return {"slices": s.slices, "nexpand": r.nexpand, "ncontract": r.ncontract, "failed_slices": r.nfail,
            "failed_slice_percent": round(100.0 * r.nfail / max(walks * s.slices, 1), 4)}


def rate(case, iters, warm=5, seed=0, sample="rwalk"):
    s = sampler(case, seed, sample=sample)
    s._open()
    live, _ = s.initial_live()
    L = _capi.lib()
    dp = C.POINTER(C.c_double)
    ns = L.mp_nested_create(s.handle._h, NLIVE, NBATCH, 1, s.ndim, None, C.c_uint64(seed), WALKS, 0.0, 0.1, 1e-300,
                            s.lower.ctypes.data_as(dp), s.upper.ctypes.data_as(dp), nested.TARGETS[s.target])
    assert ns, _capi.last_error()
    try:
        if s.slices:
            _capi.check(L.mp_nested_set_slice(ns, s.slices, s.slice_mu, s.max_steps_out, s.max_shrink), "set_slice")
        _capi.check(L.mp_nested_set_live(ns, np.ascontiguousarray(live).ctypes.data_as(dp)), "set_live")
        _capi.check(L.mp_nested_run(ns, warm, None), "run")
        st0 = nested.get_state(L, ns, 1, NLIVE, s.ndim)
        t0 = time.perf_counter()
        _capi.check(L.mp_nested_run(ns, iters, None), "run")
        dt = time.perf_counter() - t0
        st1 = nested.get_state(L, ns, 1, NLIVE, s.ndim)
    finally:
        L.mp_nested_destroy(ns)
        s.close()
    ev = int(st1["ncall"][0] - st0["ncall"][0])
    acc = int(st1["nacc"][0] - st0["nacc"][0])
    out = {"case": case, "sample": sample, "nlive": NLIVE, "nbatch": NBATCH, "walks": WALKS, "iterations": iters,
           "seconds": round(dt, 4), "ms_per_iteration": round(1e3 * dt / iters, 3), "iterations_per_s": round(iters / dt, 1),
           "walk_evals_per_s": round(ev / dt, 0), "evals_per_walk": round(ev / (iters * NBATCH), 2),
           "accepted_per_walk": round(acc / (iters * NBATCH), 2),
           "walks_without_a_move": int(st1["nzero"][0] - st0["nzero"][0])}
    if s.slices:
        out["slices"] = s.slices
    return out


def converge(case, seed=1, sample="rwalk"):
    sampler(case, seed, sample=sample).run_nested(maxiter=2)        # (library load, first launches)
    s = sampler(case, seed, sample=sample)
    t0 = time.perf_counter()
    r = s.run_nested(dlogz=0.01)
    dt = time.perf_counter() - t0
    s.close()
    out = {"case": case, "sample": sample, "nlive": NLIVE, "nbatch": NBATCH, "walks": WALKS, "seconds": round(dt, 3),
           "logz": round(r.logz, 4), "logzerr": round(r.logzerr, 4), "information": round(r.information, 3), "niter": r.niter,
           "ncall": r.ncall, "eff_percent": round(r.eff, 3), "walks_without_a_step": r.nzero,
           "walks_without_a_step_percent": round(100.0 * r.nzero / max(r.niter * NBATCH, 1), 4),
           "ln_f_valid": round(r.ln_f_valid, 5), "stopped": r.stopped}
    out.update(_slice_fields(s, r, r.niter * NBATCH))
    return out


def scatter(case, n_seeds=8, seed=100, sample="rwalk"):
    """n_seeds runs of one case in one launch per iteration (run r: seed of the sampler, its own Philox stream): the std of ln Z
    over the runs against their mean logzerr."""
    s = sampler(case, seed, n_runs=n_seeds, sample=sample)
    t0 = time.perf_counter()
    res = s.run_nested(dlogz=0.01)
    dt = time.perf_counter() - t0
    s.close()
    lnz = np.array([r.logz for r in res])
    err = np.array([r.logzerr for r in res])
    walks = sum(r.niter for r in res) * NBATCH
    out = {"case": case, "sample": sample, "runs": n_seeds, "seconds": round(dt, 3), "logz": [round(v, 4) for v in lnz],
           "logz_mean": round(float(lnz.mean()), 4), "logz_std": round(float(lnz.std(ddof=1)), 4),
           "logzerr_mean": round(float(err.mean()), 4), "std_over_logzerr": round(float(lnz.std(ddof=1) / err.mean()), 3),
           "niter": [r.niter for r in res], "walks_without_a_step": sum(r.nzero for r in res)}
    if s.slices:
        out["failed_slices"] = sum(r.nfail for r in res)
        out["failed_slice_percent"] = round(100.0 * out["failed_slices"] / max(walks * s.slices, 1), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("rate", "converge", "profile", "scatter"))
    ap.add_argument("--sample", choices=("rwalk", "slice", "both"), default="rwalk")
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--out")
    args = ap.parse_args()
    samples = ("rwalk", "slice") if args.sample == "both" else (args.sample,)
    if args.mode == "rate":
        rows = [rate(c, args.iters, sample=m) for c in CASES for m in samples]
    elif args.mode == "converge":
        rows = [converge(c, sample=m) for c in CASES for m in samples]
    elif args.mode == "scatter":
        rows = [scatter(c, sample=m) for c in CASES for m in samples]
    else:
        rows = [rate(c, 10, warm=0, sample=m) for c in ("Humped", "gaussian6") for m in samples]
    line = json.dumps({"mode": args.mode, "sample": args.sample, "rows": rows})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
