"""Throughput and time to the stop rule of the nested sampler (magprop_amd.nested), one GPU.

    python tools/nest_bench.py rate       iterations/s and evaluations/s inside walks: a fixed number of iterations
    python tools/nest_bench.py converge   wall time to the stop rule (dlogz = 0.01), ln Z +- error, iterations, ncall
    python tools/nest_bench.py profile    a short run to profile (rocprofv3 --kernel-trace --stats -- python tools/nest_bench.py profile)

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


def sampler(case, seed=0, n_runs=1):
    if case == "gaussian6":
        return nested.NestedSampler(nlive=NLIVE, nbatch=NBATCH, walks=WALKS, target="gaussian", bounds=np.stack([G_LO, G_HI], axis=1),
                                    seed=seed, n_runs=n_runs)
    g = np.load(os.path.join(ROOT, "tests", "golden", "golden_synth.npz"))
    f = 10.0 if case.endswith("yerr10") else 1.0
    return nested.NestedSampler(g["Humped_x"], g["Humped_y"], f * g["Humped_yerr"], nlive=NLIVE, nbatch=NBATCH, walks=WALKS,
                                seed=seed, n_runs=n_runs)


def rate(case, iters, warm=5, seed=0):
    s = sampler(case, seed)
    s._open()
    live, _ = s.initial_live()
    L = _capi.lib()
    dp = C.POINTER(C.c_double)
    ns = L.mp_nested_create(s.handle._h, NLIVE, NBATCH, 1, s.ndim, None, C.c_uint64(seed), WALKS, 0.0, 0.1, 1e-300,
                            s.lower.ctypes.data_as(dp), s.upper.ctypes.data_as(dp), nested.TARGETS[s.target])
    assert ns, _capi.last_error()
    try:
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
    return {"case": case, "nlive": NLIVE, "nbatch": NBATCH, "walks": WALKS, "iterations": iters, "seconds": round(dt, 4),
            "ms_per_iteration": round(1e3 * dt / iters, 3), "iterations_per_s": round(iters / dt, 1),
            "walk_evals_per_s": round(ev / dt, 0), "evals_per_walk": round(ev / (iters * NBATCH), 2),
            "accepted_per_walk": round(acc / (iters * NBATCH), 2)}


def converge(case, seed=1):
    sampler(case, seed).run_nested(maxiter=2)                       # (library load, first launches)
    s = sampler(case, seed)
    t0 = time.perf_counter()
    r = s.run_nested(dlogz=0.01)
    dt = time.perf_counter() - t0
    s.close()
    return {"case": case, "nlive": NLIVE, "nbatch": NBATCH, "walks": WALKS, "seconds": round(dt, 3), "logz": round(r.logz, 4),
            "logzerr": round(r.logzerr, 4), "information": round(r.information, 3), "niter": r.niter, "ncall": r.ncall,
            "eff_percent": round(r.eff, 3), "walks_without_a_step": r.nzero, "ln_f_valid": round(r.ln_f_valid, 5),
            "stopped": r.stopped}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("rate", "converge", "profile"))
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.mode == "rate":
        rows = [rate(c, args.iters) for c in CASES]
    elif args.mode == "converge":
        rows = [converge(c) for c in CASES]
    else:
        rows = [rate("Humped", 10, warm=0), rate("gaussian6", 10, warm=0)]
    line = json.dumps({"mode": args.mode, "rows": rows})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
