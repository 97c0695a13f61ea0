"""Throughput and time to convergence of the differential-evolution optimizer (magprop_amd.optimize), one GPU.

    python tools/opt_bench.py rate       generations/s and member evaluations/s, 1 and 4 populations per light curve
    python tools/opt_bench.py converge   wall time, nit and best lnprob of differential_evolution with its defaults
    python tools/opt_bench.py profile    a short run to profile (rocprofv3 --kernel-trace --stats -- python tools/opt_bench.py profile)

Light curves: the four synthetic sets and the 1 921-point Swift light curve of GRB 060614 (tests/golden).  Rate: popsize 15 x 6
= 90 members per population from a Latin hypercube over the prior box, 20 warm generations, then --gens timed generations with
tol = atol = 0 (no population converges: every generation evaluates every member); mp_optimizer_run returns when they are done.
Prints one JSON line; --out also writes it to a file.
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

from magprop_amd import _capi, engine, optimize, synth  # noqa: E402

SETS = ("Humped", "Classic", "Sloped", "Stuttering", "swift_060614")


def data(name):
    if name.startswith("swift"):
        g = np.load(os.path.join(ROOT, "tests", "golden", "golden_swift.npz"))
        return tuple(g[f"{name}_ds"])
    g = np.load(os.path.join(ROOT, "tests", "golden", "golden_synth.npz"))
    return g[f"{name}_x"], g[f"{name}_y"], g[f"{name}_yerr"]


def rate(name, n_pops, gens, warm=20, members=90, seed=0):
    h = _capi.Handle(_capi.cfg_synth(), engine.grid(None))
    h.set_prior(synth.PRIOR_LOWER, synth.PRIOR_UPPER, synth.LOG_MASK)
    h.set_dataset(0, *data(name))
    L = _capi.lib()
    lo, hi = synth.PRIOR_LOWER.copy(), synth.PRIOR_UPPER.copy()
    dp = C.POINTER(C.c_double)
    o = L.mp_optimizer_create(h._h, members, n_pops, 6, None, C.c_uint64(seed), _capi.DE_BEST1BIN, 0.5, 1.0, 0.7, 0.0, 0.0,
                              lo.ctypes.data_as(dp), hi.ctypes.data_as(dp), 0)
    assert o, _capi.last_error()
    try:
        rng = np.random.default_rng(seed)
        pop = np.ascontiguousarray(np.concatenate([optimize.latin_hypercube(rng, members, lo, hi) for _ in range(n_pops)]))
        _capi.check(L.mp_optimizer_set_population(o, pop.ctypes.data_as(dp)), "set_population")
        _capi.check(L.mp_optimizer_run(o, warm, None), "run")
        t0 = time.perf_counter()
        _capi.check(L.mp_optimizer_run(o, gens, None), "run")
        dt = time.perf_counter() - t0
    finally:
        L.mp_optimizer_destroy(o)
        h.close()
    return {"set": name, "n_pops": n_pops, "members": members * n_pops, "generations": gens, "seconds": round(dt, 4),
            "ms_per_generation": round(1e3 * dt / gens, 4), "generations_per_s": round(gens / dt, 1),
            "member_evals_per_s": round(gens * members * n_pops / dt, 0)}


def converge(name, n_starts, seed=1):
    x, y, yerr = data(name)
    optimize.differential_evolution(x, y, yerr, maxiter=2, seed=seed)          # (library load, first launches)
    t0 = time.perf_counter()
    res = optimize.differential_evolution(x, y, yerr, n_starts=n_starts, seed=seed)
    dt = time.perf_counter() - t0
    res = res if isinstance(res, list) else [res]
    return {"set": name, "n_starts": n_starts, "seconds": round(dt, 3), "nit": [r.nit for r in res], "nfev": [r.nfev for r in res],
            "success": [bool(r.success) for r in res], "best_lnprob": [round(r.lnprob, 4) for r in res]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("rate", "converge", "profile"))
    ap.add_argument("--gens", type=int, default=200)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.mode == "rate":
        rows = [rate(s, n, args.gens) for s in SETS for n in (1, 4)]
    elif args.mode == "converge":
        rows = [converge(s, n) for s in SETS for n in (1, 4)]
    else:
        rows = [rate("Humped", 4, 100), rate("swift_060614", 1, 100)]
    line = json.dumps({"mode": args.mode, "rows": rows})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
