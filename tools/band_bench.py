"""Timing of the posterior-predictive band (mp_model_band) on one GPU.

Synchronised calls after warm-up (the entry returns when the band is in host memory) at S = 1 024, 4 096, 16 384 rows,
components {Ltot} and {Ltot, Lprop, Ldip}, three quantiles; and the host alternative at S = 4 096: one
lnprob_batch(want_ltot=True) call for the curves, then np.nanquantile over them.  Rows: the Humped truth with a 0.02
spread in sampler coordinates (a burnt-in chain's rows).  Prints one JSON line; --out also writes it to a file.

    python tools/band_bench.py --reps 5 --out profiles/r06_band_bench.json
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from magprop_amd import _capi, engine, synth  # noqa: E402

TRUTH = np.array([1.0, 5.0, -3.0, 2.0, -1.0, 0.0])
Q = (0.025, 0.5, 0.975)


def timed(fn, reps):
    fn()                                                # warm-up (workspace growth, code objects)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(np.min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="1024,4096,16384")
    ap.add_argument("--host-size", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    g = np.load(os.path.join(ROOT, "tests", "golden", "golden_synth.npz"))
    h = _capi.Handle(_capi.cfg_synth(), engine.grid(None), 0)
    h.set_dataset(0, g["Humped_x"], g["Humped_y"], g["Humped_yerr"])
    h.set_prior(synth.PRIOR_LOWER, synth.PRIOR_UPPER, synth.LOG_MASK)
    rng = np.random.default_rng(0)
    res = {"what": "mp_model_band", "q": list(Q), "n_grid": int(h.tgrid.size), "rows": "Humped truth + 0.02 N(0,1)", "band": []}
    for S in (int(s) for s in args.sizes.split(",")):
        P = TRUTH + 0.02 * rng.standard_normal((S, 6))
        for comps in (("Ltot",), ("Ltot", "Lprop", "Ldip")):
            med, best = timed(lambda: h.model_band(P, Q, comps), args.reps)
            used = h.model_band(P, Q, comps)[2]
            res["band"].append({"S": S, "components": list(comps), "ms_median": med * 1e3, "ms_min": best * 1e3, "n_used": used})
        if S == args.host_size:
            def host():
                _, lt = h.lnprob_batch(P, ds_id=0, want_ltot=True)
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore", RuntimeWarning)
                    return np.nanquantile(lt, Q, axis=0)
            med, best = timed(host, max(1, args.reps // 2))
            res["host_alternative"] = {"S": S, "components": ["Ltot"], "ms_median": med * 1e3, "ms_min": best * 1e3}
            dev = [r for r in res["band"] if r["S"] == S and r["components"] == ["Ltot"]][0]
            res["host_alternative"]["speedup_of_band"] = med / (dev["ms_median"] * 1e-3)
    h.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
