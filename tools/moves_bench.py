"""Throughput and mixing of the sampler's proposal moves (EnsembleSampler(..., moves=...)) on Humped, one GPU.

    python tools/moves_bench.py rate [--sizes 64,512,1024,4096]   walker-steps/s and acceptance of every configuration
    python tools/moves_bench.py tau                               integrated autocorrelation time per move, 512 walkers x 6 000 steps
    python tools/moves_bench.py profile --walkers 1024 [--move kde|slice|walk|gaussian]  a short DE (KDE, ...) run to profile (rocprofv3 --kernel-trace --stats -- ...)
    python tools/moves_bench.py normal [--sizes 512,1024]         the walk and Gaussian moves: rate, acceptance and tau at --walkers, ms per step next to DE's half-steps

Configurations: stretch with its default launch (a whole step per launch where it fits), stretch with whole_step=False (the
launches DE and snooker run: two half-step launches per step), DE, snooker, the mixture 0.8 DE + 0.2 snooker, KDE, the
mixture 0.8 KDE + 0.2 DE, and the slice move (its rows also carry the evaluations per walker and step, the failed slices and
mu; its warm-up covers its tuning steps where --warm is at least 100), the walk move over all of the other half and over
subsets of 3, the mixture 0.5 walk + 0.5 DE, and the Gaussian move with the covariance 2.38^2 / ndim x that of a DE burn-in
(GaussianMove.from_samples, 200 tuning steps, which --warm covers; its rows also carry sigma) alone and as 0.8 KDE + 0.2 Gaussian.
Rate: every sampler starts at the Humped truth (1e-4 ball), runs --warm steps unstored, then --steps timed steps unstored
(mp_sampler_run returns when its steps are done).  Tau: --tau-steps stored steps, the first quarter discarded; effective samples
per second = walker-steps/s of the rate run at the same size / mean tau over the six parameters.
Prints one JSON line; --out also writes it to a file.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from magprop_amd import DEMove, DESnookerMove, EnsembleSampler, GaussianMove, KDEMove, SliceMove, WalkMove  # noqa: E402

TRUTH = [1.0, 5.0, -3.0, 2.0, -1.0, 0.0]     # Humped, sampler coordinates
CONFIGS = {
    "stretch": dict(),
    "stretch_half_steps": dict(whole_step=False),
    "de": dict(moves=DEMove()),
    "snooker": dict(moves=DESnookerMove()),
    "de0.8_snooker0.2": dict(moves=[(DEMove(), 0.8), (DESnookerMove(), 0.2)]),
    "kde": dict(moves=KDEMove()),
    "kde0.8_de0.2": dict(moves=[(KDEMove(), 0.8), (DEMove(), 0.2)]),
    "slice": dict(moves=SliceMove()),
    "walk": dict(moves=WalkMove()),
    "walk_s3": dict(moves=WalkMove(s=3)),
    "walk0.5_de0.5": dict(moves=[(WalkMove(), 0.5), (DEMove(), 0.5)]),
}
NORMAL = ("de", "kde", "walk", "walk_s3", "walk0.5_de0.5", "gaussian", "kde0.8_gaussian0.2")   # the rows of `normal`


def gaussian_configs(nwalk):
    """The configurations with a GaussianMove: its covariance comes from the last 100 of 400 DE steps at this size."""
    x, y, yerr = data()
    s = EnsembleSampler(nwalk, 6, x, y, yerr, seed=3, moves=DEMove())
    s.run_mcmc(_start(nwalk, 2), 400)
    burn = s.get_chain()[300:].reshape(-1, 6)
    s.close()
    return {"gaussian": dict(moves=GaussianMove.from_samples(burn, tune=200)),
            "kde0.8_gaussian0.2": dict(moves=[(KDEMove(), 0.8), (GaussianMove.from_samples(burn, tune=200), 0.2)])}


def configs(nwalk, only=None):
    c = dict(CONFIGS)
    c.update(gaussian_configs(nwalk))
    return c if only is None else {k: c[k] for k in only}


def slice_row(s, walker_steps):
    """What the slice move adds to a row: evaluations per walker and step, failed slices per update, mu."""
    st = s.get_slice_stats()
    return {"evaluations_per_walker_step": float(st["neval"].sum()) / walker_steps,
            "expansions_per_walker_step": float(st["nexpand"].sum()) / walker_steps,
            "contractions_per_walker_step": float(st["ncontract"].sum()) / walker_steps,
            "failed_slice_fraction": float(st["nfail"].sum()) / walker_steps, "mu": [float(v) for v in st["mu"]]}


def data():
    g = np.load(os.path.join(ROOT, "tests", "golden", "golden_synth.npz"))
    return g["Humped_x"], g["Humped_y"], g["Humped_yerr"]


def _start(nwalk, seed):
    return np.array(TRUTH) + 1.0e-4 * np.random.default_rng(seed).standard_normal((nwalk, 6))


def rate_at(nwalk, warm, steps, only=None):
    x, y, yerr = data()
    rows = {}
    for name, kw in configs(nwalk, only).items():
        s = EnsembleSampler(nwalk, 6, x, y, yerr, seed=1, **kw)
        s.run_mcmc(_start(nwalk, 0), warm, store=False)
        a0 = s.get_last_sample()[2].copy()
        t0 = time.perf_counter()
        s.run_mcmc(None, steps, store=False)
        dt = time.perf_counter() - t0
        acc = (s.get_last_sample()[2] - a0) / steps
        nbad, _ = s.get_bad()
        rows[name] = {"ms_per_step": dt / steps * 1e3, "walker_steps_per_s": nwalk * steps / dt,
                      "acceptance": float(acc.mean()), "failed_proposal_fraction": nbad / (nwalk * (warm + steps))}
        if name == "slice":
            rows[name].update(slice_row(s, nwalk * (warm + steps)))
        if "gaussian" in name:
            rows[name]["sigma"] = [float(v) for v in s.get_gaussian_stats()["sigma"]]
        s.close()
    if only is not None:
        return rows
    base, half = rows["stretch"]["walker_steps_per_s"], rows["stretch_half_steps"]["walker_steps_per_s"]
    for r in rows.values():
        r["over_stretch_default"] = r["walker_steps_per_s"] / base
        r["over_stretch_half_steps"] = r["walker_steps_per_s"] / half
    return rows


def rate(args):
    out = {"what": "proposal moves, walker-steps/s on Humped near the truths", "warm": args.warm, "steps": args.steps, "sizes": {}}
    for n in [int(v) for v in args.sizes.split(",")]:
        out["sizes"][str(n)] = rate_at(n, args.warm, args.steps)
    # gate: DE and snooker at >= 0.85 x the stretch move on the same launches (whole_step=False)
    out["gate_min_over_half_steps"] = min(r[k]["over_stretch_half_steps"] for r in out["sizes"].values()
                                          for k in ("de", "snooker", "de0.8_snooker0.2"))
    # gate: KDE half-steps at >= 0.85 x the DE move's
    for r in out["sizes"].values():
        r["kde"]["over_de"] = r["kde"]["walker_steps_per_s"] / r["de"]["walker_steps_per_s"]
    out["gate_kde_min_over_de"] = min(r["kde"]["over_de"] for r in out["sizes"].values())
    return out


def tau(args, only=None):
    x, y, yerr = data()
    nwalk, n_steps = args.walkers, args.tau_steps
    rates = rate_at(nwalk, args.warm, args.steps, only)
    out = {"what": f"integrated autocorrelation time on Humped, {nwalk} walkers x {n_steps} steps from the truths, first quarter "
                   "discarded; effective samples/s = walker-steps/s / mean tau", "walkers": nwalk, "steps": n_steps, "moves": {}}
    for name, kw in configs(nwalk, only).items():
        if name == "stretch_half_steps":
            continue                                   # the chain of "stretch", bit for bit
        s = EnsembleSampler(nwalk, 6, x, y, yerr, seed=2, **kw)
        s.run_mcmc(_start(nwalk, 1), n_steps)
        chain = s.get_chain()[n_steps // 4:]
        from magprop_amd.mcmc_io import integrated_time
        t = integrated_time(chain, c=5.0, tol=50, quiet=True)
        r = rates[name]
        out["moves"][name] = {"tau": [float(v) for v in t], "tau_mean": float(np.mean(t)),
                              "acceptance": float(s.acceptance_fraction.mean()), "walker_steps_per_s": r["walker_steps_per_s"],
                              "effective_samples_per_s": r["walker_steps_per_s"] / float(np.mean(t)),
                              "median": [float(v) for v in np.median(chain.reshape(-1, 6), axis=0)],
                              "std": [float(v) for v in chain.reshape(-1, 6).std(axis=0)]}
        if name == "slice":
            out["moves"][name].update(slice_row(s, nwalk * n_steps))
        if "gaussian" in name:
            out["moves"][name]["sigma"] = [float(v) for v in s.get_gaussian_stats()["sigma"]]
        s.close()
    if only is None:
        ref = out["moves"]["stretch"]["effective_samples_per_s"]
        for r in out["moves"].values():
            r["ess_rate_over_stretch"] = r["effective_samples_per_s"] / ref
    return out


def normal(args):
    """The walk and Gaussian moves next to DE and KDE: rate, acceptance and tau at --walkers, and ms per step at --sizes next
    to the DE move's, whose two half-step launches are the launches these moves run."""
    out = tau(args, NORMAL)
    out["what"] = "walk and Gaussian moves on Humped: " + out["what"]
    out["ms_per_step"] = {}
    for n in [int(v) for v in args.sizes.split(",")]:
        rows = rate_at(n, args.warm, args.steps, NORMAL)
        out["ms_per_step"][str(n)] = {k: {"ms_per_step": r["ms_per_step"], "over_de": r["ms_per_step"] / rows["de"]["ms_per_step"],
                                          "acceptance": r["acceptance"]} for k, r in rows.items()}
    return out


def profile(args):
    x, y, yerr = data()
    mv = {"kde": KDEMove(), "slice": SliceMove(), "de": DEMove(), "walk": WalkMove(), "gaussian": GaussianMove(1.0e-4, tune=200)}[args.move]
    s = EnsembleSampler(args.walkers, 6, x, y, yerr, seed=1, moves=mv)
    s.run_mcmc(_start(args.walkers, 0), args.steps, store=False)
    s.close()
    return {"what": f"profiling run ({args.move})", "walkers": args.walkers, "steps": args.steps}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=("rate", "tau", "profile", "normal"))
    ap.add_argument("--sizes", default="64,512,1024,4096")
    ap.add_argument("--walkers", type=int, default=512)
    ap.add_argument("--warm", type=int, default=200)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--tau-steps", type=int, default=6000)
    ap.add_argument("--move", choices=("de", "kde", "slice", "walk", "gaussian"), default="de", help="profile: the move of the run")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {"rate": rate, "tau": tau, "profile": profile, "normal": normal}[args.mode](args)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
