"""Timing and evidence figures of parallel tempering (EnsembleSampler(..., betas=...)) on one GPU.

    python tools/pt_bench.py rate        walker-steps/s of 8 temperatures x 64 walkers against 512 untempered walkers on Humped
    python tools/pt_bench.py swap        a short tempered run to profile (rocprofv3 --kernel-trace --stats -- python ...)
    python tools/pt_bench.py evidence    lnZ +- dlnZ of the four synthetic datasets, two seeds each
    python tools/pt_bench.py hotfail     failed-proposal rate at the hottest temperature of the evidence ladders (--ev-beta-min)
    python tools/pt_bench.py adapt       walker-steps/s of 8 x 64 and 128 x 32 tempered walkers with the ladder adaptation off,
                                         adapting and frozen, and with the thermodynamic monitor on (medians of --rounds rounds
                                         that alternate the variants)
    python tools/pt_bench.py ladder      lnZ, dlnZ and the pair acceptances of fixed geometric and adapted ladders on the
                                         brute-force case (Humped, yerr x 10) at T = 16, 32, 64, 128, four seeds each

Rate: both samplers start at the Humped truth (1e-4 ball), run --warm steps unstored (the hot chains spread over the prior
box), then --steps timed steps unstored (synchronised: mp_sampler_run returns when the steps are done).  Prints one JSON line;
--out also writes it to a file.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from magprop_amd import EnsembleSampler, synth, tempering  # noqa: E402

TRUTHS = {"Humped": [1.0, 5.0, -3.0, 2.0, -1.0, 0.0], "Classic": [1.0, 5.0, -3.0, 3.0, -1.0, 0.0],
          "Sloped": [1.0, 1.0, -3.0, 2.0, 1.0, 1.0], "Stuttering": [1.0, 5.0, -5.0, 2.0, -1.0, 2.0]}


def data(name):
    g = np.load(os.path.join(ROOT, "tests", "golden", "golden_synth.npz"))
    return g[name + "_x"], g[name + "_y"], g[name + "_yerr"]


def rate(args):
    x, y, yerr = data("Humped")
    rng = np.random.default_rng(0)
    out = {"what": "parallel tempering, walker-steps/s on Humped", "warm": args.warm, "steps": args.steps}
    for label, nwalk, betas in (("tempered 8 x 64", 64, tempering.geometric_ladder(8, args.beta_min)),
                                ("untempered 512", 512, None)):
        s = EnsembleSampler(nwalk, 6, x, y, yerr, seed=1, betas=betas)
        s.run_mcmc(np.array(TRUTHS["Humped"]) + 1.0e-4 * rng.standard_normal((s.ntotal, 6)), args.warm, store=False)
        t0 = time.perf_counter()
        s.run_mcmc(None, args.steps, store=False)
        dt = time.perf_counter() - t0
        row = {"walkers": s.ntotal, "ms_per_step": dt / args.steps * 1e3, "walker_steps_per_s": s.ntotal * args.steps / dt,
               "acceptance": float(s.acceptance_fraction.mean())}
        if betas is not None:
            row["betas"] = [float(b) for b in betas]
            row["swap_acceptance"] = [float(v) for v in s.swap_acceptance_fraction.ravel()]
        nbad, _ = s.get_bad()
        row["failed_proposal_fraction"] = nbad / (s.ntotal * (args.warm + args.steps))
        out[label] = row
        s.close()
    out["tempered_over_untempered"] = out["tempered 8 x 64"]["walker_steps_per_s"] / out["untempered 512"]["walker_steps_per_s"]
    return out


def swap(args):
    x, y, yerr = data("Humped")
    s = EnsembleSampler(64, 6, x, y, yerr, seed=1, betas=tempering.geometric_ladder(8, args.beta_min))
    s.run_mcmc(np.array(TRUTHS["Humped"]) + 1.0e-4 * np.random.default_rng(0).standard_normal((s.ntotal, 6)), args.steps,
               store=False)
    return {"what": "profiling run", "walkers": s.ntotal, "steps": args.steps}


def evidence(args):
    out = {"what": "log evidence of the synthetic datasets", "n_temps": args.temps, "beta_min": args.ev_beta_min,
           "walkers_per_temp": args.walkers, "steps": args.ev_steps, "discard": args.ev_steps // 4, "runs": []}
    betas = tempering.geometric_ladder(args.temps, args.ev_beta_min)
    lo, hi = synth.PRIOR_LOWER, synth.PRIOR_UPPER
    for name in TRUTHS:
        x, y, yerr = data(name)
        for seed in (1, 2):
            rng = np.random.default_rng(seed)
            s = EnsembleSampler(args.walkers, 6, x, y, yerr, seed=seed, betas=betas)
            start = lo + (hi - lo) * rng.random((4 * s.ntotal, 6))
            start = start[np.isfinite(s.handle.lnprob_batch(start, ds_id=0))][:s.ntotal]
            t0 = time.perf_counter()
            s.run_mcmc(start, args.ev_steps)
            t_run = time.perf_counter() - t0
            lnz, dlnz = s.log_evidence(discard=args.ev_steps // 4)
            out["runs"].append({"dataset": name, "seed": seed, "lnZ": lnz, "dlnZ": dlnz, "run_s": t_run,
                                "cold_max_lnprob": float(np.max(s.get_log_prob(temp=0)))})
            s.close()
    return out


def hotfail(args):
    """The fbad log does not say which temperature a failed proposal came from, so the rate at the hottest temperature is
    measured on a ladder whose temperatures are all that hot but the first (which must be 1): 1, then 7 temperatures within
    1 % of --ev-beta-min.  The beta = 1 ensemble starts at the truth and stays there (its rate, from an untempered run
    alongside, is subtracted)."""
    x, y, yerr = data("Humped")
    lo, hi = synth.PRIOR_LOWER, synth.PRIOR_UPPER
    betas = np.concatenate([[1.0], args.ev_beta_min * np.linspace(1.01, 1.0, 7)])
    rng = np.random.default_rng(5)
    s = EnsembleSampler(args.walkers, 6, x, y, yerr, seed=5, betas=betas)
    start = lo + (hi - lo) * rng.random((16 * s.ntotal, 6))
    start = start[np.isfinite(s.handle.lnprob_batch(start, ds_id=0))][:s.ntotal]
    start[:args.walkers] = np.array(TRUTHS["Humped"]) + 1.0e-4 * rng.standard_normal((args.walkers, 6))
    s.run_mcmc(start, args.ev_steps, store=False)
    nbad, _ = s.get_bad()
    c = EnsembleSampler(args.walkers, 6, x, y, yerr, seed=5)
    c.run_mcmc(start[:args.walkers], args.ev_steps, store=False)
    nbad_cold, _ = c.get_bad()
    n_hot = 7 * args.walkers * args.ev_steps
    return {"what": "failed proposals at the hottest temperature", "betas": [float(b) for b in betas], "steps": args.ev_steps,
            "walkers_per_temp": args.walkers, "failed_all": nbad, "failed_cold_alone": nbad_cold,
            "hot_rate": (nbad - nbad_cold) / n_hot, "drain_window_rate": 1.0 / 32}


def adapt(args):
    """Every variant is a sampler of its own, warmed --warm steps; a round times --steps unstored steps of each in turn.  The
    adapting sampler adapts for as long as the benchmark runs, the frozen one froze inside its warm-up."""
    x, y, yerr = data("Humped")
    out = {"what": "ladder adaptation, walker-steps/s on Humped", "warm": args.warm, "steps": args.steps, "rounds": args.rounds,
           "shapes": {}}
    total = args.warm + args.rounds * args.steps
    for label, n_temps, nwalk in (("8 x 64", 8, 64), ("128 x 32", 128, 32)):
        betas = tempering.geometric_ladder(n_temps, args.beta_min)
        variants = {"off": (None, False), "adapting": ({"steps": 2 * total}, False), "frozen": ({"steps": args.warm // 2}, False),
                    "off + thermo monitor": (None, True)}
        rng = np.random.default_rng(0)
        start = np.array(TRUTHS["Humped"]) + 1.0e-4 * rng.standard_normal((n_temps * nwalk, 6))
        samplers, times = {}, {k: [] for k in variants}
        for name, (ad, thermo) in variants.items():
            s = EnsembleSampler(nwalk, 6, x, y, yerr, seed=1, betas=betas, adapt_ladder=ad)
            if thermo:
                s.monitor_thermo()
            s.run_mcmc(start, args.warm, store=False)
            samplers[name] = s
        for _ in range(args.rounds):
            for name, s in samplers.items():
                t0 = time.perf_counter()
                s.run_mcmc(None, args.steps, store=False)
                times[name].append(time.perf_counter() - t0)
        row = {}
        for name, s in samplers.items():
            ms = np.array(times[name]) / args.steps * 1e3
            row[name] = {"ms_per_step_median": float(np.median(ms)), "ms_per_step_min": float(ms.min()),
                         "ms_per_step_max": float(ms.max()),
                         "walker_steps_per_s": s.ntotal / (float(np.median(ms)) * 1e-3), "ladder_updates": s.ladder_updates[0]}
            s.close()
        out["shapes"][label] = row
    return out


def ladder(args):
    """Equal step counts: --ev-steps steps, the first half adapting (lag 50, time 5) where the ladder adapts; both evidences are
    taken over the second half.  Reported, not asserted: dlnZ holds no statistical error."""
    x, y, yerr = data("Humped")
    yerr = yerr * 10.0
    lo, hi = synth.PRIOR_LOWER, synth.PRIOR_UPPER
    half = args.ev_steps // 2
    out = {"what": "fixed geometric against adapted ladders on the brute-force case (Humped, yerr x 10; brute force -5.5046)",
           "beta_min": 1e-12, "walkers_per_temp": args.walkers, "steps": 2 * half, "adapt": {"steps": half, "lag": 50.0, "time": 5.0},
           "runs": []}
    for n_temps in (16, 32, 64, 128):
        betas = tempering.geometric_ladder(n_temps, 1e-12)
        for seed in (1, 2, 3, 4):
            for ad in (None, dict(out["adapt"])):
                rng = np.random.default_rng(seed)
                s = EnsembleSampler(args.walkers, 6, x, y, yerr, seed=seed, betas=betas, adapt_ladder=ad)
                start = lo + (hi - lo) * rng.random((4 * s.ntotal, 6))
                start = start[np.isfinite(s.handle.lnprob_batch(start, ds_id=0))][:s.ntotal]
                s.monitor_thermo(discard=half)
                s.run_mcmc(start, half, store=False)
                before = s.swap_acceptance_fraction * half
                s.run_mcmc(None, half, store=False)
                acc = (s.swap_acceptance_fraction * 2 * half - before)[0] / half
                lnz, dlnz = s.log_evidence(device=True, prior_draws=args.prior_draws)
                out["runs"].append({"n_temps": n_temps, "seed": seed, "ladder": "adapted" if ad else "fixed", "lnZ": lnz, "dlnZ": dlnz,
                                    "acc_min": float(acc.min()), "acc_max": float(acc.max()),
                                    "swap_spread": float(tempering.swap_spread(acc)), "dropped": int(s.ladder_updates[1][0])})
                s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("rate", "swap", "evidence", "hotfail", "adapt", "ladder"))
    ap.add_argument("--warm", type=int, default=300)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--beta-min", type=float, default=1e-3)
    ap.add_argument("--temps", type=int, default=128)
    ap.add_argument("--walkers", type=int, default=32)
    ap.add_argument("--ev-beta-min", type=float, default=1e-14)
    ap.add_argument("--ev-steps", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--prior-draws", type=int, default=2 ** 20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {"rate": rate, "swap": swap, "evidence": evidence, "hotfail": hotfail, "adapt": adapt, "ladder": ladder}[args.mode](args)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
