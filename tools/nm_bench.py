"""Time per iteration and time to the stop rule of the Nelder-Mead simplex search (magprop_amd.nelder_mead, mp_simplex_*), one GPU.

    python tools/nm_bench.py [--iters 200] [--out profiles/r19_nm_bench.json]

iteration  n_simplex = 1, 64 and 512 simplexes on Humped, ndim 6 (10 candidates each), scipy's default simplex around points near
           the truth, xatol = fatol = 0 (nothing stops: every iteration evaluates every candidate).  Per size, in the same call
           and on the same handle: ms per iteration of mp_simplex_run; ms per call of mp_lnprob_batch_dev for a batch of the
           same n_simplex x 10 rows (the candidates of the last iteration), enqueued back to back and synchronised once -- the
           expectation is one such launch plus a decide kernel of a few microseconds per iteration; and ms per iteration of the
           same scheme driven from the host, one mp_lnprob_batch call per iteration with the decisions in numpy.
polish     differential_evolution(maxiter=20) on the four synthetic sets with and without polish=True: wall time of both, the
           polish's nit / nfev / outcomes, the gain in lnprob and the distance to the truths before and after.
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

TYPES = ("Humped", "Classic", "Sloped", "Stuttering")
TRUTHS = {"Humped": [1.0, 5.0, -3.0, 2.0, -1.0, 0.0], "Classic": [1.0, 5.0, -3.0, 3.0, -1.0, 0.0],
          "Sloped": [1.0, 1.0, -3.0, 2.0, 1.0, 1.0], "Stuttering": [1.0, 5.0, -5.0, 2.0, -1.0, 2.0]}     # synth_mcmc.py:16-21


def data(name):
    g = np.load(os.path.join(ROOT, "tests", "golden", "golden_synth.npz"))
    return g[f"{name}_x"], g[f"{name}_y"], g[f"{name}_yerr"]


def host_iteration(h, sim, lnp, lo, hi):
    """One iteration of every simplex with the candidates evaluated by one mp_lnprob_batch call and the decisions in numpy
    (vectorised over the simplexes; the scheme of include/magprop_amd.h with the standard coefficients)."""
    n, nv, N = sim.shape
    xbar = sim[:, :N].sum(axis=1) / N
    worst, best = sim[:, N], sim[:, 0]
    cand = np.empty((n, N + 4, N))
    cand[:, 0], cand[:, 1], cand[:, 2], cand[:, 3] = 2 * xbar - worst, 3 * xbar - 2 * worst, 1.5 * xbar - 0.5 * worst, 0.5 * xbar + 0.5 * worst
    cand[:, 4:] = best[:, None] + 0.5 * (sim[:, 1:] - best[:, None])
    cand = np.clip(cand, lo, hi)
    fc = -np.nan_to_num(h.lnprob_batch(cand.reshape(-1, N), ds_id=0), nan=-np.inf).reshape(n, N + 4)
    f = -lnp
    fr, fe, fo, fi = fc[:, 0], fc[:, 1], fc[:, 2], fc[:, 3]
    take = np.where(fr < f[:, 0], np.where(fe < fr, 1, 0), np.where(fr < f[:, N - 1], 0, np.where(
        fr < f[:, N], np.where(fo <= fr, 2, -1), np.where(fi < f[:, N], 3, -1))))
    k = np.arange(n)
    shrink = take < 0
    sim[k, N], f[k, N] = cand[k, np.maximum(take, 0)], fc[k, np.maximum(take, 0)]
    sim[shrink, 1:], f[shrink, 1:] = cand[shrink, 4:], fc[shrink, 4:]
    order = np.argsort(f, axis=1, kind="stable")
    return np.take_along_axis(sim, order[:, :, None], axis=1), -np.take_along_axis(f, order, axis=1)


def iteration(n_simplex, iters, warm=20, seed=0):
    import torch
    N = 6
    h = _capi.Handle(_capi.cfg_synth(), engine.grid(None))
    h.set_prior(synth.PRIOR_LOWER, synth.PRIOR_UPPER, synth.LOG_MASK)
    h.set_dataset(0, *data("Humped"))
    L = _capi.lib()
    lo, hi = synth.PRIOR_LOWER.copy(), synth.PRIOR_UPPER.copy()
    rng = np.random.default_rng(seed)
    sim0 = np.stack([optimize.default_simplex(np.array(TRUTHS["Humped"]) + 0.05 * rng.standard_normal(N)) for _ in range(n_simplex)])
    sim0 = np.ascontiguousarray(np.clip(sim0, lo, hi))
    s = L.mp_simplex_create(h._h, n_simplex, N, None, 1.0, 2.0, 0.5, 0.5, 0.0, 0.0, _capi.ptr(lo), _capi.ptr(hi), 0)
    assert s, _capi.last_error()
    try:
        _capi.check(L.mp_simplex_set_vertices(s, _capi.ptr(sim0)), "set_vertices")
        _capi.check(L.mp_simplex_run(s, warm, None), "run")
        t0 = time.perf_counter()
        _capi.check(L.mp_simplex_run(s, iters, None), "run")
        dt = time.perf_counter() - t0
        st = optimize.get_simplex_state(L, s, n_simplex, N)
    finally:
        L.mp_simplex_destroy(s)
    # a batch of the launch's size on the same handle: the simplexes' vertices and three more rows each
    rows = np.concatenate([st["sim"], st["sim"][:, :3]], axis=1).reshape(-1, N)
    d_pars = torch.tensor(rows, device="cuda")
    d_out = torch.empty(len(rows), dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def batches(k):
        for _ in range(k):
            h.lnprob_batch_dev(d_pars.data_ptr(), len(rows), N, d_out.data_ptr(), stream=stream)
        torch.cuda.synchronize()

    batches(warm)
    t0 = time.perf_counter()
    batches(iters)
    dt_batch = time.perf_counter() - t0
    # the same scheme from the host
    sim, lnp = st["sim"].copy(), st["lnprob"].copy()
    for _ in range(5):
        sim, lnp = host_iteration(h, sim, lnp, lo, hi)
    host_iters = max(iters // 4, 10)
    t0 = time.perf_counter()
    for _ in range(host_iters):
        sim, lnp = host_iteration(h, sim, lnp, lo, hi)
    dt_host = time.perf_counter() - t0
    h.close()
    return {"n_simplex": n_simplex, "workgroups": 10 * n_simplex, "iterations": iters, "ms_per_iteration": round(1e3 * dt / iters, 4),
            "ms_per_lnprob_batch_dev": round(1e3 * dt_batch / iters, 4), "ratio_to_batch": round(dt / dt_batch, 3),
            "ms_per_host_iteration": round(1e3 * dt_host / host_iters, 4), "outcomes": st["outcomes"].sum(axis=0).tolist(),
            "nit": [int(st["nit"].min()), int(st["nit"].max())]}


def polish():
    ds = [data(t) for t in TYPES]
    optimize.differential_evolution(datasets=ds, seed=3, maxiter=2, polish=True)          # (library load, first launches)
    t0 = time.perf_counter()
    plain = optimize.differential_evolution(datasets=ds, seed=3, maxiter=20)
    t1 = time.perf_counter()
    res = optimize.differential_evolution(datasets=ds, seed=3, maxiter=20, polish=True)
    t2 = time.perf_counter()
    rows = [{"set": t, "lnprob_de": r0.lnprob, "lnprob_polished": r.lnprob, "gain": r.lnprob - r0.lnprob, "polish_nit": r.polish.nit,
             "polish_nfev": r.polish.nfev, "polish_success": bool(r.polish.success), "outcomes": r.polish.outcomes,
             "max_abs_x_minus_truth_de": float(np.abs(r0.x - TRUTHS[t]).max()),
             "max_abs_x_minus_truth_polished": float(np.abs(r.x - TRUTHS[t]).max())} for t, r0, r in zip(TYPES, plain, res)]
    return {"de_maxiter": 20, "seconds_de": round(t1 - t0, 4), "seconds_de_and_polish": round(t2 - t1, 4), "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out")
    args = ap.parse_args()
    line = json.dumps({"iteration": [iteration(n, args.iters) for n in (1, 64, 512)], "polish": polish()})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
