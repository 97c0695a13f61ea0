"""numpy restatement of the ensemble sampler's step (magprop_amd/csrc mp_sampler_run): the two-way split, the two half-steps
with the step's move drawn from the table (tests/moves_restated.py: stretch, DE, snooker; tests/kde_restated.py: KDE), the
decision against beta and, for a tempered sampler, the swap sweep.  Test infrastructure: the one step loop that the GPU tests
compare the device chains with and that the CPU tests draw their statistics from; oracle/stretch_oracle.run, which restates
the stretch move alone, is its independent check (tests/test_moves_cpu.py).  With evaluate= the log-probabilities of a half-step come
from ONE call for the proposals of all slots of all ensembles, as the device evaluates them in one launch: the hook of the GPU
tests that hold the chains on the real posterior to mp_lnprob_batch (tests/test_gpu_sampler_posterior.py)."""
from typing import NamedTuple

import numpy as np

from kde_restated import KDE, bandwidth, fit, normals_batch, propose_kde
from moves_restated import draw_move, propose, resolve
from oracle.stretch_oracle import gaussian_lnprob, philox4x32_10, split, u01

M32 = 0xFFFFFFFF
MP_STATUS_OK, MP_STATUS_FLAG, MP_STATUS_NONFINITE, MP_STATUS_PRIOR = 0, 1, 2, 3      # include/magprop_amd.h


class Run(NamedTuple):
    chain: np.ndarray        # (n_steps, n_total, ndim), the rows after the step's swaps
    lnp: np.ndarray          # (n_steps, n_total)
    acc: np.ndarray          # (n_total,) accepted proposals per walker (added to acc= where given)
    drawn: np.ndarray        # (n_steps,) index of the step's move in the table
    accepted: np.ndarray     # (n_steps, n_total) the walker's proposal of that step was accepted
    swaps: np.ndarray        # (n_groups, n_temps - 1) accepted swaps of this call; (0, 0) without a swap sweep
    # with evaluate= only (None otherwise):
    bad: np.ndarray = None       # (n_bad, ndim) evaluated proposals of status MP_STATUS_FLAG / MP_STATUS_NONFINITE: the fbad log
    counts: dict = None          # per ensemble: "accepted" / "rejected" evaluated proposals; "outside": proposals outside box=;
                                 # "unevaluated": NaN proposals of the KDE move; "swap_refused": (n_groups, n_temps - 1)


def run(pos, n_steps, seed, table, lnprob_fn=gaussian_lnprob, n_ensembles=1, step0=0, lnp=None, acc=None, betas=None,
        n_temps=0, zero_hastings=False, evaluate=None, box=None, kde_device=None):
    """table = [(kind, weight, p0, p1)] over MP_MOVE_* as mp_sampler_set_moves takes it.  betas[e] per ensemble: the decision
    (h + b lnp(q)) - b lnp(x) > ln u (b = 1 untempered, which rounds as (h + lnp(q)) - lnp(x) does); with n_temps > 1 also one
    swap sweep per group of n_temps ensembles after every step, hottest pair first, slot i of temperature t - 1 against slot i
    of temperature t (slot = position in the step's split), accepted if ln u < (beta_{t-1} - beta_t)(L_hot - L_cold), u keyed
    (seed; step, 2, cold walker, 0).  pos, and lnp / acc where given (to continue a run from step0), are advanced in place.
    evaluate(rows, walkers) -> (lnprob, status) replaces lnprob_fn (without lnp= the start is one call too): per half-step the proposals of all
    slots of all ensembles are built first -- the other half stands still during a half-step, so they are the proposals of the
    loop below --, ONE call evaluates them (walkers: the global index of each row's walker), then the decisions follow in the
    order of the loop below.  A NaN proposal of the KDE move (covariance not positive definite) is not evaluated: lnprob 0,
    its NaN Hastings term rejects it, as in stretch_kernel.  A proposal outside box = (lower, upper) is evaluated like any other
    (the library answers -inf, MP_STATUS_PRIOR) and counted.  kde_device = (wavefronts of the launch's workgroup, an object with
    the device's log, sqrt, cos and sin), with evaluate= only: the KDE proposal in the kernel's own order of sums and through the
    device's functions (kde_restated.fit, normals_batch), which makes it the kernel's bit for bit."""
    n_total, ndim = pos.shape
    n = n_total // n_ensembles
    half_n = n // 2
    n_comp = n - half_n
    moves, cum = resolve(table, ndim)   # (KDE entries pass through as they are)
    tempered = betas is not None and n_temps > 1
    if lnp is None:
        lnp = np.array([lnprob_fn(p) for p in pos]) if evaluate is None else np.array(evaluate(pos.copy(), np.arange(n_total))[0])
    if acc is None:
        acc = np.zeros(n_total, dtype=np.int64)
    chain = np.empty((n_steps, n_total, ndim))
    chain_lnp = np.empty((n_steps, n_total))
    accepted = np.zeros((n_steps, n_total), dtype=bool)
    drawn = np.empty(n_steps, dtype=np.int64)
    swaps = np.zeros((n_ensembles // n_temps, n_temps - 1) if tempered else (0, 0), dtype=np.int64)
    refused = np.zeros_like(swaps)
    bad = []
    counts = {k: np.zeros(n_ensembles, dtype=np.int64) for k in ("accepted", "rejected", "outside", "unevaluated")}
    for s in range(n_steps):
        step = step0 + s
        m = drawn[s] = draw_move(seed, step, cum)
        kde = table[m][0] == KDE
        perms = [split(seed, step, e, n) for e in range(n_ensembles)]
        for half in range(2):
            if evaluate is not None:
                _half_step(pos, lnp, acc, accepted[s], table[m], moves[m], perms, half, n, betas, seed, step, zero_hastings,
                           evaluate, box, bad, counts, kde_device)
                continue
            for e in range(n_ensembles):
                base, perm = e * n, perms[e]
                b = 1.0 if betas is None else float(betas[e])
                comp = [base + perm[(1 - half) * half_n + c] for c in range(n_comp)]
                L = fit(pos[comp], bandwidth(table[m][2], n_comp, ndim))[1] if kde else None
                for slot in range(half_n):
                    k = base + perm[half * half_n + slot]
                    if kde:
                        q, h, logu = propose_kde(pos, k, comp, seed, step, half, L, zero_hastings)
                    else:
                        q, h, logu = propose(moves[m], pos, k, comp, seed, step, half, zero_hastings)
                    new = lnprob_fn(q)
                    with np.errstate(invalid="ignore"):
                        accept = (h + b * new) - b * lnp[k] > logu
                    if accept:
                        pos[k] = q
                        lnp[k] = new
                        acc[k] += 1
                        accepted[s, k] = True
        if tempered:
            for e0 in range(0, n_ensembles, n_temps):
                for t in range(n_temps - 1, 0, -1):
                    ec, eh = e0 + t - 1, e0 + t
                    dbeta = float(betas[ec]) - float(betas[eh])
                    for i in range(n):
                        kc, kh = ec * n + perms[ec][i], eh * n + perms[eh][i]
                        r = philox4x32_10(seed & M32, seed >> 32, step, 2, kc, 0)
                        with np.errstate(divide="ignore"):
                            lnu = np.log(u01(r[0], r[1]))
                        if lnu < dbeta * (lnp[kh] - lnp[kc]):
                            pos[[kc, kh]] = pos[[kh, kc]]
                            lnp[kc], lnp[kh] = lnp[kh], lnp[kc]
                            swaps[e0 // n_temps, t - 1] += 1
                        else:
                            refused[e0 // n_temps, t - 1] += 1
        chain[s] = pos
        chain_lnp[s] = lnp
    if evaluate is None:
        return Run(chain, chain_lnp, acc, drawn, accepted, swaps)
    counts["swap_refused"] = refused
    return Run(chain, chain_lnp, acc, drawn, accepted, swaps, np.array(bad).reshape(-1, ndim), counts)


def _half_step(pos, lnp, acc, accepted, entry, move, perms, half, n, betas, seed, step, zero_hastings, evaluate, box, bad, counts,
               kde_device=None):
    """One half-step of run() with evaluate=: proposals of every slot of every ensemble, one evaluate call, the decisions."""
    half_n = n // 2
    n_comp = n - half_n
    kde = entry[0] == KDE
    ks, props = [], []
    waves, libm = kde_device if kde and kde_device else (0, None)
    nrm = None
    if libm is not None:      # the normals of every walker of the half, through the device's functions, in one batch
        every = [e * n + perm[half * half_n + slot] for e, perm in enumerate(perms) for slot in range(half_n)]
        nrm = normals_batch(seed, step, half, every, pos.shape[1], libm)
    for e, perm in enumerate(perms):
        base = e * n
        comp = [base + perm[(1 - half) * half_n + c] for c in range(n_comp)]
        L = None
        if kde:
            L = fit(pos[comp], bandwidth(entry[2], n_comp, pos.shape[1]), waves, *(() if libm is None else (libm.sqrt,)))[1]
        for slot in range(half_n):
            k = base + perm[half * half_n + slot]
            props.append(propose_kde(pos, k, comp, seed, step, half, L, zero_hastings, None if nrm is None else nrm[len(ks)])
                         if kde else propose(move, pos, k, comp, seed, step, half, zero_hastings))
            ks.append(k)
    ks = np.array(ks)
    rows = np.array([p[0] for p in props])
    live = ~np.isnan(rows[:, 0])
    new, status = np.zeros(len(ks)), np.full(len(ks), MP_STATUS_OK, dtype=np.int64)
    if live.any():
        new[live], status[live] = evaluate(rows[live], ks[live])
    if box is not None:
        with np.errstate(invalid="ignore"):
            out = live & np.any((rows < box[0]) | (rows > box[1]), axis=1)
        np.add.at(counts["outside"], ks[out] // n, 1)
    np.add.at(counts["unevaluated"], ks[~live] // n, 1)
    for i, k in enumerate(ks):
        q, h, logu = props[i]
        b = 1.0 if betas is None else float(betas[k // n])
        with np.errstate(invalid="ignore"):
            accept = (h + b * new[i]) - b * lnp[k] > logu
        if status[i] in (MP_STATUS_FLAG, MP_STATUS_NONFINITE):
            bad.append(q.copy())
        if live[i]:
            counts["accepted" if accept else "rejected"][k // n] += 1
        if accept:
            pos[k] = q
            lnp[k] = new[i]
            acc[k] += 1
            accepted[k] = True
