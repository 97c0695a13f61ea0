"""numpy restatement of the sampler's deciding operations (magprop_amd/csrc/mp_kernels.hip: stretch_step_commit_kernel,
stretch_apply_kernel, stretch_swap_kernel, order_kernel), written from the comments above the kernels and DESIGN.md: what a
whole step decides from its outcome rows, what a half-step commits from gathered rows, the swap sweep of a tempered step and
the launch order of a mixed-length batch.  Test infrastructure: tests/test_gpu_commit_kernels.py compares the kernels with it
bit for bit on the cases of tests/commit_cases.py; tests/test_commit_cases_cpu.py ties it to the step loop of
tests/sampler_restated.py.  Every product, sum and difference is a separately rounded float64 operation.

A state is the dict {pos[n_total][ndim], lnprob[n_total], n_accepted[n_total], chain[n_rows][n_total][ndim] or None,
chain_lnp[n_rows][n_total] or None}; every operation changes it in place.  perm[n_ensembles][n_walkers] is the step's split:
the first n_walkers / 2 entries of a row are the walkers of half 0 in slot order."""
import numpy as np

from oracle.stretch_oracle import philox4x32_10, u01

M32 = 0xFFFFFFFF
SPEC_EXTRA = 6            # columns behind the proposal: lnprob, status, Hastings term, ln u, lnprob before the move, partner's slot
FLAG, NONFINITE = 1, 2    # MP_STATUS_*: the model of the proposal failed; such a proposal goes to the log of failed proposals
ORDER_BOUNDS = (1024, 512, 256, 128, 64)   # classes 0 .. 4: more points than this; class 5: the rest


def accepted(h, lnp, lnp_old, lnu, beta=None):
    """emcee's test (h + lnp) - lnp_old > ln u; against beta x lnprob: (h + beta lnp) - beta lnp_old > ln u.  NaN rejects."""
    with np.errstate(invalid="ignore", over="ignore"):
        h, lnp, lnp_old, lnu = np.float64(h), np.float64(lnp), np.float64(lnp_old), np.float64(lnu)
        if beta is None:
            return bool((h + lnp) - lnp_old > lnu)
        b = np.float64(beta)
        return bool((h + b * lnp) - b * lnp_old > lnu)


def _commit_one(state, k, accept, q, lnp, lnp_old, status, chain_row, failed):
    """The commit of a decision on walker k: an accepted proposal becomes the state, the chain row is written from the state
    after that, a proposal whose model failed is logged whether or not it was accepted."""
    if accept:
        state["pos"][k] = q
        state["lnprob"][k] = lnp
        state["n_accepted"][k] += 1
    if state.get("chain") is not None:
        state["chain"][chain_row, k] = state["pos"][k]
        state["chain_lnp"][chain_row, k] = lnp if accept else lnp_old
    if status in (FLAG, NONFINITE):
        failed.append(np.array(q, dtype=np.float64))


def commit(state, perm, spec, betas=None, chain_row=0):
    """The decisions of a whole step from its outcome rows spec[3][slots][ndim + 6] (slots = n_half x n_ensembles, slot gs = e
    n_half + s): block 0 the proposals of the first half, blocks 1 and 2 the two candidates of every walker of the second half,
    with its partner of the first half where it stood (1) or at the partner's own proposal (2).  In index order: the first half
    decides, then every walker of the second half takes candidate 2 if its partner (the first-half slot named in candidate 1's
    row, of its own ensemble) was accepted, else candidate 1, and decides on it.  The walker's lnprob before the move is the
    row's.  Returns (decided[n_total] bool, chosen[n_total] block of the row decided on, failed: the logged proposals in index
    order)."""
    perm = np.asarray(perm)
    n_ens, n = perm.shape
    n_half = n // 2
    ndim = state["pos"].shape[1]
    n_slots = n_half * n_ens
    spec = np.asarray(spec).reshape(3, n_slots, ndim + SPEC_EXTRA)
    decided = np.zeros(n_ens * n, dtype=bool)
    chosen = np.full(n_ens * n, -1, dtype=np.int64)
    failed = []

    def acc(u, e):
        return accepted(u[ndim + 2], u[ndim], u[ndim + 4], u[ndim + 3], None if betas is None else betas[e])
    moved0 = [acc(spec[0, gs], gs // n_half) for gs in range(n_slots)]
    for half in range(2):
        for gs in range(n_slots):
            e, slot = divmod(gs, n_half)
            k = e * n + int(perm[e, half * n_half + slot])
            block = 0
            if half == 1:
                partner = int(spec[1, gs, ndim + 5])
                block = 2 if moved0[e * n_half + partner] else 1
            u = spec[block, gs]
            assert chosen[k] < 0, "a walker decided twice"
            chosen[k] = block
            decided[k] = acc(u, e)
            _commit_one(state, k, decided[k], u[:ndim], u[ndim], u[ndim + 4], int(u[ndim + 1]), chain_row, failed)
    return decided, chosen, failed


def decode_order(ens_order, n_ens):
    """Ensemble at every position of a half-step launch: four bits per position, 0 = the ensembles as they are numbered."""
    if not ens_order:
        return list(range(n_ens))
    return [(int(ens_order) >> (4 * p)) & 15 for p in range(n_ens)]


def encode_order(order):
    return sum(int(e) << (4 * p) for p, e in enumerate(order))


def apply(state, perm, upd, half, ens_order=0, chain_row=0):
    """The commit of one half-step from gathered rows upd[slots][ndim + 3] = (proposal, lnprob, accepted 0/1, status): row gs
    is slot gs % n_half of the ensemble at position gs // n_half of the launch order.  The lnprob before the move is the state's.
    Returns (decided[n_total], touched[n_total], failed)."""
    perm = np.asarray(perm)
    n_ens, n = perm.shape
    n_half = n // 2
    ndim = state["pos"].shape[1]
    upd = np.asarray(upd).reshape(n_half * n_ens, ndim + 3)
    order = decode_order(ens_order, n_ens)
    decided = np.zeros(n_ens * n, dtype=bool)
    touched = np.zeros(n_ens * n, dtype=bool)
    failed = []
    for gs in range(n_half * n_ens):
        e, slot = order[gs // n_half], gs % n_half
        k = e * n + int(perm[e, half * n_half + slot])
        u = upd[gs]
        assert not touched[k], "a walker committed twice"
        touched[k] = True
        decided[k] = u[ndim + 1] != 0.0
        _commit_one(state, k, decided[k], u[:ndim], u[ndim], state["lnprob"][k].copy(), int(u[ndim + 2]), chain_row, failed)
    return decided, touched, failed


def swap_lnu(seed, step, cold_walker):
    r = philox4x32_10(seed & M32, seed >> 32, step & M32, 2, cold_walker, 0)
    with np.errstate(divide="ignore"):
        return np.log(np.float64(u01(r[0], r[1])))


def swap(state, perm, betas, n_temps, seed, step, chain_row=0, hottest_first=True):
    """The swap sweep of a tempered step: ensemble e is temperature e % n_temps of group e // n_temps.  Per slot i (walker
    perm[e][i] of every ensemble e of the group) the neighbouring pairs t - 1, t from the hottest down, each pair seeing the
    outcome of the one before: accept if ln u < (beta[t - 1] - beta[t]) (L_hot - L_cold), u keyed (seed; step, 2, cold walker, 0).
    An accepted swap exchanges position and lnprob of the two walkers and rewrites their entries of the chain row; n_accepted
    stays.  Returns (counts[n_groups][n_temps - 1] of this sweep, swapped[n_total]: took part in an accepted swap,
    taken[n_groups][n_walkers][n_temps - 1]: slot i of the group swapped at pair t - 1, t).
    hottest_first=False runs the pairs in the other order (no kernel does: the CPU test shows with it that the order matters)."""
    perm = np.asarray(perm)
    n_ens, n = perm.shape
    pos, lnp = state["pos"], state["lnprob"]
    counts = np.zeros((n_ens // n_temps, n_temps - 1), dtype=np.int64)
    swapped = np.zeros(n_ens * n, dtype=bool)
    taken = np.zeros((n_ens // n_temps, n, n_temps - 1), dtype=bool)
    pairs = range(n_temps - 1, 0, -1) if hottest_first else range(1, n_temps)
    for g in range(n_ens // n_temps):
        for i in range(n):
            for t in pairs:
                ec, eh = g * n_temps + t - 1, g * n_temps + t
                kc, kh = ec * n + int(perm[ec, i]), eh * n + int(perm[eh, i])
                with np.errstate(invalid="ignore", over="ignore"):
                    dbeta = np.float64(betas[ec]) - np.float64(betas[eh])
                    ok = bool(swap_lnu(seed, step, kc) < dbeta * (lnp[kh] - lnp[kc]))
                if not ok:
                    continue
                pos[[kc, kh]] = pos[[kh, kc]]
                lnp[[kc, kh]] = lnp[[kh, kc]]
                counts[g, t - 1] += 1
                taken[g, i, t - 1] = True
                swapped[kc] = swapped[kh] = True
                if state.get("chain") is not None:
                    for k in (kc, kh):
                        state["chain"][chain_row, k] = pos[k]
                        state["chain_lnp"][chain_row, k] = lnp[k]
    return counts, swapped, taken


def order(n_obs, ds_id):
    """Launch order of a mixed-length batch, longest light curve first: the class of every walker (0: more than 1 024 points,
    1: more than 512, ... 4: more than 64, 5: the rest; a dataset id that names no light curve counts as length 0) and the class
    counts.  The order inside a class is unspecified."""
    n_obs = np.asarray(n_obs, dtype=np.int64)
    cls = np.empty(len(ds_id), dtype=np.int64)
    for i, d in enumerate(np.asarray(ds_id, dtype=np.int64)):
        length = int(n_obs[d]) if 0 <= d < len(n_obs) else 0
        cls[i] = next((c for c, bound in enumerate(ORDER_BOUNDS) if length > bound), len(ORDER_BOUNDS))
    return cls, np.bincount(cls, minlength=len(ORDER_BOUNDS) + 1)
