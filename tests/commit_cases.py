"""Named cases for the sampler's deciding kernels (magprop_amd/csrc/mp_kernels.hip: stretch_step_commit_kernel,
stretch_apply_kernel, stretch_swap_kernel, order_kernel) and for the index draws pick / pick_skip / pick_skip2 (mp_math.hpp).
numpy only, seeded and deterministic, one launch each, the smallest shapes at which each path exists.  A case holds the inputs
of one launch; `expected(case)` runs the restatement (tests/commit_restated.py) on copies whose output buffers are filled with
canaries, as the GPU test fills them.  tests/test_commit_cases_cpu.py checks that every case has the property its docstring
claims; tests/test_gpu_commit_kernels.py and tests/test_gpu_math.py run the same lists through the kernels (libmp_probe_commit.so,
libmp_probe.so), so that no case exists on one side only."""
import zlib
from collections import namedtuple
from functools import lru_cache

import numpy as np

import commit_restated as cr

MAX_NDIM, SPEC_EXTRA = 9, cr.SPEC_EXTRA
ACC0 = 2 ** 40                      # n_accepted starts at 2^40 + i: a 32-bit counter would show
CANARY, ICANARY = np.nan, -777      # what every output buffer holds before the launch
INF, NAN = np.inf, np.nan
INT32_MAX = 2 ** 31 - 1

# bad_cap: None = no log (bad_log = nullptr); chain_rows: 0 = no chain
CommitCase = namedtuple("CommitCase", "name doc n_walkers n_ensembles ndim pos lnprob perm spec betas chain_rows chain_row bad_cap twin")
ApplyCase = namedtuple("ApplyCase", "name doc n_walkers n_ensembles ndim pos lnprob perm upd half ens_order chain_rows chain_row bad_cap")
SwapCase = namedtuple("SwapCase", "name doc n_walkers n_ensembles ndim pos lnprob perm betas n_temps seed step chain_rows chain_row swaps0")
OrderCase = namedtuple("OrderCase", "name doc n_obs ds_id")


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def perms(kind, n_ens, n, rng):
    """perm[n_ens][n]: identity, reversal, or a seeded permutation per ensemble."""
    if kind == "identity":
        return np.tile(np.arange(n, dtype=np.int32), (n_ens, 1))
    if kind == "reversal":
        return np.tile(np.arange(n, dtype=np.int32)[::-1], (n_ens, 1)).copy()
    return np.stack([rng.permutation(n).astype(np.int32) for _ in range(n_ens)])


def state_of(c):
    """The state of the case as it goes into the launch: n_accepted = 2^40 + i, chain buffers full of canaries."""
    nt = c.n_walkers * c.n_ensembles
    s = {"pos": c.pos.copy(), "lnprob": c.lnprob.copy(), "n_accepted": ACC0 + np.arange(nt, dtype=np.int64), "chain": None, "chain_lnp": None}
    if c.chain_rows:
        s["chain"] = np.full((c.chain_rows, nt, c.ndim), CANARY)
        s["chain_lnp"] = np.full((c.chain_rows, nt), CANARY)
    return s


def bad_buffers(c):
    """(bad_log[bad_cap + 1][ndim] with its guard row, or None; bad_count[1]) full of canaries / zero."""
    log = None if c.bad_cap is None else np.full((c.bad_cap + 1, c.ndim), CANARY)
    return log, np.zeros(1, dtype=np.uint32)


# ================================================================ commit
def _partner(kind, n_half, n_slots, rng):
    slot = np.arange(n_slots) % n_half
    return {"zero": np.zeros(n_slots), "last": np.full(n_slots, n_half - 1.0), "own": slot.astype(float),
            "seeded": rng.integers(0, n_half, n_slots).astype(float)}[kind]


def _spec_for(decide, betas, n_half, ndim, rng, partner, status=None):
    """Outcome rows [3][slots][ndim + 6] whose decisions are decide[3][slots] by a margin of at least 0.25: h, ln u and the
    lnprob before the move are drawn, the proposal's lnprob is put on the wanted side of the threshold."""
    n_slots = decide.shape[1]
    spec = np.empty((3, n_slots, ndim + SPEC_EXTRA))
    spec[:, :, :ndim] = rng.standard_normal((3, n_slots, ndim)) + 10.0 * np.arange(1, 4)[:, None, None]   # the block shows in the value
    h = 0.5 * rng.standard_normal((3, n_slots))
    lnu = np.log(rng.random((3, n_slots)))
    old = -3.0 * rng.random((3, n_slots))
    b = np.ones(n_slots) if betas is None else np.repeat(np.asarray(betas, dtype=float), n_half)
    margin = (0.25 + rng.random((3, n_slots))) * np.where(decide, 1.0, -1.0)
    spec[:, :, ndim] = old + ((lnu - h) + margin) / b
    spec[:, :, ndim + 1] = rng.integers(0, 5, (3, n_slots)) if status is None else status
    spec[:, :, ndim + 2], spec[:, :, ndim + 3], spec[:, :, ndim + 4] = h, lnu, old
    spec[:, :, ndim + 5] = partner
    return spec


def _wanted_decisions(n_ens, n_half, rng):
    """First half: a seeded decision per slot in ensemble 0 and the opposite one in every other ensemble, so that a partner
    looked up without the ensemble term is seen with the wrong outcome.  Second half: candidates 1 and 2 disagree for two slots
    in three."""
    first = rng.random(n_half) < 0.5
    d0 = np.concatenate([first if e == 0 else ~first for e in range(n_ens)])
    d1 = rng.random(n_ens * n_half) < 0.5
    d2 = np.where(np.arange(n_ens * n_half) % 3 == 0, d1, ~d1)
    return np.stack([d0, d1, d2])


def _state_values(nt, ndim, rng):
    """(pos, lnprob) of a state: values no outcome row holds (rows carry their own lnprob before the move)."""
    return rng.standard_normal((nt, ndim)) - 50.0, -100.0 - rng.random(nt)


def commit_generic(name, doc, nw, ne, ndim, perm_kind, partner_kind, chain, bad, betas=None, twin=None, data_name=None):
    """chain = (rows, row) or None; bad = "fewer" / "equal" / "more" / "zero" / None against the number of logged proposals."""
    rng = _rng(data_name or name)
    n_half, nt = nw // 2, nw * ne
    perm = perms(perm_kind, ne, nw, rng)
    spec = _spec_for(_wanted_decisions(ne, n_half, rng), betas, n_half, ndim, rng, _partner(partner_kind, n_half, n_half * ne, rng))
    pos, lnprob = _state_values(nt, ndim, rng)
    rows, row = chain or (0, 0)
    c = CommitCase(name, doc, nw, ne, ndim, pos, lnprob, perm, spec, None if betas is None else np.asarray(betas, dtype=float), rows, row, 0, twin)
    n_failed = len(cr.commit(state_of(c), perm, spec, c.betas, row)[2])
    cap = {"fewer": n_failed + 3, "equal": n_failed, "more": n_failed // 2, "zero": 0, None: None}[bad]
    return c._replace(bad_cap=cap)


def commit_ties(name, doc, betas):
    """Integers (even ones, so that beta = 0.5 stays exact): ln u equal to the difference (the strict > rejects), the double
    below it (accepts) and the double above it (rejects), in turn over the rows."""
    rng = _rng(name)
    ne = 1 if betas is None else len(betas)
    nw, ndim = 20, 3
    n_half, nt = nw // 2, nw * ne
    n_slots = n_half * ne
    spec = np.empty((3, n_slots, ndim + SPEC_EXTRA))
    spec[:, :, :ndim] = rng.standard_normal((3, n_slots, ndim)) + 10.0 * np.arange(1, 4)[:, None, None]
    h = 2.0 * rng.integers(-3, 4, (3, n_slots))
    lnp = 2.0 * rng.integers(-20, -5, (3, n_slots))
    old = lnp + 2.0 * rng.integers(1, 6, (3, n_slots)) + h         # (h + lnp) - old in -10 .. -2
    b = np.ones(n_slots) if betas is None else np.repeat(np.asarray(betas, dtype=float), n_half)
    diff = (h + b * lnp) - b * old
    kind = (np.arange(3 * n_slots).reshape(3, n_slots) + np.arange(3)[:, None]) % 3
    lnu = np.where(kind == 0, diff, np.where(kind == 1, np.nextafter(diff, -INF), np.nextafter(diff, INF)))
    spec[:, :, ndim], spec[:, :, ndim + 1], spec[:, :, ndim + 2], spec[:, :, ndim + 3], spec[:, :, ndim + 4] = lnp, 0.0, h, lnu, old
    spec[:, :, ndim + 5] = _partner("seeded", n_half, n_slots, rng)
    pos, lnprob = _state_values(nt, ndim, rng)
    return CommitCase(name, doc, nw, ne, ndim, pos, lnprob, perms("seeded", ne, nw, rng), spec,
                      None if betas is None else np.asarray(betas, dtype=float), 3, 1, 8, None)


# (proposal's lnprob, lnprob before the move, ln u, h): every non-finite corner of the decision
NONFINITE_ROWS = ((-INF, -1.0, -0.5, 0.0), (INF, -1.0, -0.5, 0.0), (NAN, -1.0, -0.5, 0.0), (-INF, -INF, -0.5, 0.0),
                  (-1.0, -INF, -0.5, 0.0), (-1.0, INF, -0.5, 0.0), (INF, INF, -0.5, 0.0), (-2.0, -1.0, -INF, 0.0),
                  (-INF, -1.0, -INF, 0.0), (-1.0, -2.0, -0.5, NAN), (-1.0, -2.0, -0.5, 0.0), (-2.0, -1.0, -0.1, 0.0))


def commit_nonfinite(name, doc, betas):
    """The rows of NONFINITE_ROWS in turn over the blocks and slots, each block starting at another one."""
    rng = _rng(name)
    ne = 1 if betas is None else len(betas)
    nw, ndim = 26, 2
    n_half, nt = nw // 2, nw * ne
    n_slots = n_half * ne
    spec = np.empty((3, n_slots, ndim + SPEC_EXTRA))
    spec[:, :, :ndim] = rng.standard_normal((3, n_slots, ndim)) + 10.0 * np.arange(1, 4)[:, None, None]
    for blk in range(3):
        for gs in range(n_slots):
            lnp, old, lnu, h = NONFINITE_ROWS[(gs + 5 * blk) % len(NONFINITE_ROWS)]
            spec[blk, gs, ndim:] = lnp, float((gs + blk) % 5), h, lnu, old, (gs * 7 + blk) % n_half
    pos, lnprob = _state_values(nt, ndim, rng)
    return CommitCase(name, doc, nw, ne, ndim, pos, lnprob, perms("seeded", ne, nw, rng), spec,
                      None if betas is None else np.asarray(betas, dtype=float), 3, 2, 4 * n_slots, None)


def commit_ladder_zero():
    """Ladder (1, 0.5, 0): proposals of lnprob -inf in every ensemble with h = 0 and ln u = -1.  At beta = 0 the product 0 x -inf
    is NaN and rejects; a kernel that skipped the product there would accept (0 > -1)."""
    name = "commit-ladder-zero-minus-inf"
    rng = _rng(name)
    betas, nw, ndim = (1.0, 0.5, 0.0), 12, 3
    ne, n_half = 3, 6
    n_slots = n_half * ne
    dec = _wanted_decisions(ne, n_half, rng)
    # (a finite row at beta = 0 decides by h > ln u whatever its lnprob: give those rows a beta of 1 for the construction)
    spec = _spec_for(dec, (1.0, 0.5, 1.0), n_half, ndim, rng, _partner("seeded", n_half, n_slots, rng), status=0.0)
    minus = (np.arange(3 * n_slots).reshape(3, n_slots) % 2) == 0
    spec[:, :, ndim][minus] = -INF
    spec[:, :, ndim + 2][minus] = 0.0
    spec[:, :, ndim + 3][minus] = -1.0
    pos, lnprob = _state_values(nw * ne, ndim, rng)
    return CommitCase(name, commit_ladder_zero.__doc__, nw, ne, ndim, pos, lnprob, perms("seeded", ne, nw, rng), spec,
                      np.asarray(betas), 3, 0, 4, None)


def commit_beta_per_ensemble():
    """Three ensembles with the same rows, the same split and betas (1, 0.5, 0.125): h = 0, lnprob differences in (-6, 0) and ln u
    in (-3, 0), so the decision of a slot differs from ensemble to ensemble.  Catches beta[0] for beta[w_ens]."""
    name = "commit-beta-per-ensemble"
    rng = _rng(name)
    betas, nw, ndim, ne = (1.0, 0.5, 0.125), 40, 3, 3
    n_half = nw // 2
    one = np.empty((3, n_half, ndim + SPEC_EXTRA))
    one[:, :, :ndim] = rng.standard_normal((3, n_half, ndim))
    old = -3.0 * rng.random((3, n_half))
    one[:, :, ndim] = old - 6.0 * rng.random((3, n_half))
    one[:, :, ndim + 1], one[:, :, ndim + 2], one[:, :, ndim + 3], one[:, :, ndim + 4] = 0.0, 0.0, -3.0 * rng.random((3, n_half)), old
    one[:, :, ndim + 5] = rng.integers(0, n_half, n_half)
    spec = np.concatenate([one] * ne, axis=1)
    pos, lnprob = _state_values(nw * ne, ndim, rng)
    perm = np.tile(rng.permutation(nw).astype(np.int32), (ne, 1))
    return CommitCase(name, commit_beta_per_ensemble.__doc__, nw, ne, ndim, pos, lnprob, perm, spec, np.asarray(betas), 0, 0, None, None)


@lru_cache(maxsize=None)
def commit_cases():
    g = commit_generic
    return (
        g("commit-2", "One walker per half (2 threads), ndim 1, partner slot 0 = n_half - 1 = its own; no chain; a log larger than the "
          "failures.", 2, 1, 1, "identity", "zero", None, "fewer"),
        g("commit-254-reversal", "254 threads of one block, the split reversed, every partner in the last slot, chain row 0 of 3; "
          "fewer failures than the log holds.", 254, 1, 6, "reversal", "last", (3, 0), "fewer"),
        g("commit-256-16-ensembles", "Exactly one block, 16 ensembles of 16, ndim 9, every partner in the walker's own slot number, "
          "the last chain row of 3; as many failures as the log holds.", 16, 16, 9, "seeded", "own", (3, 2), "equal"),
        g("commit-258-3-ensembles", "Two threads in a second block, 3 ensembles of 86, seeded partners; more failures than the log "
          "holds: every logged row is a failing one, the count exact, the guard row untouched.  Catches u1 / u2 exchanged and "
          "gs_j without the ensemble term.", 86, 3, 6, "seeded", "seeded", (3, 2), "more", twin="commit-258-3-ensembles-betas-1"),
        g("commit-258-3-ensembles-betas-1", "The same launch through the TEMPERED build with betas all 1: every output equals the "
          "untempered build's to the bit.", 86, 3, 6, "seeded", "seeded", (3, 2), "more", betas=(1.0, 1.0, 1.0),
          twin="commit-258-3-ensembles", data_name="commit-258-3-ensembles"),
        g("commit-514", "Three blocks, ndim 1, no chain, bad_cap = 0: the count runs, nothing is logged.", 514, 1, 1, "seeded",
          "seeded", None, "zero"),
        g("commit-30-no-log", "3 ensembles of 10, bad_log = nullptr: nothing is counted either.", 10, 3, 6, "seeded", "seeded", (3, 0), None),
        g("commit-tempered-ladder", "3 ensembles of 34 on the ladder (1, 0.5, 0.125), the TEMPERED build with every margin scaled by "
          "the ensemble's beta.", 34, 3, 6, "seeded", "seeded", (3, 1), "fewer", betas=(1.0, 0.5, 0.125)),
        commit_ties("commit-ties", "Exact ties of the untempered test: integers with ln u equal to the difference reject, one ulp "
                    "below accepts, one ulp above rejects.  Catches >= for >.", None),
        commit_ties("commit-ties-tempered", "The same ties through the TEMPERED build on betas (1, 0.5, 0): even integers keep beta x "
                    "lnprob exact.", (1.0, 0.5, 0.0)),
        commit_nonfinite("commit-nonfinite", "lnprob of the proposal -inf, +inf, NaN; of the walker -inf (-inf - -inf = NaN rejects) "
                         "and +inf; ln u = -inf against a finite and a -inf proposal; h NaN.", None),
        commit_nonfinite("commit-nonfinite-tempered", "The same rows through the TEMPERED build on betas (1, 0.5, 0): 0 x inf = NaN "
                         "rejects.", (1.0, 0.5, 0.0)),
        commit_ladder_zero(),
        commit_beta_per_ensemble(),
    )


@lru_cache(maxsize=None)
def commit_expected(name):
    c = by_name(name)
    s = state_of(c)
    decided, chosen, failed = cr.commit(s, c.perm, c.spec, c.betas, c.chain_row)
    return s, decided, chosen, failed


# ================================================================ apply
def apply_case(name, doc, nw, ne, ndim, half, order, chain, bad, perm_kind="seeded"):
    """order: None (ens_order = 0) or the ensemble at every position."""
    rng = _rng(name)
    n_half, nt = nw // 2, nw * ne
    n_slots = n_half * ne
    upd = np.empty((n_slots, ndim + 3))
    upd[:, :ndim] = rng.standard_normal((n_slots, ndim)) + 10.0 * (1 + np.arange(n_slots) // n_half)[:, None]   # the position shows
    upd[:, ndim] = -rng.random(n_slots) - np.arange(n_slots) // n_half
    upd[:, ndim + 1] = rng.integers(0, 2, n_slots)
    upd[:, ndim + 2] = rng.integers(0, 5, n_slots)
    pos, lnprob = _state_values(nt, ndim, rng)
    rows, row = chain or (0, 0)
    c = ApplyCase(name, doc, nw, ne, ndim, pos, lnprob, perms(perm_kind, ne, nw, rng), upd, half,
                  0 if order is None else cr.encode_order(order), rows, row, 0)
    n_failed = len(cr.apply(state_of(c), c.perm, upd, half, c.ens_order, row)[2])
    cap = {"fewer": n_failed + 3, "equal": n_failed, "more": n_failed // 2, "zero": 0, None: None}[bad]
    return c._replace(bad_cap=cap)


def order16():
    """A seeded permutation of 16 ensembles with ensemble 15 at position 15 (the field at a shift of 60) and ensemble 0 away
    from position 0."""
    p = list(_rng("order16").permutation(15))
    if p[0] == 0:
        p[0], p[1] = p[1], p[0]
    return [int(e) for e in p] + [15]


@lru_cache(maxsize=None)
def apply_cases():
    a = apply_case
    return (
        a("apply-255-reversed", "255 slots (one short of a block), 3 ensembles of 170 launched in reversed order, half 0, the last "
          "chain row; accepted flags mixed, statuses 0 to 4 beside either flag; fewer failures than the log holds.",
          170, 3, 6, 0, [2, 1, 0], (3, 2), "fewer"),
        a("apply-256-permutation-of-16", "256 slots (one block), 16 ensembles in a seeded order with ensemble 15 at position 15 (a "
          "shift by 60) and ensemble 0 not at position 0, half 1, ndim 9; more failures than the log holds.",
          32, 16, 9, 1, order16(), (3, 0), "more"),
        a("apply-257-identity", "257 slots (one thread in a second block), one ensemble, ens_order = 0, half 1, ndim 1, no chain, "
          "no log.", 514, 1, 1, 1, None, None, None),
        a("apply-two-swapped", "Two ensembles of 6 launched as (1, 0), every row different: a decode that is off by one field "
          "commits the rows to the other ensemble.  Half 0; as many failures as the log holds.", 6, 2, 3, 0, [1, 0], (3, 1), "equal"),
        a("apply-three-identity-half-1", "3 ensembles of 10, ens_order = 0, half 1, reversed split; bad_cap = 0.", 10, 3, 6, 1, None,
          (3, 1), "zero", perm_kind="reversal"),
        a("apply-three-rotated-half-0", "3 ensembles of 10 launched as (1, 2, 0), half 0.", 10, 3, 6, 0, [1, 2, 0], (3, 0), "fewer"),
    )


@lru_cache(maxsize=None)
def apply_expected(name):
    c = by_name(name)
    s = state_of(c)
    decided, touched, failed = cr.apply(s, c.perm, c.upd, c.half, c.ens_order, c.chain_row)
    return s, decided, touched, failed


# ================================================================ swap
SEED = 0xC0FFEE1234567           # bits above 32
LAST_STEP = 2 ** 32 - 1
BIG = 1.0e6                      # a lnprob difference no ln u (>= -36.8 for u > 0) stands against


def swap_case(name, doc, nw, n_temps, n_groups, ndim, step, betas=None, chain=None, edit=None, seed=SEED):
    """Slot i of a group (walker perm[e][i] of each of its ensembles), on a falling ladder: i % 4 == 1 swaps at no pair (lnprob
    falls by 1e6 per temperature), i % 4 == 0 at every pair (the same, but the hottest walker holds +1e6, which travels down: each
    pair is accepted only because the one before was), the others as the draw has it.  betas: per temperature or per ensemble;
    edit(lnprob_by_slot[n_ens][nw], betas, perm, rng) changes the lnprob of the slots in place."""
    rng = _rng(name)
    ne = n_temps * n_groups
    nt = nw * ne
    perm = perms("seeded", ne, nw, rng)
    by_slot = -3.0 * rng.random((ne, nw))
    t = (np.arange(ne) % n_temps)[:, None]
    i = np.arange(nw)[None, :]
    by_slot = np.where(i % 4 == 0, np.where(t == n_temps - 1, BIG, -BIG * t), by_slot)
    by_slot = np.where(i % 4 == 1, -BIG * t, by_slot)
    b = np.asarray(0.5 ** np.arange(n_temps) if betas is None else betas, dtype=float)
    if len(b) == n_temps:
        b = np.tile(b, n_groups)      # (else: one beta per ensemble as given)
    if edit is not None:
        edit(by_slot, b, perm, rng)
    lnprob = np.empty(nt)
    for e in range(ne):
        lnprob[e * nw + perm[e]] = by_slot[e]
    pos = rng.standard_normal((nt, ndim)) + 10.0 * (np.arange(nt) // nw)[:, None]
    rows, row = chain or (0, 0)
    swaps0 = (1000 * (1 + np.arange(n_groups))[:, None] + np.arange(n_temps - 1)[None, :]).astype(np.int64)
    return SwapCase(name, doc, nw, ne, ndim, pos, lnprob, perm, b, n_temps, seed, step, rows, row, swaps0)


def _swap_nonfinite(by_slot, b, perm, rng):
    pairs = ((-INF, 0.0), (0.0, -INF), (INF, 0.0), (0.0, INF), (NAN, 0.0), (0.0, NAN), (-INF, -INF), (INF, INF), (-INF, INF), (INF, -INF))
    for g in range(by_slot.shape[0] // 2):
        for i in range(by_slot.shape[1]):
            by_slot[2 * g, i], by_slot[2 * g + 1, i] = pairs[i % len(pairs)]


def _swap_tie(by_slot, b, perm, rng):
    """dbeta = 1, L_cold = 0 and L_hot = ln u of the pair's own draw (the strict < rejects) for even slots, the double above it
    (accepts) for odd ones."""
    nw = by_slot.shape[1]
    for i in range(nw):
        lnu = cr.swap_lnu(SEED, 7, int(perm[0, i]))
        by_slot[0, i] = 0.0
        by_slot[1, i] = lnu if i % 2 == 0 else np.nextafter(lnu, INF)


@lru_cache(maxsize=None)
def swap_cases():
    s = swap_case
    return (
        s("swap-2-walkers", "Two walkers, two temperatures, ndim 1, step 0, no chain: two lanes of one wavefront.", 2, 2, 1, 1, 0),
        s("swap-62-three-groups", "62 walkers (a partial wavefront), 3 temperatures, 3 groups, ndim 9, the last step 2^32 - 1, chain: "
          "counts per group and per pair, no group leaks into another.", 62, 3, 3, 9, LAST_STEP, chain=(3, 2)),
        s("swap-64-eight-temperatures", "64 walkers (one full wavefront), 8 temperatures: a slot's swap at pair t decides its pair t - "
          "1 (the huge lnprob of the hottest walker travels down all 7 pairs).  Catches ascending t.", 64, 8, 1, 1, 5, chain=(3, 0)),
        s("swap-66-three-groups", "66 walkers (a second wavefront of 2 lanes: the ballot and one atomic per wavefront), 2 "
          "temperatures, 3 groups.", 66, 2, 3, 3, 0, chain=(3, 1)),
        s("swap-256", "256 walkers: every thread of the block once, 3 temperatures.", 256, 3, 1, 1, LAST_STEP),
        s("swap-258", "258 walkers: two threads run the loop a second time.", 258, 2, 1, 9, 0, chain=(3, 1)),
        s("swap-600-three-groups", "600 walkers (three turns of the loop, the last one 88 lanes), 3 temperatures, 3 groups.",
          600, 3, 3, 3, 11, chain=(3, 2)),
        s("swap-equal-betas", "Equal betas (dbeta = 0): 0 x finite = 0 > ln u always swaps.", 16, 3, 1, 3, 3, betas=(0.5, 0.5, 0.5), chain=(3, 0)),
        s("swap-reversed-ladder", "A ladder that rises with t (dbeta < 0).", 16, 3, 1, 3, 3, betas=(0.125, 0.5, 1.0), chain=(3, 0)),
        s("swap-hot-end-zero", "beta = 0 at the hot end.", 16, 3, 1, 3, 3, betas=(1.0, 0.25, 0.0), chain=(3, 0)),
        s("swap-nonfinite", "lnprob -inf, +inf and NaN on either side and on both (-inf - -inf = NaN rejects, a finite dbeta times +inf "
          "accepts); a second group with equal betas (0 x inf = NaN rejects).", 20, 2, 2, 2, 3, betas=(1.0, 0.5, 0.5, 0.5), chain=(3, 1),
          edit=_swap_nonfinite),
        s("swap-tie", "dbeta = 1, L_cold = 0 and L_hot = ln u of the pair's draw rejects, the double above accepts.  Catches <= for <.",
          12, 2, 1, 2, 7, betas=(1.0, 0.0), chain=(3, 1), edit=_swap_tie),
    )


@lru_cache(maxsize=None)
def swap_expected(name):
    c = by_name(name)
    s = state_of(c)
    counts, swapped, taken = cr.swap(s, c.perm, c.betas, c.n_temps, c.seed, c.step, c.chain_row)
    return s, counts, swapped, taken


# ================================================================ order
N_OBS = (0, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 1944)     # either side of every class threshold
BAD_IDS = (-1, len(N_OBS), INT32_MAX)


def _order_case(name, doc, n, n_obs=N_OBS, ids=None):
    rng = _rng(name)
    if ids is None:
        ids = rng.integers(0, len(n_obs), n)
        if n >= 6:
            ids[rng.choice(n, 3, replace=False)] = BAD_IDS
    return OrderCase(name, doc, np.asarray(n_obs, dtype=np.int32), np.asarray(ids, dtype=np.int32))


@lru_cache(maxsize=None)
def order_cases():
    o = _order_case
    return (
        o("order-1", "One walker.", 1),
        o("order-6-one-per-class", "Six walkers, one per class, listed shortest first.", 6, ids=[0, 2, 4, 6, 8, 10]),
        o("order-12-every-length", "Every length of the list once: 64 / 65 up to 1 024 / 1 025 fall either side of a threshold.  "
          "Catches a threshold off by one.", 12, ids=list(range(12))),
        o("order-bad-ids", "Ids -1, n_ds and INT32_MAX among valid ones count as length 0.", 9, ids=[11, -1, 9, len(N_OBS), 5, INT32_MAX, 0, 11, 3]),
        o("order-1023", "One short of the 1 024-thread stride.", 1023),
        o("order-1024", "Every thread once.", 1024),
        o("order-1025", "One thread twice.", 1025),
        o("order-5000", "Five turns of the stride.", 5000),
        o("order-all-in-one-class", "1 025 walkers on the longest light curve: one counter takes every atomic.", 1025, ids=[11] * 1025),
        o("order-no-datasets", "n_ds = 0 (ds = nullptr): every walker in the last class.", 100, n_obs=(), ids=list(range(-50, 50))),
    )


# ================================================================ pick
PICK_MAX_M, PICK_ALL_PAIRS_M = 70, 12
U_LAST = 1.0 - 2.0 ** -53


def boundary_us(m):
    """u around every j / m' of the reduced ranges m' = m, m - 1, m - 2 (those that exist): the double below, at and above the
    rounded quotient, kept inside [0, 1); and 0 and 1 - 2^-53."""
    us = {0.0, U_LAST}
    for mr in (m, m - 1, m - 2):
        for j in range(1, mr):
            b = j / mr
            us.update((np.nextafter(b, 0.0), b, np.nextafter(b, 1.0)))
    return sorted(us)


@lru_cache(maxsize=None)
def pick_cases():
    """(u, m, c0, c1) as four float64 arrays, padded with (0, 1, 0, 0) to a multiple of 64: m = 1 .. 70, the values of
    boundary_us(m), every c0 != c1 for m <= 12 and four seeded pairs above (m = 1: c0 = c1 = 0)."""
    rng = _rng("pick")
    rows = []
    for m in range(1, PICK_MAX_M + 1):
        if m == 1:
            pairs = [(0, 0)]
        elif m <= PICK_ALL_PAIRS_M:
            pairs = [(a, b) for a in range(m) for b in range(m) if a != b]
        else:
            pairs = [tuple(rng.choice(m, 2, replace=False)) for _ in range(4)]
        rows += [(u, m, a, b) for u in boundary_us(m) for a, b in pairs]
    rows += [(0.0, 1, 0, 0)] * (-len(rows) % 64)
    a = np.array(rows, dtype=np.float64)
    return tuple(np.ascontiguousarray(a[:, k]) for k in range(4))


@lru_cache(maxsize=None)
def pick_expected():
    """[n][3]: moves_restated.pick / pick_skip / pick_skip2 per element, -1 where m is below the draw's smallest size."""
    from moves_restated import pick, pick_skip, pick_skip2
    u, m, c0, c1 = pick_cases()
    out = np.full((len(u), 3), -1.0)
    for i in range(len(u)):
        mm, a, b = int(m[i]), int(c0[i]), int(c1[i])
        out[i, 0] = pick(float(u[i]), mm)
        if mm >= 2:
            out[i, 1] = pick_skip(float(u[i]), mm, a)
        if mm >= 3:
            out[i, 2] = pick_skip2(float(u[i]), mm, a, b)
    return out


def all_cases():
    return commit_cases() + apply_cases() + swap_cases() + order_cases()


def by_name(name):
    return next(c for c in all_cases() if c.name == name)
