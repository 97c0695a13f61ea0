"""CPU checks of the restatement of the sampler's deciding operations (tests/commit_restated.py) and of the named cases of
tests/commit_cases.py: structural properties (every walker decided once, accepted walkers hold their row, a sweep conserves what
a slot holds), the restatement against the step loop the device chains are compared with (tests/sampler_restated.py) bit for
bit, and every case against the claim of its docstring."""
import ctypes as C
import os

import numpy as np
import pytest

import commit_cases as cc
import commit_restated as cr
import probe_lib
from moves_restated import STRETCH, pick, pick_skip, pick_skip2
from oracle import stretch_oracle as so
from sampler_restated import run

STRETCH_TABLE = [(STRETCH, 1.0, 2.0, 0.0)]
LADDER = (1.0, 0.5, 0.2)


def _fresh(pos, lnp, acc):
    return {"pos": pos.copy(), "lnprob": lnp.copy(), "n_accepted": acc.copy(), "chain": np.full((1,) + pos.shape, np.nan),
            "chain_lnp": np.full((1, len(pos)), np.nan)}


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype == np.float64)


# ---------------------------------------------------------------- the restatement against the step loop
@pytest.mark.parametrize("betas", [None, LADDER], ids=["untempered", "tempered"])
def test_commit_equals_a_step_of_the_restated_loop(betas):
    """3 ensembles of 10 walkers, 3 dims, 6 steps on the Gaussian target: the outcome rows of every step from
    oracle.stretch_oracle (step_rows: _draw over the split) through commit() give the chain row, lnprob and counters of
    sampler_restated.run, untempered and against betas (1, 0.5, 0.2) without a swap sweep."""
    n, ne, ndim, seed, steps = 10, 3, 3, 20261018, 6
    pos = np.random.default_rng(5).normal(size=(ne * n, ndim)) * 1.5
    ref = run(pos.copy(), steps, seed, STRETCH_TABLE, n_ensembles=ne, betas=None if betas is None else list(betas), n_temps=0)
    lnp = np.array([so.gaussian_lnprob(p) for p in pos])
    s = _fresh(pos, lnp, np.zeros(ne * n, dtype=np.int64))
    for step in range(steps):
        perms = [so.split(seed, step, e, n) for e in range(ne)]
        rows = so.step_rows(s["pos"], s["lnprob"], perms, seed, step, 0, 3 * (n // 2) * ne, n)
        decided, chosen, failed = cr.commit(s, perms, rows, betas)
        assert np.array_equal(s["chain"][0], ref.chain[step]) and np.array_equal(s["chain_lnp"][0], ref.lnp[step]), step
        assert np.array_equal(decided, ref.accepted[step]) and not failed and np.all(chosen >= 0)
    assert np.array_equal(s["n_accepted"], ref.acc) and 0 < ref.acc.sum() < steps * ne * n
    if betas is not None:
        plain = run(pos.copy(), steps, seed, STRETCH_TABLE, n_ensembles=ne)
        assert not np.array_equal(plain.chain, ref.chain)           # the betas decided something


def test_apply_equals_the_half_steps_of_the_restated_loop():
    """The same run, every half-step committed by apply() from oracle.stretch_oracle.halfstep_rows."""
    n, ne, ndim, seed, steps = 10, 3, 3, 20261018, 6
    pos = np.random.default_rng(5).normal(size=(ne * n, ndim)) * 1.5
    ref = run(pos.copy(), steps, seed, STRETCH_TABLE, n_ensembles=ne)
    s = _fresh(pos, np.array([so.gaussian_lnprob(p) for p in pos]), np.zeros(ne * n, dtype=np.int64))
    for step in range(steps):
        perms = [so.split(seed, step, e, n) for e in range(ne)]
        for half in range(2):
            rows = so.halfstep_rows(s["pos"], s["lnprob"], perms, seed, step, half, 0, (n // 2) * ne, n)
            _, touched, _ = cr.apply(s, perms, rows, half)
            assert touched.sum() == (n // 2) * ne
        assert np.array_equal(s["chain"][0], ref.chain[step]) and np.array_equal(s["chain_lnp"][0], ref.lnp[step]), step
    assert np.array_equal(s["n_accepted"], ref.acc)


def test_swap_equals_the_sweep_of_the_restated_loop():
    """2 groups of 3 temperatures, 10 walkers each, 8 steps: the state of the loop without a sweep (n_temps = 0: the same
    decisions), taken step by step through swap(), is the tempered loop's; the counts add up to its counts."""
    n, ne, ndim, seed, steps = 10, 6, 3, 77, 8
    betas = list(LADDER) * 2
    pos = np.random.default_rng(6).normal(size=(ne * n, ndim)) * 1.5
    ref = run(pos.copy(), steps, seed, STRETCH_TABLE, n_ensembles=ne, betas=betas, n_temps=3)
    p, lnp, acc, total = pos.copy(), None, None, 0
    for step in range(steps):
        one = run(p, 1, seed, STRETCH_TABLE, n_ensembles=ne, betas=betas, n_temps=0, step0=step, lnp=lnp, acc=acc)
        lnp, acc = one.lnp[-1].copy(), one.acc
        s = {"pos": p, "lnprob": lnp, "n_accepted": acc.copy(), "chain": one.chain.copy(), "chain_lnp": one.lnp.copy()}
        counts, swapped, _ = cr.swap(s, [so.split(seed, step, e, n) for e in range(ne)], betas, 3, seed, step)
        total = total + counts
        assert np.array_equal(s["chain"][0], ref.chain[step]) and np.array_equal(s["chain_lnp"][0], ref.lnp[step]), step
        assert np.array_equal(s["n_accepted"], acc)
    assert np.array_equal(total, ref.swaps) and np.all(ref.swaps > 0) and ref.swaps.sum() < steps * n * 4


# ---------------------------------------------------------------- structure of every case
@pytest.mark.parametrize("case", cc.commit_cases() + cc.apply_cases(), ids=lambda c: c.name)
def test_commit_and_apply_cases_decide_every_walker_once(case):
    """Every walker of the step (commit) or of the active half (apply) is decided exactly once; an accepted walker holds its row
    and one more acceptance, every other walker is unchanged; the chain row is the state after the update and every other row
    keeps its canaries; the partner slots and the split are inside their ranges (the probe refuses anything else)."""
    nt, ndim, n_half = case.n_walkers * case.n_ensembles, case.ndim, case.n_walkers // 2
    before = cc.state_of(case)
    if isinstance(case, cc.CommitCase):
        s, decided, chosen, failed = cc.commit_expected(case.name)
        active = np.ones(nt, dtype=bool)
        assert np.all(chosen >= 0) and case.spec.shape == (3, n_half * case.n_ensembles, ndim + cc.SPEC_EXTRA)
        partner = case.spec[:, :, ndim + 5]
        assert np.all((partner >= 0) & (partner < n_half) & (partner == np.floor(partner)))
        assert case.betas is None or len(case.betas) == case.n_ensembles
    else:
        s, decided, active, failed = cc.apply_expected(case.name)
        assert active.sum() == n_half * case.n_ensembles and case.upd.shape == (n_half * case.n_ensembles, ndim + 3)
        assert sorted(cr.decode_order(case.ens_order, case.n_ensembles)) == list(range(case.n_ensembles))
    assert all(sorted(p) == list(range(case.n_walkers)) for p in case.perm) and case.perm.dtype == np.int32
    assert 1 <= ndim <= cc.MAX_NDIM and not np.any(decided & ~active)
    assert same(s["pos"][~decided], before["pos"][~decided]) and same(s["lnprob"][~decided], before["lnprob"][~decided])
    assert np.array_equal(s["n_accepted"], before["n_accepted"] + decided) and np.all(before["n_accepted"] >= 2 ** 40)
    rows = case.spec.reshape(-1, case.spec.shape[-1]) if isinstance(case, cc.CommitCase) else case.upd
    for k in np.flatnonzero(decided):
        assert any(np.array_equal(s["pos"][k], r[:ndim]) and same(s["lnprob"][k:k + 1], r[ndim:ndim + 1]) for r in rows), k
    if case.chain_rows:
        other = [r for r in range(case.chain_rows) if r != case.chain_row]
        assert np.all(np.isnan(s["chain"][other])) and np.all(np.isnan(s["chain_lnp"][other]))
        assert same(s["chain"][case.chain_row][active], s["pos"][active]) and np.all(np.isnan(s["chain"][case.chain_row][~active]))
        assert same(s["chain_lnp"][case.chain_row][decided], s["lnprob"][decided])
    assert all(np.all(np.isfinite(q)) for q in failed)              # (the sorted comparison of the log needs no NaN rule)
    assert len({tuple(q) for q in failed}) == len(failed)


def _decisions(c):
    """decide[3][slots] of the rows of a commit case."""
    nd, n_half = c.ndim, c.n_walkers // 2
    return np.array([[cr.accepted(u[nd + 2], u[nd], u[nd + 4], u[nd + 3], None if c.betas is None else c.betas[gs // n_half])
                      for gs, u in enumerate(block)] for block in c.spec])


def test_commit_cases_do_what_their_docstrings_claim():
    cases = cc.commit_cases()
    assert {c.ndim for c in cases} >= {1, 6, 9} and {c.n_ensembles for c in cases} >= {1, 3, 16}
    assert {c.n_walkers * c.n_ensembles for c in cases} >= {2, 254, 256, 258, 514}
    assert {(c.chain_rows, c.chain_row) for c in cases} >= {(0, 0), (3, 0), (3, 2)}
    for name, perm in (("commit-2", np.arange(2)), ("commit-254-reversal", np.arange(254)[::-1])):
        assert np.array_equal(cc.by_name(name).perm[0], perm)
    c = cc.by_name("commit-254-reversal")
    assert np.all(c.spec[:, :, c.ndim + 5] == 126)
    c = cc.by_name("commit-256-16-ensembles")
    assert np.array_equal(c.spec[1, :, c.ndim + 5], np.arange(128) % 8) and len({tuple(p) for p in c.perm}) == 16
    assert np.all(cc.by_name("commit-2").spec[:, :, 1 + 5] == 0)
    # the log of failed proposals against its capacity
    n_failed = {c.name: len(cc.commit_expected(c.name)[3]) for c in cases}
    for name, rel in (("commit-2", "fewer"), ("commit-254-reversal", "fewer"), ("commit-256-16-ensembles", "equal"),
                      ("commit-258-3-ensembles", "more"), ("commit-514", "zero"), ("commit-30-no-log", None)):
        cap, n = cc.by_name(name).bad_cap, n_failed[name]
        assert {"fewer": cap is not None and n < cap, "equal": n == cap and n > 0, "more": cap is not None and n > cap >= 1,
                "zero": cap == 0 and n > 0, None: cap is None and n > 0}[rel], (name, n, cap)
    # statuses 0 .. 4 on chosen and on losing candidates; a losing candidate that failed beside a chosen one that did not
    c = cc.by_name("commit-258-3-ensembles")
    _, decided, chosen, _ = cc.commit_expected(c.name)
    n_half, n_slots, st = c.n_walkers // 2, (c.n_walkers // 2) * c.n_ensembles, c.spec[:, :, c.ndim + 1]
    second = np.array([[e * c.n_walkers + c.perm[e, n_half + s] for s in range(n_half)] for e in range(c.n_ensembles)]).ravel()
    blk = chosen[second]
    st_chosen, st_lost = st[blk, np.arange(n_slots)], st[3 - blk, np.arange(n_slots)]
    assert set(st_chosen) == set(st_lost) == {0.0, 1.0, 2.0, 3.0, 4.0}
    assert np.any(np.isin(st_lost, (1, 2)) & ~np.isin(st_chosen, (1, 2))) and np.any(np.isin(st_chosen, (1, 2)) & ~decided[second])
    # candidates 1 and 2 disagree for at least a third of the second half; both candidates are taken; the same slot of another
    # ensemble carries the opposite decision of the first half, so a partner looked up in ensemble 0 picks the other candidate
    dec = _decisions(c)
    assert np.count_nonzero(dec[1] != dec[2]) * 3 >= n_slots and set(blk) == {1, 2}
    d0 = dec[0].reshape(c.n_ensembles, n_half)
    assert np.all(d0[1:] != d0[0])
    mutant = c.spec.copy()
    mutant[0] = np.tile(c.spec[0, :n_half], (c.n_ensembles, 1))                     # gs_j without the ensemble term
    wrong = cr.commit(cc.state_of(c), c.perm, mutant, None, c.chain_row)[1][second]
    assert np.all(wrong[n_half:] != blk[n_half:]) and np.array_equal(wrong[:n_half], blk[:n_half])
    flipped = c.spec[[0, 2, 1]].copy()                                              # u1 and u2 exchanged
    flipped[[1, 2], :, c.ndim + 5] = c.spec[[1, 2], :, c.ndim + 5]
    s2 = cc.state_of(c)
    cr.commit(s2, c.perm, flipped, None, c.chain_row)
    assert not np.array_equal(s2["pos"], cc.commit_expected(c.name)[0]["pos"])
    # betas all 1: the twin holds the same inputs and the restatement the same outputs
    t = cc.by_name(c.twin)
    assert t.twin == c.name and np.all(t.betas == 1.0) and all(same(getattr(c, f), getattr(t, f)) for f in ("pos", "lnprob", "perm", "spec"))
    assert all(same(cc.commit_expected(c.name)[0][k], cc.commit_expected(t.name)[0][k]) for k in ("pos", "lnprob", "n_accepted", "chain", "chain_lnp"))
    # ties
    for name in ("commit-ties", "commit-ties-tempered"):
        c = cc.by_name(name)
        nd, n_half = c.ndim, c.n_walkers // 2
        dec = _decisions(c)
        for b in range(3):
            for gs in range(c.spec.shape[1]):
                u = c.spec[b, gs]
                beta = 1.0 if c.betas is None else c.betas[gs // n_half]
                assert all(v == np.floor(v) for v in (u[nd], u[nd + 2], u[nd + 4]))
                diff = (u[nd + 2] + beta * u[nd]) - beta * u[nd + 4]                      # exact: small even integers
                kind = (b * c.spec.shape[1] + gs + b) % 3
                assert u[nd + 3] == (diff, np.nextafter(diff, -np.inf), np.nextafter(diff, np.inf))[kind]
                assert dec[b, gs] == (kind == 1)
        assert 0 < cc.commit_expected(name)[1].sum() < len(cc.commit_expected(name)[1])
    # non-finite values
    want = {(-np.inf, -1.0, -0.5, 0.0): False, (np.inf, -1.0, -0.5, 0.0): True, (-np.inf, -np.inf, -0.5, 0.0): False,
            (-1.0, -np.inf, -0.5, 0.0): True, (-1.0, np.inf, -0.5, 0.0): False, (np.inf, np.inf, -0.5, 0.0): False,
            (-2.0, -1.0, -np.inf, 0.0): True, (-np.inf, -1.0, -np.inf, 0.0): False, (-1.0, -2.0, -0.5, 0.0): True}
    for row, ok in want.items():
        assert row in cc.NONFINITE_ROWS and cr.accepted(row[3], row[0], row[1], row[2]) == ok, row
    assert not cr.accepted(0.0, np.nan, -1.0, -0.5) and not cr.accepted(np.nan, -1.0, -2.0, -0.5)
    assert not cr.accepted(0.0, -np.inf, -1.0, -1.0, 0.0) and not cr.accepted(0.0, np.inf, -1.0, -1.0, 0.0)   # 0 x inf = NaN
    assert cr.accepted(0.0, -5.0, -1.0, -1.0, 0.0)                                                          # finite at beta = 0: h > ln u
    for name in ("commit-nonfinite", "commit-nonfinite-tempered"):
        c = cc.by_name(name)
        s, decided, chosen, _ = cc.commit_expected(name)
        used = {tuple(np.nan_to_num(c.spec[b, gs, c.ndim:][[0, 4, 3, 2]], nan=123.0)) for b in range(3) for gs in range(c.spec.shape[1])}
        assert len(used) == len(cc.NONFINITE_ROWS) and 0 < decided.sum() < len(decided)
        assert np.any(np.isposinf(s["lnprob"])) and not np.any(np.isnan(s["lnprob"])) and not np.any(np.isneginf(s["lnprob"]))
        assert np.any(np.isneginf(s["chain_lnp"][c.chain_row]))      # a refused walker's chain_lnp is the row's lnprob before the move
    # the ladder with beta = 0: -inf proposals are refused in every ensemble, although h > ln u
    c = cc.by_name("commit-ladder-zero-minus-inf")
    dec, lnp = _decisions(c), c.spec[:, :, c.ndim]
    assert tuple(c.betas) == (1.0, 0.5, 0.0) and not np.any(dec[np.isneginf(lnp)]) and np.any(dec[~np.isneginf(lnp)])
    hot = np.isneginf(lnp[:, 2 * 6:])
    assert hot.sum() >= 6 and np.all(c.spec[:, 2 * 6:, c.ndim + 2][hot] > c.spec[:, 2 * 6:, c.ndim + 3][hot])
    # one beta per ensemble over the same rows
    c = cc.by_name("commit-beta-per-ensemble")
    n_half = c.n_walkers // 2
    assert all(np.array_equal(c.spec[:, :n_half], c.spec[:, e * n_half:(e + 1) * n_half]) for e in (1, 2)) and np.all(c.perm == c.perm[0])
    dec = _decisions(c).reshape(3, 3, n_half)
    assert np.count_nonzero(dec[:, 0] != dec[:, 1]) >= 6 and np.count_nonzero(dec[:, 1] != dec[:, 2]) >= 6
    s0 = cc.state_of(c)
    cr.commit(s0, c.perm, c.spec, np.full(3, c.betas[0]))                                                    # beta[0] for beta[w_ens]
    assert not np.array_equal(s0["pos"], cc.commit_expected(c.name)[0]["pos"])


def test_apply_cases_do_what_their_docstrings_claim():
    cases = cc.apply_cases()
    assert {(c.n_walkers // 2) * c.n_ensembles for c in cases} >= {255, 256, 257} and {c.half for c in cases} == {0, 1}
    assert cc.by_name("apply-255-reversed").ens_order == 0x012 and cc.by_name("apply-257-identity").ens_order == 0
    c = cc.by_name("apply-256-permutation-of-16")
    order = cr.decode_order(c.ens_order, 16)
    assert order[15] == 15 and order[0] != 0 and sorted(order) == list(range(16)) and c.ens_order >> 60 == 15
    for c in cases:
        s, decided, touched, failed = cc.apply_expected(c.name)
        before = cc.state_of(c)
        if touched.sum() >= 255:
            acc, st = c.upd[:, c.ndim + 1], c.upd[:, c.ndim + 2]
            assert 0 < decided.sum() < touched.sum() and np.any((st == 1) & (acc == 0)) and np.any((st == 1) & (acc == 1))
            assert set(st) == {0.0, 1.0, 2.0, 3.0, 4.0}
        if c.chain_rows:      # a refused walker's chain_lnp is the state's lnprob, which no row holds
            refused = touched & ~decided
            assert same(s["chain_lnp"][c.chain_row][refused], before["lnprob"][refused]) and not np.any(np.isin(before["lnprob"], c.upd[:, c.ndim]))
        if c.ens_order:       # launched in the numbered order the rows go to other walkers
            s2 = cc.state_of(c)
            cr.apply(s2, c.perm, c.upd, c.half, 0, c.chain_row)
            assert not np.array_equal(s2["pos"], s["pos"])
    n_failed = {c.name: (len(cc.apply_expected(c.name)[3]), c.bad_cap) for c in cases}
    assert n_failed["apply-256-permutation-of-16"][0] > n_failed["apply-256-permutation-of-16"][1] >= 1
    assert n_failed["apply-two-swapped"][0] == n_failed["apply-two-swapped"][1] >= 1
    assert n_failed["apply-255-reversed"][0] < n_failed["apply-255-reversed"][1]
    assert n_failed["apply-three-identity-half-1"] [1] == 0 < n_failed["apply-three-identity-half-1"][0]
    assert n_failed["apply-257-identity"][1] is None


@pytest.mark.parametrize("case", cc.swap_cases(), ids=lambda c: c.name)
def test_swap_cases_conserve_what_a_slot_holds(case):
    """Per group and slot the sweep permutes the (position, lnprob) pairs of the slot's walkers and touches nothing else:
    n_accepted stays, walkers outside accepted swaps keep their chain canaries, the others hold their new state there."""
    s, counts, swapped, taken = cc.swap_expected(case.name)
    before = cc.state_of(case)
    n, nt = case.n_walkers, case.n_temps
    assert all(sorted(p) == list(range(n)) for p in case.perm) and len(case.betas) == case.n_ensembles == len(case.lnprob) // n
    assert np.array_equal(s["n_accepted"], before["n_accepted"]) and np.array_equal(counts, taken.sum(axis=1))
    for g in range(case.n_ensembles // nt):
        for i in range(n):
            ks = [e * n + case.perm[e, i] for e in range(g * nt, (g + 1) * nt)]
            rows = lambda st: np.column_stack([st["pos"][ks], st["lnprob"][ks]])      # noqa: E731
            a, b = rows(before), rows(s)
            assert same(a[np.lexsort(a.T[::-1])], b[np.lexsort(b.T[::-1])]), (g, i)
            assert swapped[ks].any() == taken[g, i].any()
    assert same(s["pos"][~swapped], before["pos"][~swapped]) and same(s["lnprob"][~swapped], before["lnprob"][~swapped])
    if case.chain_rows:
        row = case.chain_row
        assert np.all(np.isnan(s["chain"][row][~swapped])) and np.all(np.isnan(s["chain_lnp"][row][~swapped]))
        assert same(s["chain"][row][swapped], s["pos"][swapped]) and same(s["chain_lnp"][row][swapped], s["lnprob"][swapped])
        other = [r for r in range(case.chain_rows) if r != row]
        assert np.all(np.isnan(s["chain"][other]))


def test_swap_cases_do_what_their_docstrings_claim():
    cases = cc.swap_cases()
    assert {c.n_walkers for c in cases} >= {2, 62, 64, 66, 256, 258, 600} and {c.n_temps for c in cases} >= {2, 3, 8}
    assert {c.n_ensembles // c.n_temps for c in cases} >= {1, 3} and {c.ndim for c in cases} >= {1, 9}
    assert {c.step for c in cases} >= {0, 2 ** 32 - 1} and all(c.seed >> 32 for c in cases) and {c.chain_rows for c in cases} == {0, 3}
    for name in ("swap-62-three-groups", "swap-64-eight-temperatures", "swap-600-three-groups", "swap-256"):
        c = cc.by_name(name)
        taken = cc.swap_expected(name)[3]
        slot = np.arange(c.n_walkers)
        assert np.all(taken[:, slot % 4 == 0]) and not np.any(taken[:, slot % 4 == 1])          # at every pair, at none
        rest = taken[:, slot % 4 >= 2]
        assert 0 < rest.sum() < rest.size
        assert len({tuple(row) for row in cc.swap_expected(name)[1]}) == len(cc.swap_expected(name)[1]) or c.n_temps == 2
    # a slot's swap at pair t decides pair t - 1: the other order of the pairs gives another state
    c = cc.by_name("swap-64-eight-temperatures")
    s2 = cc.state_of(c)
    counts2, _, taken2 = cr.swap(s2, c.perm, c.betas, c.n_temps, c.seed, c.step, c.chain_row, hottest_first=False)
    s, counts, _, taken = cc.swap_expected(c.name)
    assert not np.array_equal(s2["pos"], s["pos"]) and not np.array_equal(counts2, counts)
    assert np.all(taken[0, ::4]) and np.all(taken2[0, ::4, -1]) and not np.any(taken2[0, ::4, :-1])
    # betas
    assert np.all(cc.swap_expected("swap-equal-betas")[3]) and len(set(cc.by_name("swap-equal-betas").betas)) == 1
    b = cc.by_name("swap-reversed-ladder").betas
    assert np.all(np.diff(b) > 0) and 0 < cc.swap_expected("swap-reversed-ladder")[1].sum()
    assert cc.by_name("swap-hot-end-zero").betas[-1] == 0.0
    # non-finite values: which pairs of (L_cold, L_hot) swap at dbeta = 0.5, and none at dbeta = 0
    c = cc.by_name("swap-nonfinite")
    taken = cc.swap_expected(c.name)[3]
    inf = np.inf
    want = {(-inf, 0.0): True, (0.0, -inf): False, (inf, 0.0): False, (0.0, inf): True, (-inf, -inf): False, (inf, inf): False,
            (-inf, inf): True, (inf, -inf): False}
    for i in range(c.n_walkers):
        lc, lh = c.lnprob[c.perm[0, i]], c.lnprob[c.n_walkers + c.perm[1, i]]
        assert taken[0, i, 0] == (False if np.isnan(lc) or np.isnan(lh) else want[(lc, lh)]), (i, lc, lh)
    assert np.isnan(c.lnprob).sum() == 2 * 2 * 2 and not np.any(taken[1]) and c.betas[2] == c.betas[3]
    # the tie
    c = cc.by_name("swap-tie")
    taken = cc.swap_expected(c.name)[3]
    assert c.betas[0] - c.betas[1] == 1.0
    for i in range(c.n_walkers):
        kc, kh = c.perm[0, i], c.n_walkers + c.perm[1, i]
        lnu = cr.swap_lnu(c.seed, c.step, int(kc))
        assert c.lnprob[kc] == 0.0 and c.lnprob[kh] == (lnu if i % 2 == 0 else np.nextafter(lnu, np.inf)) and np.isfinite(lnu)
        assert taken[0, i, 0] == (i % 2 == 1)
    # counts start at distinct values per group and pair
    assert all(len(set(c.swaps0.ravel())) == c.swaps0.size for c in cases)


# ---------------------------------------------------------------- order
def test_order_restatement_and_cases():
    cls, counts = cr.order(cc.N_OBS, np.arange(12))
    assert cls.tolist() == [5, 5, 4, 4, 3, 3, 2, 2, 1, 1, 0, 0] and counts.tolist() == [2] * 6
    assert cr.order(cc.N_OBS, cc.BAD_IDS)[0].tolist() == [5, 5, 5] and cr.order((), [0, 1, -1])[0].tolist() == [5, 5, 5]
    cases = cc.order_cases()
    assert {len(c.ds_id) for c in cases} >= {1, 6, 1023, 1024, 1025, 5000} and tuple(cases[0].n_obs) == cc.N_OBS
    for c in cases:
        cls, counts = cr.order(c.n_obs, c.ds_id)
        assert counts.sum() == len(c.ds_id) and c.ds_id.dtype == np.int32 and c.n_obs.dtype == np.int32
        order = np.argsort(cls, kind="stable")                       # one valid answer: it has the properties the GPU test asks for
        assert np.array_equal(np.sort(order), np.arange(len(cls))) and np.all(np.diff(cls[order]) >= 0)
        assert np.array_equal(np.bincount(cls[order], minlength=6), counts)
    assert cr.order(*cc.by_name("order-6-one-per-class")[2:])[1].tolist() == [1] * 6
    assert cr.order(*cc.by_name("order-all-in-one-class")[2:])[1].tolist() == [1025, 0, 0, 0, 0, 0]
    assert cr.order(*cc.by_name("order-no-datasets")[2:])[1].tolist() == [0, 0, 0, 0, 0, 100]
    for name in ("order-5000", "order-1023", "order-bad-ids"):
        c = cc.by_name(name)
        assert set(cc.BAD_IDS) <= set(c.ds_id.tolist()) and (np.all(cr.order(c.n_obs, c.ds_id)[1] > 0) or len(c.ds_id) < 1000)


# ---------------------------------------------------------------- pick
def test_pick_cases_and_the_restated_draws():
    u, m, c0, c1 = cc.pick_cases()
    want = cc.pick_expected()
    assert len(u) % 64 == 0 and len(u) <= 1 << 20 and set(m) == set(np.arange(1.0, 71.0))
    assert np.all((u >= 0.0) & (u < 1.0)) and np.all((c0 >= 0) & (c0 < m) & (c1 >= 0) & (c1 < m)) and np.all((c0 != c1) | (m == 1))
    assert u.max() == 1.0 - 2.0 ** -53 and u.min() == 0.0
    # in range, and distinct from the indices stepped over
    assert np.all((want[:, 0] >= 0) & (want[:, 0] < m))
    two, three = m >= 2, m >= 3
    assert np.all(want[~two, 1] == -1) and np.all(want[~three, 2] == -1)
    assert np.all((want[two, 1] >= 0) & (want[two, 1] < m[two]) & (want[two, 1] != c0[two]))
    assert np.all((want[three, 2] >= 0) & (want[three, 2] < m[three]) & (want[three, 2] != c0[three]) & (want[three, 2] != c1[three]))
    for mm in range(2, cc.PICK_ALL_PAIRS_M + 1):
        sel = m == mm
        assert {(a, b) for a, b in zip(c0[sel], c1[sel])} == {(a, b) for a in range(mm) for b in range(mm) if a != b}
    # around every boundary j / m': the double above the rounded quotient falls in j, the quotient and the double below it in j - 1
    # or j (the product with m' is rounded once more); over the doubles above, every target index of the reduced range is hit
    # exactly once
    for mm in range(1, cc.PICK_MAX_M + 1):
        us = set(cc.boundary_us(mm))
        hits = [pick(np.nextafter(j / mm, 1.0), mm) for j in range(1, mm)] + [pick(0.0, mm)]
        assert sorted(hits) == list(range(mm)) and pick(1.0 - 2.0 ** -53, mm) == mm - 1
        for j in range(1, mm):
            b = j / mm
            assert {np.nextafter(b, 0.0), b, np.nextafter(b, 1.0)} <= us
            assert pick(np.nextafter(b, 0.0), mm) in (j - 1, j) and pick(np.nextafter(b, 1.0), mm) == j and pick(b, mm) in (j - 1, j)
        if mm >= 2:       # the skipping draws hit every remaining index equally often over the doubles above the boundaries of m - 1
            above = [0.0] + [np.nextafter(j / (mm - 1), 1.0) for j in range(1, mm - 1)]
            assert all(sorted(pick_skip(x, mm, c) for x in above) == [t for t in range(mm) if t != c] for c in range(mm))
        if 3 <= mm <= 20:
            above = [0.0] + [np.nextafter(j / (mm - 2), 1.0) for j in range(1, mm - 2)]
            assert all(sorted(pick_skip2(x, mm, a, b) for x in above) == [t for t in range(mm) if t not in (a, b)]
                       for a in range(mm) for b in range(mm) if a != b)
    # why the doubles around a boundary are cases: 49 fl(1 / 49) rounds below 1, and 6 times the double below fl(5 / 6) rounds to 5
    assert pick(1.0 / 49, 49) == 0 and pick(np.nextafter(5.0 / 6, 0.0), 6) == 5


# ---------------------------------------------------------------- the probe's caps and refusals (no launch, no GPU)
def test_cases_fit_the_caps_of_the_built_probe():
    from magprop_amd import _capi
    L = probe_lib.load("commit")
    cap = {n: getattr(L, "mpc_max_" + n)() for n in ("ndim", "walkers", "ensembles", "total", "rows", "bad_cap", "order_n", "datasets")}
    assert cap["ndim"] == cc.MAX_NDIM and L.mpc_spec_extra() == cc.SPEC_EXTRA
    for c in cc.commit_cases() + cc.apply_cases() + cc.swap_cases():
        assert c.n_walkers <= cap["walkers"] and c.n_ensembles <= cap["ensembles"] and c.n_walkers * c.n_ensembles <= cap["total"]
        assert c.chain_rows <= cap["rows"] and (getattr(c, "bad_cap", None) or 0) <= cap["bad_cap"] and c.ndim <= cap["ndim"]
    assert all(len(c.ds_id) <= cap["order_n"] and len(c.n_obs) <= cap["datasets"] for c in cc.order_cases())
    assert L.mpc_order(None, 0, None, 0, None) == -1 and L.mpc_commit(*[None] * 5, 2, 1, 1, None, None, 0, 0, None, None, None, 0) == -1
