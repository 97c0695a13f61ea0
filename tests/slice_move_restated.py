"""numpy restatement of the sampler's ensemble slice-sampling move (include/magprop_amd.h MP_MOVE_SLICE): one slice update of a
walker as the kernel's rounds (magprop_amd/csrc/mp_slice.hip slice_half_kernel; the slice itself is walk_restated.slice_rounds,
which the nested sampler's slice mode shares), the tune rule, and a step loop that runs slice
steps here and hands every other move of a mixture, one step at a time, to tests/sampler_restated.py.  Test infrastructure: the
GPU tests compare the device chains with the loop bit for bit, the CPU tests draw their statistics from it.  Every product and
sum is a separately rounded float64 operation in the kernel's order."""
from typing import NamedTuple

import numpy as np

import nest_restated as nr
import sampler_restated
from moves_restated import draw_move, pick, pick_skip, resolve
from oracle.stretch_oracle import gaussian_lnprob, philox4x32_10, split, u01
from walk_restated import slice_rounds

M32 = 0xFFFFFFFF
SLICE = 4                   # MP_MOVE_SLICE
SLICE_CTR = 0x51C00000
STATUS_FLAG, STATUS_NONFINITE = 1, 2


def slice_draw(seed, step, half, k, c):
    """Philox (seed; step, half, k, 0x51C00000 + c)."""
    seed = int(seed)
    return philox4x32_10(seed & M32, seed >> 32, int(step) & M32, int(half), int(k), SLICE_CTR + int(c))


class Update(NamedTuple):
    x: list                 # the walker's position after the update
    lnp: float              # its (untempered) lnprob
    status: int
    moved: int
    n_eval: int
    n_exp: int
    n_con: int
    n_fail: int
    budgets: tuple          # (J, K) as drawn; None where the direction was zero


def slice_update_rounds(x, lnp_x, k, comp_pts, seed, step, half, mu, beta, max_steps_out, max_shrink, box=None, drop_lnu=False):
    """One slice update of walker k at x (a list of floats, stored lnprob lnp_x) as the kernel's rounds: a generator that yields
    the next point to evaluate, is sent its (lnprob, status), and returns an Update.  comp_pts[n_comp]: the other half in split
    order.  box = (lower, upper): points outside it are outside without an evaluation (target 0); None: no box.  drop_lnu (the
    negative control of the tests): the level is beta lnp_x itself, without ln u."""
    m, nd = len(comp_pts), len(x)
    u = slice_draw(seed, step, half, k, 0)
    c1 = pick(u01(u[0], u[1]), m)
    c2 = pick_skip(u01(u[2], u[3]), m, c1)
    d = [float(comp_pts[c1][i]) - float(comp_pts[c2][i]) for i in range(nd)]
    if not any(v != 0.0 for v in d):
        return Update(x, lnp_x, 0, 0, 0, 0, 0, 1, None)
    u = slice_draw(seed, step, half, k, 2)
    with np.errstate(divide="ignore"):
        lny = float(beta * lnp_x) if drop_lnu else float(beta * lnp_x + np.log(u01(u[0], u[1])))
    o = yield from slice_rounds(x, d, mu, max_steps_out, max_shrink, lambda c: slice_draw(seed, step, half, k, c), 3,
                                lambda lq: beta * lq > lny, box)
    if o.q is None:
        return Update(x, lnp_x, 0, 0, o.n_eval, o.n_exp, o.n_con, 1, o.budgets)
    return Update(o.q, o.lnp, o.status, 1, o.n_eval, o.n_exp, o.n_con, 0, o.budgets)


def tune(mu, nexpand_s, ncontract_s):
    """zeus's rule on one step's counts: mu (2 a / (a + ncontract_s)), a = max(1, nexpand_s)."""
    a = float(max(1, int(nexpand_s)))
    return float(mu) * ((2.0 * a) / (a + float(int(ncontract_s))))


class State:
    """What the move keeps per ensemble between steps (and calls): mu, the slice steps taken and the totals; `bad` collects the
    evaluated rows whose status is FLAG or NONFINITE, `updates` the Update of every slice (for the conditions of the tests)."""

    def __init__(self, n_ensembles, mu0):
        self.mu = np.full(n_ensembles, float(mu0))
        self.n_tuned = np.zeros(n_ensembles, dtype=np.int64)
        self.nexpand = np.zeros(n_ensembles, dtype=np.int64)
        self.ncontract = np.zeros(n_ensembles, dtype=np.int64)
        self.nfail = np.zeros(n_ensembles, dtype=np.int64)
        self.neval = np.zeros(n_ensembles, dtype=np.int64)
        self.bad, self.updates = [], []

    def counters(self):
        return {k: getattr(self, k).copy() for k in ("nexpand", "ncontract", "nfail", "neval", "n_tuned")}


class Run(NamedTuple):
    chain: np.ndarray        # (n_steps, n_total, ndim), the rows after the step's swaps
    lnp: np.ndarray          # (n_steps, n_total)
    acc: np.ndarray          # (n_total,)
    drawn: np.ndarray        # (n_steps,) index of the step's move in the table
    mu: np.ndarray           # (n_steps, n_ensembles) mu behind every step
    swaps: np.ndarray        # (n_groups, n_temps - 1) accepted swaps of this call; (0, 0) without a swap sweep
    state: State


def slice_entry(table):
    """Index of the table's slice entry (None: none)."""
    at = [m for m, t in enumerate(table) if t[0] == SLICE]
    assert len(at) <= 1
    return at[0] if at else None


def run(pos, n_steps, seed, table, limits=(32, 64), lnprob_fn=gaussian_lnprob, n_ensembles=1, step0=0, lnp=None, acc=None,
        betas=None, n_temps=0, state=None, evaluate=None, box=None, drop_lnu=False):
    """The step loop of mp_sampler_run for a table [(kind, weight, p0, p1)] with a slice entry (SLICE, w, mu0, tune_steps);
    limits = (max_steps_out, max_shrink).  evaluate(rows[k, ndim], walkers[k]) -> (lnprob[k], status[k]): every round of a
    half-step's slices in ONE call, as the device launch evaluates them; None: lnprob_fn(q) one point at a time.  state: the
    move's State of an earlier call (to continue a run from step0 with lnp / acc), advanced in place; None: a fresh one.  pos,
    and lnp / acc where given, are advanced in place."""
    n_total, ndim = pos.shape
    n = n_total // n_ensembles
    half_n = n // 2
    n_comp = n - half_n
    _, cum = resolve(table, ndim)
    at = slice_entry(table)
    tune_steps = int(table[at][3])
    if state is None:
        state = State(n_ensembles, table[at][2])
    tempered = betas is not None and n_temps > 1
    if lnp is None:
        lnp = np.array([lnprob_fn(p) for p in pos])
    if acc is None:
        acc = np.zeros(n_total, dtype=np.int64)
    chain = np.empty((n_steps, n_total, ndim))
    chain_lnp = np.empty((n_steps, n_total))
    drawn = np.empty(n_steps, dtype=np.int64)
    mus = np.empty((n_steps, n_ensembles))
    swaps = np.zeros((n_ensembles // n_temps, n_temps - 1) if tempered else (0, 0), dtype=np.int64)

    def evaluate_logged(rows, walkers):
        out, st = evaluate(rows, walkers)
        state.bad.extend(rows[i].copy() for i in range(len(rows)) if int(st[i]) in (STATUS_FLAG, STATUS_NONFINITE))
        return out, st

    for s in range(n_steps):
        step = step0 + s
        m = drawn[s] = draw_move(seed, step, cum)
        if m != at:   # another move of the mixture: one step of the restated sampler (its swap sweep included)
            r = sampler_restated.run(pos, 1, seed, table, lnprob_fn=lnprob_fn, n_ensembles=n_ensembles, step0=step, lnp=lnp, acc=acc,
                                     betas=betas, n_temps=n_temps)
            swaps += r.swaps
            chain[s], chain_lnp[s], mus[s] = pos, lnp, state.mu
            continue
        perms = [split(seed, step, e, n) for e in range(n_ensembles)]
        ex = np.zeros(n_ensembles, dtype=np.int64)
        co = np.zeros(n_ensembles, dtype=np.int64)
        for half in range(2):
            gens, who = [], []
            for e in range(n_ensembles):
                base, perm = e * n, perms[e]
                b = 1.0 if betas is None else float(betas[e])
                comp_pts = pos[[base + perm[(1 - half) * half_n + c] for c in range(n_comp)]].copy()
                for slot in range(half_n):
                    k = base + perm[half * half_n + slot]
                    gens.append(slice_update_rounds([float(v) for v in pos[k]], float(lnp[k]), k, comp_pts, seed, step, half,
                                                    float(state.mu[e]), b, limits[0], limits[1], box, drop_lnu))
                    who.append(k)
            if evaluate is not None:
                out = nr.in_rounds(gens, who, evaluate_logged)
            else:
                out = [nr.one_at_a_time(g, lambda q: (lnprob_fn(q), 0)) for g in gens]
            for k, o in zip(who, out):
                e = k // n
                if o.moved:
                    pos[k], lnp[k] = o.x, o.lnp
                    acc[k] += 1
                ex[e] += o.n_exp
                co[e] += o.n_con
                state.nfail[e] += o.n_fail
                state.neval[e] += o.n_eval
                state.updates.append(o)
        for e in range(n_ensembles):
            state.nexpand[e] += ex[e]
            state.ncontract[e] += co[e]
            if state.n_tuned[e] < tune_steps:
                state.mu[e] = tune(state.mu[e], ex[e], co[e])
            state.n_tuned[e] += 1
        if tempered:   # (the swap sweep of sampler_restated.run)
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
        chain[s], chain_lnp[s], mus[s] = pos, lnp, state.mu
    return Run(chain, chain_lnp, acc, drawn, mus, swaps, state)


def autocorr_time(x, c=5.0):
    """Integrated autocorrelation time of the series x[steps, walkers] (emcee's estimator: the walkers' mean autocorrelation
    function by FFT, Sokal's window with constant c)."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    size = 1 << (2 * n - 1).bit_length()
    f = np.zeros(n)
    for w in range(x.shape[1]):
        y = x[:, w] - x[:, w].mean()
        ft = np.fft.rfft(y, n=size)
        a = np.fft.irfft(ft * np.conjugate(ft))[:n].real
        f += a / a[0]
    f /= x.shape[1]
    taus = 2.0 * np.cumsum(f) - 1.0
    ok = np.arange(n) >= c * taus
    win = int(np.argmax(ok)) if np.any(ok) else n - 1
    return float(taus[win])
