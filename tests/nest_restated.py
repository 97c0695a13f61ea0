"""numpy restatement of the nested sampler (include/magprop_amd.h mp_nested_*): the ranking, the Philox draw layout, the
constrained DE walks with the unfused arithmetic of the kernels (magprop_amd/csrc/mp_nest.hip), the volume bookkeeping and the
stop rule.  Test infrastructure: the GPU tests compare the device state with it bit for bit (ln X and ln Z to rounding: the
device's log1p / exp / expm1 are not numpy's), the CPU tests check with it that the scheme samples the constrained prior.
Every product and sum is a separately rounded float64 operation in the kernel's order (Python floats).
A walk is a generator with the kernel's round structure (it names a point, is sent the point's lnL and status, decides); the
walks of an iteration run a point at a time (evaluate_one) or all together, one evaluate(rows, runs) call per round (in_rounds),
which is how the GPU tests put an mp_lnprob_batch call of the launch's own size behind every likelihood."""
import math

import numpy as np

from moves_restated import pick, pick_skip
from oracle.stretch_oracle import philox4x32_10, u01
from walk_restated import de_step

M32 = 0xFFFFFFFF
CTR = 0x4E000000


def draw(seed, t, r, slot, j):
    """Philox (seed; t, r, slot, 0x4E000000 + j)."""
    seed = int(seed)
    return philox4x32_10(seed & M32, seed >> 32, int(t) & M32, int(r), int(slot), CTR + int(j))


def logaddexp(x, y):
    m = max(x, y)
    if m == -math.inf:
        return m
    return m + math.log1p(math.exp(-abs(x - y)))


def stops(lmax, lnx, lnz, dlogz):
    """log1p(exp((lnL_max + ln X) - ln Z)) < dlogz (NaN: no)."""
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.log1p(np.exp((np.float64(lmax) + np.float64(lnx)) - np.float64(lnz)))
    return bool(v < dlogz)


def resolve(g0, sigma, ndim):
    """(g0, s3) as the library keeps them."""
    return (g0 if g0 > 0.0 else 2.38 / math.sqrt(2.0 * ndim)), sigma * math.sqrt(3.0)


class State:
    """live[n_runs, N, ndim], lnl, status, acc [n_runs, N]; per run nit, stopped, lnx, lnz, ncall, nacc, nzero; dead rows per run."""

    def __init__(self, live, lnl, status):
        n_runs, n = lnl.shape
        self.live, self.lnl, self.status = live, lnl, status
        self.acc = np.zeros((n_runs, n), dtype=np.int32)
        self.nit = np.zeros(n_runs, dtype=np.int32)
        self.stopped = np.zeros(n_runs, dtype=np.int32)
        self.lnx = np.zeros(n_runs)
        self.lnz = np.full(n_runs, -np.inf)
        self.ncall = np.zeros(n_runs, dtype=np.int64)
        self.nacc = np.zeros(n_runs, dtype=np.int64)
        self.nzero = np.zeros(n_runs, dtype=np.int64)
        self.dead_pars = [[] for _ in range(n_runs)]
        self.dead_lnl = [[] for _ in range(n_runs)]
        self.dead_n = [[] for _ in range(n_runs)]


def _clean(v):
    return -math.inf if v != v else float(v)


def start(live0, evaluate, with_runs=False):
    """The live set live0 (n_runs, N, ndim) evaluated: evaluate(rows[n, ndim]) -> (lnL, status); with_runs: evaluate(rows,
    runs[n]), the run of every row with it."""
    live = np.array(live0, dtype=np.float64)
    n_runs, n, ndim = live.shape
    rows = live.reshape(-1, ndim)
    lnl, st = evaluate(rows, np.repeat(np.arange(n_runs), n)) if with_runs else evaluate(rows)
    lnl = np.array([_clean(v) for v in lnl]).reshape(n_runs, n)
    return State(live, lnl, np.asarray(st, dtype=np.int32).reshape(n_runs, n))


def order(lnl):
    """Slots in ascending (lnL, slot)."""
    return sorted(range(len(lnl)), key=lambda j: (lnl[j], j))


def walk_rounds(s, r, slot, t, surv, lstar, seed, walks, g0, s3, lower, upper):
    """The constrained walk into dead slot `slot` of run r, iteration t, as the kernel's rounds: a generator that yields the
    next point to evaluate (a proposal inside the box), is sent its (lnL, status), and returns (end point, lnL, status,
    accepted steps, evaluations)."""
    m = len(surv)
    u = draw(seed, t, r, slot, 0)
    fr = surv[pick(u01(u[0], u[1]), m)]
    x = [float(v) for v in s.live[r, fr]]
    lnl, st = float(s.lnl[r, fr]), int(s.status[r, fr])
    n_acc = n_eval = 0
    for k in range(walks):
        u = draw(seed, t, r, slot, 2 * k + 1)
        v = draw(seed, t, r, slot, 2 * k + 2)
        c1 = pick(u01(u[0], u[1]), m)
        c2 = pick_skip(u01(u[2], u[3]), m, c1)
        q, inside = de_step(x, s.live[r, surv[c1]], s.live[r, surv[c2]], g0, s3, u01(v[0], v[1]), lower, upper)
        if not inside:
            continue
        q = [float(c) for c in q]
        lq, sq = yield np.array(q)
        lq = _clean(lq)
        n_eval += 1
        if lq > lstar:
            x, lnl, st = q, lq, int(sq)
            n_acc += 1
    return x, lnl, st, n_acc, n_eval


def one_at_a_time(gen, evaluate_one):
    """Drives one walk to its end, every point it names through evaluate_one(q) -> (lnL, status); returns what the walk returns."""
    try:
        q = next(gen)
        while True:
            q = gen.send(evaluate_one(q))
    except StopIteration as e:
        return e.value


def in_rounds(gens, runs, evaluate):
    """Drives the walks gens (gens[i] a walk of run runs[i]) together, a round at a time as the device launch does: every
    unfinished walk names its next point, ONE evaluate(rows[k, ndim], runs[k]) -> (lnL[k], status[k]) answers them all (in the
    order of gens), every walk decides.  As many calls as the longest walk has rounds.  Returns what the walks return."""
    out, pending = [None] * len(gens), {}

    def advance(i, answer):
        try:
            pending[i] = next(gens[i]) if answer is None else gens[i].send(answer)
        except StopIteration as e:
            pending.pop(i, None)
            out[i] = e.value

    for i in range(len(gens)):
        advance(i, None)
    while pending:
        idx = sorted(pending)
        lnl, st = evaluate(np.array([pending[i] for i in idx]), np.array([runs[i] for i in idx]))
        assert len(lnl) == len(idx) and len(st) == len(idx)
        for k, i in enumerate(idx):
            advance(i, (lnl[k], st[k]))
    return out


def drive(gens, runs, evaluate_one=None, evaluate=None):
    """The walks of an iteration through evaluate (in_rounds) where one is given, else one after the other through evaluate_one."""
    if evaluate is not None:
        return in_rounds(gens, runs, evaluate)
    return [one_at_a_time(g, evaluate_one) for g in gens]


def walk(s, r, slot, t, surv, lstar, seed, walks, g0, s3, lower, upper, evaluate_one):
    """walk_rounds, one evaluate_one(q) per round: (end point, lnL, status, accepted steps, evaluations)."""
    return one_at_a_time(walk_rounds(s, r, slot, t, surv, lstar, seed, walks, g0, s3, lower, upper), evaluate_one)


def select(lnl, lnx, lnz, nbatch, dlogz):
    """The select step of one run on the live lnL `lnl` (a NaN ranks, and is listed, as -inf): None where the stop rule fires on
    the live set as it stands, else (dead slots in ascending (lnL, slot), survivors in slot order, L*, the dead lnL, the live
    counts n_k of the dead, the new ln X, the new ln Z)."""
    key = [_clean(v) for v in lnl]
    n = len(key)
    o = order(key)
    if stops(key[o[-1]], lnx, lnz, dlogz):
        return None
    dead, surv = o[:nbatch], sorted(o[nbatch:])
    lnx, lnz = float(lnx), float(lnz)
    dead_lnl, dead_n = [], []
    for k, j in enumerate(dead):
        dead_lnl.append(key[j])
        dead_n.append(n - k)
        inv = 1.0 / float(n - k)
        lnw = (key[j] + lnx) + math.log(-math.expm1(-inv))
        lnx = lnx - inv
        lnz = logaddexp(lnz, lnw)
    return dead, surv, key[dead[-1]], dead_lnl, dead_n, lnx, lnz


def retire(s, nbatch, dlogz):
    """The select step of every run not stopped, booked into s (stopped flags, dead lists, ln X, ln Z): the list of
    (r, dead slots, survivors, L*, t) of the runs that go on to their walks."""
    jobs = []
    for r in range(s.lnl.shape[0]):
        if s.stopped[r]:
            continue
        sel = select(s.lnl[r], s.lnx[r], s.lnz[r], nbatch, dlogz)
        if sel is None:
            s.stopped[r] = 1
            continue
        dead, surv, lstar, dead_lnl, dead_n, s.lnx[r], s.lnz[r] = sel
        s.dead_pars[r].extend(s.live[r, j].copy() for j in dead)
        s.dead_lnl[r].extend(dead_lnl)
        s.dead_n[r].extend(dead_n)
        jobs.append((r, dead, surv, lstar, int(s.nit[r])))
    return jobs


def iteration(s, nbatch, seed, walks, g0, sigma, dlogz, lower, upper, evaluate_one=None, evaluate=None):
    """One iteration of every run not stopped (the stop rule first, on the live set as it stands).  evaluate(rows, runs): the
    walks of all runs and slots advance together, one call per round (in_rounds); else evaluate_one(q), a point at a time."""
    g0, s3 = resolve(g0, sigma, s.live.shape[2])
    jobs = retire(s, nbatch, dlogz)
    where = [(r, j) for r, dead, *_ in jobs for j in dead]
    gens = [walk_rounds(s, r, j, t, surv, lstar, seed, walks, g0, s3, lower, upper)
            for r, dead, surv, lstar, t in jobs for j in dead]
    out = drive(gens, [r for r, _ in where], evaluate_one, evaluate)      # (survivors are only read, dead slots written behind)
    for (r, j), (x, lq, sq, na, ne) in zip(where, out):
        s.live[r, j], s.lnl[r, j], s.status[r, j], s.acc[r, j] = x, lq, sq, na
        s.ncall[r] += ne
        s.nacc[r] += na
        s.nzero[r] += na == 0
    for r, *_ in jobs:
        s.nit[r] += 1


def check_stops(s, dlogz):
    for r in range(len(s.nit)):
        if not s.stopped[r] and stops(np.max(s.lnl[r]), s.lnx[r], s.lnz[r], dlogz):
            s.stopped[r] = 1


def run(s, iterations, nbatch, seed, walks=25, g0=0.0, sigma=0.1, dlogz=0.01, lower=None, upper=None, evaluate_one=None,
        evaluate=None):
    """Up to `iterations` iterations and the stop check behind them (mp_nested_run); s is advanced in place.  evaluate_one /
    evaluate: as iteration takes them."""
    if iterations <= 0 or np.all(s.stopped):
        return s
    for _ in range(iterations):
        if np.all(s.stopped):
            break
        iteration(s, nbatch, seed, walks, g0, sigma, dlogz, lower, upper, evaluate_one, evaluate)
    check_stops(s, dlogz)
    return s


def gaussian_one(q):
    """The unit-Gaussian target of the kernels (lnL = lnL - (0.5 x_d) x_d in index order), status 0."""
    lp = 0.0
    for v in q:
        lp = lp - (0.5 * float(v)) * float(v)
    return lp, 0


def gaussian(P):
    out = np.array([gaussian_one(p)[0] for p in P])
    return out, np.zeros(len(P), dtype=np.int32)
