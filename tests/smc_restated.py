"""numpy restatement of the tempered SMC sampler (include/magprop_amd.h mp_smc_*): the stage (weights, the bisection for the next
beta, ln Z, integer units, systematic resampling in Python integers) and the moves (the Philox draw layout, the DE proposals over
the resampled population with the unfused arithmetic of magprop_amd/csrc/mp_smc.hip, the tempered Metropolis decision).  Test
infrastructure: the GPU tests compare the device state with it bit for bit, the CPU tests check with it that the scheme gives
the evidence and the posterior of a case with a closed form.

Sums are formed in the kernel's order (wg_sum): thread k of 256 adds its particles k, k + 256, ... in order, then the xor
butterfly inside each wavefront and the four wavefronts in order, so that with the device's exp and log handed in (exp=, log=)
every number of a stage is the device's, bit for bit.  The moves of a stage run all slots together, a step at a time: one
evaluate(rows, runs) call per step answers every proposal inside the box, which is how the GPU tests put an mp_lnprob_batch call
of the launch's own size behind every likelihood."""
import math

import numpy as np

from oracle.stretch_oracle import philox4x32_10
from walk_restated import de_step

M32 = 0xFFFFFFFF
CTR = 0x534D0000
RUNNING, DONE, FAILED, STAGE_LIMIT = 0, 1, 2, 3
MAX_STAGES = 1024
WG = 256


def draws(seed, t, r, slots, c):
    """Philox (seed; t, r, slot, 0x534D0000 + c) of every slot of `slots`: four uint64 arrays (the project's generator, on arrays)."""
    seed, n = int(seed), len(slots)
    full = lambda v: np.full(n, int(v), dtype=np.uint64)
    return philox4x32_10(seed & M32, seed >> 32, full(int(t) & M32), full(r), np.asarray(slots, dtype=np.uint64), full(CTR + int(c)))


def u01(hi, lo):
    """The 53-bit uniform of two words, on arrays."""
    return (((hi << np.uint64(32)) | lo) >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def pick(u, m):
    return np.minimum((u * m).astype(np.int64), m - 1)


def pick_skip(u, m, c):
    t = pick(u, m - 1)
    return t + (t >= c)


def wg_sum(v):
    """The sum of v in the order of the stage kernel (smc_sums, then wg_sum of mp_wg.h)."""
    v = np.asarray(v, dtype=np.float64)
    rows = -(-v.size // WG)
    pad = np.zeros(rows * WG)
    pad[:v.size] = v
    acc = np.zeros(WG)
    for row in pad.reshape(rows, WG):
        acc = acc + row
    acc = acc.reshape(WG // 64, 64)
    lane = np.arange(64)
    for dist in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lane ^ dist]
    out = acc[0, 0]
    for w in range(1, WG // 64):
        out = out + acc[w, 0]
    return float(out)


def weights(lnl, big, d, exp=np.exp):
    """w_i(d) = exp(d (lnl_i - M)), 0 where lnl_i is not finite."""
    fin = np.isfinite(lnl)
    w = np.zeros(lnl.size)
    w[fin] = exp(d * (lnl[fin] - big))
    return w


def sums(lnl, big, d, exp=np.exp):
    """(sum w, sum w^2, max w, w) at increment d."""
    w = weights(lnl, big, d, exp)
    return wg_sum(w), wg_sum(w * w), float(np.max(w)), w


def ess_of(s1, s2):
    return (s1 * s1) / s2


def next_increment(lnl, beta, ess, exp=np.exp):
    """(d, last, M, n_fin) of a stage: the increment of beta, whether the new beta is exactly 1, the largest finite lnl and the
    number of finite ones; None where no lnl is finite."""
    fin = np.isfinite(lnl)
    n_fin = int(np.sum(fin))
    if n_fin == 0:
        return None
    big = float(np.max(lnl[fin]))
    target = ess * float(n_fin)
    rem = 1.0 - beta
    if ess_of(*sums(lnl, big, rem, exp)[:2]) >= target:
        return rem, True, big, n_fin
    lo, hi = 0.0, rem
    for _ in range(128):
        mid = 0.5 * (lo + hi)
        if mid == lo or mid == hi:
            break
        if ess_of(*sums(lnl, big, mid, exp)[:2]) >= target:
            lo = mid
        else:
            hi = mid
    return (lo if lo > 0.0 else hi), False, big, n_fin


def units_of(w, wmax):
    """u_i = rint((2^31 w_i) / max w) as Python integers."""
    return [int(v) for v in np.rint((2147483648.0 * w) / wmax)]


def offset(seed, t, r, total):
    """s = floor(u01(r0, r1) * U), one rounded product."""
    k = draws(seed, t, r, [0], 0)
    return int(float(u01(k[0], k[1])[0]) * float(total))


def resample(units, s):
    """Systematic resampling in integers: anc[j] = the least i with C_i > P_j, P_j = floor((j U + s) / N).  Returns (anc, P)."""
    n = len(units)
    cum, run = [], 0
    for u in units:
        run += int(u)
        cum.append(run)
    total = run
    pos = [(j * total + int(s)) // n for j in range(n)]
    anc = np.searchsorted(np.array(cum, dtype=np.int64), np.array(pos, dtype=np.int64), side="right")
    return anc.astype(np.int32), pos


def stage(lnl, beta, lnz, ess, seed, t, r, exp=np.exp, log=math.log, norm_term=True):
    """One stage of a run on its particles' lnl: None where no lnl is finite (FAILED), else a dict of beta, d, ess, lnz, units,
    cum, anc and the increment of ln Z.  norm_term=False drops ln(sum w / N) from ln Z (the tests show that the evidence is
    then wrong)."""
    lnl = np.asarray(lnl, dtype=np.float64)
    inc = next_increment(lnl, float(beta), ess, exp)
    if inc is None:
        return None
    d, last, big, _ = inc
    s1, s2, wmax, w = sums(lnl, big, d, exp)
    units = units_of(w, wmax)
    anc, _ = resample(units, offset(seed, t, r, sum(units)))
    dlnz = d * big + (float(log(s1 / float(lnl.size))) if norm_term else 0.0)
    return {"beta": 1.0 if last else float(beta) + d, "d": d, "ess": ess_of(s1, s2), "lnz": float(lnz) + dlnz, "dlnz": dlnz,
            "units": np.array(units, dtype=np.uint32), "cum": np.cumsum(np.array(units, dtype=np.uint64)), "anc": anc}


def resolve(g0, sigma, ndim):
    """(g0, s3) as the library keeps them."""
    return (g0 if g0 > 0.0 else 2.38 / math.sqrt(2.0 * ndim)), sigma * math.sqrt(3.0)


def _clean(v):
    v = np.array(v, dtype=np.float64)
    v[np.isnan(v)] = -np.inf
    return v


class State:
    """x[n_runs, N, ndim], lnl, status, acc [n_runs, N]; per run beta, lnz, nstage, run_status, ncall, nacc, nfail; anc of the
    last stage [n_runs, N]; log: per run the rows (beta, d, ess, lnz, accept, ncall) of its stages."""

    def __init__(self, x, lnl, status):
        n_runs, n = lnl.shape
        self.x, self.lnl, self.status = x, lnl, status
        self.acc = np.zeros((n_runs, n), dtype=np.int32)
        self.anc = np.zeros((n_runs, n), dtype=np.int32)
        self.beta = np.zeros(n_runs)
        self.lnz = np.zeros(n_runs)
        self.nstage = np.zeros(n_runs, dtype=np.int32)
        self.run_status = np.zeros(n_runs, dtype=np.int32)
        self.ncall = np.full(n_runs, n, dtype=np.int64)
        self.nacc = np.zeros(n_runs, dtype=np.int64)
        self.nfail = np.sum(status != 0, axis=1).astype(np.int64)
        self.log = [[] for _ in range(n_runs)]


def start(x0, evaluate):
    """The particles x0 (n_runs, N, ndim) evaluated: evaluate(rows[n, ndim], runs[n]) -> (lnl, status)."""
    x = np.array(x0, dtype=np.float64)
    n_runs, n, ndim = x.shape
    lnl, st = evaluate(x.reshape(-1, ndim), np.repeat(np.arange(n_runs), n))
    return State(x, _clean(lnl).reshape(n_runs, n), np.asarray(st, dtype=np.int32).reshape(n_runs, n))


def moves(s, jobs, seed, walks, g0, s3, lower, upper, evaluate, log=np.log):
    """The moves of stage t of the runs of jobs = [(r, t)] (their anc and beta are in s), all slots together, a step at a time;
    s is advanced in place.  walks = 0 leaves every slot at its ancestor."""
    if not jobs:
        return
    n, nd = s.lnl.shape[1], s.x.shape[2]
    lower, upper = np.asarray(lower, dtype=np.float64), np.asarray(upper, dtype=np.float64)
    pop = {r: s.x[r][s.anc[r]].copy() for r, _ in jobs}        # the resampled population: fixed during the moves
    cur = {r: pop[r].copy() for r, _ in jobs}
    lcur = {r: s.lnl[r][s.anc[r]].copy() for r, _ in jobs}
    scur = {r: s.status[r][s.anc[r]].copy() for r, _ in jobs}
    nacc = {r: np.zeros(n, dtype=np.int32) for r, _ in jobs}
    slots = np.arange(n)
    for k in range(walks):
        props, lnus, inside = {}, {}, {}
        for r, t in jobs:
            u, v = draws(seed, t, r, slots, 2 * k + 1), draws(seed, t, r, slots, 2 * k + 2)
            c1 = pick(u01(u[0], u[1]), n)
            c2 = pick_skip(u01(u[2], u[3]), n, c1)
            props[r], inside[r] = de_step(cur[r], pop[r][c1], pop[r][c2], g0, s3, u01(v[0], v[1]), lower, upper)
            with np.errstate(divide="ignore"):
                lnus[r] = log(u01(v[2], v[3]))
        rows = np.concatenate([props[r][inside[r]] for r, _ in jobs])
        runs = np.concatenate([np.full(int(np.sum(inside[r])), r) for r, _ in jobs])
        if rows.shape[0] == 0:
            continue
        lq_all, sq_all = evaluate(rows, runs)
        lq_all, sq_all, at = _clean(lq_all), np.asarray(sq_all, dtype=np.int32), 0
        for r, _ in jobs:
            m = int(np.sum(inside[r]))
            lq, sq = lq_all[at:at + m], sq_all[at:at + m]
            at += m
            idx = np.nonzero(inside[r])[0]
            beta = float(s.beta[r])
            with np.errstate(invalid="ignore"):
                ok = (beta * lq - beta * lcur[r][idx]) > lnus[r][idx]
            s.ncall[r] += m
            s.nfail[r] += int(np.sum(sq != 0))
            take = idx[ok]
            cur[r][take], lcur[r][take], scur[r][take] = props[r][take], lq[ok], sq[ok]
            nacc[r][take] += 1
    for r, _ in jobs:
        s.x[r], s.lnl[r], s.status[r], s.acc[r] = cur[r], lcur[r], scur[r], nacc[r]
        s.nacc[r] += int(np.sum(nacc[r]))


def step(s, seed, walks, ess, g0, sigma, lower, upper, evaluate, exp=np.exp, log=math.log, log_u=np.log, norm_term=True):
    """One stage and its moves of every run still running; s is advanced in place."""
    g0, s3 = resolve(g0, sigma, s.x.shape[2])
    jobs = []
    for r in range(s.lnl.shape[0]):
        if s.run_status[r] != RUNNING:
            continue
        if s.nstage[r] >= MAX_STAGES:
            s.run_status[r] = STAGE_LIMIT
            continue
        t = int(s.nstage[r])
        out = stage(s.lnl[r], s.beta[r], s.lnz[r], ess, seed, t, r, exp, log, norm_term)
        if out is None:
            s.run_status[r] = FAILED
            continue
        s.log[r].append([out["beta"], out["d"], out["ess"], out["lnz"], int(s.ncall[r]), int(s.nacc[r])])
        s.beta[r], s.lnz[r], s.anc[r], s.nstage[r] = out["beta"], out["lnz"], out["anc"], t + 1
        if out["beta"] >= 1.0:
            s.run_status[r] = DONE
        jobs.append((r, t))
    moves(s, jobs, seed, walks, g0, s3, lower, upper, evaluate, log_u)


def run(s, stages, seed, walks, ess, g0, sigma, lower, upper, evaluate, **kw):
    """Up to `stages` stages (mp_smc_run); s is advanced in place."""
    for _ in range(stages):
        if not np.any(s.run_status == RUNNING):
            break
        step(s, seed, walks, ess, g0, sigma, lower, upper, evaluate, **kw)
    return s


def stages_of(s, r, n, walks):
    """The log of run r as mp_smc_get_stages returns it: beta, d, ess, lnz, accept, ncall per stage."""
    rows = s.log[r]
    cnt = [(row[4], row[5]) for row in rows] + [(int(s.ncall[r]), int(s.nacc[r]))]
    f = lambda k: np.array([row[k] for row in rows], dtype=np.float64)
    accept = np.array([(cnt[k + 1][1] - cnt[k][1]) / (float(n) * float(walks)) for k in range(len(rows))])
    ncall = np.array([cnt[k + 1][0] - cnt[k][0] for k in range(len(rows))], dtype=np.int64)
    return f(0), f(1), f(2), f(3), accept, ncall


def gaussian(rows, runs=None):
    """The unit-Gaussian target of the kernels (lnl = lnl - (0.5 x_d) x_d in index order), status 0."""
    rows = np.asarray(rows, dtype=np.float64)
    lp = np.zeros(rows.shape[0])
    for d in range(rows.shape[1]):
        lp = lp - (0.5 * rows[:, d]) * rows[:, d]
    return lp, np.zeros(rows.shape[0], dtype=np.int32)


def box_lnz(a, ndim):
    """ln Z of exp(-0.5 |x|^2) under the uniform prior on [-a, a]^ndim."""
    return ndim * math.log(math.sqrt(2.0 * math.pi) * math.erf(a / math.sqrt(2.0)) / (2.0 * a))
