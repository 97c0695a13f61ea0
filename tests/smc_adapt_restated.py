"""numpy restatement of the adaptive moves of the tempered SMC sampler (include/magprop_amd.h mp_smc_set_adaptive): on top of
tests/smc_restated.py, whose stage it takes as it is, the rounds of `walks` steps (round 0 from the ancestors, every later
round in place, the partners always drawn over the stage's resampled population, the steps' draws counted across the rounds),
the tune rule behind every round in the kernel's summation order (magprop_amd/csrc/mp_smc.hip smc_tune_kernel), and the scale
update at the round that stops.  Test infrastructure: the GPU tests compare the device with it bit for bit, handing in the
device's exp and log as they do for smc_restated."""
import math

import numpy as np

import smc_restated as sm


class Adapt:
    """The settings of mp_smc_set_adaptive as the library keeps them (g_min, g_max <= 0: g0 / 16 and 4 g0)."""

    def __init__(self, g0, min_rounds=1, max_rounds=16, corr=0.2, gain=1.0, accept_target=0.234, g_min=0.0, g_max=0.0):
        self.min_rounds, self.max_rounds, self.corr, self.gain, self.accept_target = min_rounds, max_rounds, corr, gain, accept_target
        self.g_min = g_min if g_min > 0.0 else g0 / 16.0
        self.g_max = g_max if g_max > 0.0 else 4.0 * g0


def rho_of(a, b):
    """rho_d of one dimension between a (where the slots started) and b (where they are): two passes, the means first, then
    the centred values scaled by the power of two 2^-ilogb(their largest size) and their sums Saa, Sbb, Sab in the order of
    sm.wg_sum.  1.0 where b has not spread (min b = max b: Sbb = 0), else 0.0 where a is one point (min a = max a: Saa = 0)."""
    n = float(a.size)
    if np.min(b) == np.max(b):
        return 1.0
    if np.min(a) == np.max(a):
        return 0.0
    da, db = a - sm.wg_sum(a) / n, b - sm.wg_sum(b) / n
    ha, hb = float(np.max(np.abs(da))), float(np.max(np.abs(db)))
    u, v = np.ldexp(da, 1 - math.frexp(ha)[1]), np.ldexp(db, 1 - math.frexp(hb)[1])
    saa, sbb, sab = sm.wg_sum(u * u), sm.wg_sum(v * v), sm.wg_sum(u * v)
    return sab / math.sqrt(saa * sbb)


def tune(start, now, acc, walks, made, g, cfg, exp=np.exp):
    """The tune kernel behind the round that made the stage's rounds `made`: (rho_d[ndim], rho, go_on, the next g).  The next g
    is the run's scale for the next stage where the round stops (go_on False) and g itself where it does not."""
    start, now = np.asarray(start, dtype=np.float64), np.asarray(now, dtype=np.float64)
    n, nd = now.shape
    rho_d = np.array([rho_of(start[:, d], now[:, d]) for d in range(nd)])
    rho = -math.inf
    for v in rho_d:
        if v > rho or v != v:
            rho = float(v)
    go_on = made < cfg.min_rounds or (not rho <= cfg.corr and made < cfg.max_rounds)
    if go_on:
        return rho_d, rho, True, g
    share = float(int(np.sum(acc, dtype=np.int64))) / (float(n) * float(made * walks))
    step = float(np.asarray(exp(np.array([cfg.gain * (share - cfg.accept_target)])))[0])
    return rho_d, rho, False, min(max(g * step, cfg.g_min), cfg.g_max)


def round_of(s, jobs, pop, first, walks, g, s3, seed, lower, upper, evaluate, log=np.log):
    """One round of the runs of jobs = [(r, t)]: `walks` steps of every slot in place from s.x, s.lnl, s.status, the steps first ..
    first + walks - 1 of stage t (their draws), partners over pop[r] (the stage's resampled population, fixed), scale g[r];
    all slots together, a step at a time, one evaluate call per step as in sm.moves.  s.acc grows by the round's accepted steps."""
    n = s.lnl.shape[1]
    slots = np.arange(n)
    for k in range(first, first + walks):
        props, lnus, inside = {}, {}, {}
        for r, t in jobs:
            u, v = sm.draws(seed, t, r, slots, 2 * k + 1), sm.draws(seed, t, r, slots, 2 * k + 2)
            c1 = sm.pick(sm.u01(u[0], u[1]), n)
            c2 = sm.pick_skip(sm.u01(u[2], u[3]), n, c1)
            props[r], inside[r] = sm.de_step(s.x[r], pop[r][c1], pop[r][c2], g[r], s3, sm.u01(v[0], v[1]), lower, upper)
            with np.errstate(divide="ignore"):
                lnus[r] = log(sm.u01(v[2], v[3]))
        rows = np.concatenate([props[r][inside[r]] for r, _ in jobs])
        runs = np.concatenate([np.full(int(np.sum(inside[r])), r) for r, _ in jobs])
        if rows.shape[0] == 0:
            continue
        lq_all, sq_all = evaluate(rows, runs)
        lq_all, sq_all, at = sm._clean(lq_all), np.asarray(sq_all, dtype=np.int32), 0
        for r, _ in jobs:
            m = int(np.sum(inside[r]))
            lq, sq = lq_all[at:at + m], sq_all[at:at + m]
            at += m
            idx = np.nonzero(inside[r])[0]
            beta = float(s.beta[r])
            with np.errstate(invalid="ignore"):
                ok = (beta * lq - beta * s.lnl[r][idx]) > lnus[r][idx]
            take = idx[ok]
            s.x[r][take], s.lnl[r][take], s.status[r][take] = props[r][take], lq[ok], sq[ok]
            s.acc[r][take] += 1
            s.ncall[r] += m
            s.nacc[r] += int(np.sum(ok))
            s.nfail[r] += int(np.sum(sq != 0))


def begin(s, g0, sigma):
    """The adaptive part of a state made by sm.start: g per run, and per run the rows (rounds, g used, rho) of its stages."""
    g0r, _ = sm.resolve(g0, sigma, s.x.shape[2])
    s.g = np.full(s.lnl.shape[0], g0r)
    s.tune = [[] for _ in range(s.lnl.shape[0])]
    return s


def step(s, seed, walks, ess, g0, sigma, lower, upper, evaluate, cfg, exp=np.exp, log=math.log, log_u=np.log, norm_term=True):
    """One stage of every run still running and its rounds; s (begun by begin) is advanced in place."""
    _, s3 = sm.resolve(g0, sigma, s.x.shape[2])
    lower, upper = np.asarray(lower, dtype=np.float64), np.asarray(upper, dtype=np.float64)
    before = s.nstage.copy()
    # the stage itself, every slot left at its ancestor: sm.step with moves of no step
    sm.step(s, seed, 0, ess, g0, sigma, lower, upper, evaluate, exp=exp, log=log, log_u=log_u, norm_term=norm_term)
    moving = [(r, int(before[r])) for r in range(s.lnl.shape[0]) if s.nstage[r] != before[r]]
    pop = {r: s.x[r].copy() for r, _ in moving}
    for k in range(cfg.max_rounds):
        if not moving:
            break
        round_of(s, moving, pop, k * walks, walks, s.g, s3, seed, lower, upper, evaluate, log_u)
        still = []
        for r, t in moving:
            _, rho, go_on, g_next = tune(pop[r], s.x[r], s.acc[r], walks, k + 1, float(s.g[r]), cfg, exp)
            if go_on:
                still.append((r, t))
            else:
                s.tune[r].append([k + 1, float(s.g[r]), rho])
                s.g[r] = g_next
        moving = still


def run(s, stages, seed, walks, ess, g0, sigma, lower, upper, evaluate, cfg, **kw):
    """Up to `stages` adaptive stages (mp_smc_run); s is advanced in place."""
    for _ in range(stages):
        if not np.any(s.run_status == sm.RUNNING):
            break
        step(s, seed, walks, ess, g0, sigma, lower, upper, evaluate, cfg, **kw)
    return s


def stages_of(s, r, n, walks):
    """sm.stages_of with the accepted share over the steps the stage made (walks x its rounds)."""
    beta, d, ess, lnz, accept, ncall = sm.stages_of(s, r, n, walks)
    rounds = np.array([row[0] for row in s.tune[r]], dtype=np.float64)
    rows = s.log[r]
    cnt = [row[5] for row in rows] + [int(s.nacc[r])]
    accept = np.array([(cnt[k + 1] - cnt[k]) / (float(n) * float(walks * int(rounds[k]))) for k in range(len(rows))])
    return beta, d, ess, lnz, accept, ncall


def tuning_of(s, r):
    """The tuning log of run r as mp_smc_get_tuning returns it: rounds, g, rho per stage."""
    rows = s.tune[r]
    return (np.array([row[0] for row in rows], dtype=np.int32), np.array([row[1] for row in rows], dtype=np.float64),
            np.array([row[2] for row in rows], dtype=np.float64))
