"""numpy restatement of the differential-evolution optimizer (include/magprop_amd.h mp_optimizer_*): scipy's deferred-updating
DE with the draw layout, the unfused arithmetic and the stop rule of the kernels (magprop_amd/csrc/mp_opt.hip).  Test
infrastructure: the CPU tests check with it that the scheme minimises, the GPU tests compare the device state with it bit for
bit.  Every product and sum is a separately rounded float64 operation in the kernel's order (Python floats)."""
import math

import numpy as np

from moves_restated import pick, pick_skip, pick_skip2
from oracle.stretch_oracle import philox4x32_10, u01

M32 = 0xFFFFFFFF
BEST1BIN, RAND1BIN = 0, 1           # MP_DE_*


def uniform(seed, gen, pop, member, j):
    """u_j of member `member` of population `pop` in generation `gen`: Philox (seed; gen, pop, member, 0xDE00 + j // 2)."""
    seed, gen, pop, member, j = int(seed), int(gen), int(pop), int(member), int(j)   # (Python ints: Philox's products are 64-bit)
    r = philox4x32_10(seed & M32, seed >> 32, gen & M32, pop, member, 0xDE00 + (j >> 1))
    return u01(r[2], r[3]) if j & 1 else u01(r[0], r[1])


def dither(seed, gen, f_lo, f_hi):
    """F of generation `gen`: f_lo + (f_hi - f_lo) u01(r0, r1), r = Philox (seed; gen, 0xFFFF, 0, 0xDEFF)."""
    r = philox4x32_10(seed & M32, seed >> 32, gen & M32, 0xFFFF, 0, 0xDEFF)
    return f_lo + (f_hi - f_lo) * u01(r[0], r[1])


def partners(seed, gen, pop, i, popsize):
    """The three distinct members r0, r1, r2 (indices inside the population), none of them i."""
    m = popsize - 1
    a0 = pick(uniform(seed, gen, pop, i, 0), m)
    a1 = pick_skip(uniform(seed, gen, pop, i, 1), m, a0)
    a2 = pick_skip2(uniform(seed, gen, pop, i, 2), m, a0, a1)
    return tuple(a + (a >= i) for a in (a0, a1, a2))


def fill_point(seed, gen, pop, i, ndim):
    return pick(uniform(seed, gen, pop, i, 3), ndim)


def trial(X, best, seed, gen, pop, i, strategy, F, cr, lower, upper):
    """Trial vector of member i of population X (popsize, ndim) of population number `pop`; best = index of its best member."""
    popsize, ndim = X.shape
    r0, r1, r2 = partners(seed, gen, pop, i, popsize)
    xb, x1, x2 = (X[best], X[r0], X[r1]) if strategy == BEST1BIN else (X[r0], X[r1], X[r2])
    fill = fill_point(seed, gen, pop, i, ndim)
    t = np.empty(ndim)
    for d in range(ndim):
        if d == fill or uniform(seed, gen, pop, i, 4 + d) < cr:
            v = float(xb[d]) + F * (float(x1[d]) - float(x2[d]))
        else:
            v = float(X[i, d])
        if not (lower[d] <= v <= upper[d]):
            v = float(lower[d]) + uniform(seed, gen, pop, i, 4 + ndim + d) * (float(upper[d]) - float(lower[d]))
        t[d] = v
    return t


def reduce(lnp, tol, atol):
    """(best index, converged) of one population's lnprob: largest lnprob, lowest index on ties; std(E) <= atol + tol |mean(E)|,
    E = -lnprob, population std with sums in member order; any -inf means not converged."""
    n = len(lnp)
    b = 0
    for i in range(n):
        if lnp[i] > lnp[b]:
            b = i
    finite = all(v > -math.inf for v in lnp)
    s = 0.0
    for v in lnp:
        s = s + (-float(v))
    mean = s / n
    q = 0.0
    for v in lnp:
        e = -float(v) - mean
        q = q + e * e
    sd = math.sqrt(q / n)
    return b, bool(finite and sd <= atol + tol * abs(mean))


def gaussian(P):
    """The unit-Gaussian target of the kernels (lnp = lnp - (0.5 x_d) x_d in index order) and status 0 for every row."""
    out = np.empty(len(P))
    for k, p in enumerate(P):
        lp = 0.0
        for v in p:
            lp = lp - (0.5 * float(v)) * float(v)
        out[k] = lp
    return out, np.zeros(len(P), dtype=np.int32)


class State:
    """pop[n_pops, popsize, ndim], lnp[n_pops, popsize], status, best[n_pops], nit, converged, nfev."""

    def __init__(self, pop, lnp, status):
        n_pops, popsize = pop.shape[:2]
        self.pop, self.lnp, self.status = pop, lnp, status
        self.best = np.zeros(n_pops, dtype=np.int32)
        self.nit = np.zeros(n_pops, dtype=np.int32)
        self.converged = np.zeros(n_pops, dtype=np.int32)
        self.nfev = np.full(n_pops, popsize, dtype=np.int64)


def _evaluate(evaluate, rows):
    lnp, st = evaluate(rows)
    lnp = np.where(np.isnan(lnp), -np.inf, lnp)
    return lnp, np.asarray(st, dtype=np.int32)


def start(pop0, evaluate, tol=0.01, atol=0.0):
    """Generation 0 of pop0 (n_pops, popsize, ndim): evaluate(rows[n_total, ndim]) -> (lnprob, status) over the WHOLE batch."""
    pop = np.array(pop0, dtype=np.float64)
    n_pops, popsize, ndim = pop.shape
    lnp, st = _evaluate(evaluate, pop.reshape(-1, ndim))
    s = State(pop, lnp.reshape(n_pops, popsize), st.reshape(n_pops, popsize))
    for p in range(n_pops):
        s.best[p] = reduce(s.lnp[p], tol, atol)[0]
    return s


def generation(s, gen, evaluate, seed, strategy=BEST1BIN, f_lo=0.5, f_hi=1.0, cr=0.7, tol=0.01, atol=0.0, lower=None, upper=None):
    """Generation `gen` (>= 1) of every population that has not converged; the batch handed to `evaluate` holds every member
    (the trials, and the members of converged populations as they are), as the device launch does."""
    n_pops, popsize, ndim = s.pop.shape
    F = dither(seed, gen, f_lo, f_hi)
    T = s.pop.copy()
    for p in range(n_pops):
        if not s.converged[p]:
            for i in range(popsize):
                T[p, i] = trial(s.pop[p], s.best[p], seed, gen, p, i, strategy, F, cr, lower, upper)
    lnp, st = _evaluate(evaluate, T.reshape(-1, ndim))
    lnp, st = lnp.reshape(n_pops, popsize), st.reshape(n_pops, popsize)
    for p in range(n_pops):
        if s.converged[p]:
            continue
        take = lnp[p] >= s.lnp[p]
        s.pop[p][take] = T[p][take]
        s.lnp[p][take] = lnp[p][take]
        s.status[p][take] = st[p][take]
        s.best[p], c = reduce(s.lnp[p], tol, atol)
        s.converged[p] = int(c)
        s.nit[p] += 1
        s.nfev[p] += popsize
    return s


def run(pop0, generations, evaluate, seed, strategy=BEST1BIN, f_lo=0.5, f_hi=1.0, cr=0.7, tol=0.01, atol=0.0, lower=None,
        upper=None):
    """Generation 0 and then `generations` generations (converged populations frozen); returns the State."""
    s = start(pop0, evaluate, tol, atol)
    for g in range(1, generations + 1):
        if np.all(s.converged):
            break
        generation(s, g, evaluate, seed, strategy, f_lo, f_hi, cr, tol, atol, lower, upper)
    return s
