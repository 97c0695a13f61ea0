"""numpy restatement of the sampler's Gaussian (Metropolis) and walk moves (include/magprop_amd.h MP_MOVE_GAUSSIAN, MP_MOVE_WALK;
magprop_amd/csrc/mp_normal.hip): Floyd's subset and the walk proposal, the Gaussian proposal in its three modes, the tune rule,
and a step loop that runs the steps of these two moves here and hands every other move of a mixture, one step at a time, to
tests/sampler_restated.py.  Test infrastructure: the GPU tests compare the device chains with the loop (decisions and the rational
tune state exactly, positions to the accuracy of the device's log / sqrt / cos / sin), the CPU tests draw their statistics from it.
Every product and sum is a separately rounded float64 operation in the kernel's order; the proposals of a half-step are formed
for all its walkers at once (the other half stands still during a half-step), with a Philox over arrays that
tests/test_moves_normal_cpu.py holds to oracle.stretch_oracle's."""
import math
from typing import NamedTuple

import numpy as np

import sampler_restated
from kde_restated import TWO_PI, kernel_sum
from moves_restated import draw_move, pick, resolve
from oracle.stretch_oracle import gaussian_lnprob, philox4x32_10, split, u01

M32 = 0xFFFFFFFF
GAUSSIAN, WALK = 5, 6                     # MP_MOVE_GAUSSIAN, MP_MOVE_WALK
WALK_MAX_S = 64                           # MP_WALK_MAX_S
VECTOR, RANDOM, SEQUENTIAL = 0, 1, 2      # MP_GAUSS_*
GAUSS_CTR = 0x47410000                    # axis and ln u; + 1 + p: normals 2p, 2p + 1
WALK_CTR = 0x57410000                     # ln u
WALK_MEMBER_CTR = 0x57410100              # + i // 2: Floyd's draws
WALK_NORMAL_CTR = 0x57800000              # + p: normals 2p, 2p + 1


def philox_batch(seed, step, half, k, c3):
    """philox4x32_10(seed; step, half, k, c3) over arrays k and c3 (broadcast against each other): four uint64 arrays."""
    k, c3 = np.broadcast_arrays(np.asarray(k, dtype=np.uint64), np.asarray(c3, dtype=np.uint64))
    m32 = np.uint64(M32)
    c0 = np.full(k.shape, int(step) & M32, dtype=np.uint64)
    c1 = np.full(k.shape, int(half), dtype=np.uint64)
    c2, c3 = k.copy(), c3.copy()
    k0, k1 = int(seed) & M32, int(seed) >> 32
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0)) & m32, p1 & m32, ((p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)) & m32, p0 & m32
        k0 = (k0 + 0x9E3779B9) & M32
        k1 = (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def u01_batch(hi, lo):
    return (((hi << np.uint64(32)) | lo) >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def normals(seed, step, half, ks, count, ctr):
    """Standard normals [len(ks), count] by the KDE move's Box-Muller formula, pair p from Philox(...; ctr + p)."""
    pairs = (count + 1) // 2
    s = philox_batch(seed, step, half, np.asarray(ks)[:, None], ctr + np.arange(pairs)[None, :])
    rad = np.sqrt(-2.0 * np.log(1.0 - u01_batch(s[0], s[1])))
    ang = TWO_PI * u01_batch(s[2], s[3])
    n = np.empty((len(ks), 2 * pairs))
    n[:, 0::2], n[:, 1::2] = rad * np.cos(ang), rad * np.sin(ang)
    return n[:, :count]


def log_u(seed, step, half, ks, ctr):
    """(ln u01(r2, r3), u01(r0, r1)) of r = Philox(...; ctr) for the walkers ks."""
    r = philox_batch(seed, step, half, np.asarray(ks), ctr)
    with np.errstate(divide="ignore"):
        return np.log(u01_batch(r[2], r[3])), u01_batch(r[0], r[1])


def floyd_draws(seed, step, half, k, n_comp, s):
    """Floyd's raw draws for walker k: t_i = pick(u_i, n_comp - s + i + 1), u_i from the words (0, 1) for even i, (2, 3) for odd i,
    of Philox(...; 0x57410100 + i // 2)."""
    seed = int(seed)
    out = []
    for i in range(s):
        if i % 2 == 0:
            r = philox4x32_10(seed & M32, seed >> 32, int(step) & M32, int(half), int(k), WALK_MEMBER_CTR + i // 2)
        out.append(pick(u01(r[0], r[1]) if i % 2 == 0 else u01(r[2], r[3]), n_comp - s + i + 1))
    return out


def floyd(seed, step, half, k, n_comp, s):
    """s distinct slots of range(n_comp) for walker k by Floyd's algorithm, in the order they are drawn: member_i = t_i unless
    that is a member already, then j = n_comp - s + i."""
    mem = []
    for i, t in enumerate(floyd_draws(seed, step, half, k, n_comp, s)):
        mem.append(n_comp - s + i if t in mem else t)
    return mem


def resolve_s(p0, n_comp):
    """The members per proposal the library keeps for params[0]: 0 is all of the other half."""
    return n_comp if p0 == 0 else int(p0)


def walk_proposals(pos, ks, comp, seed, step, half, s, waves=0):
    """(proposals [len(ks), ndim], ln u, member slots [len(ks), s]) of the walkers ks of one ensemble; comp = global indices of
    the other half in split order, s resolved (2 .. n_comp).  waves > 0: both sums in the kernel's order on a workgroup of that
    many wavefronts (kde_restated.kernel_sum); 0: in member order."""
    n_comp, comp = len(comp), np.asarray(comp)
    assert 2 <= s <= n_comp and (s == n_comp or s <= WALK_MAX_S)
    if s == n_comp:
        mem = np.tile(np.arange(n_comp), (len(ks), 1))
    else:
        mem = np.array([floyd(seed, step, half, k, n_comp, s) for k in ks])
    total = (lambda t: kernel_sum(t, waves)) if waves else (lambda t: np.add.accumulate(t, axis=0)[-1])
    x = pos[comp[mem]].transpose(1, 0, 2)                      # [s, walkers, ndim]
    z = normals(seed, step, half, ks, s, WALK_NORMAL_CTR)     # [walkers, s]
    m = total(x) / float(s)
    t = total(z.T[:, :, None] * (x - m[None]))
    q = pos[np.asarray(ks)] + t / math.sqrt(s - 1.0)
    return q, log_u(seed, step, half, ks, WALK_CTR)[0], mem


def gauss_proposals(pos, ks, seed, step, half, L, mode, sigma):
    """(proposals, ln u) of the walkers ks; L[ndim, ndim] lower triangular, sigma[len(ks)] the scale of each walker's ensemble."""
    d = pos.shape[1]
    x = pos[np.asarray(ks)]
    logu, ua = log_u(seed, step, half, ks, GAUSS_CTR)
    sigma = np.asarray(sigma, dtype=np.float64)
    if mode == VECTOR:
        n = normals(seed, step, half, ks, d, GAUSS_CTR + 1)
        q = np.empty_like(x)
        for a in range(d):
            s = np.zeros(len(ks))
            for b in range(a + 1):
                s = s + L[a, b] * n[:, b]
            q[:, a] = x[:, a] + sigma * s
        return q, logu
    n0 = normals(seed, step, half, ks, 1, GAUSS_CTR + 1)[:, 0]
    axis = np.array([pick(u, d) for u in ua]) if mode == RANDOM else np.full(len(ks), (int(step) & M32) % d)
    q = x.copy()
    rows = np.arange(len(ks))
    q[rows, axis] = x[rows, axis] + sigma * (np.diag(L)[axis] * n0)
    return q, logu


def tune(sigma, n_tuned, accepted, n_walkers, target):
    """One update of the scale: sigma (1 + g (f - 1)), f = (r + t) / (2 t), g = 8 / (8 + n_tuned), r = accepted / n_walkers."""
    r = float(int(accepted)) / float(n_walkers)
    f = (r + target) / (2.0 * target)
    g = 8.0 / (8.0 + float(int(n_tuned)))
    return float(sigma) * (1.0 + g * (f - 1.0))


class Gauss(NamedTuple):
    """What mp_sampler_set_gaussian takes."""
    L: np.ndarray            # [ndim, ndim] lower triangular
    mode: int = VECTOR
    target: float = 0.25


class State:
    """What the Gaussian move keeps per ensemble between steps (and calls)."""

    def __init__(self, n_ensembles, scale0):
        self.sigma = np.full(n_ensembles, float(scale0))
        self.n_tuned = np.zeros(n_ensembles, dtype=np.int64)
        self.n_proposed = np.zeros(n_ensembles, dtype=np.int64)
        self.n_accepted = np.zeros(n_ensembles, dtype=np.int64)

    def stats(self):
        return {k: getattr(self, k).copy() for k in ("sigma", "n_proposed", "n_accepted", "n_tuned")}


class Run(NamedTuple):
    chain: np.ndarray        # (n_steps, n_total, ndim), the rows after the step's swaps
    lnp: np.ndarray          # (n_steps, n_total)
    acc: np.ndarray          # (n_total,)
    drawn: np.ndarray        # (n_steps,) index of the step's move in the table
    accepted: np.ndarray     # (n_steps, n_total) the walker's proposal of that step was accepted
    sigma: np.ndarray        # (n_steps, n_ensembles) the Gaussian scales behind every step (NaN without the move)
    swaps: np.ndarray        # (n_groups, n_temps - 1) accepted swaps of this call; (0, 0) without a swap sweep
    state: State             # None without a Gaussian entry


def gaussian_rows(x):
    """oracle.stretch_oracle.gaussian_lnprob of every row, the same operations in the same order."""
    lnp = np.zeros(len(x))
    for d in range(x.shape[1]):
        lnp = lnp - (0.5 * x[:, d]) * x[:, d]
    return lnp


def entry(table, kind):
    """Index of the table's entry of that kind (None: none)."""
    at = [m for m, t in enumerate(table) if t[0] == kind]
    return at[0] if at else None


def run(pos, n_steps, seed, table, gauss=None, lnprob_fn=gaussian_lnprob, n_ensembles=1, step0=0, lnp=None, acc=None, betas=None,
        n_temps=0, state=None, waves=0):
    """The step loop of mp_sampler_run for a table [(kind, weight, p0, p1)] with Gaussian (GAUSSIAN, w, scale0, tune_steps) and /
    or walk (WALK, w, s, 0) entries; gauss: the Gauss of mp_sampler_set_gaussian.  Decision: beta lnprob(q) - beta lnprob(x) > ln u.
    state: the Gaussian move's State of an earlier call (to continue a run from step0 with lnp / acc), advanced in place; None: a
    fresh one.  waves: the wavefronts of the launch's workgroup (walk_proposals).  pos, and lnp / acc where given, are advanced in
    place."""
    n_total, ndim = pos.shape
    n = n_total // n_ensembles
    half_n = n // 2
    n_comp = n - half_n
    _, cum = resolve(table, ndim)
    g_at = entry(table, GAUSSIAN)
    assert sum(t[0] == GAUSSIAN for t in table) <= 1 and (g_at is None or gauss is not None)
    if g_at is not None and state is None:
        state = State(n_ensembles, table[g_at][2])
    tempered = betas is not None and n_temps > 1
    rows_lnprob = gaussian_rows if lnprob_fn is gaussian_lnprob else (lambda x: np.array([lnprob_fn(p) for p in x]))
    if lnp is None:
        lnp = rows_lnprob(pos)
    if acc is None:
        acc = np.zeros(n_total, dtype=np.int64)
    beta_of = np.ones(n_ensembles) if betas is None else np.asarray(betas, dtype=np.float64)
    chain = np.empty((n_steps, n_total, ndim))
    chain_lnp = np.empty((n_steps, n_total))
    accepted = np.zeros((n_steps, n_total), dtype=bool)
    drawn = np.empty(n_steps, dtype=np.int64)
    sigmas = np.full((n_steps, n_ensembles), np.nan)
    swaps = np.zeros((n_ensembles // n_temps, n_temps - 1) if tempered else (0, 0), dtype=np.int64)
    for s in range(n_steps):
        step = step0 + s
        m = drawn[s] = draw_move(seed, step, cum)
        kind = table[m][0]
        if kind not in (GAUSSIAN, WALK):   # another move of the mixture: one step of the restated sampler (its swap sweep included)
            r = sampler_restated.run(pos, 1, seed, table, lnprob_fn=lnprob_fn, n_ensembles=n_ensembles, step0=step, lnp=lnp, acc=acc,
                                     betas=betas, n_temps=n_temps)
            swaps += r.swaps
            accepted[s] = r.accepted[0]
            chain[s], chain_lnp[s] = pos, lnp
            if state is not None:
                sigmas[s] = state.sigma
            continue
        perms = [split(seed, step, e, n) for e in range(n_ensembles)]
        for half in range(2):
            active = [np.array([e * n + perms[e][half * half_n + slot] for slot in range(half_n)]) for e in range(n_ensembles)]
            ks = np.concatenate(active)
            if kind == GAUSSIAN:
                q, logu = gauss_proposals(pos, ks, seed, step, half, gauss.L, gauss.mode, state.sigma[ks // n])
            else:
                parts = []
                for e in range(n_ensembles):
                    comp = [e * n + perms[e][(1 - half) * half_n + c] for c in range(n_comp)]
                    parts.append(walk_proposals(pos, active[e], comp, seed, step, half, resolve_s(table[m][2], n_comp), waves)[:2])
                q, logu = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
            new = rows_lnprob(q)
            new[np.isnan(new)] = -np.inf
            b = beta_of[ks // n]
            with np.errstate(invalid="ignore"):
                ok = b * new - b * lnp[ks] > logu
            pos[ks[ok]], lnp[ks[ok]] = q[ok], new[ok]
            acc[ks[ok]] += 1
            accepted[s, ks[ok]] = True
        if kind == GAUSSIAN:
            tune_steps = int(table[g_at][3])
            for e in range(n_ensembles):
                a = int(np.sum(accepted[s, e * n:(e + 1) * n]))
                state.n_proposed[e] += n
                state.n_accepted[e] += a
                if state.n_tuned[e] < tune_steps:
                    state.sigma[e] = tune(state.sigma[e], state.n_tuned[e], a, n, gauss.target)
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
        chain[s], chain_lnp[s] = pos, lnp
        if state is not None:
            sigmas[s] = state.sigma
    return Run(chain, chain_lnp, acc, drawn, accepted, sigmas, swaps, state)
