"""numpy restatement of the nested sampler's slice mode (include/magprop_amd.h mp_nested_set_slice): the walk into a dead slot as
`slices` slice updates along survivor differences, with the Philox layout and the unfused arithmetic of the kernel
(magprop_amd/csrc/mp_nest.hip nest_slice_kernel).  The slice update itself is walk_restated.slice_rounds, which the ensemble slice
move shares; the ranking, the volume bookkeeping and the stop rule are nest_restated's.
Test infrastructure: the GPU tests compare the device state with it bit for bit, the CPU tests check with it that a slice walk
leaves the constrained prior invariant.  Every product and sum is a separately rounded float64 operation in the kernel's order."""
import numpy as np

import nest_restated as nr
from moves_restated import pick, pick_skip
from oracle.stretch_oracle import philox4x32_10, u01
from walk_restated import slice_rounds

M32 = 0xFFFFFFFF
SLICE_CTR = 0x4E400000


def slice_draw(seed, t, r, slot, s, c):
    """Philox (seed; t, r, slot, 0x4E400000 + 0x100 s + c)."""
    seed = int(seed)
    return philox4x32_10(seed & M32, seed >> 32, int(t) & M32, int(r), int(slot), SLICE_CTR + 0x100 * int(s) + int(c))


def slice_walk_rounds(x, lnl, st, t, r, slot, surv_pts, lstar, seed, slices, mu, max_steps_out, max_shrink, lower, upper,
                      broken=None):
    """`slices` slice updates of x (a list of floats; lnL lnl, status st) at iteration t, run r, dead slot `slot`, as the kernel's
    rounds: a generator that yields the next point to evaluate (a named point inside the box), is sent its (lnL, status), and
    returns (x, lnl, st, slices moved, evaluations, expansions, contractions, failed slices).  surv_pts[m]: the survivors in
    slot order (the directions).  broken="forward": the negative control of walk_restated.slice_rounds."""
    m, nd = len(surv_pts), len(x)
    moved = n_eval = n_exp = n_con = n_fail = 0
    for s in range(slices):
        u = slice_draw(seed, t, r, slot, s, 0)
        c1 = pick(u01(u[0], u[1]), m)
        c2 = pick_skip(u01(u[2], u[3]), m, c1)
        a, b = surv_pts[c1], surv_pts[c2]
        d = [float(a[k]) - float(b[k]) for k in range(nd)]
        if not any(v != 0.0 for v in d):
            n_fail += 1
            continue
        o = yield from slice_rounds(x, d, mu, max_steps_out, max_shrink, lambda c: slice_draw(seed, t, r, slot, s, c), 2,
                                    lambda lq: lq > lstar, (lower, upper), broken)
        n_eval, n_exp, n_con = n_eval + o.n_eval, n_exp + o.n_exp, n_con + o.n_con
        if o.q is None:
            n_fail += 1
        else:
            x, lnl, st = o.q, o.lnp, o.status
            moved += 1
    return x, lnl, st, moved, n_eval, n_exp, n_con, n_fail


def slice_walk(x, lnl, st, t, r, slot, surv_pts, lstar, seed, slices, mu, max_steps_out, max_shrink, lower, upper, evaluate_one,
               broken=None):
    """slice_walk_rounds, one evaluate_one(q) per round."""
    return nr.one_at_a_time(slice_walk_rounds(x, lnl, st, t, r, slot, surv_pts, lstar, seed, slices, mu, max_steps_out, max_shrink,
                                              lower, upper, broken), evaluate_one)


def start(live0, evaluate, with_runs=False):
    """nest_restated.start with the slice counters (nexpand, ncontract, nfail per run) at 0."""
    s = nr.start(live0, evaluate, with_runs)
    n_runs = s.lnl.shape[0]
    s.nexpand = np.zeros(n_runs, dtype=np.int64)
    s.ncontract = np.zeros(n_runs, dtype=np.int64)
    s.nfail = np.zeros(n_runs, dtype=np.int64)
    return s


def iteration(s, nbatch, seed, slices, mu, max_steps_out, max_shrink, dlogz, lower, upper, evaluate_one=None, evaluate=None):
    """One iteration of every run not stopped, in slice mode (nest_restated.iteration with the slice walk)."""
    jobs = nr.retire(s, nbatch, dlogz)
    where, gens = [], []
    for r, dead, surv, lstar, t in jobs:
        surv_pts = s.live[r, surv].copy()
        for j in dead:
            u = nr.draw(seed, t, r, j, 0)
            fr = surv[pick(u01(u[0], u[1]), len(surv))]
            where.append((r, j))
            gens.append(slice_walk_rounds([float(v) for v in s.live[r, fr]], float(s.lnl[r, fr]), int(s.status[r, fr]), t, r, j,
                                          surv_pts, lstar, seed, slices, mu, max_steps_out, max_shrink, lower, upper))
    out = nr.drive(gens, [r for r, _ in where], evaluate_one, evaluate)
    for (r, j), (x, lq, sq, mv, ne, nx, nc, nf) in zip(where, out):
        s.live[r, j], s.lnl[r, j], s.status[r, j], s.acc[r, j] = x, lq, sq, mv
        s.ncall[r] += ne
        s.nacc[r] += mv
        s.nzero[r] += mv == 0
        s.nexpand[r] += nx
        s.ncontract[r] += nc
        s.nfail[r] += nf
    for r, *_ in jobs:
        s.nit[r] += 1


def run(s, iterations, nbatch, seed, slices, mu=1.0, max_steps_out=8, max_shrink=64, dlogz=0.01, lower=None, upper=None,
        evaluate_one=None, evaluate=None):
    """Up to `iterations` slice-mode iterations and the stop check behind them (mp_nested_run); s is advanced in place."""
    if iterations <= 0 or np.all(s.stopped):
        return s
    for _ in range(iterations):
        if np.all(s.stopped):
            break
        iteration(s, nbatch, seed, slices, mu, max_steps_out, max_shrink, dlogz, lower, upper, evaluate_one, evaluate)
    nr.check_stops(s, dlogz)
    return s
