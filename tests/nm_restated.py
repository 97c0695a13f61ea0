"""numpy restatement of the Nelder-Mead simplex search (include/magprop_amd.h mp_simplex_*): scipy's minimize(method=
"Nelder-Mead") with bounds in the speculative form of the kernels (magprop_amd/csrc/mp_nm.hip) -- all N + 4 candidates of an
iteration evaluated in one batch, then scipy's decision tree, a stable sort and the stop rule.  Test infrastructure: the CPU
tests hold it against scipy bit for bit, the GPU tests compare the device state with it bit for bit.  Every product, sum and
division is a separately rounded float64 operation in the kernel's order (numpy element-wise operations over the simplexes)."""
import numpy as np

REFLECT, EXPAND, OUTSIDE, INSIDE, SHRINK = range(5)     # the columns of the outcome counters


def coefficients(ndim, adaptive=False):
    """(rho, chi, psi, sigma) as scipy sets them."""
    if adaptive:
        dim = float(ndim)
        return 1.0, 1 + 2 / dim, 0.75 - 1 / (2 * dim), 1 - 1 / dim
    return 1.0, 2.0, 0.5, 0.5


def default_simplex(x0, lower=None, upper=None):
    """scipy's initial simplex around x0 (clipped into the box first): vertex k + 1 moves coordinate k by 5 %, or to 0.00025
    where it is zero."""
    x0 = np.asarray(x0, dtype=np.float64)
    if lower is not None:
        x0 = np.clip(x0, lower, upper)
    sim = np.tile(x0, (x0.size + 1, 1))
    for k in range(x0.size):
        sim[k + 1, k] = (1 + 0.05) * x0[k] if x0[k] != 0 else 0.00025
    return sim


def into_box(sim, lower, upper):
    """scipy's rule for vertices outside the box: a coordinate above upper is reflected (2 upper - x), then everything is clipped."""
    sim = np.asarray(sim, dtype=np.float64)
    return np.clip(np.where(sim > upper, 2 * upper - sim, sim), lower, upper)


def gaussian(P):
    """Target 1, the unit Gaussian of the kernels (lnp = lnp - (0.5 x_d) x_d in index order), and status 0 for every row."""
    P = np.asarray(P, dtype=np.float64)
    lp = np.zeros(len(P))
    for d in range(P.shape[1]):
        lp = lp - (0.5 * P[:, d]) * P[:, d]
    return lp, np.zeros(len(P), dtype=np.int32)


def terraced(P):
    """Target 2: the unit Gaussian minus 1e-3 floor(37 x_0): plateaus and ties."""
    P = np.asarray(P, dtype=np.float64)
    lp, st = gaussian(P)
    return lp - 1.0e-3 * np.floor(37.0 * P[:, 0]), st


def candidates(sim, rho, chi, psi, sigma, lower, upper):
    """[n, N + 4, N] from the sorted simplexes sim[n, N + 1, N]: reflection, expansion, outside contraction, inside contraction,
    the N shrunk vertices."""
    n, nv, N = sim.shape
    xbar = sim[:, 0].copy()
    for j in range(1, N):
        xbar = xbar + sim[:, j]
    xbar = xbar / float(N)
    worst, best = sim[:, N], sim[:, 0]
    rc, pr = rho * chi, psi * rho
    out = np.empty((n, N + 4, N))
    out[:, 0] = (1 + rho) * xbar - rho * worst
    out[:, 1] = (1 + rc) * xbar - rc * worst
    out[:, 2] = (1 + pr) * xbar - pr * worst
    out[:, 3] = (1 - psi) * xbar + psi * worst
    for j in range(1, nv):
        out[:, 3 + j] = best + sigma * (sim[:, j] - best)
    return np.minimum(np.maximum(out, lower), upper)


def stop_rule(sim, lnp, xatol, fatol):
    """scipy's test on one sorted simplex, every term <= (a NaN difference means go on)."""
    with np.errstate(invalid="ignore"):
        f = -lnp
        return bool(np.all(np.abs(sim[1:] - sim[0]) <= xatol) and np.all(np.abs(f[0] - f[1:]) <= fatol))


class State:
    """sim[n, N + 1, N] sorted, lnp[n, N + 1], status[n, N + 1], nit, stopped, nfev [n], outcomes[n, 5]."""

    def __init__(self, sim):
        n, nv, _ = sim.shape
        self.sim = sim
        self.lnp = np.empty((n, nv))
        self.status = np.zeros((n, nv), dtype=np.int32)
        self.nit = np.ones(n, dtype=np.int32)
        self.stopped = np.zeros(n, dtype=np.int32)
        self.nfev = np.full(n, nv, dtype=np.int64)
        self.outcomes = np.zeros((n, 5), dtype=np.int64)


def _evaluate(evaluate, rows):
    lnp, st = evaluate(rows)
    lnp = np.asarray(lnp, dtype=np.float64)
    return np.where(np.isnan(lnp), -np.inf, lnp), np.asarray(st, dtype=np.int32)


def _sort(s, k, xatol, fatol):
    order = np.argsort(-s.lnp[k], kind="stable")
    s.sim[k], s.lnp[k], s.status[k] = s.sim[k][order], s.lnp[k][order], s.status[k][order]
    s.stopped[k] = int(stop_rule(s.sim[k], s.lnp[k], xatol, fatol))


def start(sim0, evaluate, lower, upper, xatol=1e-4, fatol=1e-4):
    """The initial evaluation of sim0[n, N + 1, N]: evaluate(rows[n (N + 4), N]) -> (lnprob, status) over a batch of the
    iterations' size, rows c = 0 .. N of a simplex its vertices, the others filled with vertex 0."""
    s = State(into_box(np.array(sim0, dtype=np.float64), lower, upper))
    n, nv, N = s.sim.shape
    rows = np.repeat(s.sim[:, :1], N + 4, axis=1)
    rows[:, :nv] = s.sim
    lnp, st = _evaluate(evaluate, rows.reshape(-1, N))
    s.lnp[:], s.status[:] = lnp.reshape(n, N + 4)[:, :nv], st.reshape(n, N + 4)[:, :nv]
    for k in range(n):
        _sort(s, k, xatol, fatol)
    return s


def iterate(s, evaluate, rho, chi, psi, sigma, lower, upper, xatol=1e-4, fatol=1e-4):
    """One iteration of every simplex that has not stopped; the batch handed to `evaluate` holds every candidate (those of a
    stopped simplex filled with its vertex 0: the device evaluates nothing there)."""
    n, nv, N = s.sim.shape
    cand = candidates(s.sim, rho, chi, psi, sigma, lower, upper)
    frozen = s.stopped.astype(bool)
    cand[frozen] = s.sim[frozen, :1]
    lnp, st = _evaluate(evaluate, cand.reshape(-1, N))
    lnp, st = lnp.reshape(n, N + 4), st.reshape(n, N + 4)
    for k in range(n):
        if s.stopped[k]:
            continue
        f, fc = -s.lnp[k], -lnp[k]
        fr, fe, fo, fi = fc[:4]
        take, evals = None, 2
        if fr < f[0]:
            take, outcome = (1, EXPAND) if fe < fr else (0, REFLECT)
        elif fr < f[N - 1]:
            take, outcome, evals = 0, REFLECT, 1
        elif fr < f[N]:
            take, outcome = (2, OUTSIDE) if fo <= fr else (None, SHRINK)
        else:
            take, outcome = (3, INSIDE) if fi < f[N] else (None, SHRINK)
        if take is None:
            s.sim[k, 1:], s.lnp[k, 1:], s.status[k, 1:] = cand[k, 4:], lnp[k, 4:], st[k, 4:]
            evals = N + 2
        else:
            s.sim[k, N], s.lnp[k, N], s.status[k, N] = cand[k, take], lnp[k, take], st[k, take]
        s.nit[k] += 1
        s.nfev[k] += evals
        s.outcomes[k, outcome] += 1
        _sort(s, k, xatol, fatol)
    return s


def run(sim0, iterations, evaluate, rho=1.0, chi=2.0, psi=0.5, sigma=0.5, lower=None, upper=None, xatol=1e-4, fatol=1e-4, state=None):
    """The initial evaluation (unless `state` continues an earlier run) and then `iterations` loop bodies (stopped simplexes
    frozen); returns the State.  scipy's maxiter counts from 1: maxiter - 1 loop bodies."""
    s = start(sim0, evaluate, lower, upper, xatol, fatol) if state is None else state
    for _ in range(iterations):
        if np.all(s.stopped):
            break
        iterate(s, evaluate, rho, chi, psi, sigma, lower, upper, xatol, fatol)
    return s
