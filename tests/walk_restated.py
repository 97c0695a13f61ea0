"""numpy restatement of what the walk kernels share on the device (magprop_amd/csrc/mp_walk.h): one stepping-out and shrinkage
slice update as the kernels' rounds, and the DE step of a constrained random walk.  Test infrastructure: the restatements of the
nested sampler's slice mode (tests/nest_slice_restated.py) and of the ensemble slice move (tests/slice_move_restated.py) run
their slices through slice_rounds with their own draws, inside test and box; nest_restated.walk_rounds, smc_restated.moves and
smc_adapt_restated.round_of form their proposals with de_step.  Every product and sum is a separately rounded float64 operation
in the header's order."""
from typing import NamedTuple

import numpy as np

from oracle.stretch_oracle import u01


class Slice(NamedTuple):
    q: list                 # the point the slice moved to; None: it failed at the cap
    lnp: float              # its value and status as the evaluation gave them (NaN as -inf); None where q is
    status: int
    n_eval: int
    n_exp: int
    n_con: int
    budgets: tuple          # (J, K): the steps out allowed to the left and to the right, as the slice started with them


def slice_rounds(x, d, mu, max_steps_out, max_shrink, draw, shrink_c, inside, box=None, broken=None):
    """One slice update of x (a list of floats) along d as the kernels' rounds: a generator that yields the next point to evaluate
    (a named point inside the box), is sent its (value, status), and returns a Slice.  draw(c): the four Philox words of the
    caller's counter c; c = 1 places the interval and splits the budgets, c = shrink_c + i gives shrink point i.  inside(value):
    the caller's level test.  box = (lower, upper): points outside it are outside without an evaluation; None: no box.
    broken="forward" (the negative control of the tests): the interval starts at x and steps out forward only (L = 0, R = mu,
    J = 0, K = m - 1), so that the update moves along +d alone and is not reversible."""
    nd = len(x)
    n_eval = n_exp = n_con = 0
    u = draw(1)
    lo = -(mu * u01(u[0], u[1]))
    hi = lo + mu
    left = int(u01(u[2], u[3]) * float(max_steps_out))
    right = max_steps_out - 1 - left
    if broken == "forward":
        lo, hi, left, right = 0.0, mu, 0, max_steps_out - 1
    budgets = (left, right)

    def named(t):
        """(q, inside, value, status) of the point x + t d; outside the box: not evaluated."""
        nonlocal n_eval
        q = [x[k] + t * d[k] for k in range(nd)]
        if box is not None and not all(box[0][k] <= q[k] <= box[1][k] for k in range(nd)):
            return q, False, None, None
        lq, sq = yield np.array(q)
        lq = -np.inf if lq != lq else float(lq)
        n_eval += 1
        return q, inside(lq), lq, int(sq)

    while left > 0 and (yield from named(lo))[1]:
        lo = lo - mu
        left -= 1
        n_exp += 1
    while right > 0 and (yield from named(hi))[1]:
        hi = hi + mu
        right -= 1
        n_exp += 1
    for i in range(max_shrink):
        u = draw(shrink_c + i)
        t = lo + u01(u[0], u[1]) * (hi - lo)
        q, ok, lq, sq = yield from named(t)
        if ok:
            return Slice(q, lq, sq, n_eval, n_exp, n_con, budgets)
        n_con += 1
        if t < 0.0:
            lo = t
        else:
            hi = t
    return Slice(None, None, None, n_eval, n_exp, n_con, budgets)


def de_step(cur, x1, x2, g, s3, u, lower, upper):
    """The DE step q = cur + gamma (x1 - x2), gamma = g (1 + s3 (2 u - 1)), of one point (u a float) or of rows of points (u an
    array, one per row): (q, whether q lies in the box [lower, upper])."""
    gamma = np.asarray(g * (1.0 + s3 * (2.0 * u - 1.0)))
    q = np.asarray(cur, dtype=np.float64) + gamma[..., None] * (np.asarray(x1, dtype=np.float64) - np.asarray(x2, dtype=np.float64))
    return q, np.all((q >= lower) & (q <= upper), axis=-1)
