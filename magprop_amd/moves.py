"""Proposal moves of the ensemble sampler, with emcee 3's names and defaults (include/magprop_amd.h MP_MOVE_*).

    EnsembleSampler(..., moves=DEMove())
    EnsembleSampler(..., moves=[(DEMove(), 0.8), (DESnookerMove(), 0.2)])
    EnsembleSampler(..., moves=KDEMove())
    EnsembleSampler(..., moves=SliceMove())
    EnsembleSampler(..., moves=[(WalkMove(s=3), 0.5), (KDEMove(), 0.5)])
    EnsembleSampler(..., moves=GaussianMove(cov, tune=200))

Every move runs inside the fused half-step kernels; these classes only carry the parameters.  One move is drawn per step for
the whole sampler, with probability proportional to its weight, as in emcee.  Two deviations from emcee 3.1:
the jitter of DEMove's gamma is uniform with standard deviation sigma, not normal, and the snooker move draws its three
partners from the other half of a two-way split, not from a four-way split.
"""
import math

import numpy as np

MOVE_STRETCH, MOVE_DE, MOVE_SNOOKER, MOVE_KDE, MOVE_SLICE, MOVE_GAUSSIAN, MOVE_WALK = 0, 1, 2, 3, 4, 5, 6   # include/magprop_amd.h MP_MOVE_*
WALK_MAX_S = 64                                     # MP_WALK_MAX_S
GAUSS_MODES = {"vector": 0, "random": 1, "sequential": 2}   # MP_GAUSS_*
MAX_MOVES = 8                                       # MP_MAX_MOVES
SLICE_MAX_STEPS_OUT, SLICE_MAX_SHRINK = 4096, 252   # MP_NEST_MAX_STEPS_OUT, MP_SLICE_MAX_SHRINK


class Move:
    kind = None

    def params(self, ndim):
        """The two doubles mp_sampler_set_moves takes for this move."""
        raise NotImplementedError

    def __eq__(self, other):
        return type(self) is type(other) and self.params(0) == other.params(0)

    def __hash__(self):
        return hash((type(self).__name__, self.params(0)))


class StretchMove(Move):
    """The affine-invariant stretch move (Goodman & Weare 2010), scale a > 1; emcee's default move."""
    kind = MOVE_STRETCH

    def __init__(self, a=2.0):
        a = float(a)
        if not (math.isfinite(a) and a > 1.0):
            raise ValueError(f"StretchMove: a must be finite and > 1, got {a}")
        self.a = a

    def params(self, ndim):
        return (self.a, 0.0)

    def __repr__(self):
        return f"StretchMove(a={self.a})"


class DEMove(Move):
    """Differential evolution (ter Braak 2006): q = x + gamma (x_j1 - x_j2), two distinct partners from the other half.
    gamma0=None: 2.38 / sqrt(2 ndim).  gamma = gamma0 (1 + jitter), the jitter uniform with standard deviation sigma
    (sigma < 1/sqrt(3), so gamma keeps its sign)."""
    kind = MOVE_DE

    def __init__(self, sigma=1.0e-5, gamma0=None):
        sigma = float(sigma)
        if not (0.0 <= sigma and sigma * math.sqrt(3.0) < 1.0):
            raise ValueError(f"DEMove: sigma must be in [0, 1/sqrt(3)), got {sigma}")
        if gamma0 is not None:
            gamma0 = float(gamma0)
            if not (math.isfinite(gamma0) and gamma0 > 0.0):
                raise ValueError(f"DEMove: gamma0 must be finite and > 0 (or None), got {gamma0}")
        self.sigma, self.gamma0 = sigma, gamma0

    def params(self, ndim):
        return (0.0 if self.gamma0 is None else self.gamma0, self.sigma)   # 0: the library's 2.38 / sqrt(2 ndim)

    def __repr__(self):
        return f"DEMove(sigma={self.sigma}, gamma0={self.gamma0})"


class DESnookerMove(Move):
    """The snooker move (ter Braak & Vrugt 2008): along the line through x and a partner z, by gammas times the projection of
    the difference of two further partners, with its Hastings term (ndim - 1) ln(|q - z| / |x - z|)."""
    kind = MOVE_SNOOKER

    def __init__(self, gammas=1.7):
        gammas = float(gammas)
        if not (math.isfinite(gammas) and gammas > 0.0):
            raise ValueError(f"DESnookerMove: gammas must be finite and > 0, got {gammas}")
        self.gammas = gammas

    def params(self, ndim):
        return (self.gammas, 0.0)

    def __repr__(self):
        return f"DESnookerMove(gammas={self.gammas})"


class KDEMove(Move):
    """emcee's KDEMove: q drawn from a Gaussian kernel density estimate of the other half of the ensemble (kernel covariance
    f^2 S, S the half's sample covariance), with the Hastings term ln KDE(x) - ln KDE(q).  bw_method as scipy.stats.gaussian_kde
    takes it: None or "scott" (f = n^(-1/(ndim+4))), "silverman" (f = (n (ndim+2)/4)^(-1/(ndim+4))) or a positive factor f,
    n = the walkers of the other half.  Needs n >= ndim + 1."""
    kind = MOVE_KDE

    def __init__(self, bw_method=None):
        if bw_method is None or (isinstance(bw_method, str) and bw_method in ("scott", "silverman")):
            self.bw_method = "scott" if bw_method is None else bw_method
            return
        if isinstance(bw_method, (str, bool)):
            raise ValueError(f"KDEMove: bw_method must be None, 'scott', 'silverman' or a positive number, got {bw_method!r}")
        try:
            f = float(bw_method)
        except (TypeError, ValueError):
            raise ValueError(f"KDEMove: bw_method must be None, 'scott', 'silverman' or a positive number, got {bw_method!r}") from None
        if not (math.isfinite(f) and f > 0.0):
            raise ValueError(f"KDEMove: a bandwidth factor must be finite and > 0, got {bw_method!r}")
        self.bw_method = f

    def params(self, ndim):
        codes = {"scott": 0.0, "silverman": -1.0}   # the library's codes; a factor goes as it is
        return (codes[self.bw_method] if isinstance(self.bw_method, str) else self.bw_method, 0.0)

    def __repr__(self):
        return f"KDEMove(bw_method={self.bw_method!r})"


class SliceMove(Move):
    """Ensemble slice sampling (Karamanis & Beutler 2021, the sampler known as zeus): a slice update by Neal's stepping out and
    shrinkage along the difference of two walkers of the other half.  Every update moves the walker unless the slice fails
    (max_shrink rejected points); a failed model evaluation is a point outside the slice.  mu: the initial scale of the
    interval, in units of the direction; it tunes itself over the first `tune` slice steps, which the user discards.
    max_steps_out, max_shrink: the stepping-out budget and the shrink points of a slice (mp_sampler_set_slice_limits)."""
    kind = MOVE_SLICE

    def __init__(self, mu=1.0, tune=100, max_steps_out=32, max_shrink=64):
        mu = float(mu)
        if not (math.isfinite(mu) and mu > 0.0):
            raise ValueError(f"SliceMove: mu must be finite and > 0, got {mu}")
        if isinstance(tune, bool) or int(tune) != tune or not 0 <= int(tune) <= 2 ** 31 - 1:
            raise ValueError(f"SliceMove: tune must be a whole number in [0, 2^31 - 1], got {tune!r}")
        for name, v, hi in (("max_steps_out", max_steps_out, SLICE_MAX_STEPS_OUT), ("max_shrink", max_shrink, SLICE_MAX_SHRINK)):
            if isinstance(v, bool) or int(v) != v or not 1 <= int(v) <= hi:
                raise ValueError(f"SliceMove: {name} must be a whole number in [1, {hi}], got {v!r}")
        self.mu, self.tune, self.max_steps_out, self.max_shrink = mu, int(tune), int(max_steps_out), int(max_shrink)

    def params(self, ndim):
        return (self.mu, float(self.tune))

    def limits(self):
        """(max_steps_out, max_shrink) as mp_sampler_set_slice_limits takes them."""
        return (self.max_steps_out, self.max_shrink)

    def __eq__(self, other):
        return Move.__eq__(self, other) and self.limits() == other.limits()

    def __hash__(self):
        return hash((type(self).__name__, self.params(0), self.limits()))

    def __repr__(self):
        return f"SliceMove(mu={self.mu}, tune={self.tune}, max_steps_out={self.max_steps_out}, max_shrink={self.max_shrink})"


class WalkMove(Move):
    """The walk move (Goodman & Weare 2010; emcee's WalkMove): q = x + sum_i z_i (x_i - mean) / sqrt(s - 1) over s walkers of the
    other half and standard normals z_i, a Gaussian step with the sample covariance of those walkers.  Affine invariant like the
    stretch move; no factorisation is needed, so it runs where KDEMove is refused (fewer than ndim + 1 walkers in the other
    half).  s=None: all walkers of the other half (emcee's default); else 2 <= s <= min(nwalkers / 2, 64), drawn afresh for
    every proposal: a small s gives local proposals."""
    kind = MOVE_WALK

    def __init__(self, s=None):
        if s is not None:
            if isinstance(s, bool) or not isinstance(s, (int, np.integer)) or s < 2:
                raise ValueError(f"WalkMove: s must be None or a whole number >= 2, got {s!r}")
            s = int(s)
        self.s = s

    def params(self, ndim):
        return (0.0 if self.s is None else float(self.s), 0.0)   # 0: the library's "all of the other half"

    def __repr__(self):
        return f"WalkMove(s={self.s})"


class GaussianMove(Move):
    """Metropolis steps with a fixed Gaussian proposal (emcee's GaussianMove): the one move that reads nothing of the other
    walkers, so it runs with 2 walkers and keeps a step size of its own per ensemble (per temperature of a tempered run).
    cov: a scalar (isotropic), a vector (the diagonal) or a matrix, in sampler coordinates; mode "vector" moves all coordinates
    at once, "random" one coordinate drawn per proposal, "sequential" coordinate step mod ndim (the single-axis modes need a
    diagonal cov, as in emcee).  The proposal is scale x the Gaussian of cov; over the first `tune` Gaussian steps, which the
    user discards, every ensemble adjusts its scale towards the acceptance fraction target_accept (None: 0.25 for "vector", 0.44
    for a single axis; include/magprop_amd.h states the rule).  emcee's factor= (a random scale per proposal) is not offered:
    tuning takes its place."""
    kind = MOVE_GAUSSIAN

    def __init__(self, cov, mode="vector", scale=1.0, tune=0, target_accept=None):
        if mode not in GAUSS_MODES:
            raise ValueError(f"GaussianMove: mode must be 'vector', 'random' or 'sequential', got {mode!r}")
        try:
            c = np.asarray(cov, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"GaussianMove: cov must be a scalar, a vector or a matrix, got {cov!r}") from None
        if c.ndim > 2 or (c.ndim == 2 and c.shape[0] != c.shape[1]) or c.size == 0 or not np.all(np.isfinite(c)):
            raise ValueError(f"GaussianMove: cov must be a finite scalar, vector or square matrix, got shape {c.shape}")
        if c.ndim == 2 and not np.array_equal(c, c.T):
            raise ValueError("GaussianMove: cov must be symmetric")
        if c.ndim < 2 and not np.all(c > 0.0):
            raise ValueError("GaussianMove: variances must be > 0")
        if c.ndim == 2:
            try:
                factor = np.linalg.cholesky(c)
            except np.linalg.LinAlgError:
                raise ValueError("GaussianMove: cov is not positive definite") from None
            if mode != "vector" and np.any(c != np.diag(np.diag(c))):
                raise ValueError(f"GaussianMove: mode {mode!r} needs a diagonal cov")
        else:
            factor = np.sqrt(c)           # a scalar or the diagonal; factor() expands it to ndim
        scale = float(scale)
        if not (math.isfinite(scale) and scale > 0.0):
            raise ValueError(f"GaussianMove: scale must be finite and > 0, got {scale}")
        if isinstance(tune, bool) or int(tune) != tune or not 0 <= int(tune) <= 2 ** 31 - 1:
            raise ValueError(f"GaussianMove: tune must be a whole number in [0, 2^31 - 1], got {tune!r}")
        if target_accept is None:
            target_accept = 0.25 if mode == "vector" else 0.44
        target_accept = float(target_accept)
        if not 0.0 < target_accept < 1.0:
            raise ValueError(f"GaussianMove: target_accept must lie in (0, 1), got {target_accept}")
        self._factor, self.mode, self.scale, self.tune, self.target_accept = factor, mode, scale, int(tune), target_accept

    @classmethod
    def from_samples(cls, x, **kw):
        """The move with cov = np.cov(x.T) 2.38^2 / ndim of samples x[n, ndim] (the optimal scaling of a Gaussian target)."""
        x = np.asarray(x, dtype=np.float64)
        if x.ndim != 2 or x.shape[0] < 2:
            raise ValueError(f"GaussianMove.from_samples: x must be [n >= 2, ndim], got shape {x.shape}")
        return cls(np.atleast_2d(np.cov(x.T)) * (2.38 ** 2 / x.shape[1]), **kw)

    def factor(self, ndim):
        """The Cholesky factor of cov for ndim coordinates, [ndim, ndim] lower triangular."""
        f = self._factor
        if f.ndim == 0:
            return np.eye(ndim) * float(f)
        if f.shape[0] != ndim:
            raise ValueError(f"GaussianMove: cov is for {f.shape[0]} coordinates, the sampler has {ndim}")
        return np.diag(f) if f.ndim == 1 else f

    def packed_factor(self, ndim):
        """factor(ndim) as mp_sampler_set_gaussian takes it: the lower triangle by rows."""
        return np.ascontiguousarray(self.factor(ndim)[np.tril_indices(ndim)], dtype=np.float64)

    def params(self, ndim):
        return (self.scale, float(self.tune))

    def _key(self):
        return (self.params(0), self.mode, self.target_accept, self._factor.shape, self._factor.tobytes())

    def __eq__(self, other):
        return type(self) is type(other) and self._key() == other._key()

    def __hash__(self):
        return hash((type(self).__name__,) + self._key())

    def __repr__(self):
        return (f"GaussianMove(<cov {self._factor.shape}>, mode={self.mode!r}, scale={self.scale}, tune={self.tune}, "
                f"target_accept={self.target_accept})")


def slice_move(table):
    """The SliceMove of a parsed table, or None."""
    for mv, _ in table:
        if isinstance(mv, SliceMove):
            return mv
    return None


def gaussian_move(table):
    """The GaussianMove of a parsed table, or None."""
    for mv, _ in table:
        if isinstance(mv, GaussianMove):
            return mv
    return None


def parse_moves(moves):
    """emcee's forms of moves=: a move, a list of moves (equal weights) or a list of (move, weight).  Returns a list of
    (move, weight).  Weights are kept as given (emcee normalises them; the draw is the same up to rounding)."""
    if isinstance(moves, Move):
        return [(moves, 1.0)]
    try:
        items = list(moves)
    except TypeError:
        raise ValueError(f"moves must be a move, a list of moves or a list of (move, weight), got {moves!r}") from None
    if not items:
        raise ValueError("moves is empty")
    if len(items) > MAX_MOVES:
        raise ValueError(f"at most {MAX_MOVES} moves, got {len(items)}")
    out = []
    for it in items:
        if isinstance(it, Move):
            out.append((it, 1.0))
            continue
        try:
            mv, w = it
        except (TypeError, ValueError):
            raise ValueError(f"moves entries must be moves or (move, weight) pairs, got {it!r}") from None
        if not isinstance(mv, Move):
            raise ValueError(f"not a move: {mv!r} (StretchMove, DEMove, DESnookerMove, KDEMove, SliceMove, GaussianMove, WalkMove)")
        w = float(w)
        if not (math.isfinite(w) and w > 0.0):
            raise ValueError(f"move weights must be finite and > 0, got {w}")
        out.append((mv, w))
    if any(isinstance(it, Move) for it in items) and not all(isinstance(it, Move) for it in items):
        raise ValueError("moves mixes bare moves and (move, weight) pairs")
    if sum(isinstance(mv, SliceMove) for mv, _ in out) > 1:
        raise ValueError("at most one SliceMove in a table (its scale mu is the sampler's)")
    if sum(isinstance(mv, GaussianMove) for mv, _ in out) > 1:
        raise ValueError("at most one GaussianMove in a table (its covariance and scales are the sampler's)")
    return out


def move_table(moves, ndim):
    """(kinds, weights, params[n][2]) of a parsed list, as mp_sampler_set_moves takes them."""
    table = parse_moves(moves)
    kinds = [m.kind for m, _ in table]
    weights = [w for _, w in table]
    params = [m.params(ndim) for m, _ in table]
    return kinds, weights, params


def parse_spec(spec):
    """'de:0.8,snooker:0.2' (the command-line form of tools/run_synth_mcmc.py) -> [(DEMove(), 0.8), (DESnookerMove(), 0.2)].
    Names: stretch, de, snooker, kde, slice, awalk (the walk move); a missing weight is 1.  GaussianMove needs a covariance
    and has no name here."""
    names = {"stretch": StretchMove, "de": DEMove, "snooker": DESnookerMove, "kde": KDEMove, "slice": SliceMove, "awalk": WalkMove}
    out = []
    for part in str(spec).split(","):
        name, _, w = part.strip().partition(":")
        if name not in names:
            raise ValueError(f"unknown move {name!r} in {spec!r} (stretch, de, snooker, kde, slice, awalk)")
        out.append((names[name](), float(w) if w else 1.0))
    return out
