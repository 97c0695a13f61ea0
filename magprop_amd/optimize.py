"""Best fits on the GPU: differential evolution after ``scipy.optimize.differential_evolution`` and a Nelder-Mead simplex search
after ``scipy.optimize.minimize(method="Nelder-Mead")``, both device-resident.

Every generation of every population is one kernel launch that builds the trial vectors, evaluates their log-posterior and
keeps the better of trial and member (include/magprop_amd.h mp_optimizer_*); the host only reads the convergence flags back
between chunks of generations.  Every iteration of every simplex is one launch that evaluates all the points scipy's serial
algorithm may ask for, and a small one that takes its decisions (mp_simplex_*): ``nelder_mead`` on its own, or as the polish
of ``differential_evolution(polish=True)``.  ``initial_ball`` turns a result into the starting walkers of ``EnsembleSampler.run_mcmc``, the
reference's ``p0 + 1e-4 randn`` (code/synthetic_datasets/synth_mcmc.py).
"""
import numpy as np

from . import _capi, engine
from .resident import OptimizeResult, count_datasets, finite_box

STRATEGIES = {"best1bin": _capi.DE_BEST1BIN, "rand1bin": _capi.DE_RAND1BIN}
NM_STANDARD = (1.0, 2.0, 0.5, 0.5)                                   # rho, chi, psi, sigma of scipy's Nelder-Mead
NM_OUTCOMES = ("reflect", "expand", "outside", "inside", "shrink")   # the columns of mp_simplex_get_state's outcomes
NM_MAX_SIMPLEXES = 1024                                              # include/magprop_amd.h mp_simplex_create


def latin_hypercube(rng, n, lower, upper):
    """scipy's 'latinhypercube' initialisation: one point in each of n equal slices of every coordinate, the slices paired at
    random across coordinates (rng.uniform for the offsets inside the slices, one rng.permutation per coordinate)."""
    ndim = len(lower)
    seg = 1.0 / n
    samples = seg * rng.uniform(size=(n, ndim)) + np.linspace(0.0, 1.0, n, endpoint=False)[:, None]
    unit = np.empty_like(samples)
    for j in range(ndim):
        unit[:, j] = samples[rng.permutation(n), j]
    return lower + unit * (upper - lower)


def _check_args(variant, bounds, strategy, maxiter, popsize, tol, atol, mutation, recombination, n_starts, datasets, x, polish=False):
    """(lower, upper, prior lower, prior upper, log mask, members, f_lo, f_hi): every argument check, before any device is touched."""
    if strategy not in STRATEGIES:
        raise ValueError(f"strategy must be one of {tuple(STRATEGIES)}, got {strategy!r}")
    if bounds is None:
        ndim = 6
    else:
        b = np.asarray(bounds, dtype=np.float64)
        if b.ndim != 2 or b.shape[1] != 2:
            raise ValueError("bounds must be a sequence of (lower, upper) pairs")
        ndim = b.shape[0]
    plo, phi, mask = engine.prior_box(variant, ndim, strict=True)
    lo, hi = finite_box(np.stack([plo, phi], axis=1) if bounds is None else b)
    if int(maxiter) != maxiter or maxiter < 0:
        raise ValueError("maxiter must be an integer >= 0")
    if int(popsize) != popsize or popsize < 1:
        raise ValueError("popsize must be a positive integer (a multiplier of ndim, as in scipy)")
    members = int(popsize) * ndim
    if not 5 <= members <= 1024:
        raise ValueError(f"popsize x ndim = {members} members: must be 5 .. 1024")
    if polish and members < ndim + 1:
        raise ValueError(f"polish builds a simplex from the {ndim + 1} best members: popsize x ndim = {members} are too few")
    if not (np.isfinite(tol) and tol >= 0.0 and np.isfinite(atol) and atol >= 0.0):
        raise ValueError("tol and atol must be finite and >= 0")
    f_lo, f_hi = (float(mutation), float(mutation)) if np.ndim(mutation) == 0 else tuple(float(m) for m in mutation)
    if not 0.0 <= f_lo <= f_hi < 2.0:
        raise ValueError("mutation must be F or (f_lo, f_hi) with 0 <= f_lo <= f_hi < 2")
    if not 0.0 <= recombination <= 1.0:
        raise ValueError("recombination must lie in [0, 1]")
    if int(n_starts) != n_starts or n_starts < 1:
        raise ValueError("n_starts must be a positive integer")
    n_ds = count_datasets(x, datasets)
    if n_ds * int(n_starts) > _capi.MAX_DATASETS:
        raise ValueError(f"len(datasets) x n_starts populations must be at most {_capi.MAX_DATASETS}")
    return lo, hi, plo, phi, mask, members, f_lo, f_hi


def differential_evolution(x=None, y=None, yerr=None, variant="synth", GRBtype=None, datasets=None, bounds=None, log_mask=None,
                           strategy="best1bin", maxiter=1000, popsize=15, tol=0.01, atol=0.0, mutation=(0.5, 1.0),
                           recombination=0.7, seed=0, init="latinhypercube", n_starts=1, device=-1, polish=False):
    """Maximise the log-posterior (minimise E = -lnprob) of light curve (x, y, yerr), or of every light curve of
    datasets=[(x, y, yerr), ...], with scipy's differential evolution (deferred updating), on the GPU.

    bounds: [(lower, upper)] * ndim in sampler coordinates (default: the prior box of the variant, ndim = 6); the lib variant
    takes 6 to 9 parameters, its prior box then being mcmc_eqns' default limits for that many.  popsize: a multiplier of ndim,
    as in scipy (popsize x ndim members, 5 .. 1024).  mutation: F, or (f_lo, f_hi) for a dither drawn once per generation.
    init: "latinhypercube" (scipy's scheme, drawn from np.random.default_rng(seed), one population after the other) or an
    array (popsize x ndim, ndim) or (n_populations, popsize x ndim, ndim).  n_starts: independent populations per dataset, all
    in one launch per generation (population index = dataset index x n_starts + start).  seed also keys the device's draws.

    polish=True refines every population's best fit on the same handle with the Nelder-Mead search of ``nelder_mead`` (its
    defaults), started from the population's ndim + 1 best members (by lnprob descending, then index ascending: they carry the
    posterior's scale).  As in scipy the polished point replaces x, fun and lnprob only if it is better; nfev grows by the
    polish's count, and its result is kept as res.polish.  Off by default.

    Deviations from scipy, all deliberate: the polish is derivative-free and optional (scipy refines the best member with
    L-BFGS-B by default, whose finite-difference gradient would fight the 1e-8-level noise of the adaptive ODE solver; a simplex
    search only compares values), a trial coordinate outside the bounds is redrawn uniformly inside the box in sampler
    coordinates (scipy does the same on its unit cube), and the random numbers are the device's Philox streams
    (include/magprop_amd.h).

    Returns an OptimizeResult (x, fun = -lnprob, lnprob, nit, nfev, success, message, population, population_lnprob,
    population_status; polish with polish=True), or a list of them in population order when there are several populations."""
    lo, hi, plo, phi, mask, members, f_lo, f_hi = _check_args(variant, bounds, strategy, maxiter, popsize, tol, atol, mutation,
                                                             recombination, n_starts, datasets, x, polish)
    ndim = lo.size
    if datasets is None:
        datasets = [(x, y, yerr)]
    n_pops = len(datasets) * int(n_starts)
    if isinstance(init, str):
        if init != "latinhypercube":
            raise ValueError("init must be 'latinhypercube' or an array")
        rng = np.random.default_rng(seed)
        pop0 = np.stack([latin_hypercube(rng, members, lo, hi) for _ in range(n_pops)])
    else:
        pop0 = np.asarray(init, dtype=np.float64)
        if pop0.shape == (members, ndim):
            pop0 = np.broadcast_to(pop0, (n_pops, members, ndim))
        if pop0.shape != (n_pops, members, ndim):
            raise ValueError(f"init must have shape {(members, ndim)} or {(n_pops, members, ndim)}, got {np.shape(init)}")
        if not np.all(np.isfinite(pop0)):
            raise ValueError("init must be finite")
    pop0 = np.ascontiguousarray(pop0, dtype=np.float64)
    if log_mask is not None:
        mask = log_mask
    handle = engine.open_handle(variant, GRBtype, device, (plo, phi, mask), datasets)
    L = _capi.lib()
    ids = np.repeat(np.arange(len(datasets), dtype=np.int32), int(n_starts))
    with handle, _capi.Driver("mp_optimizer", handle, members, n_pops, ndim, _capi.ptr(ids), int(seed), STRATEGIES[strategy], f_lo,
                              f_hi, float(recombination), float(tol), float(atol), _capi.ptr(lo), _capi.ptr(hi), 0) as o:
        _capi.check(L.mp_optimizer_set_population(o, _capi.ptr(pop0)), "mp_optimizer_set_population")
        _capi.check(L.mp_optimizer_run(o, int(maxiter), None), "mp_optimizer_run")
        st = get_state(L, o, n_pops, members, ndim)
        polished = None
        if polish:
            # the ndim + 1 best members of every population: lnprob descending, index ascending among equals (stable)
            best = np.argsort(-st["lnprob"], axis=1, kind="stable")[:, :ndim + 1]
            sim0 = np.ascontiguousarray(np.take_along_axis(st["pop"], best[:, :, None], axis=1))
            polished = _simplex_search(L, handle, ids, sim0, lo, hi, NM_STANDARD, 1e-4, 1e-4, 200 * ndim)
    out = []
    for p in range(n_pops):
        b = int(st["best"][p])
        conv = bool(st["converged"][p])
        out.append(OptimizeResult(
            x=st["pop"][p, b].copy(), fun=-float(st["lnprob"][p, b]), lnprob=float(st["lnprob"][p, b]), nit=int(st["nit"][p]),
            nfev=int(st["nfev"][p]), success=conv,
            message="Optimization terminated successfully." if conv else "Maximum number of iterations has been exceeded.",
            population=st["pop"][p].copy(), population_lnprob=st["lnprob"][p].copy(), population_status=st["status"][p].copy(),
            bounds=np.stack([lo, hi], axis=1)))
        if polished is not None:
            res, pol = out[-1], polished[p]
            res.polish = pol
            res.nfev += pol.nfev
            if pol.lnprob > res.lnprob:
                res.x, res.fun, res.lnprob = pol.x.copy(), pol.fun, pol.lnprob
    return out[0] if n_pops == 1 else out


def get_state(L, o, n_pops, members, ndim):
    """mp_optimizer_get_state as arrays: pop (n_pops, members, ndim), lnprob and status (n_pops, members), best, nit,
    converged, nfev (n_pops)."""
    return _capi.read_back(L.mp_optimizer_get_state, o, [
        ("pop", (n_pops, members, ndim), np.float64), ("lnprob", (n_pops, members), np.float64),
        ("status", (n_pops, members), np.int32), ("best", n_pops, np.int32), ("nit", n_pops, np.int32),
        ("converged", n_pops, np.int32), ("nfev", n_pops, np.int64)])


def nm_coefficients(ndim, adaptive):
    """(rho, chi, psi, sigma) as scipy sets them: the standard ones, or (adaptive) those of Gao and Han for ndim dimensions."""
    if not adaptive:
        return NM_STANDARD
    dim = float(ndim)
    return 1.0, 1 + 2 / dim, 0.75 - 1 / (2 * dim), 1 - 1 / dim


def default_simplex(x0):
    """scipy's initial simplex around x0 (ndim,): vertex k + 1 is x0 with coordinate k 5 % larger, or 0.00025 where it is zero."""
    sim = np.tile(np.asarray(x0, dtype=np.float64), (len(x0) + 1, 1))
    for k in range(len(x0)):
        sim[k + 1, k] = (1 + 0.05) * sim[0, k] if sim[0, k] != 0 else 0.00025
    return sim


def get_simplex_state(L, s, n_simplex, ndim):
    """mp_simplex_get_state as arrays: sim (n_simplex, ndim + 1, ndim), lnprob and status (n_simplex, ndim + 1), nit, stopped,
    nfev (n_simplex), outcomes (n_simplex, 5)."""
    return _capi.read_back(L.mp_simplex_get_state, s, [
        ("sim", (n_simplex, ndim + 1, ndim), np.float64), ("lnprob", (n_simplex, ndim + 1), np.float64),
        ("status", (n_simplex, ndim + 1), np.int32), ("nit", n_simplex, np.int32), ("stopped", n_simplex, np.int32),
        ("nfev", n_simplex, np.int64), ("outcomes", (n_simplex, 5), np.int64)])


def _simplex_search(L, handle, ids, sim0, lo, hi, coefficients, xatol, fatol, maxiter):
    """The search from sim0 (n_simplex, ndim + 1, ndim) on `handle`, simplex s on dataset ids[s]: one OptimizeResult each.
    maxiter is scipy's count, which starts at 1: maxiter - 1 loop bodies."""
    n, _, ndim = sim0.shape
    with _capi.Driver("mp_simplex", handle, n, ndim, _capi.ptr(ids), *(float(c) for c in coefficients), float(xatol), float(fatol),
                      _capi.ptr(lo), _capi.ptr(hi), 0) as s:
        _capi.check(L.mp_simplex_set_vertices(s, _capi.ptr(sim0)), "mp_simplex_set_vertices")
        _capi.check(L.mp_simplex_run(s, max(int(maxiter) - 1, 0), None), "mp_simplex_run")
        st = get_simplex_state(L, s, n, ndim)
    out = []
    for k in range(n):
        ok = bool(st["stopped"][k]) and int(st["nit"][k]) < maxiter
        out.append(OptimizeResult(
            x=st["sim"][k, 0].copy(), fun=-float(st["lnprob"][k, 0]), lnprob=float(st["lnprob"][k, 0]), nit=int(st["nit"][k]),
            nfev=int(st["nfev"][k]), success=ok, status=0 if ok else 2,
            message="Optimization terminated successfully." if ok else "Maximum number of iterations has been exceeded.",
            final_simplex=(st["sim"][k].copy(), -st["lnprob"][k]), simplex_status=st["status"][k].copy(),
            outcomes=dict(zip(NM_OUTCOMES, (int(v) for v in st["outcomes"][k]))), bounds=np.stack([lo, hi], axis=1)))
    return out


def _check_simplex_args(x0, variant, bounds, initial_simplex, xatol, fatol, maxiter, n_starts, datasets, x):
    """(lower, upper, prior lower, prior upper, log mask, sim0, maxiter): every argument check, before any device is touched."""
    x0 = np.asarray(x0, dtype=np.float64)
    if x0.ndim not in (1, 2) or x0.shape[-1] < 1:
        raise ValueError(f"x0 must have shape (ndim,) or (n_simplex, ndim), got {x0.shape}")
    ndim = x0.shape[-1]
    if bounds is not None:
        b = np.asarray(bounds, dtype=np.float64)
        if b.ndim != 2 or b.shape[1] != 2:
            raise ValueError("bounds must be a sequence of (lower, upper) pairs")
        if b.shape[0] != ndim:
            raise ValueError(f"bounds must have one (lower, upper) pair per coordinate of x0 ({ndim}), got {b.shape[0]}")
    plo, phi, mask = engine.prior_box(variant, ndim, strict=True)
    lo, hi = finite_box(np.stack([plo, phi], axis=1) if bounds is None else b)
    if not (np.isfinite(xatol) and xatol >= 0.0 and np.isfinite(fatol) and fatol >= 0.0):
        raise ValueError("xatol and fatol must be finite and >= 0")
    if maxiter is None:
        maxiter = 200 * ndim
    if int(maxiter) != maxiter or maxiter < 1:
        raise ValueError("maxiter must be an integer >= 1 (scipy's count, which starts at 1)")
    if int(n_starts) != n_starts or n_starts < 1:
        raise ValueError("n_starts must be a positive integer")
    n_ds = count_datasets(x, datasets)
    n = n_ds * int(n_starts)
    if n > NM_MAX_SIMPLEXES:
        raise ValueError(f"len(datasets) x n_starts simplexes must be at most {NM_MAX_SIMPLEXES}")
    if x0.ndim == 2 and x0.shape[0] != n:
        raise ValueError(f"x0 must have shape ({ndim},) or ({n}, {ndim}): one start per simplex, got {x0.shape}")
    if not np.all(np.isfinite(x0)):
        raise ValueError("x0 must be finite")
    if initial_simplex is None:
        sim0 = np.stack([default_simplex(r) for r in np.clip(np.broadcast_to(x0, (n, ndim)), lo, hi)])
    else:
        sim0 = np.asarray(initial_simplex, dtype=np.float64)
        if sim0.shape == (ndim + 1, ndim):
            sim0 = np.broadcast_to(sim0, (n, ndim + 1, ndim))
        if sim0.shape != (n, ndim + 1, ndim):
            raise ValueError(f"initial_simplex must have shape {(ndim + 1, ndim)} or {(n, ndim + 1, ndim)}, got {np.shape(initial_simplex)}")
        if not np.all(np.isfinite(sim0)):
            raise ValueError("initial_simplex must be finite")
    return lo, hi, plo, phi, mask, np.ascontiguousarray(sim0, dtype=np.float64), int(maxiter)


def nelder_mead(x0, x=None, y=None, yerr=None, variant="synth", GRBtype=None, datasets=None, bounds=None, log_mask=None,
                initial_simplex=None, xatol=1e-4, fatol=1e-4, adaptive=False, maxiter=None, n_starts=1, device=-1):
    """Maximise the log-posterior (minimise f = -lnprob) of light curve (x, y, yerr), or of every light curve of
    datasets=[(x, y, yerr), ...], from x0 with the Nelder-Mead simplex search of scipy.optimize.minimize(method="Nelder-Mead",
    bounds=...), on the GPU: scipy's iterate sequence exactly, every simplex in the same launches (simplex index = dataset index
    x n_starts + start, at most 1024).

    x0: (ndim,), the start of every simplex, or (n_simplex, ndim), in sampler coordinates; it is clipped into the bounds.
    bounds: [(lower, upper)] * ndim (default: the prior box of the variant; the synth variant has 6 parameters, the lib variant 6
    to 9).  initial_simplex: (ndim + 1, ndim) or (n_simplex, ndim + 1, ndim); default scipy's rule around x0 (a non-zero
    coordinate 5 % larger, 0.00025 for a zero one).  A vertex outside the bounds is reflected at the upper bound and clipped, as
    in scipy.  adaptive: scipy's coefficients for ndim dimensions, chi = 1 + 2 / ndim, psi = 0.75 - 1 / (2 ndim), sigma = 1 - 1 /
    ndim.  A simplex stops when max |v_j - v_0| <= xatol and max |f_0 - f_j| <= fatol, or at iteration maxiter (default 200 x
    ndim; scipy's count, which starts at 1 with the initial evaluation).  There is no maxfev.

    lnprob carries the noise of the adaptive ODE solver, 5e-8 relative at the default solver settings:
    tolerances should stay above it, an fatol below 5e-8 |lnprob| asks the comparisons to resolve noise.

    Returns an OptimizeResult (x, fun = -lnprob, lnprob, nit, nfev as the serial algorithm counts, success, message, status,
    final_simplex = (sim, fsim) sorted, simplex_status, outcomes = {reflect, expand, outside, inside, shrink: count}, bounds), or
    a list of them in simplex order when there are several simplexes."""
    lo, hi, plo, phi, mask, sim0, maxiter = _check_simplex_args(x0, variant, bounds, initial_simplex, xatol, fatol, maxiter,
                                                                n_starts, datasets, x)
    if datasets is None:
        datasets = [(x, y, yerr)]
    if log_mask is not None:
        mask = log_mask
    handle = engine.open_handle(variant, GRBtype, device, (plo, phi, mask), datasets)
    ids = np.repeat(np.arange(len(datasets), dtype=np.int32), int(n_starts))
    with handle:
        out = _simplex_search(_capi.lib(), handle, ids, sim0, lo, hi, nm_coefficients(sim0.shape[2], adaptive), xatol, fatol, maxiter)
    return out[0] if len(out) == 1 else out


def initial_ball(res, nwalkers, scale=1.0e-4, seed=0):
    """Starting walkers around a best fit: res.x + scale x N(0, 1) per coordinate (the reference's p0 + 1e-4 randn,
    code/synthetic_datasets/synth_mcmc.py), clipped into the result's bounds box; (nwalkers, ndim)."""
    if int(nwalkers) != nwalkers or nwalkers < 1:
        raise ValueError("nwalkers must be a positive integer")
    x = np.asarray(res["x"], dtype=np.float64)
    pos = x + float(scale) * np.random.default_rng(seed).standard_normal((int(nwalkers), x.size))
    b = res.get("bounds")
    return pos if b is None else np.clip(pos, b[:, 0], b[:, 1])
