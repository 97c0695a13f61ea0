"""Best fits on the GPU: differential evolution after ``scipy.optimize.differential_evolution``, device-resident.

Every generation of every population is one kernel launch that builds the trial vectors, evaluates their log-posterior and
keeps the better of trial and member (include/magprop_amd.h mp_optimizer_*); the host only reads the convergence flags back
between chunks of generations.  ``initial_ball`` turns a result into the starting walkers of ``EnsembleSampler.run_mcmc``, the
reference's ``p0 + 1e-4 randn`` (code/synthetic_datasets/synth_mcmc.py).
"""
import numpy as np

from . import _capi, engine

STRATEGIES = {"best1bin": _capi.DE_BEST1BIN, "rand1bin": _capi.DE_RAND1BIN}


class OptimizeResult(dict):
    """scipy.optimize.OptimizeResult's shape: a dict whose keys are also attributes."""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError as exc:
            raise AttributeError(name) from exc

    __setattr__ = dict.__setitem__


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


def _check_args(variant, bounds, strategy, maxiter, popsize, tol, atol, mutation, recombination, n_starts, datasets, x):
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
    lo, hi = (plo.copy(), phi.copy()) if bounds is None else (b[:, 0].copy(), b[:, 1].copy())
    if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi)) and np.all(lo < hi)):
        raise ValueError("every bound must be finite with lower < upper")
    if int(maxiter) != maxiter or maxiter < 0:
        raise ValueError("maxiter must be an integer >= 0")
    if int(popsize) != popsize or popsize < 1:
        raise ValueError("popsize must be a positive integer (a multiplier of ndim, as in scipy)")
    members = int(popsize) * ndim
    if not 5 <= members <= 1024:
        raise ValueError(f"popsize x ndim = {members} members: must be 5 .. 1024")
    if not (np.isfinite(tol) and tol >= 0.0 and np.isfinite(atol) and atol >= 0.0):
        raise ValueError("tol and atol must be finite and >= 0")
    f_lo, f_hi = (float(mutation), float(mutation)) if np.ndim(mutation) == 0 else tuple(float(m) for m in mutation)
    if not 0.0 <= f_lo <= f_hi < 2.0:
        raise ValueError("mutation must be F or (f_lo, f_hi) with 0 <= f_lo <= f_hi < 2")
    if not 0.0 <= recombination <= 1.0:
        raise ValueError("recombination must lie in [0, 1]")
    if int(n_starts) != n_starts or n_starts < 1:
        raise ValueError("n_starts must be a positive integer")
    n_ds = len(datasets) if datasets is not None else (1 if x is not None else 0)
    if n_ds == 0:
        raise ValueError("a dataset is required: (x, y, yerr) or datasets=[...]")
    if n_ds * int(n_starts) > _capi.MAX_DATASETS:
        raise ValueError(f"len(datasets) x n_starts populations must be at most {_capi.MAX_DATASETS}")
    return lo, hi, plo, phi, mask, members, f_lo, f_hi


def differential_evolution(x=None, y=None, yerr=None, variant="synth", GRBtype=None, datasets=None, bounds=None, log_mask=None,
                           strategy="best1bin", maxiter=1000, popsize=15, tol=0.01, atol=0.0, mutation=(0.5, 1.0),
                           recombination=0.7, seed=0, init="latinhypercube", n_starts=1, device=-1):
    """Maximise the log-posterior (minimise E = -lnprob) of light curve (x, y, yerr), or of every light curve of
    datasets=[(x, y, yerr), ...], with scipy's differential evolution (deferred updating), on the GPU.

    bounds: [(lower, upper)] * ndim in sampler coordinates (default: the prior box of the variant, ndim = 6); the lib variant
    takes 6 to 9 parameters, its prior box then being mcmc_eqns' default limits for that many.  popsize: a multiplier of ndim,
    as in scipy (popsize x ndim members, 5 .. 1024).  mutation: F, or (f_lo, f_hi) for a dither drawn once per generation.
    init: "latinhypercube" (scipy's scheme, drawn from np.random.default_rng(seed), one population after the other) or an
    array (popsize x ndim, ndim) or (n_populations, popsize x ndim, ndim).  n_starts: independent populations per dataset, all
    in one launch per generation (population index = dataset index x n_starts + start).  seed also keys the device's draws.

    Deviations from scipy, all deliberate: there is no polish step (scipy refines the best member with L-BFGS-B, whose
    finite-difference gradient would fight the 1e-8-level noise of the adaptive ODE solver), a trial coordinate outside the
    bounds is redrawn uniformly inside the box in sampler coordinates (scipy does the same on its unit cube), and the random
    numbers are the device's Philox streams (include/magprop_amd.h).

    Returns an OptimizeResult (x, fun = -lnprob, lnprob, nit, nfev, success, message, population, population_lnprob,
    population_status), or a list of them in population order when there are several populations."""
    lo, hi, plo, phi, mask, members, f_lo, f_hi = _check_args(variant, bounds, strategy, maxiter, popsize, tol, atol, mutation,
                                                             recombination, n_starts, datasets, x)
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
    return out[0] if n_pops == 1 else out


def get_state(L, o, n_pops, members, ndim):
    """mp_optimizer_get_state as arrays: pop (n_pops, members, ndim), lnprob and status (n_pops, members), best, nit,
    converged, nfev (n_pops)."""
    return _capi.read_back(L.mp_optimizer_get_state, o, [
        ("pop", (n_pops, members, ndim), np.float64), ("lnprob", (n_pops, members), np.float64),
        ("status", (n_pops, members), np.int32), ("best", n_pops, np.int32), ("nit", n_pops, np.int32),
        ("converged", n_pops, np.int32), ("nfev", n_pops, np.int64)])


def initial_ball(res, nwalkers, scale=1.0e-4, seed=0):
    """Starting walkers around a best fit: res.x + scale x N(0, 1) per coordinate (the reference's p0 + 1e-4 randn,
    code/synthetic_datasets/synth_mcmc.py), clipped into the result's bounds box; (nwalkers, ndim)."""
    if int(nwalkers) != nwalkers or nwalkers < 1:
        raise ValueError("nwalkers must be a positive integer")
    x = np.asarray(res["x"], dtype=np.float64)
    pos = x + float(scale) * np.random.default_rng(seed).standard_normal((int(nwalkers), x.size))
    b = res.get("bounds")
    return pos if b is None else np.clip(pos, b[:, 0], b[:, 1])
