"""Evidence and posterior samples on the GPU: nested sampling (Skilling 2006) with batch removal, device-resident.

Every iteration of every run is one select launch (the K lowest live points die; ln X and ln Z advance) and one walk launch
(each dead slot is refilled from a survivor by a constrained DE random walk, or with sample="slice" by slice updates along
survivor differences); the host reads the dead points back once per chunk of iterations (include/magprop_amd.h mp_nested_*).  The final estimate is host-side and pure: ``add_live``, ``estimate`` and
``resample_equal`` need no device, after dynesty's ``add_live`` and ``resample_equal``.

The prior is uniform over a box in sampler coordinates, as for ``EnsembleSampler.log_evidence``.  The live set starts from
uniform box draws with a finite lnprob, so the run integrates over the region where the model succeeds and
ln Z = ln Z_ns + ln f_valid (``tempering.validity_term``).
"""
import math
import warnings

import numpy as np

from . import _capi, resident, summaries, tempering

TARGETS = {"posterior": 0, "gaussian": 1}
SAMPLES = ("rwalk", "slice")
MAX_DRAW_ROUNDS = 4096


class Results(resident.OptimizeResult):
    """dynesty's result names as a dict whose keys are also attributes (one run)."""


def add_live(lnx_final, live_lnl):
    """dynesty's add_live: the N live points in ascending lnL with volumes X_final (1 - j / (N + 1)), j = 1 .. N; returns
    (order, ln X of every one, ln w of every one), ln w_j = lnL_j + ln(X_{j-1} - X_j) = lnL_j + ln X_final - ln(N + 1)."""
    lnl = np.asarray(live_lnl, dtype=np.float64)
    n = lnl.size
    order = np.lexsort((np.arange(n), lnl))
    j = np.arange(1, n + 1)
    lnx = float(lnx_final) + np.log1p(-j / (n + 1.0))
    lnw = lnl[order] + float(lnx_final) - math.log(n + 1.0)
    return order, lnx, lnw


def dead_weights(dead_lnl, dead_n):
    """(ln X after each dead point, ln w of each) of the dead sequence: ln X_i = ln X_{i-1} - 1 / n_i,
    ln w_i = lnL_i + ln X_{i-1} + ln(-expm1(-1 / n_i)), from ln X_0 = 0."""
    lnl = np.asarray(dead_lnl, dtype=np.float64)
    inv = 1.0 / np.asarray(dead_n, dtype=np.float64)
    lnx = -np.cumsum(inv)
    prev = np.concatenate([[0.0], lnx[:-1]])
    return lnx, lnl + prev + np.log(-np.expm1(-inv))


def _logsumexp(a):
    a = np.asarray(a, dtype=np.float64)
    m = np.max(a) if a.size else -np.inf
    if not np.isfinite(m):
        return float(m)
    return float(m + np.log(np.sum(np.exp(a - m))))


def estimate(dead_lnl, dead_n, live_lnl, nlive, ln_f_valid=0.0, dln_f_valid=0.0):
    """ln Z, its error, the information H and the weighted sequence of one run.  Dead points then the live points (add_live);
    p_i = w_i / Z, H = sum p_i ln(L_i / Z), dlnZ = sqrt(H / nlive) combined in quadrature with the error of ln f_valid.
    Returns a dict: logz, logzerr, information, logl, logwt, logvol, order (indices into the live set of the appended rows)."""
    lnx, lnw_d = dead_weights(dead_lnl, dead_n)
    lnx_final = float(lnx[-1]) if lnx.size else 0.0
    order, lnx_l, lnw_l = add_live(lnx_final, live_lnl)
    logl = np.concatenate([np.asarray(dead_lnl, dtype=np.float64), np.asarray(live_lnl, dtype=np.float64)[order]])
    logwt = np.concatenate([lnw_d, lnw_l])
    logz = _logsumexp(logwt)
    if not np.isfinite(logz):
        raise ValueError("every weight is zero: no live or dead point has a finite lnL")
    p = np.exp(logwt - logz)
    keep = p > 0.0
    h = float(max(np.sum(p[keep] * (logl[keep] - logz)), 0.0))
    err = math.sqrt(h / int(nlive) + float(dln_f_valid) ** 2)
    return {"logz": logz + float(ln_f_valid), "logzerr": err, "information": h, "logl": logl, "logwt": logwt,
            "logvol": np.concatenate([lnx, lnx_l]), "order": order}


def resample_equal(samples, logwt, rng=None):
    """Systematic resampling to equal weights (dynesty's resample_equal): n = len(samples) positions (u + i) / n, i = 0 .. n-1,
    one uniform u, against the cumulative normalised weights; the picked rows in random order."""
    samples = np.asarray(samples)
    w = np.exp(np.asarray(logwt, dtype=np.float64) - _logsumexp(logwt))
    if samples.shape[0] != w.size or w.size == 0:
        raise ValueError("one log-weight per sample expected")
    rng = np.random.default_rng(rng)
    n = w.size
    cum = np.cumsum(w)
    cum /= cum[-1]
    idx = np.minimum(np.searchsorted(cum, (rng.random() + np.arange(n)) / n, side="right"), n - 1)
    return samples[rng.permutation(idx)]


def band_exact_selection(samples, logwt, cap=None):
    """(rows, weights, weight_dropped) of a weighted band over a run's samples: weights exp(logwt - max); the rows of zero units
    go (weights below 2^-31 of the largest, mp_band_weight_units: the band gives them no part, so leaving them out changes
    nothing), and of more than `cap` (default _capi.BAND_MAX_SAMPLES) remaining rows the heaviest `cap` stay (ties: the earlier
    row), all in the run's order.  weight_dropped is the share of the run's total weight on the rows the cap cut: 0.0 when it cut
    none."""
    samples = np.asarray(samples, dtype=np.float64)
    lw = np.asarray(logwt, dtype=np.float64)
    if samples.ndim != 2 or lw.shape != (samples.shape[0],) or lw.size == 0:
        raise ValueError("one log-weight per sample expected")
    cap = _capi.BAND_MAX_SAMPLES if cap is None else int(cap)
    w = np.exp(lw - np.max(lw))
    units = np.floor(w * 2147483648.0)              # (max(w) == 1.0: the ratio of mp_band_weight_units is w itself)
    keep = np.nonzero(units > 0)[0]
    dropped = 0.0
    if keep.size > cap:
        order = np.argsort(-w[keep], kind="stable")
        dropped = float(np.sum(w[np.sort(keep[order[cap:]])])) / float(np.sum(w))
        keep = np.sort(keep[order[:cap]])
    return np.ascontiguousarray(samples[keep]), w[keep], dropped


def _check_args(x, datasets, nlive, nbatch, walks, variant, ndim, bounds, n_runs, g0, sigma, target):
    """(box lower, box upper, prior lower, prior upper, log mask, nbatch, number of datasets): every check, no device touched."""
    if target not in TARGETS:
        raise ValueError(f"target must be one of {tuple(TARGETS)}, got {target!r}")
    if int(nlive) != nlive or not _capi.NEST_MIN_LIVE <= nlive <= _capi.NEST_MAX_LIVE:
        raise ValueError(f"nlive must be an integer in {_capi.NEST_MIN_LIVE} .. {_capi.NEST_MAX_LIVE}")
    nbatch = max(1, int(nlive) // 4) if nbatch is None else nbatch
    if int(nbatch) != nbatch or not 1 <= nbatch <= nlive // 2:
        raise ValueError("nbatch must be an integer in 1 .. nlive // 2")
    if int(walks) != walks or not 1 <= walks <= _capi.NEST_MAX_WALKS:
        raise ValueError(f"walks must be an integer in 1 .. {_capi.NEST_MAX_WALKS}")
    if not np.isfinite(g0):
        raise ValueError("g0 must be finite (<= 0: 2.38 / sqrt(2 ndim))")
    if not 0.0 <= sigma < 1.0 / math.sqrt(3.0):
        raise ValueError("sigma must lie in [0, 1/sqrt(3))")
    if int(n_runs) != n_runs or n_runs < 1:
        raise ValueError("n_runs must be a positive integer")
    lo, hi, plo, phi, mask, n_ds = resident.check_box_and_runs(x, datasets, variant, ndim, bounds, n_runs, target == "posterior",
                                                               "the gaussian target needs bounds")
    return lo, hi, plo, phi, mask, int(nbatch), n_ds


def _check_slice(sample, slices, slice_mu, max_steps_out, max_shrink, ndim):
    """Slice updates per walk (0 for the random walk): every check of the walk method, no device touched."""
    if sample not in SAMPLES:
        raise ValueError(f"sample must be one of {SAMPLES}, got {sample!r}")
    if not (isinstance(slice_mu, (int, float, np.floating, np.integer)) and np.isfinite(slice_mu) and slice_mu > 0.0):
        raise ValueError("slice_mu must be finite and > 0")
    if int(max_steps_out) != max_steps_out or not 1 <= max_steps_out <= _capi.NEST_MAX_STEPS_OUT:
        raise ValueError(f"max_steps_out must be an integer in 1 .. {_capi.NEST_MAX_STEPS_OUT}")
    if int(max_shrink) != max_shrink or not 1 <= max_shrink <= _capi.NEST_MAX_SHRINK:
        raise ValueError(f"max_shrink must be an integer in 1 .. {_capi.NEST_MAX_SHRINK}")
    if sample == "rwalk":
        if slices is not None:
            raise ValueError("slices applies to sample='slice' only")
        return 0
    slices = ndim if slices is None else slices
    if int(slices) != slices or not 1 <= slices <= _capi.NEST_MAX_SLICES:
        raise ValueError(f"slices must be an integer in 1 .. {_capi.NEST_MAX_SLICES}")
    return int(slices)


class NestedSampler(resident.BoxSampler):
    """Nested sampling of the log-posterior of light curve (x, y, yerr), or of every light curve of datasets=[(x, y, yerr), ...],
    under a uniform prior over a box, on the GPU.

    nlive live points per run (16 .. 4096); nbatch of them die per iteration (1 .. nlive // 2; default nlive // 4) and are
    replaced by constrained random walks of `walks` DE steps (gamma = g0 (1 + sigma sqrt(3) (2u - 1)), g0 <= 0: 2.38 / sqrt(2
    ndim)) whose difference vectors come from the surviving live points.  variant / ndim / GRBtype / bounds follow
    optimize.differential_evolution (default box: the variant's prior box).  n_runs: independent runs per dataset, all in one
    launch per iteration (run index = dataset index x n_runs + run).  seed keys both the live-set draws (numpy) and the device's
    walks (Philox).  target="gaussian" samples the isotropic unit Gaussian -0.5 sum x^2 in `bounds` (tests, measurements).

    sample="slice" replaces the random walk by `slices` slice updates per walk (default ndim; dynesty's sample="slice" with the
    directions of ensemble slice sampling): each slice runs along the difference of two survivors, starts from an interval of
    slice_mu differences at a random offset, steps out with Neal's budget max_steps_out and shrinks at most max_shrink times (a
    slice that reaches the cap, or draws two coinciding survivors, stays where it started and counts as failed).  It needs no
    step size and moves on every slice that does not fail; walks, g0 and sigma are then unused."""

    POSTERIOR, NOT_RUN, NO_MODEL = "posterior", "run_nested first", "the gaussian target has no"

    def __init__(self, x=None, y=None, yerr=None, nlive=500, nbatch=None, walks=25, variant="synth", ndim=6, GRBtype=None,
                 datasets=None, n_runs=1, seed=0, bounds=None, log_mask=None, g0=0.0, sigma=0.1, target="posterior", device=-1,
                 sample="rwalk", slices=None, slice_mu=1.0, max_steps_out=8, max_shrink=64):
        lo, hi, plo, phi, mask, nbatch, n_ds = _check_args(x, datasets, nlive, nbatch, walks, variant, ndim, bounds, n_runs, g0,
                                                            sigma, target)
        self.slices = _check_slice(sample, slices, slice_mu, max_steps_out, max_shrink, lo.size)
        self.sample, self.slice_mu = sample, float(slice_mu)
        self.max_steps_out, self.max_shrink = int(max_steps_out), int(max_shrink)
        self.lower, self.upper = lo, hi
        self.ndim = lo.size
        self.nlive, self.nbatch, self.walks = int(nlive), nbatch, int(walks)
        self.variant, self.GRBtype, self.target = variant, GRBtype, target
        self.datasets = [] if target == "gaussian" else (list(datasets) if datasets is not None else [(x, y, yerr)])
        self.n_runs = n_ds * int(n_runs)
        self.run_ds = np.repeat(np.arange(n_ds, dtype=np.int32), int(n_runs))
        self.seed, self.g0, self.sigma, self.device = int(seed), float(g0), float(sigma), device
        self._prior = (plo, phi, mask if log_mask is None else log_mask)
        self.handle = None
        self.results = None

    def initial_live(self):
        """(live[n_runs, nlive, ndim], prior draws per run): uniform box draws from np.random.default_rng(seed), run after run;
        the first nlive with a finite lnprob are kept, and the draws up to the last one kept are counted."""
        rng = np.random.default_rng(self.seed)
        n, lo, hi = self.nlive, self.lower, self.upper
        live = np.empty((self.n_runs, n, self.ndim))
        draws = np.zeros(self.n_runs, dtype=np.int64)
        for r in range(self.n_runs):
            if self.target == "gaussian":
                live[r] = lo + (hi - lo) * rng.random((n, self.ndim))
                draws[r] = n
                continue
            got = 0
            for _ in range(MAX_DRAW_ROUNDS):
                P = lo + (hi - lo) * rng.random((2 * n, self.ndim))
                ok = np.isfinite(self.handle.lnprob_batch(P, ds_id=int(self.run_ds[r])))
                idx = np.nonzero(ok)[0][:n - got]
                live[r, got:got + idx.size] = P[idx]
                got += idx.size
                draws[r] += (idx[-1] + 1) if got == n else P.shape[0]
                if got == n:
                    break
            else:
                raise RuntimeError(f"run {r}: fewer than {n} finite draws in {MAX_DRAW_ROUNDS * 2 * n} uniform box draws")
        return live, draws

    def run_nested(self, dlogz=0.01, maxiter=None):
        """Run every run until log1p(exp(lnL_max + ln X - ln Z)) < dlogz, or for maxiter iterations; fills .results (a Results
        for one run, else a list in run order): logz, logzerr, information, samples, logl, logwt, logvol, niter (iterations of
        nbatch dead points), ncall (prior draws of the live set plus evaluations inside walks), eff (100 x dead points / ncall),
        nzero (walks that accepted nothing; slice mode: walks in which no slice moved), nacc (accepted steps; slice mode: slices
        that moved), nexpand / ncontract / nfail (slice mode: stepping-out steps, rejected shrink points, failed slices; 0 for
        the random walk), ln_f_valid, samples_n (live count of every row), stopped.  Warns (RuntimeWarning) when more than 1 %
        of the walks accepted nothing (random walk) or more than 1 % of the slices failed (slice mode)."""
        if not (np.isfinite(dlogz) and dlogz > 0.0):
            raise ValueError("dlogz must be finite and > 0")
        if maxiter is not None and (int(maxiter) != maxiter or maxiter < 0):
            raise ValueError("maxiter must be an integer >= 0")
        self._open()
        live0, draws = self.initial_live()
        L = _capi.lib()
        with _capi.Driver("mp_nested", self.handle, self.nlive, self.nbatch, self.n_runs, self.ndim, _capi.ptr(self.run_ds),
                          self.seed, self.walks, self.g0, self.sigma, float(dlogz), _capi.ptr(self.lower), _capi.ptr(self.upper),
                          TARGETS[self.target]) as ns:
            if self.slices:
                _capi.check(L.mp_nested_set_slice(ns, self.slices, self.slice_mu, self.max_steps_out, self.max_shrink),
                            "mp_nested_set_slice")
            _capi.check(L.mp_nested_set_live(ns, _capi.ptr(np.ascontiguousarray(live0))), "mp_nested_set_live")
            _capi.check(L.mp_nested_run(ns, 2 ** 31 - 1 if maxiter is None else int(maxiter), None), "mp_nested_run")
            st = get_state(L, ns, self.n_runs, self.nlive, self.ndim)
            st.update(get_slice_stats(L, ns, self.n_runs))
            dead = [get_dead(L, ns, r, self.ndim) for r in range(self.n_runs)]
        out = []
        for r in range(self.n_runs):
            lnf, dlnf = tempering.validity_term(self.nlive, draws[r]) if self.target == "posterior" else (0.0, 0.0)
            pars, lnl, nl = dead[r]
            est = estimate(lnl, nl, st["lnl"][r], self.nlive, lnf, dlnf)
            samples = np.concatenate([pars, st["live"][r][est["order"]]])
            n_dead = lnl.size
            ncall = int(draws[r]) + int(st["ncall"][r])
            walks_run = int(st["nit"][r]) * self.nbatch
            nzero, nfail = int(st["nzero"][r]), int(st["nfail"][r])
            if self.slices:
                slices_run = walks_run * self.slices
                if slices_run and nfail > 0.01 * slices_run:
                    warnings.warn(f"run {r}: {nfail} of {slices_run} slices failed (shrink cap or coinciding survivors): the "
                                  "live set may be poorly mixed (a larger max_shrink, or a smaller slice_mu)", RuntimeWarning,
                                  stacklevel=2)
            elif walks_run and nzero > 0.01 * walks_run:
                warnings.warn(f"run {r}: {nzero} of {walks_run} walks accepted no step: the live set may be poorly mixed "
                              "(more walks, or a smaller g0)", RuntimeWarning, stacklevel=2)
            out.append(Results(
                logz=est["logz"], logzerr=est["logzerr"], information=est["information"], samples=samples, logl=est["logl"],
                logwt=est["logwt"], logvol=est["logvol"], niter=int(st["nit"][r]), ncall=ncall,
                eff=100.0 * n_dead / max(ncall, 1), nzero=nzero, nacc=int(st["nacc"][r]), nexpand=int(st["nexpand"][r]),
                ncontract=int(st["ncontract"][r]), nfail=nfail, ln_f_valid=lnf,
                samples_n=np.concatenate([nl, np.arange(self.nlive, 0, -1)]), stopped=bool(st["stopped"][r]),
                device_logz=float(st["lnz"][r])))
        self.results = out[0] if self.n_runs == 1 else out
        return self.results

    def resample_equal(self, run=0, seed=None):
        """Equal-weight posterior samples of run `run` (systematic resampling of its weighted sequence)."""
        r = self._run(run)
        return resample_equal(r.samples, r.logwt, self.seed if seed is None else seed)

    def _summary_rows(self, name, run, weights=None):
        """(rows, weights, extra entries of the result) of run `run` for the front end `name`.  A band ("..._band") takes weights
        "exact": band_exact_selection of the run's samples, "weight_dropped" in the result and a RuntimeWarning above 1e-3; or
        "resample": its equal-weight samples, evenly thinned to _capi.BAND_MAX_SAMPLES, no weights.  Every other summary takes all
        of the run's samples under exp(logwt - max(logwt))."""
        self._need_posterior(name)
        if not name.endswith("band"):
            r = self._run(run)
            return r.samples, np.exp(r.logwt - np.max(r.logwt)), {}
        if weights not in ("resample", "exact"):
            raise ValueError(f"weights must be 'resample' or 'exact', got {weights!r}")
        if weights == "exact":
            r = self._run(run)
            rows, w, dropped = band_exact_selection(r.samples, r.logwt)
            if dropped > 1.0e-3:
                warnings.warn(f"run {run}: the {rows.shape[0]} heaviest samples leave {dropped:.2e} of the weight out of the band",
                              RuntimeWarning, stacklevel=3)
            return rows, w, {"weight_dropped": dropped}
        rows = self.resample_equal(run)
        if rows.shape[0] > _capi.BAND_MAX_SAMPLES:
            rows = rows[np.linspace(0, rows.shape[0] - 1, _capi.BAND_MAX_SAMPLES).astype(int)]
        return rows, None, {}

    def get_model_band(self, q=(0.025, 0.5, 0.975), components=("Ltot",), run=0, weights="resample"):
        """Posterior-predictive band of run `run` on this sampler's handle.  weights="resample" (the default): the quantiles q
        of the model light curves of its equal-weight samples (at most _capi.BAND_MAX_SAMPLES, evenly thinned; mp_model_band).
        Returns {"t": grid, "Ltot": (nq, n_grid), ..., "n_used": rows that entered}.  weights="exact": no resampling -- the
        run's own samples under their weights (band_exact_selection; mp_model_band_weighted), a function of the run alone; the
        result also holds "n_eff" (Kish's effective sample size of the rows that entered) and "weight_dropped", the share of
        the run's weight on rows the cap of _capi.BAND_MAX_SAMPLES cut (a RuntimeWarning above 1e-3)."""
        rows, w, extra = self._summary_rows("get_model_band", run, weights)
        return summaries.band(summaries.on(self.handle), rows, q, components, w, extra=extra)

    def get_derived(self, q=(0.16, 0.5, 0.84), run=0):
        """Energy budgets and light-curve landmarks of run `run` (magprop_amd.derived.NAMES): the model of every one of its
        weighted samples, evaluated and reduced on this sampler's handle (mp_model_derived), and the quantiles q under the
        samples' weights exp(logwt - max(logwt)) (the posterior weights up to a common factor) -- no resampling.  Returns {"values": (n, 16), "status", "n_used",
        "summary": derived.summarize(values, q, weights)}."""
        rows, w, _ = self._summary_rows("get_derived", run)
        return summaries.derived(summaries.on(self.handle), rows, q, w)

    def get_flows(self, q=(0.16, 0.5, 0.84), run=0, curves=()):
        """Mass budget, angular-momentum budget and propeller / accretor regime of run `run` (magprop_amd.flows.NAMES): the
        model of every one of its weighted samples, evaluated and reduced on this sampler's handle (mp_model_flows), and the
        quantiles q under the samples' weights exp(logwt - max(logwt)) -- no resampling.  Returns {"values": (n, 16), "status",
        "n_used", "summary": flows.summarize(values, q, weights)} and the cell curves named in `curves`."""
        rows, w, _ = self._summary_rows("get_flows", run)
        return summaries.flows(summaries.on(self.handle), rows, q, w, curves)

    def get_flow_band(self, q=(0.025, 0.5, 0.975), curves=("fastness",), run=0, weights="exact"):
        """Bands of the radii, mass-flow rates and torques of run `run` (flows.CURVES without "branch"; mp_model_flow_band), with
        get_model_band's two choices of rows: weights="exact" (the default here) the run's own samples under their weights
        (band_exact_selection), with "n_eff" and "weight_dropped" in the result; "resample" its equal-weight samples."""
        rows, w, extra = self._summary_rows("get_flow_band", run, weights)
        return summaries.flow_band(summaries.on(self.handle), rows, q, curves, w, extra=extra)


def get_state(L, ns, n_runs, nlive, ndim):
    """mp_nested_get_state as arrays: live (n_runs, nlive, ndim), lnl / status / acc (n_runs, nlive), per run nit, stopped, lnx,
    lnz, ncall, nacc, nzero."""
    f8, i4, i8 = np.float64, np.int32, np.int64
    return _capi.read_back(L.mp_nested_get_state, ns, [
        ("live", (n_runs, nlive, ndim), f8), ("lnl", (n_runs, nlive), f8), ("status", (n_runs, nlive), i4),
        ("acc", (n_runs, nlive), i4), ("nit", n_runs, i4), ("stopped", n_runs, i4), ("lnx", n_runs, f8), ("lnz", n_runs, f8),
        ("ncall", n_runs, i8), ("nacc", n_runs, i8), ("nzero", n_runs, i8)])


def get_slice_stats(L, ns, n_runs):
    """mp_nested_get_slice_stats as arrays: per run nexpand, ncontract, nfail."""
    return _capi.read_back(L.mp_nested_get_slice_stats, ns, [(k, n_runs, np.int64) for k in ("nexpand", "ncontract", "nfail")])


def get_dead(L, ns, run, ndim):
    """mp_nested_get_dead of one run: (pars[n, ndim], lnl[n], live count[n])."""
    n = int(_capi.read_back(L.mp_nested_get_dead, ns, [("pars", None, None), ("lnl", None, None), ("n_live", None, None),
                                                        ("n", (), np.int64)], int(run), 0)["n"])
    d = _capi.read_back(L.mp_nested_get_dead, ns, [("pars", (n, ndim), np.float64), ("lnl", n, np.float64), ("n_live", n, np.int32),
                                                   ("n", (), np.int64)], int(run), n)
    return d["pars"], d["lnl"], d["n_live"]
