"""Evidence and posterior samples on the GPU without a temperature ladder: sequential Monte Carlo over the tempering path
prior x L^beta (Del Moral, Doucet & Jasra 2006; the scheme of PyMC's sample_smc and of pocoMC), device-resident.

N particles per run start as uniform draws in the prior box (beta = 0) and end as N equally weighted posterior samples
(beta = 1).  Every stage is one stage launch (reweight; the next beta from the particles' own weights by an effective-sample-size
rule; ln Z advances; systematic resampling) and one move launch (every slot walks `walks` tempered Metropolis steps from its
ancestor, its DE proposals drawn over the resampled population); include/magprop_amd.h mp_smc_* states the arithmetic.  It needs
no starting ball, no burn-in, no autocorrelation time and no ladder.

The prior is uniform over a box in sampler coordinates, as for ``NestedSampler``.  Particles whose model fails have lnl = -inf:
they carry no weight and die at the first stage, and since ln Z divides by every particle the first stage carries ln f_valid by
itself.
"""
import math

import numpy as np

from . import _capi, resident, summaries

TARGETS = {"posterior": 0, "gaussian": 1, "terraced": 2}
STATUS = ("running", "done", "failed", "stage_limit")


class Results(resident.OptimizeResult):
    """The outcome of one run as a dict whose keys are also attributes."""


# The adaptive moves' defaults, chosen from the sweep of tools/smc_bench.py: rounds of WALKS_ADAPTIVE steps
# until every dimension's correlation with the start of the stage is at most corr, at most max_rounds rounds.
ADAPT_DEFAULTS = dict(min_rounds=1, max_rounds=80, corr=0.5, gain=1.0, accept_target=0.234, g_min=0.0, g_max=0.0)
WALKS_FIXED, WALKS_ADAPTIVE = 10, 2


def _check_adapt(adapt, walks, g0):
    """The settings of mp_smc_set_adaptive as a dict (None: adaptation off) from adapt = False, True or a dict of overrides;
    g0 is the scale the library will keep."""
    if adapt is None or adapt is False:
        return None
    if adapt is True:
        adapt = {}
    if not isinstance(adapt, dict) or set(adapt) - set(ADAPT_DEFAULTS):
        raise ValueError(f"adapt must be False, True or a dict with keys among {tuple(ADAPT_DEFAULTS)}, got {adapt!r}")
    a = {**ADAPT_DEFAULTS, **adapt}
    for k in ("min_rounds", "max_rounds"):
        if isinstance(a[k], bool) or int(a[k]) != a[k]:
            raise ValueError(f"adapt: {k} must be an integer")
        a[k] = int(a[k])
    if not 1 <= a["min_rounds"] <= a["max_rounds"]:
        raise ValueError("adapt: min_rounds must lie in 1 .. max_rounds")
    if walks * a["max_rounds"] > _capi.SMC_MAX_WALKS:
        raise ValueError(f"adapt: walks * max_rounds must be <= {_capi.SMC_MAX_WALKS}")
    if not 0.0 <= a["corr"] < 1.0:
        raise ValueError("adapt: corr must lie in [0, 1)")
    if not (np.isfinite(a["gain"]) and a["gain"] >= 0.0):
        raise ValueError("adapt: gain must be finite and >= 0")
    if not 0.0 < a["accept_target"] < 1.0:
        raise ValueError("adapt: accept_target must lie in (0, 1)")
    lo = a["g_min"] if a["g_min"] > 0.0 else g0 / 16.0
    hi = a["g_max"] if a["g_max"] > 0.0 else 4.0 * g0
    if not (np.isfinite(lo) and np.isfinite(hi) and lo <= g0 <= hi):
        raise ValueError("adapt: need 0 < g_min <= g0 <= g_max, finite (<= 0: g0 / 16 and 4 g0)")
    return {k: (a[k] if k.endswith("rounds") else float(a[k])) for k in ADAPT_DEFAULTS}


def _check_args(x, datasets, nparticles, walks, ess, variant, ndim, bounds, n_runs, g0, sigma, target, adapt=False):
    """(box lower, box upper, prior lower, prior upper, log mask, number of datasets, target code, adaptation settings or
    None): every check, no device touched."""
    if target in TARGETS:
        target = TARGETS[target]
    if target not in TARGETS.values() or isinstance(target, bool):
        raise ValueError(f"target must be one of {tuple(TARGETS)} (or 0, 1, 2), got {target!r}")
    if int(nparticles) != nparticles or not _capi.SMC_MIN_PARTICLES <= nparticles <= _capi.SMC_MAX_PARTICLES:
        raise ValueError(f"nparticles must be an integer in {_capi.SMC_MIN_PARTICLES} .. {_capi.SMC_MAX_PARTICLES}")
    if int(walks) != walks or not 1 <= walks <= _capi.SMC_MAX_WALKS:
        raise ValueError(f"walks must be an integer in 1 .. {_capi.SMC_MAX_WALKS}")
    if not 0.0 < ess < 1.0:
        raise ValueError("ess must lie in (0, 1)")
    if not np.isfinite(g0):
        raise ValueError("g0 must be finite (<= 0: 2.38 / sqrt(2 ndim))")
    if not 0.0 <= sigma < 1.0 / math.sqrt(3.0):
        raise ValueError("sigma must lie in [0, 1/sqrt(3))")
    if int(n_runs) != n_runs or n_runs < 1:
        raise ValueError("n_runs must be a positive integer")
    lo, hi, plo, phi, mask, n_ds = resident.check_box_and_runs(x, datasets, variant, ndim, bounds, n_runs, target == 0,
                                                               "the gaussian targets need bounds")
    adapt = _check_adapt(adapt, int(walks), g0 if g0 > 0.0 else 2.38 / math.sqrt(2.0 * lo.size))
    return lo, hi, plo, phi, mask, n_ds, int(target), adapt


class SMCSampler(resident.BoxSampler):
    """Tempered SMC of the log-posterior of light curve (x, y, yerr), or of every light curve of datasets=[(x, y, yerr), ...],
    under a uniform prior over a box, on the GPU.

    nparticles particles per run (4 .. 16 384); a stage raises beta until the effective sample size of the incremental weights
    falls to ess x (the particles with a finite lnprob), resamples, and moves every particle `walks` Metropolis steps against
    prior x L^beta with DE proposals gamma = g0 (1 + sigma sqrt(3) (2u - 1)) (g0 <= 0: 2.38 / sqrt(2 ndim)) along differences of
    the resampled population.  variant / ndim / GRBtype / bounds follow NestedSampler (default box: the variant's prior box).
    n_runs: independent runs per dataset, all in one launch per stage (run index = dataset index x n_runs + run); they differ by
    their index in the Philox key and by their prior draws.  seed keys both the prior draws (numpy) and the device (Philox).
    target 1 / "gaussian" samples the isotropic unit Gaussian -0.5 sum x^2 in `bounds`, 2 / "terraced" the same on terraces
    (tests, measurements).
    adapt=True (or a dict overriding ADAPT_DEFAULTS: min_rounds, max_rounds, corr, gain, accept_target, g_min, g_max) lets every
    run choose its move length and scale on the device (mp_smc_set_adaptive): `walks` is then the length of a round (default 2
    where the fixed-length move's is 10), a stage's
    moves go on round after round until the correlation between where the slots started and where they are has fallen to corr
    in every dimension (at most max_rounds rounds), and the run's g follows the stage's acceptance towards accept_target.  The
    results gain rounds, scale and rho per stage.  adapt=False (the default) is the fixed-length run, unchanged."""

    POSTERIOR, NOT_RUN, NO_MODEL = 0, "run first", "the gaussian targets have no"

    def __init__(self, x=None, y=None, yerr=None, nparticles=1024, walks=None, ess=0.5, variant="synth", ndim=6, GRBtype=None,
                 bounds=None, seed=0, n_runs=1, datasets=None, g0=0.0, sigma=0.1, target=0, device=-1, log_mask=None, adapt=False):
        if walks is None:                   # 10 steps per move; with adaptation rounds of 2
            walks = WALKS_FIXED if adapt is None or adapt is False else WALKS_ADAPTIVE
        lo, hi, plo, phi, mask, n_ds, target, adapt = _check_args(x, datasets, nparticles, walks, ess, variant, ndim, bounds,
                                                                  n_runs, g0, sigma, target, adapt)
        self.adapt = adapt
        self.lower, self.upper = lo, hi
        self.ndim = lo.size
        self.nparticles, self.walks, self.ess = int(nparticles), int(walks), float(ess)
        self.variant, self.GRBtype, self.target = variant, GRBtype, target
        self.datasets = [] if target != 0 else (list(datasets) if datasets is not None else [(x, y, yerr)])
        self.runs_per_dataset = int(n_runs)
        self.n_runs = n_ds * int(n_runs)
        self.run_ds = np.repeat(np.arange(n_ds, dtype=np.int32), int(n_runs))
        self.seed, self.g0, self.sigma, self.device = int(seed), float(g0), float(sigma), device
        self._prior = (plo, phi, mask if log_mask is None else log_mask)
        self.handle = None
        self.results = None

    def initial_particles(self):
        """particles[n_runs, nparticles, ndim]: uniform box draws from np.random.default_rng(seed), run after run.  Every draw is
        kept: one whose model fails weighs nothing at the first stage, which is how ln Z comes to hold ln f_valid."""
        rng = np.random.default_rng(self.seed)
        lo, hi = self.lower, self.upper
        return lo + (hi - lo) * rng.random((self.n_runs, self.nparticles, self.ndim))

    def run(self, max_stages=None):
        """Run every run to beta = 1 (or for max_stages stages); fills .results (a Results for one run, else a list in run
        order): samples (nparticles, ndim) equally weighted, logl (their untempered lnprob), logz, logzerr (the standard error
        of the mean over the runs that share the run's dataset; NaN for a single run: no single-run error is made up), beta,
        betas / ess / accept / ncall_stage (per stage: the new beta, the effective sample size at it, the accepted share of the
        stage's N walks proposals, its evaluations), ncall (all evaluations, the first N included), nacc, nfail (evaluations
        whose model failed), rounds / scale / rho (per stage: the rounds of `walks` steps its moves made, the DE scale they used
        and the correlation at which they stopped; without adaptation 1, g0 and NaN, and with it accept counts the proposals
        of all rounds), nstages and status ("done", "running" when max_stages ended it, "failed": no particle had a finite
        lnprob, "stage_limit")."""
        if max_stages is not None and (int(max_stages) != max_stages or max_stages < 0):
            raise ValueError("max_stages must be an integer >= 0")
        self._open()
        x0 = self.initial_particles()
        L = _capi.lib()
        with _capi.Driver("mp_smc", self.handle, self.nparticles, self.n_runs, self.ndim, _capi.ptr(self.run_ds), self.seed,
                          _capi.ptr(self.lower), _capi.ptr(self.upper), self.ess, self.walks, self.g0, self.sigma,
                          self.target) as s:
            if self.adapt is not None:
                _capi.check(L.mp_smc_set_adaptive(s, *(self.adapt[k] for k in ADAPT_DEFAULTS)), "mp_smc_set_adaptive")
            _capi.check(L.mp_smc_set_particles(s, _capi.ptr(np.ascontiguousarray(x0))), "mp_smc_set_particles")
            _capi.check(L.mp_smc_run(s, 2 ** 31 - 1 if max_stages is None else int(max_stages), None), "mp_smc_run")
            st = get_state(L, s, self.n_runs, self.nparticles, self.ndim)
            logs = [get_stages(L, s, r) for r in range(self.n_runs)]
            tunes = [get_tuning(L, s, r) for r in range(self.n_runs)]
        k = self.runs_per_dataset
        out = []
        for r in range(self.n_runs):
            group = st["lnz"][(r // k) * k:(r // k + 1) * k]
            err = float(np.std(group, ddof=1) / math.sqrt(k)) if k > 1 else float("nan")
            log = logs[r]
            out.append(Results(
                samples=st["x"][r], logl=st["lnl"][r], logz=float(st["lnz"][r]), logzerr=err, beta=float(st["beta"][r]),
                betas=log["beta"], ess=log["ess"], accept=log["accept"], ncall_stage=log["ncall"], ncall=int(st["ncall"][r]),
                nacc=int(st["nacc"][r]), nfail=int(st["nfail"][r]), nstages=int(st["nstage"][r]),
                status=STATUS[int(st["run_status"][r])], particle_status=st["status"][r],
                rounds=tunes[r]["rounds"], scale=tunes[r]["g"], rho=tunes[r]["rho"]))
        self.results = out[0] if self.n_runs == 1 else out
        return self.results

    def _rows(self, name, run):
        """The samples of run `run` for the front end `name`: equally weighted, so every summary takes them without weights."""
        self._need_posterior(name)
        return self._run(run).samples

    def get_model_band(self, q=(0.025, 0.5, 0.975), components=("Ltot",), run=0):
        """Posterior-predictive band of run `run` on this sampler's handle: the quantiles q of the model light curves of its
        samples (mp_model_band).  Returns {"t": grid, "Ltot": (nq, n_grid), ..., "n_used": rows that entered}."""
        return summaries.band(summaries.on(self.handle), self._rows("get_model_band", run), q, components)

    def get_derived(self, q=(0.16, 0.5, 0.84), run=0):
        """Energy budgets and light-curve landmarks of run `run` (magprop_amd.derived.NAMES) over its samples (mp_model_derived):
        {"values": (n, 16), "status", "n_used", "summary": derived.summarize(values, q)}."""
        return summaries.derived(summaries.on(self.handle), self._rows("get_derived", run), q)

    def get_flows(self, q=(0.16, 0.5, 0.84), run=0, curves=()):
        """Mass budget, angular-momentum budget and regime of run `run` (magprop_amd.flows.NAMES) over its samples
        (mp_model_flows), and the cell curves named in `curves`."""
        return summaries.flows(summaries.on(self.handle), self._rows("get_flows", run), q, None, curves)

    def get_flow_band(self, q=(0.025, 0.5, 0.975), curves=("fastness",), run=0):
        """Bands of the radii, mass-flow rates and torques of run `run` over its samples (mp_model_flow_band)."""
        return summaries.flow_band(summaries.on(self.handle), self._rows("get_flow_band", run), q, curves)

    def get_pointwise(self, run=0):
        """Pointwise predictive scores (PSIS-LOO, WAIC) of run `run` over its samples against the run's dataset, in the order
        the dataset was given (mp_model_pointwise)."""
        rows = self._rows("get_pointwise", run)
        ds = int(self.run_ds[int(run)])
        return summaries.pointwise(summaries.on(self.handle, ds, np.asarray(self.datasets[ds][0], dtype=np.float64)), rows)


def get_state(L, s, n_runs, n, ndim):
    """mp_smc_get_state as arrays: x (n_runs, n, ndim), lnl / status / acc (n_runs, n), per run beta, lnz, nstage, run_status,
    ncall, nacc, nfail."""
    f8, i4, i8 = np.float64, np.int32, np.int64
    return _capi.read_back(L.mp_smc_get_state, s, [
        ("x", (n_runs, n, ndim), f8), ("lnl", (n_runs, n), f8), ("status", (n_runs, n), i4), ("acc", (n_runs, n), i4),
        ("beta", n_runs, f8), ("lnz", n_runs, f8), ("nstage", n_runs, i4), ("run_status", n_runs, i4), ("ncall", n_runs, i8),
        ("nacc", n_runs, i8), ("nfail", n_runs, i8)])


def get_stages(L, s, run):
    """mp_smc_get_stages of one run: {"beta", "d", "ess", "lnz", "accept", "ncall"}, one entry per stage."""
    f8 = np.float64
    none = [(k, None, None) for k in ("beta", "d", "ess", "lnz", "accept", "ncall")]
    n = int(_capi.read_back(L.mp_smc_get_stages, s, none + [("n", (), np.int32)], int(run), 0)["n"])
    d = _capi.read_back(L.mp_smc_get_stages, s, [("beta", n, f8), ("d", n, f8), ("ess", n, f8), ("lnz", n, f8), ("accept", n, f8),
                                                 ("ncall", n, np.int64), ("n", (), np.int32)], int(run), n)
    d.pop("n")
    return d


def get_tuning(L, s, run):
    """mp_smc_get_tuning of one run: {"rounds", "g", "rho"}, one entry per stage (without adaptation 1, g0 and NaN)."""
    none = [(k, None, None) for k in ("rounds", "g", "rho")]
    n = int(_capi.read_back(L.mp_smc_get_tuning, s, none + [("n", (), np.int32)], int(run), 0)["n"])
    d = _capi.read_back(L.mp_smc_get_tuning, s, [("rounds", n, np.int32), ("g", n, np.float64), ("rho", n, np.float64),
                                                 ("n", (), np.int32)], int(run), n)
    d.pop("n")
    return d


def get_ancestors(L, s, n_runs, n):
    """mp_smc_get_ancestors: anc (n_runs, n) of every run's last stage."""
    return _capi.read_back(L.mp_smc_get_ancestors, s, [("anc", (n_runs, n), np.int32)])["anc"]
