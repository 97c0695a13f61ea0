"""Device-resident ensemble sampler with the slice of emcee's API that the reference driver uses.

`code/synthetic_datasets/synth_mcmc.py:175-226` does

    sampler = em.EnsembleSampler(Nwalk, Npars, lnprob, args=(x, y, yerr, fbad), pool=pool)
    sampler.run_mcmc(pos, Nstep, progress=True)
    sampler.chain[i, j, k]; sampler.lnprobability[i, j]; sampler.acceptance_fraction; sampler.get_autocorr_time()

`EnsembleSampler` here keeps positions, log-posteriors, acceptance counters and the chain in HBM and runs every
stretch-move half-step as one fused kernel (propose -> lnprob -> accept -> store), so there is no host round
trip per half-step.  Several independent ensembles (e.g. one per GRB dataset) can be advanced together.
With a ladder of inverse temperatures (betas=...) every dataset gets one ensemble per temperature and the sampler runs
parallel tempering: tempered decisions in the same fused kernels plus one swap kernel per step (magprop_amd.tempering,
EnsembleSampler.log_evidence).  moves=... selects emcee's differential-evolution and snooker moves, or a weighted mixture
(magprop_amd.moves), proposed inside the same fused half-step kernels.
"""
import ctypes as C

import numpy as np

from . import _capi, bridge, engine, posterior, summaries, tempering
from . import moves as _moves


class EnsembleSampler:
    def __init__(self, nwalkers, ndim=6, x=None, y=None, yerr=None, variant="synth", GRBtype=None, seed=0, a=2.0,
                 datasets=None, lower="default", upper="default", log_mask=None, device=-1, target="posterior",
                 fbad=None, sweep_tol=None, max_stride=None, whole_step=True, betas=None, moves=None, adapt_ladder=None):
        """One ensemble on dataset (x, y, yerr), or one ensemble per entry of `datasets` = [(x, y, yerr), ...].
        whole_step: small ensembles run a whole step per launch (include/magprop_amd.h mp_sampler_set_whole_step; same
        chain bit for bit as one launch per half-step, which False selects).
        fbad: file that receives the proposals whose model failed, like the reference's lnprob(…, fbad)
        (code/synthetic_datasets/mcmc_eqns.py:72-79); written after every run_mcmc call.
        betas: None (untempered, as emcee), or a ladder 1 = beta_0 > beta_1 > ... > 0 (magprop_amd.tempering.check_ladder):
        parallel tempering with one ensemble per (dataset, temperature), nensembles = len(datasets) x T (T for
        target="gaussian"), positions in ensemble order (group g, temperature t: walkers [(g T + t) nwalkers, + nwalkers)).
        moves: None (the stretch move with scale a, as emcee), or emcee's moves= forms over magprop_amd.moves (StretchMove,
        DEMove, DESnookerMove, KDEMove, SliceMove, GaussianMove, WalkMove): a move, a list of moves, or a list of (move, weight); one move is drawn per step
        (include/magprop_amd.h mp_sampler_set_moves).  Give the stretch scale as StretchMove(a) then: moves together with a
        non-default a is refused.
        adapt_ladder: None (the ladder stays as given), or the number of steps over which every group spaces its own ladder on
        the device until its neighbouring pairs swap equally often, both ends fixed (include/magprop_amd.h
        mp_sampler_set_ladder_adaptation), or a dict {"steps", "lag", "time", "history"} (ptemcee's lag = 10000, time = 100;
        history=True keeps the ladder after every update for ladder_history()).  Needs betas= with 3 or more temperatures.  The
        ladder is frozen from step ladder_frozen_at on; estimates belong to those steps (log_evidence refuses earlier ones)."""
        if nwalkers % 2 or nwalkers < 2:
            raise ValueError("nwalkers must be even")            # emcee requires an even number too
        move_tab = None
        if moves is not None:
            if float(a) != 2.0:
                raise ValueError("give the stretch scale as moves=StretchMove(a=...) when moves= is set, not as a=")
            move_tab = _moves.move_table(moves, int(ndim))
            gm = _moves.gaussian_move(_moves.parse_moves(moves))
            gauss_L = None if gm is None else gm.packed_factor(int(ndim))   # (refuses a covariance of another size)
        self.nwalkers, self.ndim = int(nwalkers), int(ndim)
        self._L = _capi.lib()
        lo, hi, mask = engine.prior_box(variant, ndim)   # (no range check of ndim: target="gaussian" takes any)
        if not isinstance(lower, str):
            lo, hi = lower, upper
        if log_mask is not None:
            mask = log_mask
        self.handle = engine.open_handle(variant, GRBtype, device, (lo, hi, mask), (), sweep_tol, max_stride)
        self._prior = (lo, hi)
        self._target = {"posterior": 0, "gaussian": 1}[target]
        if datasets is None:
            datasets = [(x, y, yerr)] if x is not None else []
        if self._target == 0 and not datasets:
            raise ValueError("a dataset is required")
        for k, (dx, dy, de) in enumerate(datasets):
            self.handle.set_dataset(k, dx, dy, de)
        self._times = [np.array(dx, dtype=np.float64) for dx, _, _ in datasets]   # (get_pointwise reports in the caller's order)
        self.betas = None if betas is None else tempering.check_ladder(betas)
        self.ntemps = 1 if self.betas is None else int(self.betas.size)
        self.ngroups = max(1, len(datasets))
        self.nensembles = self.ngroups * self.ntemps
        ids = np.repeat(np.arange(self.ngroups, dtype=np.int32), self.ntemps)   # the temperatures of a group share its dataset
        self._s = _capi.Driver("mp_sampler", self.handle, self.nwalkers, self.nensembles, self.ndim, _capi.ptr(ids), int(seed),
                               float(a), self._target)
        if self.betas is not None:
            _capi.check(self._L.mp_sampler_set_temperatures(self._s, self.ntemps, _capi.ptr(self.betas)), "mp_sampler_set_temperatures")
        self._adapt = None              # (steps, lag, time, history) of the ladder adaptation; None: a fixed ladder
        if adapt_ladder is not None:
            if self.betas is None:
                raise ValueError("adapt_ladder needs a tempered sampler (betas=...)")
            self._adapt = tempering.adaptation_settings(adapt_ladder)
            steps, lag, time, history = self._adapt
            _capi.check(self._L.mp_sampler_set_ladder_adaptation(self._s, steps, lag, time, int(history)),
                        "mp_sampler_set_ladder_adaptation")
        _capi.check(self._L.mp_sampler_set_whole_step(self._s, int(bool(whole_step))), "mp_sampler_set_whole_step")
        self.moves = None if moves is None else _moves.parse_moves(moves)
        if move_tab is not None:
            kinds = np.asarray(move_tab[0], dtype=np.int32)
            weights = np.asarray(move_tab[1], dtype=np.float64)
            params = np.ascontiguousarray(move_tab[2], dtype=np.float64)
            if gm is not None:   # the covariance goes before the table that names the move
                _capi.check(self._L.mp_sampler_set_gaussian(self._s, _capi.ptr(gauss_L), _moves.GAUSS_MODES[gm.mode],
                                                            gm.target_accept), "mp_sampler_set_gaussian")
            _capi.check(self._L.mp_sampler_set_moves(self._s, int(kinds.size), _capi.ptr(kinds), _capi.ptr(weights), _capi.ptr(params)),
                        "mp_sampler_set_moves")
            sl = _moves.slice_move(self.moves)
            if sl is not None:
                _capi.check(self._L.mp_sampler_set_slice_limits(self._s, *sl.limits()), "mp_sampler_set_slice_limits")
        self.seed = int(seed)
        self._chain = None
        self._lnp = None
        self._steps = np.empty(0, dtype=np.int64)   # the step index of every stored row
        self._thermo = False        # the device thermodynamic monitor is on
        self._res = None            # (size, seed, discard) of the device sample reservoir; None: off
        self.iteration = 0
        self.fbad = fbad
        self._bad_written = 0
        self._warned_bad = False
        self._have_positions = False
        self._acf = None            # (max_lag, discard) of the device autocorrelation monitor; None: off
        self._post = None           # (bins, bins2, lower, upper) of the device posterior monitor; None: off
        self.converged = False      # run_mcmc_until
        self.converged_ensembles = None
        self.tau_history = []

    def close(self):
        """Free the sampler, then its handle (garbage collection does the same: the sampler holds the handle)."""
        if getattr(self, "_s", None):
            self._s.close()
        if getattr(self, "handle", None):
            self.handle.close()

    @property
    def ntotal(self):
        return self.nwalkers * self.nensembles

    def run_mcmc(self, pos, nsteps, store=True, progress=False):
        """pos: (nwalkers, ndim) [or (nensembles*nwalkers, ndim)], or None to continue.  Returns the final positions."""
        if pos is not None:
            self.set_positions(pos)
        chain = lnp = None
        cp = lp = None
        if store and nsteps > 0:
            chain = np.empty((nsteps, self.ntotal, self.ndim))
            lnp = np.empty((nsteps, self.ntotal))
            cp, lp = _capi.ptr(chain), _capi.ptr(lnp)
        _capi.check(self._L.mp_sampler_run(self._s, int(nsteps), cp, lp), "mp_sampler_run")
        if store and nsteps > 0:
            self._append(chain, lnp, self.iteration)
        self.iteration += int(nsteps)
        self._flush_fbad()
        return self.get_last_sample()[0]

    def _append(self, chain, lnp, first_step):
        """The rows of a finished run, whose first step has the index first_step, behind the stored chain."""
        self._chain = chain if self._chain is None else np.concatenate([self._chain, chain])
        self._lnp = lnp if self._lnp is None else np.concatenate([self._lnp, lnp])
        self._steps = np.concatenate([self._steps, first_step + np.arange(len(chain), dtype=np.int64)])

    # ---- failed proposals (the reference's fbad file)
    def get_bad(self, first_row=0, max_rows=None):
        """(n_bad, pars[rows, ndim]): how many proposals inside the prior failed in the model so far (exact), and rows
        [first_row, first_row + max_rows) of the library's log of them, in sampler coordinates.  The log misses rows only
        if more than MP_BAD_WINDOW (65 536) proposals failed between two drains; a warning says so."""
        n_bad, n_logged = C.c_int64(0), C.c_int64(0)
        rc = self._L.mp_sampler_get_bad(self._s, 0, None, 0, C.byref(n_bad), C.byref(n_logged))
        if rc < 0:
            _capi.check(rc, "mp_sampler_get_bad")
        want = max(0, n_logged.value - int(first_row))
        if max_rows is not None:
            want = min(want, int(max_rows))
        buf = np.empty((want, self.ndim))
        if want:
            rows = self._L.mp_sampler_get_bad(self._s, int(first_row), _capi.ptr(buf), want, None, None)
            if rows < 0:
                _capi.check(rows, "mp_sampler_get_bad")
            buf = buf[:rows]
        if n_logged.value < n_bad.value and not self._warned_bad:
            import warnings
            warnings.warn(f"{n_bad.value - n_logged.value} of {n_bad.value} failed proposals are missing from the fbad log "
                          "(more than 65 536 failed between two drains)", RuntimeWarning)
            self._warned_bad = True
        return int(n_bad.value), buf

    def _flush_fbad(self):
        if self.fbad is None or self._target != 0:
            return
        _, new = self.get_bad(first_row=self._bad_written)
        if len(new):
            with open(self.fbad, "a") as f:
                for r in new:
                    f.write(", ".join(f"{v}" for v in r) + "\n")
            self._bad_written += len(new)

    # ---- walker-sharded driving (magprop_amd.distributed.DistributedEnsembleSampler); device pointers as ints
    @property
    def n_slots(self):
        return self._L.mp_sampler_n_slots(self._s)

    @property
    def row_doubles(self):
        return self._L.mp_sampler_row_doubles(self._s)

    def set_positions(self, pos):
        p = np.ascontiguousarray(pos, dtype=np.float64)
        if p.shape != (self.ntotal, self.ndim):
            raise ValueError(f"pos must have shape {(self.ntotal, self.ndim)}")
        _capi.check(self._L.mp_sampler_set_positions(self._s, _capi.ptr(p)), "mp_sampler_set_positions")
        self._have_positions = True

    def halfstep_shard(self, half, lo, hi, d_rows, stream=0):
        _capi.check(self._L.mp_sampler_halfstep_shard(self._s, int(half), int(lo), int(hi), C.c_void_p(d_rows or None),
                                                      C.c_void_p(stream or None)), "mp_sampler_halfstep_shard")

    def halfstep_apply(self, half, d_rows, d_chain_row=0, d_chain_lnp_row=0, stream=0):
        _capi.check(self._L.mp_sampler_halfstep_apply(self._s, int(half), C.c_void_p(d_rows), C.c_void_p(d_chain_row or None),
                                                      C.c_void_p(d_chain_lnp_row or None), C.c_void_p(stream or None)),
                    "mp_sampler_halfstep_apply")
        if half == 1:
            self.iteration += 1

    # whole-step protocol (include/magprop_amd.h mp_sampler_step_shard / _apply)
    @property
    def step_blocks(self):
        return self._L.mp_sampler_step_blocks(self._s)

    @property
    def step_row_doubles(self):
        return self._L.mp_sampler_step_row_doubles(self._s)

    def step_shard(self, lo, hi, d_rows, stream=0):
        _capi.check(self._L.mp_sampler_step_shard(self._s, int(lo), int(hi), C.c_void_p(d_rows or None), C.c_void_p(stream or None)),
                    "mp_sampler_step_shard")

    def step_apply(self, d_rows, d_chain_row=0, d_chain_lnp_row=0, stream=0):
        _capi.check(self._L.mp_sampler_step_apply(self._s, C.c_void_p(d_rows), C.c_void_p(d_chain_row or None),
                                                  C.c_void_p(d_chain_lnp_row or None), C.c_void_p(stream or None)),
                    "mp_sampler_step_apply")
        self.iteration += 1

    def get_last_sample(self):
        st = _capi.read_back(self._L.mp_sampler_get_state, self._s, [
            ("pos", (self.ntotal, self.ndim), np.float64), ("lnp", self.ntotal, np.float64), ("acc", self.ntotal, np.int64),
            ("done", (), np.int64)])
        return st["pos"], st["lnp"], st["acc"]

    # ---- emcee-shaped views (synth_mcmc.py:188-226 indexes chain[i, j, k], lnprobability[i, j])
    def get_chain(self, temp=None, flat=False):
        """(nsteps, nwalkers_total, ndim); temp=t: the walkers at beta_t of every group, in group order
        (nsteps, ngroups x nwalkers, ndim).  flat=True (emcee's): the steps folded into the rows, (nsteps x walkers, ndim)."""
        c = self._at_temp(self._chain, temp)
        return c.reshape(-1, c.shape[-1]) if flat and c is not None else c

    def get_log_prob(self, temp=None):
        """(nsteps, nwalkers_total), untempered lnprob; temp=t: as in get_chain."""
        return self._at_temp(self._lnp, temp)

    def _at_temp(self, a, temp):
        if temp is None:
            return a
        t = self._ensemble_index(0, temp)      # (group 0's beta_t ensemble has the index t)
        if a is None:
            return None
        v = a.reshape((a.shape[0], self.ngroups, self.ntemps, self.nwalkers) + a.shape[2:])[:, :, t]
        return v.reshape((a.shape[0], self.ngroups * self.nwalkers) + a.shape[2:])

    @property
    def swap_acceptance_fraction(self):
        """(ngroups, T - 1): accepted / proposed swaps of every neighbouring pair (t - 1, t); each pair is proposed nwalkers
        times per step."""
        if self.betas is None:
            raise ValueError("swap_acceptance_fraction needs a tempered sampler (betas=...)")
        acc = _capi.read_back(self._L.mp_sampler_get_swaps, self._s, [("acc", (self.ngroups, self.ntemps - 1), np.int64)])["acc"]
        done = _capi.read_back(self._L.mp_sampler_get_state, self._s, [("pos", None, None), ("lnp", None, None),
                                                                       ("acc", None, None), ("done", (), np.int64)])["done"]
        return acc / max(int(done) * self.nwalkers, 1)

    def get_slice_stats(self):
        """The state of the slice move (moves=SliceMove(...); mp_sampler_get_slice), one entry per ensemble: the scale "mu" now
        and, since the sampler was made, "nexpand" stepping-out steps, "ncontract" rejected shrink points, "nfail" failed
        slices, "neval" evaluated points and "n_tuned" slice steps taken (mu is tuned over the first SliceMove.tune of them)."""
        if self.moves is None or _moves.slice_move(self.moves) is None:
            raise ValueError("get_slice_stats needs a sampler with a SliceMove in moves=")
        n = self.nensembles
        return _capi.read_back(self._L.mp_sampler_get_slice, self._s, [("mu", n, np.float64)] + [
            (k, n, np.int64) for k in ("nexpand", "ncontract", "nfail", "neval", "n_tuned")])

    def get_gaussian_stats(self):
        """The state of the Gaussian move (moves=GaussianMove(...); mp_sampler_get_gaussian), one entry per ensemble: the scale
        "sigma" now and, since the sampler was made, "n_proposed" proposals, "n_accepted" of them accepted and "n_tuned" tuning
        updates made (at most GaussianMove.tune)."""
        if self.moves is None or _moves.gaussian_move(self.moves) is None:
            raise ValueError("get_gaussian_stats needs a sampler with a GaussianMove in moves=")
        n = self.nensembles
        return _capi.read_back(self._L.mp_sampler_get_gaussian, self._s, [("sigma", n, np.float64)] + [
            (k, n, np.int64) for k in ("n_proposed", "n_accepted", "n_tuned")])

    # ---- the ladder as the device holds it (include/magprop_amd.h mp_sampler_set_ladder_adaptation)
    @property
    def ladder_frozen_at(self):
        """The index of the first step that runs on the frozen ladder (the adaptive steps); None on a fixed ladder."""
        return None if self._adapt is None else self._adapt[0]

    def _temperatures(self):
        if self.betas is None:
            raise ValueError("the sampler is not tempered (betas=...)")
        return _capi.read_back(self._L.mp_sampler_get_temperatures, self._s, [
            ("betas", (self.ngroups, self.ntemps), np.float64), ("n_updates", (), np.int64), ("n_dropped", self.ngroups, np.int64)])

    def get_betas(self):
        """(ngroups, T): every group's ladder as the device holds it now.  On a fixed ladder: the ladder as given, per group."""
        return self._temperatures()["betas"]

    @property
    def ladder_updates(self):
        """(updates made so far, (ngroups,) updates that were not taken because they would have left no valid ladder)."""
        t = self._temperatures()
        return int(t["n_updates"]), t["n_dropped"]

    def ladder_history(self, group=0):
        """(updates so far, T): row t is group `group`'s ladder after update t (adapt_ladder={..., "history": True})."""
        if self._adapt is None or not self._adapt[3]:
            raise ValueError("ladder_history needs adapt_ladder={..., 'history': True}")
        rows = max(min(self.iteration, self._adapt[0]), 1)
        buf, n = np.empty((rows, self.ntemps)), C.c_int64(0)
        _capi.check(self._L.mp_sampler_get_ladder_history(self._s, int(group), 0, rows, _capi.ptr(buf), C.byref(n)),
                    "mp_sampler_get_ladder_history")
        return buf[:n.value]

    # ---- the device thermodynamic monitor (include/magprop_amd.h mp_sampler_set_thermo states the definition)
    def monitor_thermo(self, discard=0):
        """Turn the thermodynamic monitor on (empty, accumulating from `discard` steps from now on, and on an adaptive sampler
        only over the steps on the frozen ladder), or off with discard=None: per ensemble the sum of lnL, which is what
        log_evidence(device=True) needs of a run, so that no chain has to reach the host.  While it is on, set_positions
        (run_mcmc with pos) restarts it."""
        _capi.check(self._L.mp_sampler_set_thermo(self._s, -1 if discard is None else int(discard)), "mp_sampler_set_thermo")
        self._thermo = discard is not None

    def get_thermo(self):
        """The monitor's sums: {"sum_lnl", "n_finite", "n_nonfinite": (ngroups, T), "n_steps": monitored steps}."""
        if not self._thermo:
            raise _capi.MagpropAmdError("the thermodynamic monitor is off (monitor_thermo)")
        shape = (self.ngroups, self.ntemps)
        out = _capi.read_back(self._L.mp_sampler_get_thermo, self._s, [
            ("sum_lnl", shape, np.float64), ("n_finite", shape, np.int64), ("n_nonfinite", shape, np.int64), ("n_steps", (), np.int64)])
        out["n_steps"] = int(out["n_steps"])
        return out

    def log_evidence(self, discard=0, group=0, prior_draws=2 ** 20, device=False, method="ti", thin=1, ensemble=None, temp=None,
                     n_draws=None, repetitions=1, seed=None, neff=None, source="chain", max_iter=1000, tol=None,
                     proposal="normal", nu=5, warp=False):
        """method="ti" (the default; thin and the arguments behind it are not read): (lnZ, dlnZ) of group `group`'s dataset, the prior normalised over its box, from the stored chain of a tempered run:
        thermodynamic integration of the per-temperature mean lnL over steps[discard:] (magprop_amd.tempering) plus
        ln f_valid, the fraction of `prior_draws` uniform box draws (numpy generator seeded by the sampler seed, evaluated on
        this sampler's handle) whose lnprob is finite.  dlnZ = |TI - TI over every other temperature| in quadrature with the
        binomial error of ln f_valid.  target="gaussian" has no prior box: lnZ is the integral alone.
        With adapt_ladder= the integral runs over the group's frozen ladder (get_betas), and steps[discard:] must all lie on it:
        a step before ladder_frozen_at raises ValueError.
        device=True takes the per-temperature means from the thermodynamic monitor (monitor_thermo) instead of the stored
        chain, so a store=False run has an evidence; discard is the monitor's then.  It raises while the monitor is off or
        empty and where a mean is not finite.
        method="bridge": the evidence of an ordinary, untempered run by bridge sampling (magprop_amd.bridge, mp_bridge_logz), a
        bridge.BridgeResult (it unpacks as (lnZ, dlnZ)): a Gaussian fitted to the first half of the steps
        chain[discard::thin] of `ensemble` (default: `group`; a tempered sampler: the group's cold chain, or with temp=t its
        beta_t ensemble, whose lnprob is still the untempered one) proposes n_draws points (default N1, the rows of the second
        half) per repetition, and the second half with its stored lnprob is the estimator's: n_draws model evaluations on top
        of the run.  seed: of the draws (default: derived from the sampler's).  neff=None: N1 / max tau over the estimator
        half, tau from the autocorrelation monitor where it is on and else from get_autocorr_time's estimator on that half,
        clamped to (0, N1]; without a tau neff = N1, and a RuntimeWarning says so.  source="reservoir": the rows of
        get_samples(ensemble) split at their median step instead (monitor_samples; discard and thin stay at their defaults), so
        that run_mcmc_until(..., store=False) ends with an evidence.  repetitions > 1: lnz is the median over the repetitions'
        draws, dlnz their mean, dlnz_reps the spread of lnz over them.  max_iter, tol: of the fixed point.  proposal="t" with nu
        degrees of freedom (heavy tails: lnz_is far from lnz) and warp=True (Warp-III: a skewed posterior, or one against a wall
        of the box; one more evaluation per estimator row and per draw) are bridge.bridge_evidence's (mp_bridge_logz_warp);
        without them the call and its bits are mp_bridge_logz's."""
        if method == "bridge":
            return self._bridge_evidence(discard, thin, group if ensemble is None else ensemble, temp, n_draws, repetitions, seed, neff,
                                         source, max_iter, tol, proposal, nu, warp)
        if method != "ti":
            raise ValueError(f"method must be 'ti' or 'bridge', got {method!r}")
        if self.betas is None:
            raise ValueError("log_evidence needs a tempered sampler (betas=...)")
        group = int(group)
        if not 0 <= group < self.ngroups:
            raise ValueError(f"group must be in 0..{self.ngroups - 1}, got {group}")
        if device:
            th = self.get_thermo()
            if th["n_steps"] < 1:
                raise ValueError("the thermodynamic monitor holds no step yet" +
                                 ("" if self._adapt is None else f" (the ladder is frozen from step {self._adapt[0]} on)"))
            with np.errstate(invalid="ignore", divide="ignore"):
                means = th["sum_lnl"][group] / th["n_finite"][group]
            if np.any(th["n_nonfinite"][group] > 0) or not np.all(np.isfinite(means)):
                raise ValueError("a per-temperature mean of lnL is not finite (walkers without a valid model: discard more steps)")
        else:
            if self._lnp is None or len(self._lnp) == 0:
                raise ValueError("the chain is empty: run_mcmc(..., store=True) first")
            discard = int(discard)
            if not 0 <= discard < len(self._lnp):
                raise ValueError(f"discard={discard} leaves no step of the {len(self._lnp)} stored")
            if self._adapt is not None and np.any(self._steps[discard:] < self._adapt[0]):
                raise ValueError(f"steps[{discard}:] of the stored chain hold steps before {self._adapt[0]}, where the ladder "
                                 "was frozen: discard them")
            lnl = self._lnp[discard:].reshape(-1, self.ngroups, self.ntemps, self.nwalkers)[:, group]
            means = lnl.transpose(1, 0, 2).reshape(self.ntemps, -1).mean(axis=1)
        betas = self.betas if self._adapt is None else self.get_betas()[group]
        ti, dti = tempering.ti_log_evidence(betas, means)
        if self._target != 0:
            return ti, dti
        lo, hi = np.asarray(self._prior[0], dtype=np.float64), np.asarray(self._prior[1], dtype=np.float64)
        rng = np.random.default_rng(self.seed)
        n_draws, n_finite, chunk = int(prior_draws), 0, 1 << 16
        for first in range(0, n_draws, chunk):
            m = min(chunk, n_draws - first)
            lp = self.handle.lnprob_batch(lo + (hi - lo) * rng.random((m, lo.size)), ds_id=group)
            n_finite += int(np.count_nonzero(np.isfinite(lp)))
        lnf, dlnf = tempering.validity_term(n_finite, n_draws)
        return ti + lnf, float(np.hypot(dti, dlnf))

    def _bridge_evidence(self, discard, thin, ensemble, temp, n_draws, repetitions, seed, neff, source, max_iter, tol, proposal, nu, warp):
        """log_evidence(method="bridge")"""
        _capi.bridge_proposal(proposal, nu, warp)
        e = self._ensemble_index(ensemble, temp, grouped=self.betas is not None)
        grp = e // self.ntemps
        tau, n_seen, why = None, None, "the estimator half is too short"
        if source == "reservoir":
            if int(discard) != 0 or int(thin) != 1:
                raise ValueError(f"source='reservoir' takes every row of the reservoir: discard and thin must be 0 and 1, got "
                                 f"discard={discard}, thin={thin} (give discard to monitor_samples)")
            if self._res is None:
                raise _capi.MagpropAmdError("the sample reservoir is off (monitor_samples)")
            res = _capi.read_back(self._L.mp_sampler_get_reservoir, self._s, [
                ("x", (self._res[0], self.ndim), np.float64), ("log_prob", self._res[0], np.float64), ("step", self._res[0], np.int64),
                ("walker", None, None), ("key", None, None), ("n_rows", (), np.int32), ("n_seen", (), np.int64)], e, self._res[0])
            rows = int(res["n_rows"])
            fit, est, lnp = bridge.reservoir_split({k: res[k][:rows] for k in ("x", "log_prob", "step")})
            n_seen = float(res["n_seen"]) * est.shape[0] / max(rows, 1)     # the samples the estimator rows stand for
            if neff is None:
                why = "the autocorrelation monitor is off or holds no estimate"
                if self._acf is not None:
                    t, _, _ = self.get_autocorr_device(wait=True)
                    tau = None if t is None else np.atleast_2d(t)[grp if np.ndim(t) > 1 else 0]
        elif source == "chain":
            if self._chain is None or len(self._chain) == 0:
                raise ValueError("the chain is empty: run_mcmc(..., store=True) first")
            discard, thin = int(discard), int(thin)
            if discard < 0 or thin < 1:
                raise ValueError(f"discard must be >= 0 and thin >= 1, got discard={discard}, thin={thin}")
            w = slice(e * self.nwalkers, (e + 1) * self.nwalkers)
            fit, est, lnp, est_chain = bridge.split(self._chain[discard::thin, w], self._lnp[discard::thin, w])
            if neff is None and est_chain.shape[0] >= 4:
                from .mcmc_io import integrated_time
                tau = integrated_time(est_chain, quiet=True)
        else:
            raise ValueError(f"source must be 'chain' or 'reservoir', got {source!r}")
        if neff is None:
            neff, known = bridge.neff_from_tau(int(np.count_nonzero(np.isfinite(lnp))), tau, n_seen)
            if not known:
                bridge.warn_no_tau(why)
        seed = (self.seed ^ 0x4272696467655F7A) & 0xFFFFFFFFFFFFFFFF if seed is None else int(seed)
        lo, hi = (None, None) if self._target != 0 else self._prior
        return bridge.bridge_evidence(fit, est, lnp, summaries.on(self.handle, grp), lo, hi, n_draws=n_draws, repetitions=repetitions,
                                      seed=seed, neff=neff, max_iter=max_iter, tol=tol, target=self._target, proposal=proposal, nu=nu,
                                      warp=warp)

    @property
    def chain(self):
        return None if self._chain is None else np.swapaxes(self._chain, 0, 1)

    @property
    def lnprobability(self):
        return None if self._lnp is None else self._lnp.T

    @property
    def acceptance_fraction(self):
        return self.get_last_sample()[2] / max(self.iteration, 1)

    # ---- the device sample reservoir (include/magprop_amd.h mp_sampler_set_reservoir states the rule)
    def monitor_samples(self, size=4096, seed=None, discard=0):
        """Turn the sample reservoir on (empty, taking samples from `discard` steps from now on), or off with size=None: per
        ensemble a uniform random subset of `size` of the run's samples (all of them while fewer were seen), kept on the device
        with their lnprob, step and walker, so that a store=False run ends with posterior samples (get_samples, and source=
        "reservoir" of get_model_band, get_derived, get_flows, get_flow_band, get_pointwise and get_reweight).  seed=None derives the
        monitor's seed from the sampler's; give two runs different seeds to merge their reservoirs (magprop_amd.reservoir.merge).
        While it is on, set_positions (run_mcmc with pos) restarts it and the walker-sharded entry points refuse."""
        if size is None:
            _capi.check(self._L.mp_sampler_set_reservoir(self._s, 0, 0, 0), "mp_sampler_set_reservoir")
            self._res = None
            return
        size = int(size)
        if size < 1:
            raise ValueError(f"size must be >= 1 (None turns the monitor off), got {size}")
        seed = (self.seed ^ 0x5265735F6B657973) & 0xFFFFFFFFFFFFFFFF if seed is None else int(seed) & 0xFFFFFFFFFFFFFFFF
        self._res = None
        _capi.check(self._L.mp_sampler_set_reservoir(self._s, size, seed, int(discard)), "mp_sampler_set_reservoir")
        self._res = (size, seed, int(discard))

    def get_samples(self, ensemble=0, temp=None):
        """The reservoir of one ensemble: {"x": (rows, ndim), "log_prob", "step", "walker", "key": (rows,), "n_seen"}, the rows
        sorted by (step, walker); step is the sampler's step index (self.iteration before the step), log_prob the untempered
        lnprob, n_seen the samples the monitor drew from.  A tempered sampler: the beta = 1 ensemble of group `ensemble`, or with
        temp=t its beta_t ensemble."""
        if self._res is None:
            raise _capi.MagpropAmdError("the sample reservoir is off (monitor_samples)")
        e = self._ensemble_index(ensemble, temp, grouped=self.betas is not None)
        k = self._res[0]
        out = _capi.read_back(self._L.mp_sampler_get_reservoir, self._s, [
            ("x", (k, self.ndim), np.float64), ("log_prob", k, np.float64), ("step", k, np.int64), ("walker", k, np.int32),
            ("key", k, np.uint64), ("n_rows", (), np.int32), ("n_seen", (), np.int64)], e, k)
        rows = int(out.pop("n_rows"))
        out = {name: (v[:rows].copy() if name != "n_seen" else int(v)) for name, v in out.items()}
        return out

    def _summary_rows(self, name, discard, thin, ensemble, source="chain"):
        """The rows chain[discard::thin, ensemble's walkers] the front end `name` summarises (band_selection; tempered: the
        beta = 1 walkers of group `ensemble`); source="reservoir": the rows of get_samples(ensemble) in its order."""
        if self._target != 0:
            raise ValueError(f"{name} needs the posterior target: a target='gaussian' sampler has no "
                             f"{'trajectory' if 'flow' in name else 'light curve'}")
        if source == "reservoir":
            return reservoir_selection(self.get_samples, discard, thin, ensemble, self.ngroups)
        if source != "chain":
            raise ValueError(f"source must be 'chain' or 'reservoir', got {source!r}")
        return band_selection(self.get_chain(temp=0 if self.betas is not None else None), self.nwalkers, self.ngroups,
                              discard, thin, ensemble)

    def get_model_band(self, q=(0.025, 0.5, 0.975), components=("Ltot",), discard=0, thin=1, ensemble=0, weights=None, source="chain"):
        """Posterior-predictive band over the stored chain: the quantiles q of the model light curves of the rows
        chain[discard::thin, ensemble's walkers], evaluated on this sampler's handle (its prior, grid and configuration).
        Returns {"t": grid, "Ltot": (nq, n_grid), ..., "n_used": rows that entered}.  weights: one per selected row, in the
        order band_selection gives them (a chain reweighted to another prior, error model or temperature): the weighted band
        (mp_model_band_weighted), and "n_eff" in the result.  source="reservoir": over the rows of get_samples(ensemble), in
        its order, instead of the stored chain (monitor_samples; discard and thin must stay at their defaults)."""
        rows = self._summary_rows("get_model_band", discard, thin, ensemble, source)
        return summaries.band(summaries.on(self.handle), rows, q, components, weights)

    def get_derived(self, q=(0.16, 0.5, 0.84), discard=0, thin=1, ensemble=0, source="chain"):
        """Energy budgets and light-curve landmarks over the stored chain (magprop_amd.derived.NAMES): the model of every row of
        chain[discard::thin, ensemble's walkers], evaluated and reduced on this sampler's handle (mp_model_derived).  Returns
        {"values": (rows, 16), "status", "n_used", "summary": derived.summarize(values, q)}.  source="reservoir": as in
        get_model_band."""
        rows = self._summary_rows("get_derived", discard, thin, ensemble, source)
        return summaries.derived(summaries.on(self.handle), rows, q)

    def get_flows(self, q=(0.16, 0.5, 0.84), discard=0, thin=1, ensemble=0, curves=(), source="chain"):
        """Mass budget, angular-momentum budget and propeller / accretor regime over the stored chain (magprop_amd.flows.NAMES):
        the model of every row of chain[discard::thin, ensemble's walkers], evaluated and reduced on this sampler's handle
        (mp_model_flows).  Returns {"values": (rows, 16), "status", "n_used", "summary": flows.summarize(values, q)} and the
        cell curves named in `curves`.  source="reservoir": as in get_model_band."""
        rows = self._summary_rows("get_flows", discard, thin, ensemble, source)
        return summaries.flows(summaries.on(self.handle), rows, q, None, curves)

    def get_flow_band(self, q=(0.025, 0.5, 0.975), curves=("fastness",), discard=0, thin=1, ensemble=0, weights=None,
                      source="chain"):
        """Bands of the radii, mass-flow rates and torques over the stored chain: the quantiles q, per grid point, of the cell
        curves named in `curves` (flows.CURVES without "branch") over the rows get_model_band takes (mp_model_flow_band).
        Returns {"t": grid, name: (nq, n_grid), "n_used"}; weights and source as in get_model_band."""
        rows = self._summary_rows("get_flow_band", discard, thin, ensemble, source)
        return summaries.flow_band(summaries.on(self.handle), rows, q, curves, weights)

    def get_pointwise(self, discard=0, thin=1, ensemble=0, source="chain"):
        """Pointwise predictive scores over the stored chain: PSIS-LOO with its Pareto-k diagnostic and WAIC per observation
        of group `ensemble`'s dataset, in the order the dataset was given, over the rows chain[discard::thin, ensemble's
        walkers], evaluated and reduced on this sampler's handle (mp_model_pointwise).  Returns what synth.model_pointwise
        returns.  The selection is capped like get_model_band's: thin a longer chain, or hand its rows to
        synth.model_pointwise / mcmc_eqns.model_pointwise.  source="reservoir": as in get_model_band."""
        rows = self._summary_rows("get_pointwise", discard, thin, ensemble, source)
        return summaries.pointwise(summaries.on(self.handle, int(ensemble), self._times[int(ensemble)]), rows)

    def get_reweight(self, alternatives, discard=0, thin=1, ensemble=0, source="chain"):
        """Importance reweighting of the stored chain to other error models and data subsets: the log importance weights of the
        rows chain[discard::thin, ensemble's walkers] under every alternative (magprop_amd.reweight.gaussian / student_t)
        against group `ensemble`'s dataset, per-observation weights in the order the dataset was given, summed on this
        sampler's handle (mp_model_reweight).  Returns what synth.model_reweight returns; reweight.weights(lw, k) are the
        weights= of get_model_band and get_flow_band for the same selection.  The selection is capped like get_model_band's.
        source="reservoir": as in get_model_band."""
        rows = self._summary_rows("get_reweight", discard, thin, ensemble, source)
        return summaries.reweight(summaries.on(self.handle, int(ensemble), self._times[int(ensemble)]), rows, alternatives)

    def get_autocorr_time(self, c=5.0, tol=50, quiet=False, device=False):
        """emcee's default (quiet=False) raises when the chain is shorter than tol autocorrelation times; the
        reference calls it bare (code/synthetic_datasets/synth_mcmc.py:220).
        device=True reads the device monitor (monitor_autocorr) instead of the stored chain: (ndim,) for one ensemble, else
        (nensembles, ndim), every ensemble on its own; a tempered sampler reports its beta = 1 ensembles.  tol and quiet act as
        on the host path, over the monitor's sample count; a NaN tau (max_lag too small for the window) raises with
        quiet=False and warns with quiet=True."""
        if device:
            tau, _, n = self.get_autocorr_device(c)
            if np.any(np.isnan(tau)):
                msg = (f"no window below max_lag = {self._acf[0]} after {n} samples: raise max_lag (monitor_autocorr); tau: {tau}")
                if not quiet:
                    raise RuntimeError(msg)
                import warnings
                warnings.warn(msg, RuntimeWarning)
            if not quiet and np.any(tol * tau > n):
                raise RuntimeError(f"The chain is shorter than {tol} times the integrated autocorrelation time; tau: {tau}")
            return tau
        from .mcmc_io import integrated_time
        return integrated_time(self.get_chain(temp=0 if self.betas is not None else None), c=c, tol=tol, quiet=quiet)

    # ---- the device autocorrelation monitor (include/magprop_amd.h mp_sampler_set_autocorr states the definition)
    def monitor_autocorr(self, max_lag=1024, discard=0):
        """Turn the monitor on (empty, accumulating from `discard` steps from now on; lags 0 .. max_lag - 1), or off with
        max_lag=0.  While it is on, set_positions (run_mcmc with pos) restarts it and the walker-sharded entry points refuse."""
        _capi.check(self._L.mp_sampler_set_autocorr(self._s, int(max_lag), int(discard)), "mp_sampler_set_autocorr")
        self._acf = (int(max_lag), int(discard)) if int(max_lag) else None

    def _reported(self, a):
        """Rows of a per-ensemble array that get_autocorr_time(device=True) reports: the beta = 1 ensembles; one row squeezed."""
        a = a[::self.ntemps]
        return a[0] if len(a) == 1 else a

    def get_autocorr_device(self, c=5.0, wait=False):
        """(tau, window, n) of the monitor: n samples so far, tau and window shaped as get_autocorr_time(device=True) returns tau.
        wait=True answers (None, None, n) instead of raising while a monitor that is on holds fewer than the 2 samples an
        estimate needs (still inside its discard); every other failure raises either way."""
        n = C.c_int64(0)
        tau = np.empty((self.nensembles, self.ndim))
        win = np.empty((self.nensembles, self.ndim), dtype=np.int32)
        rc = self._L.mp_sampler_get_autocorr(self._s, float(c), _capi.ptr(tau), _capi.ptr(win), C.byref(n))
        if wait and rc == _capi.MP_ESTATE and self._acf is not None and n.value < 2:
            return None, None, int(n.value)
        _capi.check(rc, "mp_sampler_get_autocorr")
        return self._reported(tau), self._reported(win), int(n.value)

    def get_acf(self, ensemble=0, max_rows=None):
        """The walker-mean autocorrelation function f_k of one ensemble from the monitor: (min(max_rows, max_lag, n), ndim)."""
        if self._acf is None:
            raise _capi.MagpropAmdError("the autocorrelation monitor is off (monitor_autocorr)")
        rows = self._acf[0] if max_rows is None else int(max_rows)
        buf = np.empty((rows, self.ndim))
        got = self._L.mp_sampler_get_acf(self._s, int(ensemble), rows, _capi.ptr(buf))
        if got < 0:
            _capi.check(got, "mp_sampler_get_acf")
        return buf[:got]

    def get_autocorr_sums(self, ensemble=0):
        """The monitor's raw accumulators of one ensemble (tests/acf_restated.py restates them): {"S", "H", "tail": (max_lag,
        nwalkers, ndim), "T", "pivot": (nwalkers, ndim), "n": samples}."""
        if self._acf is None:
            raise _capi.MagpropAmdError("the autocorrelation monitor is off (monitor_autocorr)")
        k, w = self._acf[0], (self.nwalkers, self.ndim)
        out = _capi.read_back(self._L.mp_sampler_get_autocorr_sums, self._s, [
            ("S", (k,) + w, np.float64), ("T", w, np.float64), ("H", (k,) + w, np.float64), ("tail", (k,) + w, np.float64),
            ("pivot", w, np.float64), ("n", (), np.int64)], int(ensemble))
        out["n"] = int(out["n"])
        return out

    # ---- the device posterior monitor (include/magprop_amd.h mp_sampler_set_posterior states the definition)
    def monitor_posterior(self, bins=256, bins2=64, range=None, discard=0):
        """Turn the posterior monitor on (empty, accumulating from `discard` steps from now on), or off with bins=0: per
        ensemble, 1-D histograms of `bins` bins per dimension, 2-D histograms of bins2 x bins2 bins per pair (0: none), the
        moments and the best sample, all kept on the device (get_posterior, get_quantiles).
        range: None, the handle's prior box in sampler coordinates; "ensemble", per dimension [min - span, max + span] of the
        current positions of all ensembles, span = max - min, clipped to the prior box (for use after a burn-in; raises before
        positions are set or where a span is 0); or an array (ndim, 2) of [lower, upper) per dimension.
        While it is on, set_positions (run_mcmc with pos) restarts it and the walker-sharded entry points refuse."""
        bins, bins2 = int(bins), int(bins2)
        if bins == 0:
            _capi.check(self._L.mp_sampler_set_posterior(self._s, 0, 0, None, None, 0), "mp_sampler_set_posterior")
            self._post = None
            return
        box = tuple(np.asarray(v, dtype=np.float64) for v in self._prior)
        if range is None or isinstance(range, str):
            if box[0].shape != (self.ndim,):
                raise ValueError(f"the prior box has {box[0].size} dimensions, the sampler {self.ndim}: give range=array(ndim, 2)")
            if range is None:
                lo, hi = box
            elif range == "ensemble":
                if not self._have_positions:
                    raise ValueError("range='ensemble' needs positions: call it after set_positions or a burn-in")
                lo, hi = posterior.ensemble_range(self.get_last_sample()[0], *box)
            else:
                raise ValueError(f"range must be None, 'ensemble' or an array (ndim, 2), got {range!r}")
        else:
            r = np.asarray(range, dtype=np.float64)
            if r.shape != (self.ndim, 2):
                raise ValueError(f"range must have shape ({self.ndim}, 2), got {r.shape}")
            lo, hi = r[:, 0], r[:, 1]
        lo, hi = np.ascontiguousarray(lo, dtype=np.float64), np.ascontiguousarray(hi, dtype=np.float64)
        self._post = None
        _capi.check(self._L.mp_sampler_set_posterior(self._s, bins, bins2, _capi.ptr(lo), _capi.ptr(hi), int(discard)),
                    "mp_sampler_set_posterior")
        self._post = (bins, bins2, lo, hi)

    def _ensemble_index(self, ensemble, temp, grouped=False, note=""):
        """Index of `ensemble` in the library's order.  temp=t: `ensemble` counts the groups, as get_chain(temp=) does, and the
        index is that of the group's beta_t ensemble; temp=None: `ensemble` is that index already, or with grouped=True the
        group whose beta = 1 ensemble is meant.  note: what the message about a bad group says behind the range."""
        e = int(ensemble)
        if temp is None and not grouped:
            return e
        t = 0 if temp is None else int(temp)
        if not 0 <= t < self.ntemps:
            raise ValueError(f"temp must be in 0..{self.ntemps - 1}, got {temp}")
        if not 0 <= e < self.ngroups:
            raise ValueError(f"ensemble must be in 0..{self.ngroups - 1}{note}, got {ensemble}")
        return e * self.ntemps + t

    def _post_ensemble(self, ensemble, temp):
        if self._post is None:
            raise _capi.MagpropAmdError("the posterior monitor is off (monitor_posterior)")
        return self._ensemble_index(ensemble, temp, note=" with temp=")

    def get_posterior(self, ensemble=0, temp=None):
        """The posterior monitor's summary of one ensemble (temp=t: the beta_t ensemble of group `ensemble`): a dict with
        n (samples), edges1 (ndim, bins + 1), hist1 (ndim, bins), below, above, nonfinite (ndim,), pairs [(a, b), ...],
        edges2 (ndim, bins2 + 1), hist2 (npairs, bins2, bins2) indexed [pair][bin of a][bin of b], outside2 (npairs,)
        (edges2, hist2, outside2 None with bins2=0), mean (ndim,), cov (ndim, ndim) over the n_finite samples whose coordinates
        are all finite, best_x (ndim,), best_lnprob, best_index (t * nwalkers + w; -1 and NaN before the first sample)."""
        e = self._post_ensemble(ensemble, temp)
        bins, bins2, lo, hi = self._post
        nd = self.ndim
        pairs = [(a, b) for a in range(nd) for b in range(a + 1, nd)]
        L = self._L
        h1 = _capi.read_back(L.mp_sampler_get_posterior_hist1, self._s, [
            ("hist1", (nd, bins), np.int64), ("below", nd, np.int64), ("above", nd, np.int64), ("nonfinite", nd, np.int64),
            ("n", (), np.int64)], e)
        out = dict(h1, n=int(h1["n"]), edges1=posterior.edges(lo, hi, bins), pairs=pairs, edges2=None, hist2=None, outside2=None)
        if bins2:
            out.update(_capi.read_back(L.mp_sampler_get_posterior_hist2, self._s, [
                ("hist2", (len(pairs), bins2, bins2), np.int64), ("outside2", len(pairs), np.int64)], e))
            out["edges2"] = posterior.edges(lo, hi, bins2)
        m = _capi.read_back(L.mp_sampler_get_posterior_moments, self._s, [
            ("sum1", nd, np.float64), ("sum2", (nd, nd), np.float64), ("pivot", nd, np.float64), ("n_finite", (), np.int64)], e)
        out["n_finite"] = int(m["n_finite"])
        out["mean"], out["cov"] = posterior.mean_cov(m["sum1"], m["sum2"], m["pivot"], out["n_finite"])
        b = _capi.read_back(L.mp_sampler_get_posterior_best, self._s, [
            ("x", nd, np.float64), ("lnprob", (), np.float64), ("index", (), np.int64)], e)
        out["best_x"], out["best_lnprob"], out["best_index"] = b["x"], float(b["lnprob"]), int(b["index"])
        return out

    def get_quantiles(self, q=(0.16, 0.5, 0.84), ensemble=0, temp=None):
        """(len(q), ndim): the quantiles q of every dimension from the monitor's 1-D histograms (posterior.hist_quantiles:
        linear inside the bin that holds the rank, so good to a bin width; NaN and a RuntimeWarning where the histogram's range
        was too narrow)."""
        e = self._post_ensemble(ensemble, temp)
        bins, _, lo, hi = self._post
        h = _capi.read_back(self._L.mp_sampler_get_posterior_hist1, self._s, [
            ("hist1", (self.ndim, bins), np.int64), ("below", self.ndim, np.int64), ("above", self.ndim, np.int64),
            ("nonfinite", None, None), ("n", None, None)], e)
        return posterior.hist_quantiles(h["hist1"], h["below"], h["above"], lo, hi, q)

    def run_mcmc_until(self, pos, max_steps, check_every=100, tol=50, rtol=0.01, c=5.0, store=True, per_ensemble=False):
        """emcee's run-until-converged recipe on the device monitor: after every check_every steps read tau (the beta = 1
        ensembles of a tempered sampler) and stop once autocorr_converged(tau, previous tau, n, tol, rtol) holds, n the
        monitor's samples, or after max_steps.  Turns the monitor on (max_lag 1024, discard 0) if it is off.  Sets
        self.converged and self.tau_history = [(n, tau), ...]; returns the final positions.  store=True appends the steps
        to the stored chain (preallocated once for max_steps, trimmed); store=False: no chain reaches the host.
        The posterior monitor (monitor_posterior) runs next to it: both are fed from the same device rows, so a
        store=False run ends with tau and with the histograms, moments and best sample of get_posterior.  Both restart at
        set_positions, so give pos=None to keep what a monitor holds, and turn monitor_posterior on after the burn-in.
        The sample reservoir (monitor_samples) is fed from the same rows: with it a store=False run also ends with posterior
        samples (get_samples), and the band, derived quantities, flows and pointwise scores take them with source="reservoir".
        per_ensemble=True (ensembles that are fits of their own, one per dataset): the rule is applied to every reported ensemble
        on its own and remembered once met -- an ensemble's chain that was long enough at one check stays long enough -- and the
        run stops when every ensemble has met it; self.converged_ensembles holds the flags.  The default asks all ensembles to
        meet the rule at the same check, which many independent fits do far later than any one of them."""
        max_steps, check_every = int(max_steps), int(check_every)
        if check_every < 1 or max_steps < 0:
            raise ValueError(f"check_every must be >= 1 and max_steps >= 0, got {check_every}, {max_steps}")
        if self._acf is None:
            self.monitor_autocorr()
        if pos is not None:
            self.set_positions(pos)
        chain = np.empty((max_steps, self.ntotal, self.ndim)) if store else None
        lnp = np.empty((max_steps, self.ntotal)) if store else None
        done, prev = 0, None
        first_step = self.iteration
        self.converged, self.tau_history = False, []
        self.converged_ensembles = np.zeros(self.nensembles // self.ntemps, dtype=bool)   # one flag per reported ensemble
        while done < max_steps and not self.converged:
            k = min(check_every, max_steps - done)
            cp, lp = (_capi.ptr(chain[done:done + k]), _capi.ptr(lnp[done:done + k])) if store else (None, None)
            _capi.check(self._L.mp_sampler_run(self._s, k, cp, lp), "mp_sampler_run")
            done += k
            self.iteration += k
            self._flush_fbad()
            if k < check_every:
                break                                  # (the checks come at multiples of check_every)
            tau, _, n = self.get_autocorr_device(c, wait=True)
            if tau is None:                            # still inside the monitor's discard: fewer than 2 samples
                continue
            self.tau_history.append((n, tau))
            if per_ensemble:
                rows = np.atleast_2d(tau)
                for e in range(len(rows)):
                    self.converged_ensembles[e] |= autocorr_converged(rows[e], None if prev is None else np.atleast_2d(prev)[e], n, tol, rtol)
                self.converged = bool(np.all(self.converged_ensembles))
            else:
                self.converged = autocorr_converged(tau, prev, n, tol, rtol)
                self.converged_ensembles[:] = self.converged
            prev = tau
        if store and done > 0:
            if done < max_steps:                       # an early stop gives the unused rows back (refcheck: no other owner here)
                chain.resize((done,) + chain.shape[1:], refcheck=False)
                lnp.resize((done,) + lnp.shape[1:], refcheck=False)
            self._append(chain, lnp, first_step)
        return self.get_last_sample()[0]


def autocorr_converged(tau, tau_prev, n, tol=50, rtol=0.01):
    """emcee's stopping rule: the chain is longer than tol autocorrelation times in every dimension, all(tol tau < n), and the
    estimate has settled, all(|tau - tau_prev| / tau < rtol).  False without a previous estimate and for any NaN."""
    if tau_prev is None:
        return False
    tau, tau_prev = np.asarray(tau, dtype=float), np.asarray(tau_prev, dtype=float)
    with np.errstate(invalid="ignore", divide="ignore"):
        return bool(np.all(tol * tau < n) and np.all(np.abs(tau - tau_prev) / tau < rtol))


def reservoir_selection(get_samples, discard=0, thin=1, ensemble=0, nensembles=1):
    """The rows of the reservoir of `ensemble` (get_samples(ensemble)["x"], in its order) that the summaries evaluate with
    source="reservoir".  The reservoir is drawn from the whole monitored run, so discard and thin must be at their defaults
    (give discard to monitor_samples).  Raises ValueError for those, a bad ensemble, an empty reservoir and one of more than
    _capi.BAND_MAX_SAMPLES rows."""
    if int(discard) != 0 or int(thin) != 1:
        raise ValueError(f"source='reservoir' takes every row of the reservoir: discard and thin must be 0 and 1, got "
                         f"discard={discard}, thin={thin} (give discard to monitor_samples)")
    ensemble = int(ensemble)
    if not 0 <= ensemble < nensembles:
        raise ValueError(f"ensemble must be in 0..{nensembles - 1}, got {ensemble}")
    rows = np.ascontiguousarray(get_samples(ensemble)["x"])
    if rows.shape[0] == 0:
        raise ValueError("the reservoir is empty: run_mcmc with monitor_samples on first")
    if rows.shape[0] > _capi.BAND_MAX_SAMPLES:
        raise ValueError(f"the selection holds {rows.shape[0]} rows, more than {_capi.BAND_MAX_SAMPLES} (MP_BAND_MAX_SAMPLES): "
                         "raise thin or discard")
    return rows


def band_selection(chain, nwalkers, nensembles=1, discard=0, thin=1, ensemble=0):
    """Rows chain[discard::thin, ensemble * nwalkers:(ensemble + 1) * nwalkers] of a stored chain (nsteps, nwalkers *
    nensembles, ndim), flattened to (rows, ndim): what EnsembleSampler.get_model_band evaluates.  Raises ValueError for an
    empty chain, a bad selection and one of more than _capi.BAND_MAX_SAMPLES rows."""
    if chain is None or len(chain) == 0:
        raise ValueError("the chain is empty: run_mcmc(..., store=True) first")
    discard, thin, ensemble = int(discard), int(thin), int(ensemble)
    if discard < 0 or thin < 1:
        raise ValueError(f"discard must be >= 0 and thin >= 1, got discard={discard}, thin={thin}")
    if not 0 <= ensemble < nensembles:
        raise ValueError(f"ensemble must be in 0..{nensembles - 1}, got {ensemble}")
    sel = chain[discard::thin, ensemble * nwalkers:(ensemble + 1) * nwalkers]
    rows = sel.reshape(-1, chain.shape[-1])
    if rows.shape[0] == 0:
        raise ValueError(f"discard={discard} leaves no step of the {len(chain)} stored")
    if rows.shape[0] > _capi.BAND_MAX_SAMPLES:
        raise ValueError(f"the selection holds {rows.shape[0]} rows, more than {_capi.BAND_MAX_SAMPLES} (MP_BAND_MAX_SAMPLES): "
                         "raise thin or discard")
    return rows
