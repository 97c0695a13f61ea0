"""Bridge-sampling evidence from the samples of an ordinary run (include/magprop_amd.h mp_bridge_logz; Meng & Wong 1996, Gronau et
al. 2017): a Gaussian is fitted to one half of the posterior samples, drawn from and evaluated on the device, and a fixed point
over the other half's lnprob and the draws' gives ln Z.  The samples carry their lnprob already, so the evidence costs n_draws
model evaluations on top of the fit.  Where the Gaussian covers the posterior badly, proposal="t" draws from a Student-t
with the same covariance (heavy tails) and warp=True symmetrises the posterior about the fitted mean (Warp-III: skew, a wall of
the box), both through mp_bridge_logz_warp; without them the call and its bits are mp_bridge_logz's.

``bridge_evidence`` is the one path from rows to the result, on a *source* as magprop_amd.summaries takes it.
EnsembleSampler.log_evidence(method="bridge") hands it the two halves of its chain or of its reservoir.  The equally weighted
samples of NestedSampler.resample_equal and of an SMCSampler run can be passed by hand: split them in two, give the second half
with its lnprob as the estimator rows, and neff = their number (they are independent draws up to the resampling's repeats)."""
import warnings

import numpy as np

from . import _capi

STATUS_NAMES = {_capi.BRIDGE_OK: "OK", _capi.BRIDGE_ITER_LIMIT: "ITER_LIMIT", _capi.BRIDGE_NO_OVERLAP: "NO_OVERLAP"}


class BridgeResult:
    """lnz: the estimate (the median over the repetitions); dlnz: the approximate relative error (mp_bridge_logz's formula), the
    mean over the repetitions; dlnz_reps: the standard deviation of lnz over the repetitions (0.0 for one); reps: the
    repetitions' rows as dicts keyed by _capi.BRIDGE_COLUMNS; niter, status, n_finite: per repetition; lnz_is: the plain
    importance-sampling estimate lambda_0 - ln_volume per repetition; neff, n_est, n_draws: what the call ran with.
    proposal ("normal" or "t"), nu (None for the Gaussian), warp: the proposal the call ran with; est_mirrors: the estimator rows
    whose mirror counted, draw_mirrors: per repetition the draws whose mirror did (0 without warp).
    Unpacks as (lnz, dlnz), the pair log_evidence returns for the other methods."""

    def __init__(self, out, neff, n_est, n_draws, proposal="normal", nu=None, warp=False):
        self.out = np.asarray(out, dtype=np.float64)
        names = _capi.BRIDGE_WARP_COLUMNS[:self.out.shape[1]]          # (mp_bridge_logz's rows end before the mirror counts)
        col = {c: self.out[:, k] for k, c in enumerate(names)}
        self.reps = [dict(zip(names, row)) for row in self.out]
        self.proposal, self.nu, self.warp = proposal, (int(nu) if proposal == "t" else None), bool(warp)
        self.est_mirrors = int(col["est_mirrors"][0]) if "est_mirrors" in col else 0
        self.draw_mirrors = col["draw_mirrors"].astype(np.int64) if "draw_mirrors" in col else np.zeros(len(self.out), dtype=np.int64)
        self.lnz_reps = col["lnz"].copy()
        self.lnz = float(np.median(col["lnz"]))
        self.dlnz = float(np.mean(col["dlnz"]))
        self.dlnz_reps = float(np.std(col["lnz"])) if len(self.out) > 1 else 0.0
        self.niter = col["niter"].astype(np.int64)
        self.status = col["status"].astype(np.int64)
        self.n_finite = col["n_finite"].astype(np.int64)
        self.lnz_is = col["lambda0"] - col["ln_volume"]
        self.neff, self.n_est, self.n_draws = float(neff), int(n_est), int(n_draws)

    @property
    def ok(self):
        return bool(np.all(self.status == _capi.BRIDGE_OK))

    def __iter__(self):
        return iter((self.lnz, self.dlnz))

    def __repr__(self):
        extra = (f", proposal=t({self.nu})" if self.proposal == "t" else "") + (
            f", warp=True, est_mirrors={self.est_mirrors}, draw_mirrors={self.draw_mirrors.tolist()}" if self.warp else "")
        return (f"BridgeResult(lnz={self.lnz:.6g}, dlnz={self.dlnz:.3g}, status={[STATUS_NAMES.get(int(s), int(s)) for s in self.status]}, "
                f"niter={self.niter.tolist()}, neff={self.neff:.6g}{extra})")


def split(chain, lnp):
    """(rows_fit, rows_est, lnp_est, est_chain) of a chain (nsteps, nwalkers, ndim) with its lnprob (nsteps, nwalkers): the first
    half of the steps shapes the proposal, the second half (the longer one of an odd count) is the estimator's; est_chain is
    that half as (steps, nwalkers, ndim), for an autocorrelation time."""
    chain, lnp = np.asarray(chain, dtype=np.float64), np.asarray(lnp, dtype=np.float64)
    if chain.ndim != 3 or lnp.shape != chain.shape[:2]:
        raise ValueError(f"chain (nsteps, nwalkers, ndim) and lnp (nsteps, nwalkers) expected, got {chain.shape}, {lnp.shape}")
    if chain.shape[0] < 2:
        raise ValueError(f"two steps at least are needed to split a chain, got {chain.shape[0]}")
    half = chain.shape[0] // 2
    nd = chain.shape[2]
    return chain[:half].reshape(-1, nd), chain[half:].reshape(-1, nd), lnp[half:].reshape(-1), chain[half:]


def neff_from_tau(n_est, tau, n_seen=None):
    """The effective number of estimator rows: n_seen / max(tau) (n_seen: the samples the rows stand for, the rows themselves by
    default), clamped to (0, n_est]; (n_est, False) where tau is not available (None, NaN or not positive)."""
    t = None if tau is None else np.max(np.asarray(tau, dtype=np.float64))
    if t is None or not np.isfinite(t) or t <= 0.0:
        return float(n_est), False
    n = float(n_est if n_seen is None else n_seen) / max(float(t), 1.0)
    return float(min(max(n, 1.0), float(n_est))), True


def bridge_evidence(rows_fit, rows_est, lnp_est, source, lower=None, upper=None, n_draws=None, repetitions=1, seed=0, neff=None,
                    max_iter=1000, tol=None, target=0, details=False, proposal="normal", nu=5, warp=False):
    """ln Z by bridge sampling (Handle.bridge_logz) on the handle of `source` (magprop_amd.summaries: a function of the rows' width
    that yields (handle, dataset slot, times); summaries.on(handle, ds_id) for an open one).  rows_fit (n_fit, ndim) shape the
    Gaussian proposal, rows_est (n_est, ndim) with their lnprob lnp_est are the estimator's rows; rows of rows_est whose lnprob
    is not finite carry no posterior mass and are left out.  lower, upper: the prior box in sampler coordinates, over which the
    prior is uniform (ln Z = ln of the integral of exp(lnprob) minus the box's log-volume).  n_draws: draws per repetition
    (default n_est); repetitions: independent sets of draws; neff: the effective number of estimator rows (default n_est,
    independent rows); max_iter, tol: of the fixed point, which stops at a step of tol or less (default: 1e-10, or 8 ulp of
    the largest |lnprob| where that is more -- a step below the ulp of the result cannot be seen).  Returns a BridgeResult;
    with details=True (result, the dict of Handle.bridge_logz).
    proposal="t": a multivariate Student-t with nu (3 .. 32) degrees of freedom and the fit rows' covariance in place of the
    Gaussian: its tails dominate a heavy-tailed posterior's, so the ratios p / q stay bounded (reach for it where lnz_is lies far
    from lnz).  warp=True: Warp-III, the posterior symmetrised about the fit rows' mean -- for a skewed posterior or one piled
    against a wall of the box; it costs one more model evaluation per estimator row and per draw.  The two compose.  With the
    defaults the call and its bits are mp_bridge_logz's."""
    prop = _capi.bridge_proposal(proposal, nu, warp)
    xf = np.ascontiguousarray(rows_fit, dtype=np.float64)
    xe = np.ascontiguousarray(rows_est, dtype=np.float64)
    le = np.ascontiguousarray(lnp_est, dtype=np.float64)
    if xf.ndim != 2 or xe.ndim != 2 or xf.shape[1] != xe.shape[1] or le.shape != (xe.shape[0],):
        raise ValueError(f"rows_fit (n_fit, ndim), rows_est (n_est, ndim) and lnp_est (n_est,) expected, got {xf.shape}, {xe.shape}, {le.shape}")
    keep = np.isfinite(le)
    if not np.all(keep):
        xe, le = np.ascontiguousarray(xe[keep]), np.ascontiguousarray(le[keep])
    if xe.shape[0] < 1:
        raise ValueError("no estimator row has a finite lnprob")
    n_est = xe.shape[0]
    n_draws = n_est if n_draws is None else int(n_draws)
    tol = max(1.0e-10, 8.0 * float(np.spacing(np.max(np.abs(le))))) if tol is None else float(tol)
    neff = float(n_est) if neff is None else float(min(max(float(neff), np.finfo(float).tiny), float(n_est)))
    with source(xf.shape[1]) as (handle, ds_id, _):
        res = handle.bridge_logz(xf, xe, le, lower, upper, ds_id=ds_id, n_draws=n_draws, n_rep=int(repetitions), seed=seed, neff=neff,
                                 max_iter=max_iter, tol=tol, target=target, details=details, proposal=proposal, nu=nu, warp=warp)
    out = BridgeResult(res["out"], neff, n_est, n_draws, "t" if prop[0] == _capi.BRIDGE_STUDENT else "normal", nu, warp)
    return (out, res) if details else out


def reservoir_split(samples):
    """(rows_fit, rows_est, lnp_est) of a reservoir (EnsembleSampler.get_samples): the rows before the median step shape the
    proposal, the rows from it on are the estimator's."""
    step = np.asarray(samples["step"])
    if step.size < 2:
        raise ValueError("the reservoir holds fewer than 2 rows")
    late = step >= np.median(step)
    if np.all(late):                       # (every row from one step)
        late = np.arange(step.size) >= step.size // 2
    x, lnp = np.asarray(samples["x"], dtype=np.float64), np.asarray(samples["log_prob"], dtype=np.float64)
    return x[~late], x[late], lnp[late]


def warn_no_tau(why):
    warnings.warn(f"no autocorrelation time for the estimator rows ({why}): neff = their number, dlnz is a lower bound", RuntimeWarning)
