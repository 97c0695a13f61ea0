"""What the front ends of the device-resident drivers share (optimize, nested, smc): the result type, the checks of a bounds
box and of the datasets, and the base of the two samplers that own a handle and keep their runs' results."""
import numpy as np

from . import _capi, engine


class OptimizeResult(dict):
    """scipy.optimize.OptimizeResult's shape: a dict whose keys are also attributes."""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError as exc:
            raise AttributeError(name) from exc

    __setattr__ = dict.__setitem__


def finite_box(b):
    """(lower, upper), copies, of the (ndim, 2) array b of (lower, upper) pairs: finite, lower < upper in every coordinate."""
    lo, hi = b[:, 0].copy(), b[:, 1].copy()
    if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi)) and np.all(lo < hi)):
        raise ValueError("every bound must be finite with lower < upper")
    return lo, hi


def count_datasets(x, datasets):
    """The number of light curves given as (x, y, yerr) or datasets=[...]: at least one."""
    n_ds = len(datasets) if datasets is not None else (1 if x is not None else 0)
    if n_ds == 0:
        raise ValueError("a dataset is required: (x, y, yerr) or datasets=[...]")
    return n_ds


def check_box_and_runs(x, datasets, variant, ndim, bounds, n_runs, posterior, needs_bounds):
    """(box lower, box upper, prior lower, prior upper, log mask, number of datasets) of a sampler over a box.  The posterior
    target takes the variant's prior box unless `bounds` gives ndim pairs, and needs a dataset; a gaussian target has no prior and
    one run group, and needs `bounds` of 1 to _capi.MAX_NDIM pairs (needs_bounds: the message without them).  Then the box is finite
    and n_runs runs per dataset stay within _capi.MAX_DATASETS."""
    if not posterior:
        if bounds is None:
            raise ValueError(needs_bounds)
        b = np.asarray(bounds, dtype=np.float64)
        if b.ndim != 2 or b.shape[1] != 2 or not 1 <= b.shape[0] <= _capi.MAX_NDIM:
            raise ValueError(f"bounds must be 1 to {_capi.MAX_NDIM} (lower, upper) pairs")
        plo = phi = mask = None
        n_ds = 1
    else:
        plo, phi, mask = engine.prior_box(variant, ndim, strict=True)
        if bounds is None:
            b = np.stack([plo, phi], axis=1)
        else:
            b = np.asarray(bounds, dtype=np.float64)
            if b.shape != (ndim, 2):
                raise ValueError(f"bounds must be {ndim} (lower, upper) pairs")
        n_ds = count_datasets(x, datasets)
    lo, hi = finite_box(b)
    if n_ds * int(n_runs) > _capi.MAX_DATASETS:
        raise ValueError(f"len(datasets) x n_runs runs must be at most {_capi.MAX_DATASETS}")
    return lo, hi, plo, phi, mask, n_ds


class BoxSampler:
    """The base of NestedSampler and SMCSampler: the private handle (variant, GRBtype, device, _prior, datasets; the prior is set
    for the posterior target only) and the look-up of one run's entry of .results.  A subclass names its posterior target
    (POSTERIOR, the value of .target), and words its two refusals: NOT_RUN, and NO_MODEL for a summary of a gaussian target."""

    POSTERIOR = NOT_RUN = NO_MODEL = None

    def _open(self):
        if self.handle is not None:
            return
        self.handle = engine.open_handle(self.variant, self.GRBtype, self.device,
                                         self._prior if self.target == self.POSTERIOR else None, self.datasets)

    def close(self):
        if self.handle is not None:
            self.handle.close()
            self.handle = None

    def _run(self, run):
        res = self.results if isinstance(self.results, list) else [self.results]
        if self.results is None:
            raise ValueError(self.NOT_RUN)
        if int(run) != run or not 0 <= run < len(res):
            raise ValueError(f"run must be 0 .. {len(res) - 1}")
        return res[int(run)]

    def _need_posterior(self, name):
        if self.target != self.POSTERIOR:
            raise ValueError(f"{name} needs the posterior target: {self.NO_MODEL} "
                             f"{'trajectory' if 'flow' in name else 'light curve'}")
