"""Host side of the sampler's sample reservoir (include/magprop_amd.h mp_sampler_set_reservoir states the rule;
EnsembleSampler.monitor_samples / get_samples): the keys recomputed in numpy, and the merge of two reservoirs.

A reservoir is the dict get_samples returns: {"x": (rows, ndim), "log_prob", "step", "walker", "key": (rows,), "n_seen"}, the
rows sorted by (step, walker).  Host only: nothing here touches the device."""
import numpy as np

RES_CTR = 0x52455300            # csrc/mp_reservoir.h kResCtr
_M32 = np.uint64(0xFFFFFFFF)


def _philox4x32_10(k0, k1, c0, c1, c2, c3):
    """Philox4x32-10 over arrays of 32-bit words held in uint64 (csrc/mp_device.h philox4x32_10)."""
    k0, k1, c0, c1, c2, c3 = (np.asarray(v, dtype=np.uint64) & _M32 for v in (k0, k1, c0, c1, c2, c3))
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = ((p1 >> s32) ^ c1 ^ k0) & _M32, p1 & _M32, ((p0 >> s32) ^ c3 ^ k1) & _M32, p0 & _M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    return c0, c1, c2, c3


def keys(seed, step, walker, ensemble, n_walkers):
    """The 64-bit keys (uint64) of the samples (step, walker) of ensemble `ensemble` of a sampler of n_walkers walkers per
    ensemble under the monitor's seed; step and walker broadcast against each other."""
    step, walker = np.broadcast_arrays(np.asarray(step, dtype=np.int64), np.asarray(walker, dtype=np.int64))
    t = step.astype(np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    r = _philox4x32_10(seed & 0xFFFFFFFF, seed >> 32, t & _M32, t >> np.uint64(32),
                       (int(ensemble) * int(n_walkers) + walker).astype(np.uint64), RES_CTR)
    return (r[0] << np.uint64(32)) | r[1]


def _take(res, idx):
    return {"x": np.asarray(res["x"])[idx], "log_prob": np.asarray(res["log_prob"])[idx], "step": np.asarray(res["step"])[idx],
            "walker": np.asarray(res["walker"])[idx], "key": np.asarray(res["key"])[idx]}


def merge(a, b, size):
    """The reservoir of `size` rows of the union of the samples behind reservoirs a and b, both of `size` rows or more (or
    holding everything they saw): the `size` rows of both that are least by (key, step, walker), sorted by (step, walker), and
    n_seen the sum.  Same seed and disjoint steps (two parts of one run, two ensembles' worth of walkers apart): exactly the
    reservoir one monitor would hold over all of them.  Different seeds are allowed.  A sample present in both (same key, step,
    walker: the same run read twice) is refused, since its n_seen would count twice."""
    size = int(size)
    if size < 1:
        raise ValueError(f"size must be >= 1, got {size}")
    for r in (a, b):
        if len(r["key"]) < min(size, int(r["n_seen"])):
            raise ValueError(f"a reservoir of {len(r['key'])} rows out of {int(r['n_seen'])} seen cannot be merged to size {size}")
    if np.asarray(a["x"]).shape[1:] != np.asarray(b["x"]).shape[1:]:
        raise ValueError("the reservoirs hold rows of different dimensions")
    both = {k: np.concatenate([np.asarray(a[k]), np.asarray(b[k])]) for k in ("x", "log_prob", "step", "walker", "key")}
    order = np.lexsort((both["walker"], both["step"], both["key"]))
    trip = np.stack([both["key"][order].astype(np.uint64), both["step"][order].astype(np.uint64),
                     both["walker"][order].astype(np.uint64)], axis=1)
    if len(order) > 1 and np.any(np.all(trip[1:] == trip[:-1], axis=1)):
        raise ValueError("the reservoirs share a sample (same key, step and walker): they are not of disjoint samples")
    keep = order[:size]
    out = _take(both, keep)
    out = _take(out, np.lexsort((out["walker"], out["step"])))
    out["n_seen"] = int(a["n_seen"]) + int(b["n_seen"])
    return out
