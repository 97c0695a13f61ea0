"""The posterior monitor of the device-resident sampler (include/magprop_amd.h mp_sampler_set_posterior) restated in numpy: the
definition of the header over a whole sample sequence at once, every difference, product and sum rounded on its own (numpy never
fuses) and every sum sequential (np.cumsum from a leading 0.0, never np.sum, whose pairwise order is not the definition's).  So
every number is reproduced bit for bit, whatever chunks the device saw.  One ensemble at a time: chain[n][n_walkers][ndim],
lnp[n][n_walkers]."""
import numpy as np


def params(bins1, bins2, lower, upper):
    """(inv1, inv2, pivot) as the host forms them, in double."""
    lo, hi = np.asarray(lower, dtype=np.float64), np.asarray(upper, dtype=np.float64)
    w = hi - lo
    return bins1 / w, bins2 / w, lo + 0.5 * w


def bin_code(v, lower, upper, inv, B):
    """The bin rule on an array v of one coordinate: 0 .. B - 1 a bin, B below, B + 1 above, B + 2 not finite."""
    v = np.asarray(v, dtype=np.float64)
    fin = np.isfinite(v)
    safe = np.where(fin, v, lower)
    with np.errstate(over="ignore"):
        b = np.floor((safe - lower) * inv)
    inside = fin & (safe >= lower) & (safe < upper)
    b = np.where(inside, np.minimum(b, B - 1), 0).astype(np.int64)
    return np.where(~fin, B + 2, np.where(safe < lower, B, np.where(safe >= upper, B + 1, b)))


def pairs(ndim):
    return [(a, b) for a in range(ndim) for b in range(a + 1, ndim)]


def entries(ndim):
    """(a, b) of every moment entry in the device's order: s1[d] as (d, None), then s2[a][b] for a <= b."""
    return [(d, None) for d in range(ndim)] + [(a, b) for a in range(ndim) for b in range(a, ndim)]


def seq_sum(terms):
    """Sum over axis 0 in increasing index from 0.0."""
    z = np.zeros((1,) + terms.shape[1:])
    return np.cumsum(np.concatenate([z, terms]), axis=0)[-1]


def accumulate(chain, lnp, bins1, bins2, lower, upper):
    """Every accumulator of one ensemble: hist1 (ndim, bins1), below, above, nonfinite (ndim,), hist2 (npairs, bins2, bins2),
    outside2 (npairs,) (None with bins2 = 0), the per-walker sums mom (n_entries, n_walkers) and counts nfin (n_walkers,), their
    totals sum1 (ndim,), sum2 (ndim, ndim), n_finite, the pivot, and best_x, best_lnp, best_idx."""
    chain, lnp = np.asarray(chain, dtype=np.float64), np.asarray(lnp, dtype=np.float64)
    n, nw, ndim = chain.shape
    lo, hi = np.asarray(lower, dtype=np.float64), np.asarray(upper, dtype=np.float64)
    inv1, inv2, pivot = params(bins1, bins2, lo, hi)
    out = {"n": n * nw, "pivot": pivot}
    code = np.stack([bin_code(chain[..., d], lo[d], hi[d], inv1[d], bins1) for d in range(ndim)])      # (ndim, n, nw)
    counts = np.stack([np.bincount(c.ravel(), minlength=bins1 + 3) for c in code])
    out["hist1"], out["below"], out["above"], out["nonfinite"] = counts[:, :bins1], counts[:, bins1], counts[:, bins1 + 1], counts[:, bins1 + 2]
    out["hist2"] = out["outside2"] = None
    if bins2:
        code2 = [bin_code(chain[..., d], lo[d], hi[d], inv2[d], bins2).ravel() for d in range(ndim)]
        h2, o2 = [], []
        for a, b in pairs(ndim):
            ok = (code2[a] < bins2) & (code2[b] < bins2)
            h2.append(np.bincount(code2[a][ok] * bins2 + code2[b][ok], minlength=bins2 * bins2).reshape(bins2, bins2))
            o2.append(np.count_nonzero(~ok))
        out["hist2"] = np.array(h2, dtype=np.int64).reshape(len(h2), bins2, bins2)
        out["outside2"] = np.array(o2, dtype=np.int64)
    fin = np.all(np.isfinite(chain), axis=2)                                                           # (n, nw)
    y = np.where(fin[..., None], chain, pivot) - pivot                                                 # 0.0 where skipped
    mom = np.stack([seq_sum(y[..., a] if b is None else y[..., a] * y[..., b]) for a, b in entries(ndim)])
    out["mom"], out["nfin"] = mom, np.count_nonzero(fin, axis=0).astype(np.int64)
    tot = seq_sum(mom.T)
    out["sum1"] = tot[:ndim].copy()
    s2 = np.empty((ndim, ndim))
    for k, (a, b) in enumerate(entries(ndim)[ndim:]):
        s2[a, b] = s2[b, a] = tot[ndim + k]
    out["sum2"], out["n_finite"] = s2, int(out["nfin"].sum())
    flat = lnp.ravel()                                                                                 # index t * nw + w
    cand = flat > -np.inf                                                                              # (a NaN is not)
    out["best_x"], out["best_lnp"], out["best_idx"] = np.full(ndim, np.nan), -np.inf, -1
    if np.any(cand):
        m = np.max(flat[cand])
        i = int(np.flatnonzero(flat == m)[0])
        out["best_x"], out["best_lnp"], out["best_idx"] = chain.reshape(-1, ndim)[i].copy(), float(m), i
    return out


def holder_loop(lnp):
    """The best-sample rule as the header words it, one sample at a time: (lnprob, index) of the holder."""
    bl, bi = -np.inf, -1
    for i, v in enumerate(np.asarray(lnp, dtype=np.float64).ravel()):
        if v > bl or (v == bl and i < bi):
            bl, bi = float(v), i
    return bl, bi
