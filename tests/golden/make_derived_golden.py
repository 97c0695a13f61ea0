"""Reference values of the derived quantities (mp_model_derived): tests/golden/golden_derived.npz.

    python tests/golden/make_derived_golden.py          # rewrites the fixture (MANIFEST.json is make_golden.py's and stays as it is)

Rows: the four canonical parameter sets and the `wide_pars_physical` rows of golden_synth.npz (physical units).  For each row the
reference's model_lum runs on its full grid, once as the reference runs it (`ref`) and once with its odeint call given rtol =
atol = 1e-12 (`tight`; make_golden.py tight_lsoda).  Recorded results only, formed with plain numpy from the reference's curves:
    pars (n, 6)
    ref, tight (n, 7)           E_tot, E_prop, E_dip (np.trapz), L_peak, t_peak, Lprop_peak, t_Lprop_peak (np.max, np.argmax)
    tight_peak_idx (n, 2)       np.argmax of the tight Ltot and Lprop
    tight_peak_nbr (n, 2, 2 K + 1)   the tight curve at the K = NBR grid points either side of that index (NaN beyond the grid)
    t_first, t_last             the ends of the grid
    neighbours, versions        K and the versions of numpy, scipy and python that made the file
A row the reference flags is NaN throughout."""
import os
import sys

import numpy as np
import scipy

from make_golden import GRB_PARS, HERE, TYPES, quiet, sf, tight_lsoda

NBR = 32
trapz = getattr(np, "trapezoid", None) or np.trapz


def columns(model):
    """(the 7 columns, argmax of Ltot and Lprop, their neighbourhoods) of one model_lum result, or NaNs for a flagged one"""
    if isinstance(model, str):
        return np.full(7, np.nan), np.full(2, -1), np.full((2, 2 * NBR + 1), np.nan)
    t, ltot, lprop, ldip = model
    idx = np.array([np.argmax(ltot), np.argmax(lprop)])
    cols = np.array([trapz(ltot, t), trapz(lprop, t), trapz(ldip, t), ltot[idx[0]], t[idx[0]], lprop[idx[1]], t[idx[1]]])
    nbr = np.full((2, 2 * NBR + 1), np.nan)
    for k, (c, i) in enumerate(zip((ltot, lprop), idx)):
        for j in range(-NBR, NBR + 1):
            if 0 <= i + j < t.size:
                nbr[k, j + NBR] = c[i + j]
    return cols, idx, nbr


def main():
    g = np.load(os.path.join(HERE, "golden_synth.npz"))
    pars = np.concatenate([np.array([GRB_PARS[name] for name in TYPES]), g["wide_pars_physical"]])
    ref = np.array([columns(quiet(sf.model_lum, p))[0] for p in pars])
    with tight_lsoda():
        models = [quiet(sf.model_lum, p) for p in pars]
    tight = [columns(m) for m in models]
    t = next(m[0] for m in models if not isinstance(m, str))
    path = os.path.join(HERE, "golden_derived.npz")
    np.savez_compressed(path, pars=pars, ref=ref, tight=np.array([c[0] for c in tight]),
                        tight_peak_idx=np.array([c[1] for c in tight]), tight_peak_nbr=np.array([c[2] for c in tight]),
                        t_first=t[0], t_last=t[-1], neighbours=NBR,
                        versions=np.array(["numpy " + np.__version__, "scipy " + scipy.__version__,
                                           "python %d.%d.%d" % sys.version_info[:3]]))
    print(path, os.path.getsize(path), "bytes;", int(np.isfinite(ref).all(axis=1).sum()), "of", len(pars), "rows finished")


if __name__ == "__main__":
    main()
