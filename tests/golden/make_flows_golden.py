#!/usr/bin/env python3
"""Generate tests/golden/golden_flows.npz by RUNNING the reference's code/figure_3.py up to its plotting section.

Runs only where the reference checkout is at hand (first argument, default /root/reference); nothing of the reference is
copied: the script's text is read, cut in front of its "# === Plotting === #" line, compiled and executed in a scratch
directory (it makes a plots/ folder where it runs) with matplotlib's Agg backend, and the arrays it leaves behind are stored
as data.

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_flows_golden.py [/path/to/reference]

Stored, at every 25th grid point and at both ends (401 of the script's 10 001 points; "idx" holds the indices):
  tarr                              code/figure_3.py:20
  po_Mdisc, po_omega                the Piro & Ott integration (:193-195); b_Mdisc, b_omega: the Bucciantini one (:198-200)
  po_* and b_* of Rm, Rc, Rlc, w, Ndip, Mdotprop, Mdotacc, Nacc     the sixteen recovered arrays (:206-234, :248-275)
  pars = (B, P, MdiscI, RdiscI, epsilon, delta)  (:174-179);  consts = (n, alpha, cs7, k, I / (M R^2))  (:13-18)
MANIFEST.json is make_golden.py's and is left alone.
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
RECOVERED = ("Rm", "Rc", "Rlc", "w", "Ndip", "Mdotprop", "Mdotacc", "Nacc")
STEP = 25


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    path = os.path.join(ref, "code", "figure_3.py")
    text = open(path).read()
    cut = text.index("# === Plotting === #")
    import matplotlib
    matplotlib.use("Agg")
    ns = {"__name__": "figure_3_recovery"}
    here = os.getcwd()
    with tempfile.TemporaryDirectory() as scratch:
        os.chdir(scratch)
        try:
            exec(compile(text[:cut], path, "exec"), ns)
        finally:
            os.chdir(here)
    n_grid = ns["tarr"].size
    idx = np.unique(np.concatenate([np.arange(0, n_grid, STEP), [n_grid - 1]]))
    out = {"idx": idx, "tarr": ns["tarr"][idx],
           "pars": np.array([ns[k] for k in ("B", "P", "MdiscI", "RdiscI", "epsilon", "delta")], dtype=np.float64),
           "consts": np.array([ns["n"], ns["alpha"], ns["cs7"], ns["k"], ns["I"] / (ns["M"] * ns["R"] ** 2.0)], dtype=np.float64)}
    for m in ("po", "b"):
        for name in ("Mdisc", "omega") + RECOVERED:
            out[f"{m}_{name}"] = np.asarray(ns[f"{m}_{name}"], dtype=np.float64)[idx]
    np.savez_compressed(os.path.join(HERE, "golden_flows.npz"), **out)
    print("wrote golden_flows.npz:", len(out), "arrays,", idx.size, "grid points")


if __name__ == "__main__":
    main()
