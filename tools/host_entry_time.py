"""Wall time per call of the host-buffer entries (numpy in, numpy out: PCIe both ways + synchronisation), the path
`emcee.EnsembleSampler(..., vectorize=True)` drives, next to the kernel time of the same rows (device-pointer entry).
    python tools/host_entry_time.py [--reps 200] [--rows 512,1024]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rows", default="24,256,512,1024,4096", help="batch sizes, comma-separated")
    a = ap.parse_args()
    import pandas as pd
    import torch

    import magprop_amd as mpa
    g = np.load(os.path.join(os.path.dirname(__file__), "..", "tests", "golden", "golden_synth.npz"))
    x, y, yerr = g["Humped_x"], g["Humped_y"], g["Humped_yerr"]
    xs, ys, es = pd.Series(x), pd.Series(y), pd.Series(yerr)
    lp = mpa.LogProb(x, y, yerr)
    rng = np.random.default_rng(1)

    def timed(f):
        for _ in range(10):
            f()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            f()
        return (time.perf_counter() - t0) / a.reps * 1e3

    for n in (int(v) for v in a.rows.split(",")):
        P = np.array([1.0, 5.0, -3.0, 2.0, -1.0, 0.0]) + 1.0e-4 * rng.standard_normal((n, 6))
        dP = torch.from_numpy(P).cuda()
        out = torch.empty(n, dtype=torch.float64, device="cuda")
        for _ in range(10):
            lp.lnprob_device(dP, out=out)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.reps):
            lp.lnprob_device(dP, out=out)
        e1.record()
        torch.cuda.synchronize()
        k = e0.elapsed_time(e1) / a.reps
        t_obj = timed(lambda: lp(P))
        t_np = timed(lambda: mpa.synth.lnprob(P, x, y, yerr, None))
        t_pd = timed(lambda: mpa.synth.lnprob(P, xs, ys, es, None))
        print(f"n={n:5d}  kernel {k:.4f} ms | LogProb.__call__ {t_obj:.4f} ms | synth.lnprob (ndarray args) {t_np:.4f} ms | "
              f"synth.lnprob (pandas Series args) {t_pd:.4f} ms", flush=True)


if __name__ == "__main__":
    main()
