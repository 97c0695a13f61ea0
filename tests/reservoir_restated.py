"""The sampler's sample reservoir restated in numpy and plain Python (include/magprop_amd.h mp_sampler_set_reservoir states the
rule; magprop_amd/csrc/mp_reservoir.hip runs it): the keys from the restated Philox of oracle/stretch_oracle.py, the definition
as a sort of all keys (`brute`), the device's way through a stream in chunks and slices with a threshold and a candidate list
(`Reservoir`), and one merge launch over given entries (`merge_launch`).  Test infrastructure."""
import functools

import numpy as np

from oracle.stretch_oracle import philox4x32_10

RES_CTR = 0x52455300
CAND_CAP = 32768                 # csrc/mp_reservoir.h kResCandCap
M32 = 0xFFFFFFFF


@functools.lru_cache(maxsize=None)
def key(seed, t, index):
    """The key of the sample of step t whose walker has index e * n_walkers + w over all ensembles."""
    r = philox4x32_10(seed & M32, (seed >> 32) & M32, t & M32, (t >> 32) & M32, index, RES_CTR)
    return (r[0] << 32) | r[1]


def entries(seed, steps, n_walkers, e):
    """(key, t, w) of every sample of ensemble e over the steps."""
    return [(key(seed, t, e * n_walkers + w), t, w) for t in steps for w in range(n_walkers)]


def brute(seed, steps, n_walkers, e, size):
    """The definition: the `size` least (key, t, w) of all samples of the steps, as a list sorted by (t, w)."""
    return sorted(sorted(entries(seed, steps, n_walkers, e))[:size], key=lambda k: (k[1], k[2]))


def merge_launch(held, cand, size):
    """One merge over held entries and candidates, lists of (key, t, w): the entries held afterwards (a set) and the threshold,
    None where the union has <= size members (no cut is made then)."""
    union = sorted(list(held) + list(cand))
    if len(union) <= size:
        return set(union), None
    return set(union[:size]), union[size - 1]


class Reservoir:
    """The monitor as the device runs it: per ensemble a held set and a threshold; a chunk goes in by slices of whole steps of
    at most cand_cap samples per ensemble; a slice's samples not above the threshold become candidates and one merge follows."""

    def __init__(self, size, seed, discard, n_walkers, n_ensembles, cand_cap=CAND_CAP):
        self.size, self.seed, self.discard, self.nw, self.ne = size, seed, discard, n_walkers, n_ensembles
        self.cand_cap = max(cand_cap, n_walkers)
        self.restart()

    def restart(self):
        self.skip = self.discard
        self.held = [set() for _ in range(self.ne)]
        self.thr = [None] * self.ne
        self.n_seen = [0] * self.ne
        self.n_cand = []            # per slice fed: the candidates of every ensemble

    def feed(self, rows, step0):
        """`rows` steps whose first is the sampler's step step0."""
        first = min(self.skip, rows)
        self.skip -= first
        slice_rows = max(1, self.cand_cap // self.nw)
        for r in range(first, rows, slice_rows):
            steps = range(step0 + r, step0 + min(r + slice_rows, rows))
            counts = []
            for e in range(self.ne):
                cand = [k for k in entries(self.seed, steps, self.nw, e) if self.thr[e] is None or k <= self.thr[e]]
                counts.append(len(cand))
                self.n_seen[e] += len(steps) * self.nw
                if cand:
                    self.held[e], thr = merge_launch(self.held[e], cand, self.size)
                    self.thr[e] = thr if thr is not None else self.thr[e]
            self.n_cand.append(counts)

    def run(self, chunks, step0, restart_before=-1):
        t = step0
        for i, rows in enumerate(chunks):
            if i == restart_before:
                self.restart()
            self.feed(rows, t)
            t += rows
        return self

    def result(self, e):
        """The held entries of ensemble e sorted by (t, w)."""
        return sorted(self.held[e], key=lambda k: (k[1], k[2]))


def as_arrays(rows):
    """(step int64, walker int32, key uint64) of a list of (key, t, w)."""
    return (np.array([r[1] for r in rows], dtype=np.int64), np.array([r[2] for r in rows], dtype=np.int32),
            np.array([r[0] for r in rows], dtype=np.uint64))
