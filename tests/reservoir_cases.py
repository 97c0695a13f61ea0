"""Named cases for the kernels of the sampler's sample reservoir (magprop_amd/csrc/mp_reservoir.hip): the streams that
tests/test_reservoir_cpu.py holds to the definition on the restatement and tests/test_gpu_reservoir_kernels.py holds to the
restatement bit for bit on the device, and the merge launches over crafted keys.  Test infrastructure."""
from typing import NamedTuple

import numpy as np

from reservoir_restated import CAND_CAP

U64_MAX = (1 << 64) - 1


class RunCase(NamedTuple):
    name: str
    n_walkers: int
    n_ensembles: int
    ndim: int
    size: int
    chunks: tuple              # several chunk lists of the same stream: all must give the same reservoir
    seed: int = 0x1234567890ABCDEF
    step0: int = 1             # the sampler's index of the first step (the probe wants >= 1)
    discard: int = 0
    restart_before: int = -1   # (then `chunks` holds one list)


def n_steps(case):
    return sum(case.chunks[0])


def run_cases():
    out = []
    # 4 steps of 64 walkers are 256 samples: K = 257 is never full, 256 exactly full, 255 one past full; then the same K on a
    # stream of 40 steps, whole, step by step, and in uneven chunks with an empty one
    for k in (1, 63, 64, 65, 255, 256, 257):
        out.append(RunCase(f"K={k} 256 samples", 64, 2, 6, k, ((4,), (1, 1, 1, 1), (3, 0, 1))))
        out.append(RunCase(f"K={k} 40 steps", 64, 2, 6, k, ((40,), (1,) * 40, (7, 30, 0, 3))))
    for nw in (63, 64, 65):
        out.append(RunCase(f"{nw} walkers", nw, 2, 6, 64, ((12,), (1,) * 12, (5, 7))))
    out.append(RunCase("ndim 9", 64, 2, 9, 65, ((9,), (4, 5))))
    out.append(RunCase("1 ensemble", 64, 1, 6, 64, ((9,), (4, 5))))
    out.append(RunCase("16 ensembles", 16, 16, 6, 63, ((20,), (1,) * 20, (13, 7))))
    # K = 1 over 300 steps: nearly every late chunk has no candidate (test_reservoir_cpu.py counts them)
    out.append(RunCase("chunks without a candidate", 64, 2, 6, 1, ((1,) * 300, (300,), (7, 292, 1))))
    # one slice holds CAND_CAP samples per ensemble: a chunk of exactly that, and of one step more (two slices)
    per = CAND_CAP // 64
    out.append(RunCase("a slice at the candidate capacity", 64, 1, 6, 64, ((per,),)))
    out.append(RunCase("one step past the candidate capacity", 64, 1, 6, 64, ((per + 1,), (per, 1), (1, per))))
    out.append(RunCase("discard inside a chunk", 64, 2, 6, 64, ((7, 30, 3), (40,), (1,) * 40), discard=11))
    out.append(RunCase("discard of whole chunks", 64, 2, 6, 64, ((7, 30, 3), (40,)), discard=37))
    out.append(RunCase("restart", 64, 2, 6, 64, ((7, 10, 20, 3),), discard=2, restart_before=2))
    out.append(RunCase("steps across 2^32", 64, 2, 6, 64, ((6,), (2, 4)), step0=(1 << 32) - 3))
    return out


def run_chain(case):
    """chain[n, n_total, ndim] and lnp[n, n_total] of a case: every cell distinct, with NaN, +-inf and -0.0 cells."""
    n, nt = n_steps(case), case.n_walkers * case.n_ensembles
    rng = np.random.default_rng(len(case.name) + 31 * case.size + nt)
    chain = rng.normal(size=(n, nt, case.ndim))
    lnp = -np.abs(rng.normal(size=(n, nt))) * 100.0
    chain[0, 0, 0] = np.nan
    chain[n - 1, nt - 1, case.ndim - 1] = np.inf
    chain[n // 2, nt // 2, 1] = -0.0
    lnp[0, 1] = -np.inf
    lnp[n - 1, 0] = np.nan
    return chain, lnp


class MergeCase(NamedTuple):
    """One launch of res_merge_kernel: per ensemble the held entries and the candidates, lists of (key, t, w)."""
    name: str
    size: int
    n_walkers: int
    ndim: int
    n_rows: int                # steps of the slab, the first of them step t0
    t0: int
    held: tuple                # per ensemble
    cand: tuple


def _grid(n_rows, n_walkers, t0):
    return [(t, w) for t in range(t0, t0 + n_rows) for w in range(n_walkers)]


def merge_cases():
    out = []
    nw, rows, t0 = 8, 40, 1000
    cells = _grid(rows, nw, t0)            # 320 (t, w) of the slab; held entries lie before it
    old = _grid(70, nw, 100)               # 560 (t, w) of earlier steps
    rng = np.random.default_rng(5)

    def shuffled(a):
        a = list(a)
        rng.shuffle(a)
        return a

    for k in (1, 63, 64, 65, 255, 256, 257):
        # all keys equal: the cut is made by (t, w) alone; the held entries are older, so they all stay
        out.append(MergeCase(f"K={k} all keys equal", k, nw, 6, rows, t0,
                             (shuffled((7, t, w) for t, w in old[:k]), shuffled((7, t, w) for t, w in old[:k // 2])),
                             (shuffled((7, t, w) for t, w in cells[:300]), shuffled((7, t, w) for t, w in cells[:k]))))
        # ties straddling the cut: a third below the tied key, then more ties than fit, among held and candidates both
        lo = k // 3
        tied = shuffled(cells[:200])
        held = [(5, t, w) for t, w in old[:lo]] + [(9, t, w) for t, w in tied[:100:2]] + [(11, t, w) for t, w in old[lo:lo + k]]
        out.append(MergeCase(f"K={k} ties straddle the cut", k, nw, 9, rows, t0, (shuffled(held[:k]),),
                             (shuffled([(9, t, w) for t, w in tied[1:200:2]] + [(3, t, w) for t, w in cells[200:200 + min(lo, 5)]]),)))
    # descending keys: every candidate lies below every held entry, so the whole reservoir is replaced
    out.append(MergeCase("the whole reservoir replaced", 64, nw, 6, rows, t0,
                         ([((1 << 63) + i, t, w) for i, (t, w) in enumerate(old[:64])],),
                         ([((1 << 62) - i, t, w) for i, (t, w) in enumerate(cells[:64])],)))
    out.append(MergeCase("more winners than the reservoir holds", 64, nw, 6, rows, t0,
                         ([((1 << 63) + i, t, w) for i, (t, w) in enumerate(old[:64])],),
                         ([((1 << 62) - i, t, w) for i, (t, w) in enumerate(cells[:300])],)))
    # keys 0 and 2^64 - 1, and keys that differ in the top digit only or in the bottom digit only
    ends = [(0, *old[0]), (U64_MAX, *old[1]), (0, *old[2]), (U64_MAX, *old[3])]
    out.append(MergeCase("keys 0 and 2^64 - 1", 4, nw, 6, rows, t0, (ends,),
                         ([(0, *cells[5]), (U64_MAX, *cells[0]), (1, *cells[1]), (U64_MAX - 1, *cells[2])],)))
    top = [((d << 56) | 0x00ABCDEF01234567, t, w) for d, (t, w) in zip(shuffled(range(256)), old[:100] + cells[:156])]
    bottom = [(0x7700ABCDEF012300 | d, t, w) for d, (t, w) in zip(shuffled(range(256)), cells[:256])]
    out.append(MergeCase("top digit only", 100, nw, 6, rows, t0, (top[:100],), (top[100:],)))
    out.append(MergeCase("bottom digit only", 100, nw, 6, rows, t0, ([(k, *o) for (k, _, _), o in zip(bottom[:100], old)],), (bottom[100:],)))
    # 16 ensembles in different fill states: empty, partly filled and full, with none, few and many candidates
    keys = rng.integers(0, 1 << 62, size=(16, 600), dtype=np.int64)
    held, cand = [], []
    for e in range(16):
        h = (0, 1, 31, 64, 64)[e % 5]
        m = (0, 1, 33, 64, 300)[(e // 2) % 5]
        held.append([(int(keys[e, i]), *old[i]) for i in range(h)])
        cand.append([(int(keys[e, 64 + i]), *cells[i]) for i in range(m)])
    out.append(MergeCase("16 ensembles, every fill state", 64, nw, 6, rows, t0, tuple(held), tuple(cand)))
    return out


def merge_slab(case):
    """The slab chain[n_rows, n_total, ndim], lnp[n_rows, n_total] of a merge case, with NaN and inf cells that must be copied as
    they are, and what the held entries hold before the launch: x[n_ens, size, ndim], lnp[n_ens, size] (canaries)."""
    ne = len(case.held)
    rng = np.random.default_rng(case.size + ne)
    chain = rng.normal(size=(case.n_rows, ne * case.n_walkers, case.ndim))
    lnp = -np.abs(rng.normal(size=(case.n_rows, ne * case.n_walkers)))
    chain[:, ::3, 0] = np.nan
    chain[:, 1::3, case.ndim - 1] = np.inf
    chain[:, 2::3, 1] = -np.inf
    lnp[:, ::2] = -np.inf
    lnp[:, 1::4] = np.nan
    return chain, lnp
