"""GPU tests that hold the fused ensemble sampler on the REAL posterior (target 0) to mp_lnprob_batch bit for bit, build by
build: the device sampler and the numpy restatement (tests/sampler_restated.py, evaluate=) run in step, every likelihood of the
restatement one mp_lnprob_batch call whose row count selects the kernel build of the device launch (stretch_class), ensembles
on different light curves.  First the outcome rows of the walker-sharded entry points, which localise a failure; then the
chains of mp_sampler_run for every reachable build of stretch_step_kernel and of the DIFF and KDE builds of stretch_kernel, the
LONG builds under a launch order that is not the identity, tempered samplers, failing models, split runs; last the contract
that one launch per step and two half-step launches run one chain at the class boundaries.  No tolerance appears: every
comparison is np.array_equal."""
import ctypes as C

import numpy as np
import pytest

import probe_lib
import sampler_restated as sr
from conftest import TRUTHS, TYPES
from kde_restated import KDE
from moves_restated import DE, SNOOKER
from oracle.stretch_oracle import M32, _draw, philox4x32_10, split, step_rows, u01
from raw_abi import RawSampler, dp
from test_gpu_moves_slice import FAILS
from test_gpu_nested import (LONG_MIXED_LENGTHS, BatchEvaluator, launch_class, long_cases, long_mixed_sets, long_sets,  # noqa: F401
                             synth_sets)  # (the three handles are fixtures)

pytestmark = pytest.mark.gpu

DIFF_TABLE = [(DE, 0.5, 0.0, 1.0e-5), (SNOOKER, 0.5, 1.7, 0.0)]
KDE_TABLE = [(KDE, 1.0, 0.0, 0.0)]
DE_TABLE = [(DE, 1.0, 0.0, 1.0e-5)]
LADDER = (1.0, 0.3)
SEED = 20261301


def stretch_class(n_blocks, n_slots, ns):
    """launch_class's triple for a stretch launch of n_blocks blocks of a sampler of n_slots slots per half on ns SIMDs
    (mp_device.h stretch_waves / walker_variant): a team of four iff a WHOLE step fits half the SIMDs, 2 (3 n_slots) <= ns; a
    team is roomy iff 4 n_blocks <= ns; one wavefront per walker runs 4 steps per lane iff n_blocks <= ns."""
    if 2 * (3 * n_slots) <= ns:
        return (4, 1, 1) if 4 * n_blocks <= ns else (4, 1, 2)
    return (1, 4, 1) if n_blocks <= ns else (1, 2, 2)


def whole_step_fits(n_slots, ns):
    return 8 * 3 * n_slots <= 19 * ns


def run_blocks(n_slots, ns, table, whole):
    """(blocks launched, blocks that choose the variant) of a step of mp_sampler_run: a whole step per launch for the stretch
    move where it fits; the half-step launches of the stretch move of such a sampler (mp_sampler_set_whole_step(0)) take the
    whole step's variant; every other half-step launch is judged by its own size."""
    fits = table is None and whole_step_fits(n_slots, ns)
    if fits:
        return (3 * n_slots if whole else n_slots), 3 * n_slots
    return n_slots, n_slots


def eval_rows(cls, k, ns):
    """A row count of mp_lnprob_batch that holds k rows and runs build cls (launch_class)."""
    n = k if launch_class(k, ns) == cls else {(4, 1, 1): ns // 4, (4, 1, 2): ns // 2, (1, 4, 1): ns}.get(cls, ns + 1)
    assert k <= n and launch_class(n, ns) == cls, (cls, k, ns)
    return n


def start_near_truths(ens_ds, nw, seed, fails=False, truths=None):
    """truths + 1e-2 randn per ensemble (truths: of TYPES[d] unless given); fails: the first half of every ensemble in a ball
    of 0.05 around a point whose model fails, clipped into the prior box."""
    from magprop_amd import synth
    rng = np.random.default_rng(seed)
    truths = [TRUTHS[TYPES[d]] for d in ens_ds] if truths is None else truths
    pos = np.concatenate([np.array(t) + 1.0e-2 * rng.standard_normal((nw, 6)) for t in truths])
    if fails:
        for e in range(len(ens_ds)):
            pos[e * nw:e * nw + nw // 2] = np.clip(FAILS + 0.05 * rng.standard_normal((nw // 2, 6)), synth.PRIOR_LOWER,
                                                   synth.PRIOR_UPPER)
    return pos


def restate_posterior(at, ns, ens_ds, nw, pos, steps, seed, table=None, whole=True, betas=None, lnp0=None, kde_device=None):
    """The restatement of drive_posterior's run, from at(n) -> evaluate(rows, ensemble of every row) alone: the start by a call
    of the size of mp_sampler_set_positions' launch, the half-steps by calls of the class of the step's launches.  Returns the
    Run, the start's lnprob, (class, evaluator rows) of the step.  kde_device: the device's log, sqrt, cos and sin, with which
    the KDE proposal is restated in the kernel's own order on the workgroup of the launch's class."""
    from magprop_amd import synth
    n_ens = len(ens_ds)
    n_slots = (nw // 2) * n_ens
    launched, choosing = run_blocks(n_slots, ns, table, whole)
    cls = stretch_class(choosing, n_slots, ns)
    n_eval = eval_rows(cls, n_slots, ns)
    step_eval = at(n_eval)
    start = at(n_ens * nw)(pos, np.arange(n_ens * nw) // nw)[0]
    ref = sr.run(pos.copy(), steps, seed, table or [(0, 1.0, 2.0, 0.0)], n_ensembles=n_ens, lnp=(start if lnp0 is None else lnp0).copy(),
                 betas=None if betas is None else [betas[e % len(betas)] for e in range(n_ens)],
                 n_temps=0 if betas is None else len(betas), evaluate=lambda rows, walkers: step_eval(rows, walkers // nw),
                 box=(synth.PRIOR_LOWER, synth.PRIOR_UPPER), kde_device=kde_device and (cls[0], kde_device))
    return ref, start, (cls, n_eval)


def assert_not_vacuous(ref, n_ens, tempered=False, outside=False):
    """Read off the restatement alone: every ensemble accepted and rejected an evaluated proposal; where asked, a proposal
    left the prior box; tempered: a swap was accepted and one refused."""
    c = ref.counts
    assert np.all(c["accepted"] > 0) and np.all(c["rejected"] > 0), c
    if outside:
        assert c["outside"].sum() > 0
    if tempered:
        assert ref.swaps.sum() > 0 and c["swap_refused"].sum() > 0, (ref.swaps, c["swap_refused"])


def device_run(h, ens_ds, nw, pos, runs, seed, table=None, whole=True, betas=None, autocorr=0):
    """mp_sampler_run calls of runs[i] steps on the posterior.  Returns the start's lnprob, chain, chain lnprob, the final
    state (pos, lnprob, n_accepted), (n_bad, logged rows) and the swap counts (None untempered)."""
    with RawSampler(nw, len(ens_ds), 6, seed, target=0, handle=h, ds=ens_ds) as r:
        if betas is not None:
            r.set_temperatures(betas)
        r.set_whole_step(1 if whole else 0)
        if table is not None:
            r.set_moves(table)
        if autocorr:
            r.set_autocorr(autocorr, 0)
        r.set_positions(pos)
        lnp0 = r.state()[1]
        chain, lnp, _ = r.run_chunks(runs)
        swaps = r.swaps(len(ens_ds) // len(betas), len(betas)) if betas is not None else None
        return lnp0, chain, lnp, r.state(), r.bad(), swaps


def assert_device_equals(dev, ref, start):
    lnp0, chain, lnp, (dpos, dlnp, dacc), (n_bad, bad_rows), swaps = dev
    assert np.array_equal(lnp0, start), np.flatnonzero(lnp0 != start)[:4]
    assert np.array_equal(chain, ref.chain), np.argwhere(chain != ref.chain)[:4]
    assert np.array_equal(lnp, ref.lnp), np.argwhere(lnp != ref.lnp)[:4]
    assert np.array_equal(dpos, ref.chain[-1]) and np.array_equal(dlnp, ref.lnp[-1]) and np.array_equal(dacc, ref.acc)
    assert n_bad == len(ref.bad) == len(bad_rows), (n_bad, len(ref.bad), len(bad_rows))
    assert sorted(map(tuple, bad_rows)) == sorted(map(tuple, ref.bad))
    if swaps is not None:
        assert np.array_equal(swaps, ref.swaps), (swaps, ref.swaps)


def drive_posterior(h, ens_ds, nw, steps, seed=SEED, table=None, whole=True, betas=None, build=None, fails=False, runs=None,
                    autocorr=0, outside=False, compare=True, truths=None):
    """A sampler of len(ens_ds) ensembles of nw walkers on h (target 0) and the restatement in step.  Equal afterwards: the
    start's lnprob, chain, chain lnprob, final pos / lnprob / n_accepted, n_bad, the logged rows as multisets and, tempered, the
    swap counts (compare=False: left to the caller).  Returns the restatement's Run, the batch's start lnprob, the device's
    results and an evaluator of the step's class: rows, ensembles -> lnprob."""
    ns, n_ens = h.n_simd, len(ens_ds)
    n_slots = (nw // 2) * n_ens
    pos = start_near_truths(ens_ds, nw, seed, fails, truths)
    dev = device_run(h, ens_ds, nw, pos, runs or (steps,), seed, table, whole, betas, autocorr)
    ev = BatchEvaluator(h, ens_ds)
    # the decisions start from the device's own start values, which are compared with the batch in assert_device_equals
    ref, start, (cls, n_eval) = restate_posterior(ev.at, ns, ens_ds, nw, pos, steps, seed, table, whole, betas, lnp0=dev[0],
                                                  kde_device=DeviceLibm() if table is KDE_TABLE else None)
    if build is not None:
        assert cls == build, (cls, build, n_slots, ns)
    c = ref.counts
    print(f"{n_slots} slots, launch {run_blocks(n_slots, ns, table, whole)[0]} blocks {cls}, start launch {launch_class(n_ens * nw, ns)}, "
          f"evaluator {n_eval} rows, {ev.calls} batches, accepted {c['accepted'].tolist()} rejected {c['rejected'].tolist()} "
          f"outside {c['outside'].tolist()} unevaluated {c['unevaluated'].tolist()}, start at -inf {int(np.sum(~np.isfinite(start)))}, "
          f"n_bad {len(ref.bad)} (device {dev[4][0]}), swaps {ref.swaps.tolist()} refused {c.get('swap_refused', np.zeros(0)).tolist()}")
    if compare:
        assert_device_equals(dev, ref, start)
    assert_not_vacuous(ref, n_ens, tempered=betas is not None, outside=outside)
    return ref, start, dev, ev.at(n_eval)


def drive_long(h, ens_ds, nw, steps, **kw):
    """drive_posterior on long_mixed_sets (every set is Humped-type: starts around Humped's truths).  The ensembles mix a light
    curve of at most 64 points with longer ones and their lengths do not descend as numbered, so the launches start them in
    another order (ens_order; stable: mp_sampler.cpp stretch_args); every ensemble's best lnprob is finite (that each accepted
    and rejected an evaluated proposal: assert_not_vacuous)."""
    lens = [LONG_MIXED_LENGTHS[d] for d in ens_ds]
    assert sorted(range(len(ens_ds)), key=lambda e: -lens[e]) != list(range(len(ens_ds)))
    assert min(lens) <= 64 < max(lens)
    out = drive_posterior(h, ens_ds, nw, steps, truths=[TRUTHS["Humped"]] * len(ens_ds), **kw)
    assert np.all(np.isfinite(out[0].lnp[-1].reshape(len(ens_ds), nw).max(axis=1)))
    return out


# ---------------------------------------------------------------- rows first: the stage that localises a failure
class DeviceLibm:
    """The device runtime's log, cos, sin and sqrt, element by element (libmp_probe_libm.so mpl_libm).  ln u and the stretch move's
    ln z of an outcome row are the device log's values, which numpy's log misses by an ulp now and then (2 of 72 rows of the
    first step here); the normals of a KDE proposal go through all four."""

    def _call(self, func, x):
        x = np.asarray(x, dtype=np.float64)
        n = -(-max(x.size, 1) // 64) * 64
        buf, out = np.ones(n), np.empty(n)
        buf[:x.size] = x.ravel()
        assert probe_lib.load("libm").mpl_libm(func, dp(buf), dp(out), C.c_int(n)) == 0
        return out[:x.size].reshape(x.shape)

    def log(self, x):
        return self._call(0, x)

    def cos(self, x):
        return self._call(1, x)

    def sin(self, x):
        return self._call(2, x)

    def sqrt(self, x):
        return self._call(3, x)


def device_log(x):
    return DeviceLibm().log(x)


def _restated_step_rows(ev, ns, ens_ds, nw, pos, lnp, seed, step):
    """The rows of mp_sampler_step_shard over all blocks of one step: the draw from oracle/stretch_oracle.step_rows, lnprob and
    status from ONE batch of the launch's class over the blocks that are evaluated (type 2 with the partner's proposal outside
    the prior box: -inf, MP_STATUS_PRIOR, no evaluation).  Returns rows and the mask of those type-2 blocks."""
    from magprop_amd import synth
    n_ens = len(ens_ds)
    n_slots = (nw // 2) * n_ens
    perms = [split(seed, step, e, nw) for e in range(n_ens)]
    rows = step_rows(pos, lnp, perms, seed, step, 0, 3 * n_slots, nw, lnprob_fn=lambda q: 0.0)
    ens = np.tile(np.repeat(np.arange(n_ens), nw // 2), 3)
    zz, u = np.empty(3 * n_slots), np.empty(3 * n_slots)
    for b in range(3 * n_slots):      # (ndim - 1) ln z and ln u again, through the device's log
        half, (e, slot) = int(b >= n_slots), divmod(b % n_slots, nw // 2)
        k = e * nw + perms[e][half * (nw // 2) + slot]
        zz[b] = _draw(seed, step, half, k, nw - nw // 2, 2.0)[1]
        r2 = philox4x32_10(seed & M32, seed >> 32, step, half, k, 1)
        u[b] = u01(r2[0], r2[1])
    rows[:, 6 + 2], rows[:, 6 + 3] = (6 - 1.0) * device_log(zz), device_log(u)
    # the partner's proposal of a type-2 block is the type-0 proposal of the partner's slot
    partner = ens[2 * n_slots:] * (nw // 2) + rows[2 * n_slots:, 6 + 5].astype(int)
    yj = rows[partner, :6]
    skipped = np.zeros(3 * n_slots, dtype=bool)
    skipped[2 * n_slots:] = np.any((yj < synth.PRIOR_LOWER) | (yj > synth.PRIOR_UPPER), axis=1)
    cls = stretch_class(3 * n_slots, n_slots, ns)
    live = ~skipped
    out, st = ev.at(eval_rows(cls, int(live.sum()), ns))(rows[live, :6], ens[live])
    rows[:, 6], rows[:, 7] = -np.inf, sr.MP_STATUS_PRIOR
    rows[live, 6], rows[live, 7] = out, st
    return rows, skipped


def test_rows_of_the_sharded_entry_points_match_the_restated_draw_and_lnprob_batch(synth_sets):
    """Three ensembles of 16 walkers on three light curves, two steps through mp_sampler_step_shard / _apply and two through
    mp_sampler_halfstep_shard / _apply over the full range: every column of every row equals the restated draw and one
    mp_lnprob_batch call of the launch's class; the applied rows give the restated state.  The sharded entry points take the
    default stretch move only: with a DE / snooker or a KDE table they answer MP_ESTATE, which is asserted."""
    from magprop_amd import _capi
    h, ens_ds, nw, seed = synth_sets, [2, 0, 1], 16, SEED + 1
    ns, n_ens, n_slots = h.n_simd, 3, 24
    pos0 = start_near_truths(ens_ds, nw, seed, fails=True)      # (half of every ensemble at the edge of the box)
    ev = BatchEvaluator(h, ens_ds)
    n_skipped = 0
    with RawSampler(nw, n_ens, 6, seed, target=0, handle=h, ds=ens_ds) as r:
        r.set_positions(pos0)
        assert (r.n_slots, r.step_blocks, r.row_doubles, r.step_row_doubles) == (n_slots, 3 * n_slots, 9, 12)
        pos, lnp, acc = r.state()
        assert np.array_equal(lnp, ev.at(n_ens * nw)(pos0, np.arange(n_ens * nw) // nw)[0])
        for step in range(2):          # a whole step per launch
            got = r.step_shard(0, 3 * n_slots)
            want, skipped = _restated_step_rows(ev, ns, ens_ds, nw, pos, lnp, seed, step)
            n_skipped += int(skipped.sum())
            for col, name in enumerate(["q0", "q1", "q2", "q3", "q4", "q5", "lnprob", "status", "hastings", "ln u", "lnprob before",
                                        "partner"]):
                assert np.array_equal(got[:, col], want[:, col]), (step, name, np.flatnonzero(got[:, col] != want[:, col])[:4])
            ch, ln = r.step_apply(got)
            ref = sr.run(pos, 1, seed, [(0, 1.0, 2.0, 0.0)], n_ensembles=n_ens, step0=step, lnp=lnp, acc=acc,
                         evaluate=lambda q, w: ev.at(eval_rows(stretch_class(3 * n_slots, n_slots, ns), n_slots, ns))(q, w // nw))
            assert np.array_equal(ch, ref.chain[0]) and np.array_equal(ln, ref.lnp[0])
            dpos, dlnp, dacc = r.state()
            assert np.array_equal(dpos, pos) and np.array_equal(dlnp, lnp) and np.array_equal(dacc, acc)
        cls = stretch_class(n_slots, n_slots, ns)
        for step in range(2, 4):       # two half-step launches
            log = []

            def evaluate(q, w):
                out, st = ev.at(eval_rows(cls, n_slots, ns))(q, w // nw)
                log.append((q.copy(), w.copy(), out, st))
                return out, st
            before = pos.copy()
            ref = sr.run(pos, 1, seed, [(0, 1.0, 2.0, 0.0)], n_ensembles=n_ens, step0=step, lnp=lnp, acc=acc, evaluate=evaluate)
            for half in range(2):
                got = r.halfstep_shard(half, 0, n_slots)
                q, w, out, st = log[half]
                assert np.array_equal(got[:, :6], q) and np.array_equal(got[:, 6], out) and np.array_equal(got[:, 8], st)
                assert np.array_equal(got[:, 7] != 0.0, ref.accepted[0, w])
                ch, ln = r.halfstep_apply(half, got, *((ch, ln) if half else ()))
            assert np.array_equal(ch, ref.chain[0]) and np.array_equal(ln, ref.lnp[0]) and not np.array_equal(before, pos)
            dpos, dlnp, dacc = r.state()
            assert np.array_equal(dpos, pos) and np.array_equal(dlnp, lnp) and np.array_equal(dacc, acc)
    for table in (DIFF_TABLE, KDE_TABLE):
        with RawSampler(nw, n_ens, 6, seed, target=0, handle=h, ds=ens_ds) as r:
            r.set_moves(table)
            r.set_positions(pos0)
            assert r.halfstep_shard(0, 0, n_slots, check=False) == _capi.MP_ESTATE and "move table" in _capi.last_error()
            assert r.step_shard(0, 3 * n_slots, check=False) == _capi.MP_ESTATE and "move table" in _capi.last_error()
    print(f"rows: step launch {stretch_class(3 * n_slots, n_slots, ns)}, half-step launch {cls}, {ev.calls} batches, "
          f"{n_skipped} type-2 blocks behind a proposal outside the box, accepted {acc.reshape(n_ens, nw).sum(axis=1).tolist()}")
    assert 0 < acc.sum() < 4 * n_ens * nw and n_skipped > 0


# ---------------------------------------------------------------- chains, build by build
def family_cases(ns):
    """The smallest shape of every reachable cell of the launch table: (ensembles' datasets, walkers per ensemble, class)."""
    whole = {"team-1": ([2, 0, 1], 16, (4, 1, 1)), "team-2": ([3, 1], 3 * ns // 32, (4, 1, 2)),
             "wave-4": ([1, 2], ns // 4, (1, 4, 1)), "wave-2": ([0, 3], 3 * ns // 8, (1, 2, 2))}
    half = {"team-1": ([2, 0, 1], 16, (4, 1, 1)), "wave-4": ([1, 2], ns // 4, (1, 4, 1)), "wave-2": ([0, 3], 5 * ns // 4, (1, 2, 2))}
    return {"stretch": whole, "diff": half, "kde": half}


FAMILY_TABLE = {"stretch": None, "diff": DIFF_TABLE, "kde": KDE_TABLE}
FAMILY_IDS = [("stretch", c) for c in ("team-1", "team-2", "wave-4", "wave-2")] + [("diff", c) for c in ("team-1", "wave-4", "wave-2")]


@pytest.mark.parametrize("family,case", FAMILY_IDS)
def test_posterior_chains_match_lnprob_batch_on_every_build(synth_sets, family, case):
    """stretch by whole steps on its four builds and the DE + snooker mixture by half-steps on its three (KDE: below):
    ensembles on different light curves from truths + 1e-2 randn, three steps up to 100 slots, one beyond.  (From these starts
    no proposal of any of the cases leaves the prior box -- the restatement with the serial C oracle as evaluator says so --:
    that condition is met and asserted from the starts of the next test.)"""
    ens_ds, nw, build = family_cases(synth_sets.n_simd)[family][case]
    n_slots = (nw // 2) * len(ens_ds)
    drive_posterior(synth_sets, ens_ds, nw, 3 if n_slots <= 100 else 1, table=FAMILY_TABLE[family], build=build)


@pytest.mark.parametrize("family,case", FAMILY_IDS)
def test_posterior_chains_from_the_edge_of_the_box_on_every_build(synth_sets, family, case):
    """The same builds with half of every ensemble started in a ball of 0.05 around a point at the edge of the prior box whose
    model fails: walkers at -inf, proposals outside the box (in a whole step: candidates behind such a proposal, which are not
    evaluated), failing models in the log."""
    ens_ds, nw, build = family_cases(synth_sets.n_simd)[family][case]
    n_slots = (nw // 2) * len(ens_ds)
    ref, start, _, _ = drive_posterior(synth_sets, ens_ds, nw, 2 if n_slots <= 100 else 1, seed=SEED + 7, table=FAMILY_TABLE[family],
                                       build=build, fails=True, outside=True)
    assert np.any(~np.isfinite(start)) and len(ref.bad) > 0


# ---- the KDE move
# Its proposal goes through sums over the other half, which the kernel takes in an order of its own, and through the device's
# sqrt, log, cos and sin.  On the posterior the restatement follows both (sampler_restated.run kde_device=: the workgroup's
# order of sums, the device's functions through libmp_probe_libm.so), so that the proposal is the kernel's bit for bit; with numpy's
# order and functions the chains differ by up to 8.9e-16 and their lnprob by up to 6.3e-13, with the same decisions.  Two
# tests per case: the first holds the device to mp_lnprob_batch at the positions the DEVICE stored and needs no restated
# proposal, so it tells a wrong evaluation from a wrong restatement; the second is the comparison of the other moves.
KDE_CASES = {"team-1": dict(handle="synth_sets", family="team-1", steps=3),
             "wave-4": dict(handle="synth_sets", family="wave-4", steps=1),
             "wave-2": dict(handle="synth_sets", family="wave-2", steps=1),
             "long": dict(handle="long_sets", ens_ds=[0, 1], nw=16, steps=2, seed=SEED + 2),
             "tempered": dict(handle="synth_sets", ens_ds=[2, 2, 0, 0], nw=16, steps=3, seed=SEED + 3, betas=LADDER),
             "long-wave-4": dict(handle="long_mixed_sets", long="wave-4", steps=1, seed=SEED + 24),
             "long-wave-2": dict(handle="long_mixed_sets", long="wave-2", steps=1, seed=SEED + 25)}
_KDE_RUNS = {}


def kde_run(request, case):
    """The KDE sampler of `case` and its restatement, run once for the two tests."""
    if case not in _KDE_RUNS:
        c = dict(KDE_CASES[case])
        h = request.getfixturevalue(c.pop("handle"))
        drive = drive_posterior
        if "family" in c:
            ens_ds, nw, build = family_cases(h.n_simd)["kde"][c.pop("family")]
        elif "long" in c:
            lc = long_cases(h.n_simd)[c.pop("long")]
            ens_ds, nw, build, drive = lc["ds"], lc["half"], lc["build"], drive_long
            assert nw - nw // 2 > 6                                           # (n_comp > ndim: a full-rank covariance)
        else:
            ens_ds, nw, build = c.pop("ens_ds"), c.pop("nw"), (4, 1, 1)
        ref, start, dev, evaluate = drive(h, ens_ds, nw, c.pop("steps"), table=KDE_TABLE, build=build, compare=False, **c)
        _KDE_RUNS[case] = ref, start, dev, evaluate, nw
    return _KDE_RUNS[case]


@pytest.mark.parametrize("case", list(KDE_CASES))
def test_kde_posterior_decisions_and_stored_lnprob_match_lnprob_batch(request, case):
    """What the KDE builds can be held to without a restated proposal: the start's lnprob equals the batch; every decision, n_accepted,
    n_bad and the swap counts equal the restatement's; and the chain's lnprob of every walker that has moved equals ONE
    mp_lnprob_batch call of the launch's class at the positions the DEVICE stored, on the walker's light curve (untempered
    cases: a swap moves a lnprob of the start's class along with its walker)."""
    ref, start, dev, evaluate, nw = kde_run(request, case)
    lnp0, chain, lnp, (dpos, dlnp, dacc), (n_bad, bad_rows), swaps = dev
    assert np.array_equal(lnp0, start)
    assert np.array_equal(dacc, ref.acc) and n_bad == len(ref.bad) == len(bad_rows)
    print(f"kde {case}: max |chain - restated| {np.abs(chain - ref.chain).max():.3e}, max |lnprob - restated| "
          f"{np.abs(lnp - ref.lnp).max():.3e}, rows that differ {int(np.any(chain != ref.chain, axis=2).sum())} of {lnp.size}")
    if swaps is not None:
        assert np.array_equal(swaps, ref.swaps)
        return
    cur, ens = lnp0.copy(), np.arange(len(lnp0)) // nw
    moved = ref.accepted                       # (the restatement's decisions; the device's are its changed rows)
    for s in range(len(chain)):
        if s:
            assert np.array_equal(np.any(chain[s] != chain[s - 1], axis=1), moved[s])
        half = len(cur) // 2                   # (at most n_slots rows a call, as a half-step launch)
        for part in (np.flatnonzero(moved[s])[:half], np.flatnonzero(moved[s])[half:]):
            if len(part):
                cur[part] = evaluate(chain[s][part], ens[part])[0]
        assert np.array_equal(lnp[s], cur), (s, np.flatnonzero(lnp[s] != cur)[:4])
    assert np.array_equal(dlnp, cur) and np.array_equal(dpos, chain[-1])


@pytest.mark.parametrize("case", list(KDE_CASES))
def test_kde_posterior_chains_match_the_restatement_bit_for_bit(request, case):
    """The comparison of the other moves: chain, lnprob, final state, failure log and swap counts equal the restatement in
    bits."""
    ref, start, dev, _, _ = kde_run(request, case)
    assert_device_equals(dev, ref, start)


@pytest.mark.parametrize("what", ["stretch", "tempered"])
def test_posterior_chains_match_lnprob_batch_on_the_long_builds(long_sets, what):
    """A handle that also holds a light curve of 112 points runs the LONG builds everywhere; the 50-point set comes first,
    so the half-step launches start the ensembles in another order than they are numbered (ens_order, asserted from the
    lengths).  16 slots, 2 steps: stretch by whole steps and a tempered stretch sampler by half-step launches (KDE: above)."""
    ens_ds, nw = ([0, 0, 1, 1], 8) if what == "tempered" else ([0, 1], 16)
    lens = [50 if d == 0 else 112 for d in ens_ds]
    order = sorted(range(len(ens_ds)), key=lambda e: -lens[e])        # (stable: mp_sampler.cpp stretch_args)
    assert order != list(range(len(ens_ds)))
    drive_posterior(long_sets, ens_ds, nw, 2, seed=SEED + 2, whole=what != "tempered", betas=LADDER if what == "tempered" else None, build=(4, 1, 1))


LONG_IDS = ([("step", c) for c in ("team-2", "wave-4", "wave-2")] + [("half", c) for c in ("team-1", "team-2", "wave-4", "wave-2")]
            + [("diff", c) for c in ("team-1", "wave-4", "wave-2")])


@pytest.mark.parametrize("form,case", LONG_IDS)
def test_posterior_chains_match_lnprob_batch_on_the_long_builds_of_every_class(long_mixed_sets, form, case):
    """The LONG builds beyond (4, 1, 1) on a handle that holds light curves of 50, 112, 410 and 1 944 points, the ensembles of
    long_cases: stretch_step_kernel by whole steps (step), the plain untempered stretch_kernel by half-step launches, which
    take the whole step's class (half: mp_sampler_set_whole_step(0)), and the DIFF builds under the DE + snooker table (diff;
    their two-per-SIMD team is unreachable through the launchers).  KDE: above; TEMPERED: below."""
    h = long_mixed_sets
    c = long_cases(h.n_simd)[case]
    ens_ds, nw = c["ds"], c["half" if form == "diff" else "whole"]
    seed = SEED + 10 + LONG_IDS.index((form, case))
    ref, start, _, _ = drive_long(h, ens_ds, nw, c["iters"], seed=seed, table=DIFF_TABLE if form == "diff" else None,
                                  whole=form == "step", build=c["build"])
    if (form, case) == ("half", "team-1"):   # a kernel that read another ensemble's light curve would start from these values
        pos = start_near_truths(ens_ds, nw, seed, truths=[TRUTHS["Humped"]] * len(ens_ds))
        n = len(pos)
        other = BatchEvaluator(h, [ens_ds[1], ens_ds[0]] + ens_ds[2:]).at(n)(pos, np.arange(n) // nw)[0]
        differ = np.any((other != start).reshape(len(ens_ds), nw), axis=1)
        assert differ.tolist() == [True, True] + [False] * (len(ens_ds) - 2)


def tempered_cases(ns):
    """The smallest shapes of the TEMPERED builds beyond the roomy team, two groups x ladder (1, 0.3): (walkers of each of the
    four ensembles, class).  The stretch move by half-step launches, which take the whole step's class; DE + snooker and KDE
    by their own size (no two-per-SIMD team; their roomy team is here for its LONG build)."""
    half = {"team-1": (16, (4, 1, 1)), "wave-4": (ns // 8, (1, 4, 1)), "wave-2": (5 * ns // 8, (1, 2, 2))}
    return {"stretch": {"team-2": (3 * ns // 64, (4, 1, 2)), "wave-4": (ns // 8, (1, 4, 1)), "wave-2": (3 * ns // 16, (1, 2, 2))},
            "diff": half, "kde": half}


TEMPERED_IDS = [(f, c) for f in ("stretch", "diff", "kde") for c in ("team-1", "team-2", "wave-4", "wave-2")
                if c in tempered_cases(1024)[f]]


@pytest.mark.parametrize("handle", ["synth_sets", "long_mixed_sets"])
@pytest.mark.parametrize("family,case", TEMPERED_IDS)
def test_tempered_posterior_chains_match_lnprob_batch_beyond_the_roomy_team(request, family, case, handle):
    """TEMPERED on the classes beyond (4, 1, 1), for the stretch move by half-step launches, DE + snooker and KDE (those two
    on (4, 1, 1) as well, which no other tempered DE case and no other tempered LONG KDE case runs), on the four 50-point sets
    and on the handle with the long ones (both ensembles of the second group on the case's long set: TEMPERED LONG); two
    steps with their swap sweeps, one on the largest launches; a swap was accepted and one refused."""
    h = request.getfixturevalue(handle)
    nw, build = tempered_cases(h.n_simd)[family][case]
    long = handle == "long_mixed_sets"
    ds = long_cases(h.n_simd)[case]["ds"]
    seed = SEED + 30 + 2 * TEMPERED_IDS.index((family, case)) + long
    (drive_long if long else drive_posterior)(h, [ds[0], ds[0], ds[1], ds[1]] if long else [2, 2, 0, 0], nw, 1 if case == "wave-2" else 2,
                                              seed=seed, table=FAMILY_TABLE[family], whole=False, betas=LADDER, build=build)


def test_whole_step_launch_equals_half_step_launches_on_the_long_builds(long_mixed_sets):
    """The contract of the test at the class boundaries below on the LONG builds: 3 n_simd / 8 slots, one ensemble on Humped
    and one on 1 944 points, one step by one launch and by two half-step launches gives one chain."""
    _whole_step_equals_half_steps(long_mixed_sets, [0, 3], (3, 8), False, [TRUTHS["Humped"]] * 2)


@pytest.mark.parametrize("whole", [True, False])
def test_tempered_posterior_chains_match_lnprob_batch(synth_sets, whole):
    """Two groups x ladder (1, 0.3), 16 walkers each, both ensembles of a group on one light curve: the TEMPERED builds and the
    swap sweep on real, untempered lnprob, 4 steps of the stretch move by whole steps and by half-step launches (KDE: above);
    the swap counts are compared, a swap was accepted and one refused."""
    drive_posterior(synth_sets, [2, 2, 0, 0], 16, 4, seed=SEED + 3, whole=whole, betas=LADDER, build=(4, 1, 1))


@pytest.mark.parametrize("what", ["stretch", "de"])
def test_failed_models_reach_the_log_and_lost_walkers_escape(synth_sets, what):
    """The team shape with half of every ensemble started around a point whose model fails, 3 steps: walkers start at -inf,
    proposals fail and are counted and logged as the restatement lists them, and a walker that started at -inf ends finite."""
    ref, start, _, _ = drive_posterior(synth_sets, [2, 0, 1], 16, 3, seed=SEED + 4, table=DE_TABLE if what == "de" else None,
                                       build=(4, 1, 1), fails=True, outside=True)
    assert np.any(~np.isfinite(start)) and len(ref.bad) > 0
    assert np.any(~np.isfinite(start) & np.isfinite(ref.lnp[-1]))


@pytest.mark.parametrize("autocorr", [0, 64])
def test_runs_of_one_step_equal_one_run(synth_sets, autocorr):
    """mp_sampler_run(1) x 4 equals mp_sampler_run(4) and the restatement; likewise with the autocorrelation monitor on,
    whose chunk cap differs."""
    ens_ds, nw = [2, 0, 1], 16
    _, _, one, _ = drive_posterior(synth_sets, ens_ds, nw, 4, seed=SEED + 5, build=(4, 1, 1), autocorr=autocorr)
    _, _, many, _ = drive_posterior(synth_sets, ens_ds, nw, 4, seed=SEED + 5, build=(4, 1, 1), autocorr=autocorr, runs=(1,) * 4)
    assert np.array_equal(one[1], many[1]) and np.array_equal(one[2], many[2])


# ---------------------------------------------------------------- one chain from one launch per step and from two
@pytest.mark.parametrize("fails", [False, True])
@pytest.mark.parametrize("frac", [(3, 8), (3, 32), (1, 4)])
def test_whole_step_launch_equals_half_step_launches_at_the_class_boundaries(synth_sets, frac, fails):
    """n_slots = 3 ns / 8 (a whole-step launch of 2 steps per lane where a half-step launch of its own size would run 4) and
    3 ns / 32 (a team two wavefronts per SIMD against one per SIMD): one step of the stretch move by one launch and by two
    half-step launches (mp_sampler_set_whole_step(0)) gives one chain, lnprob, n_accepted and failure log, bit for bit --
    the half-step launches of a sampler whose whole step fits take the whole step's variant.  (While they chose by their own
    size, 557 of the 768 stored lnprob differed after the step at 3 ns / 8 from the starts near the truths; at 3 ns / 32 the
    two team builds gave the same bits.)  ns / 4, where both sizes choose 4 steps per lane, is the control; fails: half of
    every ensemble starts at the edge of the prior box around a point whose model fails, so that the log has rows."""
    _whole_step_equals_half_steps(synth_sets, [1, 2], frac, fails)


def _whole_step_equals_half_steps(h, ens_ds, frac, fails, truths=None):
    ns = h.n_simd
    n_slots = frac[0] * ns // frac[1]
    nw = n_slots
    assert whole_step_fits(n_slots, ns)
    assert (stretch_class(3 * n_slots, n_slots, ns) != stretch_class(n_slots, n_slots, ns)) == (frac != (1, 4))
    pos = start_near_truths(ens_ds, nw, SEED + 6, fails, truths)
    a = device_run(h, ens_ds, nw, pos, (1,), SEED + 6, whole=True)
    b = device_run(h, ens_ds, nw, pos, (1,), SEED + 6, whole=False)
    differ = np.flatnonzero(a[2][0] != b[2][0])
    print(f"{n_slots} slots: whole {stretch_class(3 * n_slots, n_slots, ns)}, half-steps by their own size "
          f"{stretch_class(n_slots, n_slots, ns)}: {len(differ)} of {2 * nw} chain lnprob differ, accepted {int(a[3][2].sum())} / "
          f"{int(b[3][2].sum())}")
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), differ[:8]
    assert np.array_equal(a[3][2], b[3][2]) and 0 < a[3][2].sum() < 2 * nw
    assert a[4][0] == b[4][0] and sorted(map(tuple, a[4][1])) == sorted(map(tuple, b[4][1]))
    assert a[4][0] > 0 or not fails
