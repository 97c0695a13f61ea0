"""CPU test of the LONG case table (tests/test_gpu_nested.py long_cases): on devices of 1 024, 416 and 1 216 SIMDs every named
case lands in the kernel build it names under the restated launch rules (launch_class, stretch_class), inside every driver's
size limits, on light curves of the lengths claimed; and the batches of the reference evaluator that mp_lnprob_batch evaluates
longest light curve first (launch_lnprob_ordered: a handle with a long and a short set, more than 2 n_simd rows) are recorded."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from test_gpu_nested import LONG_MIXED_LENGTHS, launch_class, long_cases
from test_gpu_sampler_posterior import eval_rows, run_blocks, stretch_class, tempered_cases, whole_step_fits

SIMDS = (1024, 416, 1216)
CLASSES = {"team-1": (4, 1, 1), "team-2": (4, 1, 2), "wave-4": (1, 4, 1), "wave-2": (1, 2, 2)}
DIFF, KDE = [("diff",)], [("kde",)]          # run_blocks only asks whether there is a move table

# include/magprop_amd.h
NEST_MIN_LIVE, NEST_MAX_LIVE, NEST_MAX_RUNS = 16, 4096, 64
SMC_MIN_PARTICLES, SMC_MAX_PARTICLES = 4, 16384
OPT_MIN_POP, OPT_MAX_POP = 5, 1024
MAX_SIMPLEXES = 1024


def test_header_limits_are_the_ones_restated_here():
    from magprop_amd import _capi
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "magprop_amd.h")).read()
    for name, value in (("MP_NEST_MIN_LIVE", NEST_MIN_LIVE), ("MP_NEST_MAX_LIVE", NEST_MAX_LIVE),
                        ("MP_SMC_MIN_PARTICLES", SMC_MIN_PARTICLES), ("MP_SMC_MAX_PARTICLES", SMC_MAX_PARTICLES)):
        assert f"#define {name} {value}\n" in header, name
    assert _capi.MAX_DATASETS >= len(LONG_MIXED_LENGTHS)


def test_the_sets_have_the_lengths_claimed():
    synth, longlc = np.load(GOLDEN + "/golden_synth.npz"), np.load(GOLDEN + "/golden_longlc.npz")
    lengths = (len(synth["Humped_x"]),) + tuple(longlc[f"synth{n}_ds"].shape[1] for n in LONG_MIXED_LENGTHS[1:])
    assert lengths == LONG_MIXED_LENGTHS == (50, 112, 410, 1944)
    assert all(longlc[f"synth{n}_ds"].shape[0] == 3 for n in LONG_MIXED_LENGTHS[1:])


@pytest.mark.parametrize("ns", SIMDS)
def test_every_case_mixes_a_short_and_a_long_set_in_an_order_that_is_not_descending(ns):
    cases = long_cases(ns)
    assert list(cases) == list(CLASSES)
    seen = set()
    for name, c in cases.items():
        lens = [LONG_MIXED_LENGTHS[d] for d in c["ds"]]
        assert c["build"] == CLASSES[name] and len(set(c["ds"])) == len(c["ds"]) >= 2
        assert min(lens) <= 64 < max(lens), name
        assert sorted(range(len(lens)), key=lambda e: -lens[e]) != list(range(len(lens))), name      # ens_order is not the identity
        assert 1 <= c["iters"] <= (3 if c["build"][0] == 1 else 8)
        seen.update(c["ds"])
    assert seen == {0, 1, 2, 3}


def ordered(n, ns):
    """Whether mp_lnprob_batch of n rows on long_mixed_sets takes the ordered path (mp_capi.cpp launch_lnprob_ordered)."""
    return n > 2 * ns


@pytest.mark.parametrize("ns", SIMDS)
def test_every_case_lands_in_its_class_inside_the_drivers_limits(ns):
    took_the_ordered_path = set()

    def batch(what, name, n):
        if ordered(n, ns):
            took_the_ordered_path.add((what, name))

    for name, c in long_cases(ns).items():
        build, n_runs = c["build"], len(c["ds"])
        # nested sampler, random walk and slices: walk launches of n_runs nbatch workgroups, nlive = 2 nbatch
        nbatch, nlive = c["nbatch"], 2 * c["nbatch"]
        assert launch_class(n_runs * nbatch, ns) == build, name
        assert NEST_MIN_LIVE <= nlive <= NEST_MAX_LIVE and 1 <= nbatch <= nlive // 2 and n_runs <= NEST_MAX_RUNS
        batch("nested walk", name, n_runs * nbatch)
        batch("nested live set", name, n_runs * nlive)
        # the ensemble slice move: nbatch slots per ensemble and launch
        assert nbatch >= 2
        # SMC: move launches of n_runs n workgroups
        assert launch_class(n_runs * c["n"], ns) == build and SMC_MIN_PARTICLES <= c["n"] <= SMC_MAX_PARTICLES
        batch("smc", name, n_runs * c["n"])
        # the optimizer: one workgroup per member
        popsize = c["pop"] // n_runs
        assert launch_class(n_runs * popsize, ns) == build and OPT_MIN_POP <= popsize <= OPT_MAX_POP
        batch("optimizer", name, n_runs * popsize)
        # the simplex search: ndim + 4 = 10 candidates per simplex
        assert launch_class(10 * c["n_simplex"], ns) == build and n_runs <= c["n_simplex"] <= MAX_SIMPLEXES
        batch("simplex", name, 10 * c["n_simplex"])
        # the ensemble sampler by whole steps and by the half-step launches of such a sampler
        nw = c["whole"]
        n_slots = (nw // 2) * n_runs
        assert whole_step_fits(n_slots, ns)
        for whole in (True, False):
            launched, choosing = run_blocks(n_slots, ns, None, whole)
            assert launched == (3 * n_slots if whole else n_slots) and choosing == 3 * n_slots
            assert stretch_class(choosing, n_slots, ns) == build, (name, whole)
        batch("sampler start, whole", name, n_runs * nw)
        batch("sampler step, whole", name, eval_rows(build, n_slots, ns))
        # DE + snooker and KDE: half-step launches judged by their own size
        if c["half"] is None:
            assert build == (4, 1, 2)                   # (unreachable through the launchers: DESIGN.md section 8)
        else:
            nw = c["half"]
            n_slots = (nw // 2) * n_runs
            for table in (DIFF, KDE):
                assert run_blocks(n_slots, ns, table, True) == (n_slots, n_slots)
            assert stretch_class(n_slots, n_slots, ns) == build, name
            assert nw // 2 >= 3 and nw - nw // 2 > 6    # snooker's three partners; KDE: n_comp > ndim
            batch("sampler start, half", name, n_runs * nw)
            batch("sampler step, half", name, eval_rows(build, n_slots, ns))
        # tempered, two groups x two temperatures: the stretch move by half-step launches of a sampler whose whole step fits,
        # DE + snooker and KDE by their own size
        for family, table in (("stretch", None), ("diff", DIFF), ("kde", KDE)):
            if name in tempered_cases(ns)[family]:
                nw, cls = tempered_cases(ns)[family][name]
                n_slots = (nw // 2) * 4
                launched, choosing = run_blocks(n_slots, ns, table, False)
                assert cls == build and launched == n_slots and choosing == (n_slots if table else 3 * n_slots)
                assert stretch_class(choosing, n_slots, ns) == build, (family, name)
                assert nw // 2 >= 3 and nw - nw // 2 > 6
                batch("sampler start, tempered " + family, name, 4 * nw)
    # whole step against half-steps at 3 ns / 8 slots on the long handle
    assert whole_step_fits(3 * ns // 8, ns)
    # the batches the restatement hands mp_lnprob_batch with more than 2 ns rows: evaluated longest light curve first, which
    # does not change a row's bits (tests/test_gpu_batched.py::test_longest_light_curves_first_launch_order and
    # tests/test_gpu_parity.py::test_batch_size_does_not_change_a_walker)
    assert took_the_ordered_path == {("nested live set", "wave-2"), ("sampler start, half", "wave-2"), ("sampler start, tempered diff", "wave-2"),
                                     ("sampler start, tempered kde", "wave-2")}
