#!/usr/bin/env python3
"""Record tests/golden/golden_slice_move.npz and golden_nest_slice.npz: one run each of the restated ensemble slice move and
of the restated nested slice mode (the cases of tests/test_slice_golden_cpu.py, which holds the restatements to them bit for
bit).  The committed fixtures were recorded at the commit before the two restatements were put on tests/walk_restated.py; to
record them again is to declare the restatements of that day the new baseline.

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_slice_golden.py

MANIFEST.json is make_golden.py's and is left alone.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]   # tests/ and the repository root

import test_slice_golden_cpu as cases  # noqa: E402


def main():
    for path, run in ((cases.MOVE_FIXTURE, cases.move_run), (cases.NEST_FIXTURE, cases.nest_run)):
        out = run()
        np.savez_compressed(path, **out)
        print("wrote", os.path.basename(path), {k: np.asarray(v).shape for k, v in out.items()})


if __name__ == "__main__":
    main()
