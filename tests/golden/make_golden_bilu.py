"""Writes tests/golden/bilu_bits.npz: the block ILU(k) factor (pattern, L, U, inverted diagonal blocks) and M^-1 b of the cases
tests/test_bilu_cpu.py names in GOLDEN_CASES, as the reference library computes them at one thread (a child process: bilu_cases).
Run from the repository root with oracle/_ref built:  python tests/golden/make_golden_bilu.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import bilu_cases  # noqa: E402
import test_bilu_cpu  # noqa: E402

jobs = [dict(kind="factor", name=name, bn=bn, fill=fill) for name, bn, fill in test_bilu_cpu.GOLDEN_CASES]
got = bilu_cases.reference_jobs(jobs)
entries = test_bilu_cpu.golden_entries({case: (f, f["psolve"]) for case, f in zip(test_bilu_cpu.GOLDEN_CASES, got)})
np.savez_compressed(test_bilu_cpu.GOLDEN, **entries)
print("wrote", test_bilu_cpu.GOLDEN, os.path.getsize(test_bilu_cpu.GOLDEN), "bytes")
