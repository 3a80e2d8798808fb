"""The block sweeps of -p ssor on BSR storage (kernels/bsptrsv.hip on kernels/level_schedule.hpp) driven through liship_bsweep_f64 with
hand-built liship_sweep_t layouts over block rows, and held to tests/bssor_oracle.py in every bit (a NaN matches any NaN: sign and payload
are not part of the contract).  Each case first proves, from the struct it built, that it has the launches it is for.

  chunks(bn)   every bn = 1 .. 8: a first level of 600 block rows, a small level (one run with the first) whose rows hold 0, 1, 63, 64, 65,
               chunk, chunk + 1 and 2 chunk + 1 terms (chunk: the terms of a long block row in LDS at once, per bn), a level of 1100 block rows
               on a launch of its own with the same long rows among short ones, and a small level of long rows only
  sizes        levels of 1, 255, 256, 257, 1023, 1024 and 1025 block rows (runs, and one level on its own launch with 4 full short-row
               workgroups and one thread more), long rows in both
  groupings    every valid way to cut five levels into launches, on the same layout
  special      +-0.0, +-inf, denormals and 1e+-300 in the blocks and in b, -0.0 in WD, on both sides of the "+0.0 start from bn = 4" rule
Every case runs the four forms (plain MUL and SUB, transposed MUL and SCAT), forward and backward, b apart from x and b as x; block
sizes, residues n mod bn and directions are spread over the cases to keep each one to a few seconds."""
import ctypes as C

import numpy as np
import pytest

import bssor_cases as cases
import lis_amd
import ssor_cases

pytestmark = pytest.mark.gpu
MUL, SUB, SCAT = 0, 1, 2
FORMS = ((MUL, 0), (SUB, 0), (MUL, 1), (SCAT, 1))


@pytest.fixture(scope="module")
def lib():
    lib = lis_amd.load()
    assert lis_amd.gpu_available(), "no HIP device: the product path has no CPU fallback"
    assert lib.initialize([]) == 0
    return lib


def check_forms(lib, case, lay, tag, b=None, forms=FORMS, want=None):
    """the four forms on one layout against the model; returns the model's results for reuse on another grouping of the same layout"""
    n = case["n"]
    rng = np.random.default_rng(17)
    if b is None:
        b = rng.uniform(-1.0, 1.0, n)
    x_before = rng.uniform(-1.0, 1.0, n)
    want = {} if want is None else want
    for mode, tr in forms:
        if (mode, tr) not in want:
            want[mode, tr] = cases.model_sweep(case, mode, tr, None if (mode == SUB and not tr) else b, x_before if (mode == SUB and not tr) else b)
        wx, wwork = want[mode, tr]
        if mode == SUB and not tr:
            runs = [(None, x_before, False)]
        else:
            runs = [(b, np.full(n, 7.0), False), (b, b, True)]
        for bb, x0, alias in runs:
            x, work = cases.kernel_sweep(lib, case, lay, mode, tr, bb, x0, alias)
            d = ssor_cases.first_difference(x, wx, nan_payload=False)
            assert d is None, (tag, mode, tr, alias) + d
            if mode == SCAT and case["bn"] > 1:                              # (bn = 1 runs the point sweep, which forms x[j] * wd[j] per term and has no work vector)
                d = ssor_cases.first_difference(work, wwork, nan_payload=False)
                assert d is None, (tag, "work", alias) + d
    return want


def chunk_levels(bn):
    ch = cases.CHUNK[bn]
    edge = [0, 1, 63, 64, 65, ch, ch + 1, 2 * ch + 1]
    long_edge = sorted({64, 65, ch, ch + 1, 2 * ch + 1})                  # (from bn = 6 on a chunk is 32 terms: rows of 32 and 33 are one lane's, 64 is two chunks)
    return [ssor_cases.level(600, first=True),
            [c for c in edge if c > 0] + [1, 2, 3],                      # (a row of 0 terms belongs to the first level)
            ssor_cases.level(1100, long_edge),
            [c for c in long_edge if c >= 64]]


@pytest.mark.parametrize("bn", range(1, 9))
def test_chunk_edges_in_runs_and_in_own_launch_levels(lib, bn):
    assert lib.dll.liship_bsweep_chunk(bn) == cases.CHUNK[bn]
    pad = 0 if bn % 2 == 0 else bn - 1
    desc = bn % 3 == 0
    case = cases.sweep_case(chunk_levels(bn), bn, pad, 100 + bn, desc=desc)
    lay = cases.layout(case)
    ch = cases.CHUNK[bn]
    counts = sorted(len(r) for r in case["gather"])
    assert {0, 1, 63, 64, 65, ch, ch + 1, 2 * ch + 1} <= set(counts)
    nlong_small = sum(c >= 64 for c in chunk_levels(bn)[1])
    nlong_big = sum(c >= 64 for c in chunk_levels(bn)[2])
    nlong_only = len(chunk_levels(bn)[3])
    assert lay["sizes"] == [600, len(chunk_levels(bn)[1]), 1100, nlong_only] and lay["nlong"] == [0, nlong_small, nlong_big, nlong_only]
    assert [tuple(g) for g in lay["groups"]] == [(0, 2, 1), (2, 3, 0), (3, 4, 1)]
    assert cases.census(lay) == [4, 3, 1, nlong_big, nlong_small + nlong_only]          # long rows in a run, in an own-launch level, and a level of long rows only
    assert lay["nshort"][3] == 0 and (case["n"] % bn == 0) == (pad == 0)
    check_forms(lib, case, lay, ("chunks", bn))


@pytest.mark.parametrize("bn,pad,desc", [(2, 1, False), (3, 0, True), (5, 0, False), (8, 3, True)])
def test_level_sizes_across_the_run_and_workgroup_borders(lib, bn, pad, desc):
    sizes = [1, 255, 256, 257, 1023, 1024, 1025]
    levels = ssor_cases._sizes(sizes, {3: (63, 64, 65), 6: (64, 65, 70)})
    case = cases.sweep_case(levels, bn, pad, 200 + bn, desc=desc)
    lay = cases.layout(case)
    assert lay["sizes"] == sizes and [tuple(g) for g in lay["groups"]] == [(0, 6, 1), (6, 7, 0)]
    assert cases.census(lay) == [7, 2, 1, 3, 2] and lay["nshort"][6] == 1022
    check_forms(lib, case, lay, ("sizes", bn))


def test_every_valid_grouping_of_levels_into_launches(lib):
    """the same layout under each of the 26 ways to launch its five levels (the level of 1100 block rows always on its own): one
    model result per form, every grouping must give it"""
    bn, sizes = 3, [3, 1100, 4, 2, 5]
    levels = ssor_cases._sizes(sizes, {1: (1, 2), 2: (64, 3), 4: (65,)})
    case = cases.sweep_case(levels, bn, 1, 300)
    groupings = cases.valid_groupings(sizes)
    assert len(groupings) == 26 and all((1, 2, 0) in g for g in groupings)
    want = None
    for g in groupings:
        lay = cases.layout(case, g)
        assert lay["sizes"] == sizes and cases.census(lay)[1] == len(g)
        want = check_forms(lib, case, lay, ("groupings", g), want=want)


@pytest.mark.parametrize("bn,pad", [(2, 0), (3, 2), (4, 1), (7, 0)])
def test_special_values(lib, bn, pad):
    levels = ssor_cases._sizes([300, 200, 100, 40], {1: (64,), 3: (70,)})
    case = cases.sweep_case(levels, bn, pad, 400 + bn, special=True)
    lay = cases.layout(case)
    n = case["n"]
    blocks = lay["val"]
    assert np.isposinf(blocks).any() and np.isneginf(blocks).any() and (blocks == 0).any() and (np.abs(blocks) > 1e290).any()      # inf * 0 and inf - inf are reached inside the terms
    assert any(len(row) >= 64 and any(np.isinf(blk).any() for _, blk in row) for row in case["gather"])                          # ... and in a long row's LDS
    rng = np.random.default_rng(5)
    b = rng.uniform(-1.0, 1.0, n)
    for value, at in ((np.inf, 7), (-np.inf, 311), (-0.0, 12), (0.0, 13), (5e-324, 50), (-2.5e-310, 51), (1e300, 90), (1e-300, 91), (-1e300, 400)):
        b[at::97] = value
    want = check_forms(lib, case, lay, ("special", bn), b=b)
    for (mode, tr), (x, _) in want.items():
        assert np.isfinite(x).sum() * 2 >= n or mode == SUB, ("the poison took everything", mode, tr)
        assert not np.isfinite(x).all() or mode == SUB, ("no special value reached a result", mode, tr)


@pytest.mark.parametrize("bn", range(1, 9))
def test_small_layouts_with_every_residue(lib, bn):
    """three small levels in one run, n = nr*bn - pad for every pad: the padding of the last block is read as +0.0 and never written"""
    for pad in range(bn):
        case = cases.sweep_case([[0, 0, 0], [1, 2], [3]], bn, pad, 500 + 10 * bn + pad, desc=bool(pad % 2))
        lay = cases.layout(case)
        assert cases.census(lay) == [3, 1, 0, 0, 0]
        check_forms(lib, case, lay, ("small", bn, pad))


def test_kernel_arguments(lib):
    """a bad mode for the direction, a block size outside 1 .. 8, a layout of another size, NULL vectors: LISHIP_ERR_ARG, no launch; n = 0: nothing to do"""
    fn = lib.dll.liship_bsweep_f64
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(cases.SweepT), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    empty = cases.SweepT()
    for bn in range(1, 9):
        assert fn(C.byref(empty), 0, bn, MUL, 0, None, None, None, None, None) == 0
        assert fn(C.byref(empty), 1, bn, MUL, 0, None, None, None, None, None) == -1          # a layout of 0 block rows for n = 1
    one = cases.SweepT()
    one.nrows = 1
    for bn, mode, tr in ((0, MUL, 0), (9, MUL, 0), (2, SCAT, 0), (2, SUB, 1), (2, 3, 0), (2, -1, 1)):
        assert fn(C.byref(one), min(max(bn, 1), 8), bn, mode, tr, None, None, None, None, None) == -1, (bn, mode, tr)
    assert fn(C.byref(one), 2, 2, MUL, 0, None, None, None, None, None) == -1                 # valid shape, NULL vectors
    assert fn(None, 2, 2, MUL, 0, None, None, None, None, None) == -1
