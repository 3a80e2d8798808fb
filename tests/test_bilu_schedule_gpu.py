"""The launch edges of the block ILU (kernels/ilu.hip on kernels/level_schedule.hpp), on BSR matrices built to order: each case first
proves through lis_amd_ilu_factor_info / lis_amd_ilu_info that it got the launches it is for -- the levels and launches the library
reports equal the ones computed here from the model's pattern with the schedule rules restated in tests/ssor_cases.py -- and then
holds factor and psolve (b apart from x, and b aliased with x) to tests/bilu_oracle.py in every bit.

  arrow(k)   block row 0 dense in U (k blocks), the last block row dense in L (k blocks), k rows between them that read row 0 and are
             read by the last: forward levels of 1, k, 1 block rows.  k = 64, 65: the first long rows (LISHIP_SWEEP_LONG_ROW = 64), in
             one run.  k = 300: a long row inside a run, one chunk of the 1024-thread workgroup.  k = 1100: the middle level has a
             launch of its own (several short-row workgroups), the dense rows sit in runs and take two chunks.
  levels     1500 independent block rows, then 1100 that read them; one of these reads 300 (a long row of L in a big level, two chunks
             of its 256-thread workgroup) and one of the 1500 is read by 300 (the same for U).
  twice      arrow(70) whose dense rows store a block column twice: `serial`, long rows by one thread.
Sizes are the smallest that reach each path; block sizes are spread over the cases to keep each one to a few seconds."""
import ctypes as C

import numpy as np
import pytest

import bilu_cases
import bilu_oracle
import lis_amd
import ssor_cases
from lis_amd import _capi as capi
from test_bilu_gpu import blocks, check_against_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    lib = lis_amd.load()
    assert lis_amd.gpu_available(), "no HIP device: the product path has no CPU fallback"
    assert lib.initialize([]) == 0
    lib.dll.lis_amd_set_residency(0)
    return lib


def block_matrix(rows, bn, pad, seed):
    """BSR arrays of the block pattern rows[i] (block columns in stored order, the diagonal among them): off-diagonal blocks small against
    the diagonal blocks (3 I + a perturbation), so every factor stays finite; n = nr*bn - pad, zero beyond n"""
    rng = np.random.default_rng(seed)
    nr, bs = len(rows), bn * bn
    n = nr * bn - pad
    bptr, bindex, value = [0], [], []
    for i, cols in enumerate(rows):
        for c in cols:
            if c == i:
                blk = rng.uniform(-0.2, 0.2, bs)
                blk[::bn + 1] += 3.0
            else:
                blk = rng.uniform(-1.0, 1.0, bs) / (bn * len(cols))
            for r in range(bn):
                for q in range(bn):
                    if i * bn + r >= n or c * bn + q >= n:
                        blk[r + q * bn] = 0.0
            bindex.append(c)
            value += blk.tolist()
        bptr.append(len(bindex))
    return np.array(bptr, np.int32), np.array(bindex, np.int32), np.array(value, np.float64), bn, n


def shuffled(rows, seed):
    rng = np.random.default_rng(seed)
    return [rng.permutation(r).tolist() for r in rows]


def arrow(k, twice=False):
    rows = [[0] + list(range(1, k + 1))] + [[0, j, k + 1] for j in range(1, k + 1)] + [list(range(1, k + 2))]
    if twice:
        rows[0].append(5)
        rows[-1].append(3)
    return shuffled(rows, k)


def levels():
    rows = [[i] for i in range(1500)] + [[q, 1500 + q] for q in range(1100)]
    for q in range(1100):
        rows[q].append(1500 + q)
    for c in range(300):                  # block row 1500 reads 300 of the first level
        if c not in rows[1500]:
            rows[1500].append(c)
            rows[c].append(1500)
    for q in range(700, 1000):            # block row 5 is read by 300 of the second
        if 5 not in rows[1500 + q]:
            rows[1500 + q].append(5)
            rows[5].append(1500 + q)
    return shuffled(rows, 7)


def expected_schedule(f, serial):
    """what lis_amd_ilu_factor_info and lis_amd_ilu_info must report, from the model's pattern: the forward levels of L; a block row is
    given to a workgroup when it holds LONG_ROW block terms or more in L and U together"""
    (lp, lc, _), (up, uc, _) = f["L"], f["U"]
    nr = len(lp) - 1
    L = [[(int(c), 0.0) for c in lc[lp[i]:lp[i + 1]]] for i in range(nr)]
    U = [[(int(c), 0.0) for c in uc[up[i]:up[i + 1]]] for i in range(nr)]
    lev = ssor_cases.levels_of(L, 0)
    nlev = max(lev) + 1 if nr else 0
    sizes, nlong = [0] * nlev, [0] * nlev
    for i, l in enumerate(lev):
        sizes[l] += 1
        nlong[l] += (len(L[i]) + len(U[i])) >= ssor_cases.LONG_ROW
    groups = ssor_cases.grouping(sizes)
    own = [g[0] for g in groups if not g[2]]
    factor_info = [nlev, len(groups), len(own), sum(nlong[l] for l in own), sum(nlong) - sum(nlong[l] for l in own), int(serial)]
    fwd, bwd = ssor_cases.sweep_stats(L, 0), ssor_cases.sweep_stats(U, 1)
    return factor_info, fwd, bwd


def run_case(lib, bsr, fill, T, tag):
    """the library's schedule of the case, after its factor and psolve were held to the model"""
    n = bsr[4]
    want = bilu_oracle.factor(*bsr, fill, T)
    b = np.random.default_rng(5).uniform(-1.0, 1.0, n)
    wx = bilu_oracle.psolve(want, b, T)
    assert np.isfinite(want["D"]).all() and np.isfinite(wx).all()
    check_against_model(lib, bsr, fill, T, want, wx, b, tag)
    rows = [bsr[1][bsr[0][i]:bsr[0][i + 1]].tolist() for i in range(len(bsr[0]) - 1)]
    dup = any(len(set(r)) != len(r) for r in rows)
    finfo, fwd, bwd = expected_schedule(want, dup)
    with blocks(lib, T):
        A = bilu_cases.make_bsr(lib, bsr)
        fi, info = (C.c_int * 6)(), (C.c_double * 6)()
        assert lib.dll.lis_amd_ilu_factor_info(A, fill, fi) == 0 and lib.dll.lis_amd_ilu_info(A, fill, info) == 0
        lib.lis_matrix_destroy(A)
    print("BILU SCHEDULE %s factor=%s psolve launches=%d blocks=%d" % (tag, list(fi), int(info[4]), int(info[1])))
    assert list(fi) == finfo, (tag, list(fi), finfo)
    assert int(info[1]) == int(want["L"][0][-1] + want["U"][0][-1]) and int(info[2]) == finfo[0]
    assert int(info[4]) == fwd["info"][1] + bwd["info"][1] and int(info[3]) == fi[1] + (want["L"][0][-1] > 0) + (want["U"][0][-1] > 0)
    return finfo, fwd, bwd


@pytest.mark.parametrize("k,bn,pad,fill,T", [(64, 1, 0, 0, 1), (64, 2, 1, 0, 1), (64, 3, 2, 1, 1), (65, 2, 0, 1, 1), (65, 3, 1, 0, 1), (65, 3, 1, 0, 3), (300, 2, 1, 0, 1)])
def test_first_long_rows_in_one_run(lib, k, bn, pad, fill, T):
    """block rows of k terms in L (the last block row) and in U (the first), everything in ONE launch; T = 3 cuts the arrow in three"""
    bsr = block_matrix(arrow(k), bn, pad, 10 * k + bn)
    finfo, fwd, bwd = run_case(lib, bsr, fill, T, ("arrow", k, bn, pad, fill, T))
    if T == 1:
        assert finfo[1] == 1 and finfo[2] == 0 and finfo[4] >= 2            # a schedule that is one run only, its long rows inside
        assert fwd["longest"] >= k and bwd["longest"] >= k and fwd["info"][1] == 1 and bwd["info"][1] == 1
        assert fwd["info"][4] >= 1 and bwd["info"][4] >= 1                  # a long row inside a run, in both sweeps


def test_dense_rows_of_1100_blocks_around_a_big_level(lib):
    bsr = block_matrix(arrow(1100), 3, 2, 1100)
    finfo, fwd, bwd = run_case(lib, bsr, 0, 1, ("arrow", 1100))
    assert finfo[:3] == [3, 3, 1]                                           # run, the level of 1100 block rows on its own launch, run
    assert fwd["sizes"] == [1, 1100, 1] and fwd["longest"] == 1100 and fwd["info"][4] == 1       # the dense row of L: in a run, two chunks of 1024
    assert bwd["sizes"] == [1, 1100, 1] and bwd["longest"] == 1100 and bwd["info"][4] == 1       # the dense row of U likewise


def test_long_rows_of_300_blocks_inside_big_levels(lib):
    bsr = block_matrix(levels(), 2, 1, 300)
    finfo, fwd, bwd = run_case(lib, bsr, 0, 1, ("levels",))
    assert finfo[:3] == [2, 2, 2] and finfo[3] >= 2                         # 1500 independent block rows, then 1100 that depend on them: two launches of their own
    assert fwd["sizes"] == [1500, 1100] and fwd["longest"] >= 300 and fwd["info"][3] == 1        # the 300-term row of L in the big level: two chunks of 256
    assert bwd["info"][2] >= 1 and bwd["longest"] >= 300 and bwd["info"][3] == 1 and max(bwd["sizes"]) > ssor_cases.SMALL_LEVEL


def test_independent_rows_then_dependents_in_a_run(lib):
    """1500 independent block rows (a launch of their own, six short-row workgroups), then 30 block rows that read them (a run)"""
    rng = np.random.default_rng(3)
    rows = [[i] for i in range(1500)]
    for q in range(30):
        cols = rng.choice(1500, 3, replace=False).tolist()
        rows.append(cols + [1500 + q])
        for c in cols:
            rows[c].append(1500 + q)
    bsr = block_matrix(shuffled(rows, 4), 3, 1, 1500)
    finfo, fwd, bwd = run_case(lib, bsr, 0, 1, ("independent",))
    assert finfo[:5] == [2, 2, 1, 0, 0] and fwd["sizes"] == [1500, 30]


def test_serial_matrix_with_long_rows(lib):
    bsr = block_matrix(arrow(70, twice=True), 2, 1, 70)
    finfo, fwd, bwd = run_case(lib, bsr, 0, 1, ("twice",))
    assert finfo[5] == 1 and finfo[3] + finfo[4] >= 2


def test_one_padded_block(lib):
    """n = 1 with bn = 3: one block, two rows of padding"""
    bsr = (np.array([0, 1], np.int32), np.array([0], np.int32), np.array([4.0, 0, 0, 0, 0, 0, 0, 0, 0]), 3, 1)
    want = bilu_oracle.factor(*bsr, 0, 1)
    assert want["D"].tolist() == [0.25, 0, 0, 0, 1, 0, 0, 0, 1]
    check_against_model(lib, bsr, 0, 1, want, np.array([0.75]), np.array([3.0]), ("n1",))


def test_no_rows_no_launch(lib):
    """n = 0: the Lis API makes no matrix without rows (lis_matrix_set_size refuses 0, 0); the kernel entries take one and launch nothing"""
    A = capi.PM()
    assert lib.lis_matrix_create(capi.LIS_COMM_WORLD, C.byref(A)) == 0
    assert lib.lis_matrix_set_size(A, 0, 0) == capi.LIS_ERR_ILL_ARG
    lib.lis_matrix_destroy(A)

    class BiluT(C.Structure):
        _fields_ = [(k, C.c_int) for k in ("n", "nr", "bn", "serial")] + [(k, C.c_void_p) for k in ("aptr", "aindex", "avalue", "lptr", "lcol", "uptr", "ucol", "uskey", "uspos", "lval", "uval", "d")]

    class SweepT(C.Structure):
        _fields_ = [(k, C.c_int) for k in ("nlev", "nrows", "nnz", "ngroups")] + [(k, C.c_void_p) for k in ("lptr", "llong", "rows", "rptr", "col", "val", "groups", "h_nrows", "h_nshort")]
    factor, sweep, gather = lib.dll.liship_bilu_factor_f64, lib.dll.liship_bilu_sweep_f64, lib.dll.liship_block_gather_f64
    factor.argtypes = [C.POINTER(BiluT), C.POINTER(SweepT), C.c_void_p]
    sweep.argtypes = [C.POINTER(SweepT), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    gather.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    for bn in (1, 2, 3):
        empty = BiluT()
        empty.bn = bn
        assert factor(C.byref(empty), C.byref(SweepT()), None) == 0
        assert sweep(C.byref(SweepT()), 0, bn, None, None, None, None) == 0
        one = BiluT()
        one.n, one.nr, one.bn = 1, 1, bn
        assert factor(C.byref(one), C.byref(SweepT()), None) == -1          # a schedule of another size, NULL arrays: an argument error, no launch
        assert sweep(C.byref(SweepT()), 1, bn, None, None, None, None) == -1
    four = BiluT()
    four.bn = 4
    assert factor(C.byref(four), C.byref(SweepT()), None) == -1 and sweep(C.byref(SweepT()), 0, 4, None, None, None, None) == -1
    assert gather(0, 9, None, None, None, None) == 0 and gather(3, 9, None, None, None, None) == -1
