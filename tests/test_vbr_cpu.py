"""VBR storage without a device: the API (malloc / set / set_blocksize with arrays / duplicate / copy / unset / get_diagonal / scale / shift), the host
conversions in both directions with the in-place sort of the CSR source, and every refusal that needs no device -- all held, bit for bit, to the
reference's own results in tests/golden/vbr_bits.npz (tests/golden/make_golden_vbr.py).  The numpy models of tests/vbr_cases.py, from which the GPU tests
take their kernel-level expectations, are held to the same fixture here."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import lis_amd
import lisdrv
import vbr_cases as vc
import vbr_drv as drv
from lis_amd import _capi as capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", vc.FIXTURE))
VBR, CSR = drv.VBR, capi.LIS_MATRIX_CSR
NOT_IMPLEMENTED, ILL_ARG = capi.LIS_ERR_NOT_IMPLEMENTED, capi.LIS_ERR_ILL_ARG
FIELDS = ("row", "col", "ptr", "bptr", "bindex", "value")
ALL = vc.FOUND + vc.GIVEN


@pytest.fixture(scope="module")
def lib():
    lib = lis_amd.load()
    assert lib.initialize([]) == 0
    return lib


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


_MODEL = {}


def model(m):
    """(vbr dict, the source's (idx, val) afterwards) of case m by the numpy model, made once"""
    if m not in _MODEL:
        csr, row, col = vc.source(m)
        _MODEL[m] = vc.csr2vbr(*csr, row, col)
    return _MODEL[m]


def sizes(v):
    return [v["nr"], v["nc"], v["bnnz"], v["nnz"]]


def holds_fixture_arrays(v, m):
    return all(same(v[f], G["%s|vbr|%s" % (m, f)]) for f in FIELDS)


# ---------------------------------------------------------------------------------------------- the models against the fixture
@pytest.mark.parametrize("m", ALL)
def test_models_give_the_reference_arrays_and_products(m):
    csr = vc.source(m)[0]
    v, (sidx, sval) = model(m)
    n = v["n"]
    x = vc.xvec(n)
    assert sizes(v) == G[m + "|sizes"].tolist()
    if m in vc.ARRAYS_RECORDED:
        assert holds_fixture_arrays(v, m)
        for got, key in zip(vc.vbr2csr(v), ("ptr", "index", "value")):
            assert same(got, G["%s|csr|%s" % (m, key)]), key
        moved = m + "|source|index" in G.files
        assert moved == (not same(sidx, csr[1]))
        if moved:
            assert same(sidx, G[m + "|source|index"]) and same(sval, G[m + "|source|value"])
        assert same(vc.shift(v, vc.SHIFT), G[m + "|shift|value"])
    assert same(vc.matvec(v, x), G[m + "|y"])
    for T in vc.THREADS:
        assert same(vc.matvech(v, x, T), G["%s|yt|T%d" % (m, T)]), T
    assert same(vc.diagonal(v, np.full(n, 7.0)), G[m + "|diag"])
    if m in vc.SCALED:
        for tag, symm in (("jacobi", False), ("symm_diag", True)):
            assert same(vc.scale(v, G["%s|scale_%s|d" % (m, tag)], symm), G["%s|scale_%s|value" % (m, tag)])


def test_the_cases_are_what_they_are_meant_to_be():
    """uniform blocks where the reference's diagonal is the diagonal, variable ones where it is not; the chunked transposed sums differ from the plain ones;
    the unsorted source is moved by the conversion and a later duplicate stays in the block"""
    for m, right in (("fem3", True), ("fem3s", True), ("sym7b", True), ("diag", True), ("mesh123", False), ("mesh123s", False), ("heights", False)):
        v = model(m)[0]
        d = vc.diagonal(v, np.full(v["n"], 7.0))
        assert same(d, vc.true_diagonal(v)) == right, m
        assert right or np.count_nonzero(d == 7.0) > 0, m             # rows the search misses keep what the vector held
    assert any(not same(G["%s|yt|T1" % m], G["%s|yt|T8" % m]) for m in ALL)
    heights = np.diff(model("heights")[0]["row"]).tolist()
    for h in list(range(1, 9)) + [17, 63, 64, 65, 255, 256, 257, vc.TILE_ROWS - 1, vc.TILE_ROWS + 1, vc.TILE_UNROLL - 1, vc.TILE_UNROLL + 1]:
        assert h in heights
    assert not same(model("heights")[0]["row"], model("heights")[0]["col"])
    assert sorted(set(np.diff(model("blockcounts")[0]["bptr"]).tolist())) == [0, 1, 2, 32, 33]
    assert model("dense70")[0]["nr"] == 1 and model("diag")[0]["nnz"] == model("diag")[0]["n"]
    csr = vc.found("unsorted")
    v, (sidx, sval) = model("unsorted")
    twice = [i for i in range(v["n"]) if len(set(csr[1][csr[0][i]:csr[0][i + 1]])) < csr[0][i + 1] - csr[0][i]]
    assert twice and not same(sidx, csr[1])
    i = twice[0]
    cols = sidx[csr[0][i]:csr[0][i + 1]]
    k = int(np.flatnonzero(cols[1:] == cols[:-1])[0]) + 1             # the later of two entries of one column, after the sort
    dense = np.zeros((v["n"], v["n"]))
    for bi in range(v["nr"]):
        for _, c0, blk in vc.blocks_of(v, bi):
            dense[v["row"][bi]:v["row"][bi + 1], c0:c0 + blk.shape[0]] = blk.T
    assert dense[i, cols[k]] == sval[csr[0][i] + k] != sval[csr[0][i] + k - 1]


# ---------------------------------------------------------------------------------------------- liblis_amd's host routines against the fixture
def converted(lib, m):
    csr, row, col = vc.source(m)
    A = lisdrv.make_csr(lib, *csr)
    err, B = drv.to_vbr(lib, A, row, col)
    assert err == 0 and B.contents.matrix_type == VBR, m
    return csr, A, B


@pytest.mark.parametrize("m", ALL)
def test_host_conversions_diagonal_shift_and_scale(lib, m):
    csr, A, B = converted(lib, m)
    v = model(m)[0]
    n = v["n"]
    a = drv.arrays(B)
    assert sizes(a) == G[m + "|sizes"].tolist() and all(same(a[f], v[f]) for f in FIELDS)
    src = lisdrv.matrix_arrays(A)                                    # the source: sorted in place where the blocks were found
    assert same(src["index"], model(m)[1][0]) and same(src["value"], model(m)[1][1])
    err, back = drv.convert(lib, B, "csr")
    assert err == 0
    for got, want in zip((lisdrv.matrix_arrays(back)[f] for f in ("ptr", "index", "value")), vc.vbr2csr(v)):
        assert same(got, want)
    # copy and duplicate + convert (VBR to VBR goes through CSR, as in the reference: blocks found anew)
    dup = drv.duplicate_as(lib, B, "vbr")
    assert lib.lis_matrix_copy(B, dup) == 0 and all(same(drv.arrays(dup)[f], a[f]) for f in FIELDS)
    lib.lis_matrix_destroy(dup)
    err, again = drv.convert(lib, B, "vbr")
    assert err == 0
    want = vc.csr2vbr(*vc.vbr2csr(v))[0]
    assert all(same(drv.arrays(again)[f], want[f]) for f in FIELDS)
    lib.lis_matrix_destroy(again)
    err, d = drv.diagonal(lib, B, np.full(n, 7.0))
    assert err == 0 and same(d, G[m + "|diag"])
    if m in vc.SCALED:
        for action, tag in ((1, "jacobi"), (2, "symm_diag")):
            fresh = lisdrv.make_csr(lib, *csr)
            err, S = drv.to_vbr(lib, fresh, *vc.source(m)[1:])
            lib.lis_matrix_destroy(fresh)
            assert err == 0 and same(drv.arrays(S)["value"], v["value"])
            err, b, d = drv.scale(lib, S, np.ones(n), action, np.full(n, vc.D_BEFORE))
            assert err == 0 and same(d, G["%s|scale_%s|d" % (m, tag)]) and same(b, G["%s|scale_%s|b" % (m, tag)])
            assert same(drv.arrays(S)["value"], G["%s|scale_%s|value" % (m, tag)])
            lib.lis_matrix_destroy(S)
    assert lib.lis_matrix_shift_diagonal(B, vc.SHIFT) == 0
    assert same(drv.arrays(B)["value"], G[m + "|shift|value"] if m in vc.ARRAYS_RECORDED else vc.shift(v, vc.SHIFT))
    for M in (back, B, A):
        lib.lis_matrix_destroy(M)


def test_malloc_set_unset_and_assemble(lib):
    v = model("blockcounts")[0]
    A = drv.make_vbr(lib, v)
    a = A.contents
    assert a.matrix_type == VBR and a.status == VBR and a.is_block and (a.nr, a.nc, a.bnnz, a.nnz) == tuple(sizes(v))
    assert all(same(drv.arrays(A)[f], v[f]) for f in FIELDS)
    # unset: the arrays are the caller's again, the matrix takes new ones
    keep = [C.cast(getattr(a, f), C.c_void_p).value for f in FIELDS]
    assert lib.lis_matrix_unset(A) == 0 and a.status == -257 and not a.row and not a.value
    p = [C.cast(k, capi.P_DBL if f == "value" else capi.P_INT) for k, f in zip(keep, FIELDS)]
    assert lib.lis_matrix_set_vbr(v["nnz"], v["nr"], v["nc"], v["bnnz"], *p, A) == 0 and lib.lis_matrix_assemble(A) == 0
    assert all(same(drv.arrays(A)[f], v[f]) for f in FIELDS)
    # set_vbr on an assembled matrix: success, nothing adopted (the reference's quirk)
    assert lib.lis_matrix_set_vbr(1, 1, 1, 1, *p, A) == 0 and A.contents.nnz == v["nnz"]
    lib.lis_matrix_destroy(A)


def test_set_type_then_assemble_or_input(lib, tmp_path):
    """lis_matrix_set_type(A, LIS_MATRIX_VBR) before element-wise assembly or lis_input: the CSR rows become VBR, blocks found by the conversion"""
    csr = vc.found("mesh123s")
    v = model("mesh123s")[0]
    n = v["n"]
    A = capi.PM()
    assert lib.lis_matrix_create(capi.LIS_COMM_WORLD, C.byref(A)) == 0 and lib.lis_matrix_set_size(A, n, 0) == 0 and lib.lis_matrix_set_type(A, VBR) == 0
    for i in range(n):
        for k in range(csr[0][i], csr[0][i + 1]):
            assert lib.lis_matrix_set_value(capi.LIS_INS_VALUE, i, int(csr[1][k]), float(csr[2][k]), A) == 0
    assert lib.lis_matrix_assemble(A) == 0 and A.contents.matrix_type == VBR
    assert all(same(drv.arrays(A)[f], v[f]) for f in FIELDS)
    lib.lis_matrix_destroy(A)
    path = tmp_path / "mesh.mtx"
    rows = np.repeat(np.arange(n), np.diff(csr[0]))
    path.write_text("%%%%MatrixMarket matrix coordinate real general\n%d %d %d\n" % (n, n, len(rows)) +
                    "".join("%d %d %s\n" % (r + 1, c + 1, repr(float(x))) for r, c, x in zip(rows, csr[1], csr[2])))
    A = capi.PM()
    assert lib.lis_matrix_create(capi.LIS_COMM_WORLD, C.byref(A)) == 0 and lib.lis_matrix_set_type(A, VBR) == 0
    assert lib.lis_input_matrix(A, str(path).encode()) == 0 and A.contents.matrix_type == VBR
    assert all(same(drv.arrays(A)[f], v[f]) for f in FIELDS)
    lib.lis_matrix_destroy(A)


def test_set_blocksize_arguments(lib, capfd):
    csr, row, col = vc.source("blockcounts")
    A = lisdrv.make_csr(lib, *csr)
    n = A.contents.n
    B = drv.duplicate_as(lib, A, "vbr")
    r, c = row.ctypes.data_as(capi.P_INT), col.ctypes.data_as(capi.P_INT)
    assert lib.lis_matrix_set_blocksize(B, 0, 3, r, c) == ILL_ARG and lib.lis_matrix_set_blocksize(B, 3, -1, None, None) == ILL_ARG
    assert lib.lis_matrix_set_blocksize(B, len(row) - 1, len(col) - 1, r, None) == ILL_ARG and lib.lis_matrix_set_blocksize(B, len(row) - 1, len(col) - 1, None, c) == ILL_ARG
    assert not B.contents.conv_row and not B.contents.conv_col
    # the arrays are COPIED (exactly nr + 1 and nc + 1 entries are read), and the counts kept
    assert lib.lis_matrix_set_blocksize(B, len(row) - 1, len(col) - 1, r, c) == 0
    assert (B.contents.conv_bnr, B.contents.conv_bnc) == (len(row) - 1, len(col) - 1)
    assert same(lisdrv._arr(B.contents.conv_row, len(row), np.int32), row) and same(lisdrv._arr(B.contents.conv_col, len(col), np.int32), col)
    assert C.cast(B.contents.conv_row, C.c_void_p).value != row.ctypes.data
    # a later call without arrays: the same counts keep them, other counts drop them (they would no longer describe the arrays)
    assert lib.lis_matrix_set_blocksize(B, len(row) - 1, len(col) - 1, None, None) == 0 and B.contents.conv_row and B.contents.conv_col
    assert lib.lis_matrix_set_blocksize(B, 2, 2, None, None) == 0 and not B.contents.conv_row and not B.contents.conv_col and B.contents.conv_bnr == 2
    assert lib.lis_matrix_set_blocksize(B, len(row) - 1, len(col) - 1, r, c) == 0
    assert lib.lis_matrix_convert(A, B) == 0 and same(drv.arrays(B)["row"], row) and same(drv.arrays(B)["col"], col)
    assert C.cast(B.contents.row, C.c_void_p).value != C.cast(B.contents.conv_row, C.c_void_p).value          # (freed once each)
    lib.lis_matrix_destroy(B)
    # a partition that does not cover the matrix, or does not ascend: refused by the conversion, source and target untouched
    capfd.readouterr()
    for bad_row, bad_col, text in ((np.array([0, 5, n - 1], np.int32), col, "row[] must run from 0 to n"), (np.array([0, 9, 9, n], np.int32), col, "row[] does not ascend"),
                                   (row, np.array([0, 7, 3, n], np.int32), "col[] does not ascend"), (row, np.array([1, n], np.int32), "row[] must run from 0 to n")):
        B = drv.duplicate_as(lib, A, "vbr")
        assert lib.lis_matrix_set_blocksize(B, len(bad_row) - 1, len(bad_col) - 1, bad_row.ctypes.data_as(capi.P_INT), bad_col.ctypes.data_as(capi.P_INT)) == 0
        assert lib.lis_matrix_convert(A, B) == ILL_ARG and text in capfd.readouterr().out
        assert B.contents.status == -257 and same(lisdrv.matrix_arrays(A)["value"], csr[2])
        lib.lis_matrix_destroy(B)
    lib.lis_matrix_destroy(A)


# ---------------------------------------------------------------------------------------------- refusals
def untouched(A, before):
    now = drv.arrays(A)
    return now["type"] == before["type"] and all(same(now[f], before[f]) for f in FIELDS) and not A.contents.is_splited


def test_refusals_leave_the_matrix_alone(lib, capfd):
    csr = vc.found("mesh123s")
    n = len(csr[0]) - 1
    A = drv.make_vbr(lib, model("mesh123s")[0])
    before = drv.arrays(A)
    capfd.readouterr()
    assert lib.lis_matrix_split(A) == NOT_IMPLEMENTED and untouched(A, before)
    assert "lis_matrix_split: VBR storage is not split" in capfd.readouterr().out
    for holder, extra in ((A, ""), (None, " -storage vbr")):
        M = holder if holder is not None else lisdrv.make_csr(lib, *csr)
        held = drv.arrays(M)
        for p, text in (("ssor", "-p ssor is served for CSR and BSR storage only"), ("is", "-p is is served for CSR storage only")):
            b, x = lisdrv.new_vector(lib, M, np.ones(n)), lisdrv.new_vector(lib, M, np.full(n, 3.0))
            S = capi.PS()
            assert lib.lis_solver_create(C.byref(S)) == 0 and lib.lis_solver_set_option(("-i cg -p %s%s" % (p, extra)).encode(), S) == 0
            assert lib.lis_solve(M, b, x, S) == NOT_IMPLEMENTED
            out = capfd.readouterr().out
            assert text in out and "A is untouched" in out, out
            now = drv.arrays(M)
            assert now["type"] == held["type"] and same(now["value"], held["value"]) and not M.contents.is_splited
            assert same(lisdrv.get_vector(lib, b), np.ones(n)) and same(lisdrv.get_vector(lib, x), np.full(n, 3.0))
            lib.lis_solver_destroy(S); lib.lis_vector_destroy(b); lib.lis_vector_destroy(x)
        if holder is None:
            lib.lis_matrix_destroy(M)
    Bc = lisdrv.make_csr(lib, *csr)
    held = lisdrv.matrix_arrays(Bc)
    for first, second in ((A, Bc), (Bc, A)):
        assert lib.lis_matrix_shift_matrix(first, second, 0.5) == NOT_IMPLEMENTED
        assert "lis_matrix_shift_matrix: VBR storage is not shifted by a matrix" in capfd.readouterr().out
        assert untouched(A, before) and same(lisdrv.matrix_arrays(Bc)["value"], held["value"])
    for first, second, extra in ((A, Bc, ""), (Bc, A, ""), (Bc, Bc, " -estorage vbr")):
        x = lisdrv.new_vector(lib, first, np.full(n, 3.0))
        E, ev = capi.PE(), C.c_double(0.0)
        assert lib.lis_esolver_create(C.byref(E)) == 0 and lib.lis_esolver_set_option(("-e gpi" + extra).encode(), E) == 0
        assert lib.lis_gesolve(first, second, x, C.byref(ev), E) == NOT_IMPLEMENTED
        assert "or in VBR storage" in capfd.readouterr().out
        assert untouched(A, before) and same(lisdrv.matrix_arrays(Bc)["value"], held["value"]) and same(lisdrv.get_vector(lib, x), np.full(n, 3.0))
        lib.lis_esolver_destroy(E); lib.lis_vector_destroy(x)
    # MSR and BSC stay refused, from VBR too and as -storage
    for fmt_id, key in ((3, "msr"), (8, "bsc")):
        M = capi.PM()
        lib.lis_matrix_duplicate(A, C.byref(M)); lib.lis_matrix_set_type(M, fmt_id)
        assert lib.lis_matrix_convert(A, M) == NOT_IMPLEMENTED and untouched(A, before)
        lib.lis_matrix_destroy(M)
        M = capi.PM()
        lib.lis_matrix_duplicate(Bc, C.byref(M)); lib.lis_matrix_set_type(M, fmt_id)
        assert lib.lis_matrix_convert(Bc, M) == NOT_IMPLEMENTED
        lib.lis_matrix_destroy(M)
    lib.lis_matrix_destroy(Bc); lib.lis_matrix_destroy(A)


RANKS_WORKER = r'''
import ctypes as C, os, sys
import numpy as np
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
import vbr_cases as vc, vbr_drv as drv, lis_amd, lisdrv
from lis_amd import _capi as capi
ALLGATHER = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t)
EXCHANGE = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_int))
class Callbacks(C.Structure):                      # lis_amd_comm_callbacks (include/lis_amd.h)
    _fields_ = [("allgather", ALLGATHER), ("neighbor_exchange", EXCHANGE), ("ctx", C.c_void_p)]
reached = []
def allgather(ctx, send, recv, nbytes): reached.append("allgather"); return 1
def exchange(ctx, nneib, neib, sendbuf, sptr, recvbuf, rptr): reached.append("exchange"); return 1
lib = lis_amd.load()
assert lib.initialize([]) == 0
csr = vc.found("mesh123s")
n = len(csr[0]) - 1
A = {"vbr": drv.make_vbr(lib, vc.csr2vbr(*csr)[0]), "csr": lisdrv.make_csr(lib, *csr)}
vx, vy = lisdrv.new_vector(lib, A["csr"], np.ones(n)), lisdrv.new_vector(lib, A["csr"], np.full(n, 3.0))
before = {f: drv.arrays(A[f]) for f in A}
# the matrices were made by a job of one rank; from here on the library believes it is rank 0 of 2 (no callback is ever reached: every call below is refused first)
cb = Callbacks(ALLGATHER(allgather), EXCHANGE(exchange), None)
lib.dll.lis_amd_comm_init_callbacks.argtypes = [C.POINTER(Callbacks), C.c_int, C.c_int]
assert lib.dll.lis_amd_comm_init_callbacks(C.byref(cb), 0, 2) == 0
assert lib.lis_matvec(A["vbr"], vx, vy) == 5 and lib.lis_matvech(A["vbr"], vx, vy) == 5
B = drv.duplicate_as(lib, A["vbr"], "csr")
assert lib.lis_matrix_convert(A["vbr"], B) == 5
B = drv.duplicate_as(lib, A["csr"], "vbr")
assert lib.lis_matrix_convert(A["csr"], B) == 5
for M, opts in ((A["vbr"], "-i cg"), (A["csr"], "-i cg -storage vbr")):
    S = capi.PS()
    assert lib.lis_solver_create(C.byref(S)) == 0 and lib.lis_solver_set_option(opts.encode(), S) == 0
    assert lib.lis_solve(M, vx, vy, S) == 5
for f in A:
    now = drv.arrays(A[f])
    assert now["type"] == before[f]["type"] and now["value"].tobytes() == before[f]["value"].tobytes()
assert lisdrv.get_vector(lib, vy).tobytes() == np.full(n, 3.0).tobytes()
assert not reached, reached
print("REFUSED")
'''


def test_several_ranks_are_refused_before_anything_is_touched():
    out = subprocess.run([sys.executable, "-c", RANKS_WORKER % {"root": ROOT}], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "REFUSED" in out.stdout, out.stderr[-3000:]
    assert out.stdout.count("VBR storage is served on one rank only (this job has 2)") >= 6, out.stderr[-3000:]
