"""VBR storage on the device, bit for bit.

Kernel level (include/liship.h through lis_amd.load()): liship_spmv_vbr_f64 on every case of tests/vbr_cases.py -- block rows of every height from 1 to
one more than a workgroup's rows, of 0, 1, 32 and 33 blocks, non-square blocks, one dense block, 1 x 1 blocks -- with unaligned arrays, special values
and a sentinel behind y; the block-row-of-row kernel and the checking kernel on the same cases and on every violation; the transposed sums in chunks of
block rows.  Expectations come from the numpy models of tests/vbr_cases.py, which tests/test_vbr_cpu.py holds to the reference's own results.

API level: products through lis_matvec / lis_matvech and the raw entry points, whole solves and eigensolves against tests/golden/vbr_bits.npz -- in the
reference-order mode every count, status, residual history and solution in every bit, fused and unfused; in the default mode the count inside the
reference's own spread over T = 1 / 8 widened by 1 and x within 1e-8 (the bar of tests/test_more_solvers_gpu.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import esolve_drv
import esolve_multi_drv
import format_cases as fc
import lis_amd
import lisdrv
import vbr_cases as vc
import vbr_drv as drv
from gpu_arrays import Out, dev
from lis_amd import DeviceArray as DA, _capi as capi, check

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", vc.FIXTURE))
ERR_ARG = -1                                    # LISHIP_ERR_ARG
NOT_IMPLEMENTED, ILL_ARG = capi.LIS_ERR_NOT_IMPLEMENTED, capi.LIS_ERR_ILL_ARG
BAD_ROW, BAD_COL, BAD_BPTR, BAD_PTR, BAD_BINDEX, BAD_SIZE = 1, 2, 4, 8, 16, 32      # LISHIP_VBR_BAD_*
INT_FIELDS = ("row", "col", "ptr", "bptr", "bindex")
ALL = vc.FOUND + vc.GIVEN
WAVE = 64


@pytest.fixture(scope="module")
def lib():
    lib = lis_amd.load()
    assert lis_amd.gpu_available(), "no HIP device: the product path has no CPU fallback"
    assert lib.initialize([]) == 0
    for f in (lib.dll.lis_amd_matrix_device_type, lib.dll.lis_amd_matrix_upload, lib.dll.lis_amd_matrix_host_written):
        f.argtypes = [capi.PM]
    return lib


class mode:
    """lis_amd_set_reference_reductions(T) for the duration of a with block (T = 0: the default mode)"""
    def __init__(self, lib, T):
        self.lib, self.T = lib, T

    def __enter__(self):
        assert self.lib.dll.lis_amd_set_reference_reductions(self.T) == 0

    def __exit__(self, *a):
        self.lib.dll.lis_amd_set_reference_reductions(0)


UNFUSED = 2                                     # LIS_AMD_LOOP_UNFUSED: one kernel per reference call


class loops:
    """lis_amd_set_loop_mode(mode) for the duration of a with block"""
    def __init__(self, lib, mode):
        self.lib, self.mode = lib, mode

    def __enter__(self):
        assert self.lib.dll.lis_amd_set_loop_mode(self.mode) == 0

    def __exit__(self, *a):
        self.lib.dll.lis_amd_set_loop_mode(0)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


_MODEL = {}


def model(m):
    """the VBR arrays of case m by the numpy model (held to the reference's by tests/test_vbr_cpu.py), made once"""
    if m not in _MODEL:
        csr, row, col = vc.source(m)
        _MODEL[m] = vc.csr2vbr(*csr, row, col)[0]
    return _MODEL[m]


def checked(lib, v, arrays):
    """liship_vbr_check on device arrays -> flags"""
    flags = C.c_int(-1)
    check(lib.liship_vbr_check(v["n"], v["n"], v["nnz"], v["nr"], v["nc"], v["bnnz"],
                               *[arrays[f][1] for f in INT_FIELDS], C.byref(flags), None))
    return flags.value


def product(lib, v, x, shift=0, val=None):
    """check, block rows and product as lis_upload.c / lis_product.c launch them -> (Out, brow)"""
    n = v["n"]
    arrays = {f: dev(v[f], np.int32) for f in INT_FIELDS}
    keep = (_, dv), (_, dx) = dev(v["value"] if val is None else val, np.float64, shift), dev(x, np.float64, shift)
    assert checked(lib, v, arrays) == 0
    brow = DA(n + 4, np.int32)
    check(lib.liship_memset(brow.ptr, 0xFF, brow.nbytes, None))
    check(lib.liship_vbr_block_rows(n, v["nr"], arrays["row"][1], brow.ptr, None))
    y = Out(n, shift)
    check(lib.liship_spmv_vbr_f64(n, *[arrays[f][1] for f in INT_FIELDS], brow.ptr, dv, dx, y.ptr, None))
    check(lib.liship_device_synchronize())
    del keep
    return y, brow.to_host()


# ================================================================ kernel level
def test_tile_constants(lib):
    info = (C.c_int * 2)()
    check(lib.liship_vbr_tile_info(info))
    assert list(info) == [vc.TILE_ROWS, vc.TILE_UNROLL]
    assert lib.liship_vbr_tile_info(None) == ERR_ARG
    assert lib.liship_spmv_vbr_f64(-1, None, None, None, None, None, None, None, None, None, None) == ERR_ARG
    assert lib.liship_vbr_check(1, 1, 1, 1, 1, 1, None, None, None, None, None, None, None) == ERR_ARG


def test_the_border_cases_have_the_layout_they_aim_at():
    """`heights`: a block row of every height 1 .. 8, 17, 63 .. 65, 255 .. 257 and the tile constants +- 1, starting at offsets into wavefronts and
    workgroups that differ from block row to block row, with block rows that lie inside one wavefront, cross a wavefront border, cross a workgroup
    border and cover a whole workgroup; widths on both sides of the unroll; `blockcounts`: block rows of 0, 1, 32 and 33 blocks"""
    v = model("heights")
    row, heights = v["row"], np.diff(v["row"]).tolist()
    for h in list(range(1, 9)) + [17, 63, 64, 65, 255, 256, 257, vc.TILE_ROWS - 1, vc.TILE_ROWS + 1, vc.TILE_UNROLL - 1, vc.TILE_UNROLL + 1]:
        assert h in heights, h
    inside = [bi for bi in range(v["nr"]) if row[bi] // WAVE == (row[bi + 1] - 1) // WAVE]
    wave = [bi for bi in range(v["nr"]) if row[bi] // WAVE != (row[bi + 1] - 1) // WAVE]
    group = [bi for bi in range(v["nr"]) if row[bi] // vc.TILE_ROWS != (row[bi + 1] - 1) // vc.TILE_ROWS]
    whole = [bi for bi in range(v["nr"]) if (row[bi + 1] - 1) // vc.TILE_ROWS - row[bi] // vc.TILE_ROWS >= 1 and row[bi + 1] - row[bi] >= vc.TILE_ROWS]
    assert inside and wave and group and whole
    assert len({int(r) % WAVE for r in row[:-1]}) > 10 and v["n"] % vc.TILE_ROWS != 0 and v["n"] > 2 * vc.TILE_ROWS
    widths = {int(v["col"][bj + 1] - v["col"][bj]) for bj in v["bindex"]}
    assert {vc.TILE_UNROLL - 1, vc.TILE_UNROLL, vc.TILE_UNROLL + 1, 2 * vc.TILE_UNROLL, 2 * vc.TILE_UNROLL + 1} <= widths, widths
    assert not same(v["row"], v["col"])
    assert sorted(set(np.diff(model("blockcounts")["bptr"]).tolist())) == [0, 1, 2, 32, 33]
    assert model("dense70")["nr"] == 1 and model("dense70")["nnz"] == 70 * 70 and set(np.diff(model("diag")["row"]).tolist()) == {1}
    assert model("one")["n"] == 1 and np.count_nonzero(np.diff(vc.found("empty_rows")[0]) == 0) == 3


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("m", ALL)
def test_forward_product_of_every_case(lib, m, shift):
    """every row the reference's chain in every bit; value, x and y one element behind an aligned address; Y_PAD elements behind y keep the sentinel;
    brow[i] the block row of row i and nothing written behind n"""
    v = model(m)
    x = vc.xvec(v["n"], 5 + shift)
    y, brow = product(lib, v, x, shift)
    y.holds(vc.matvec(v, x), (m, shift))
    assert same(brow[:v["n"]], np.repeat(np.arange(v["nr"], dtype=np.int32), np.diff(v["row"]))) and np.all(brow[v["n"]:] == -1)
    if shift == 0:
        assert same(vc.matvec(v, vc.xvec(v["n"])), G[m + "|y"])         # (the model IS the reference: the fixture's y)


@pytest.mark.parametrize("m", ["heights", "blockcounts", "mesh123s"])
def test_forward_product_special_values(lib, m):
    v = model(m)
    n, val, x = v["n"], v["value"], vc.xvec(v["n"], 9)
    bc = int(np.argmax(np.diff(v["ptr"])))                     # the largest block: its block row, its first column
    bi = int(np.searchsorted(v["bptr"], bc, side="right")) - 1
    c0, h = int(v["col"][v["bindex"][bc]]), int(v["row"][bi + 1] - v["row"][bi])
    # an infinity in x against explicit zeros of a block's column: 0 * inf is NaN in every row of the block row (zeros are multiplied)
    vz, xi = val.copy(), x.copy()
    vz[v["ptr"][bc]:v["ptr"][bc] + h] = 0.0
    xi[c0] = np.inf
    # a NaN with a payload in one stored value: its row is NaN, the others are not
    vn = val.copy()
    vn[v["ptr"][bc] + h - 1] = np.array([0x7FF8000000ABCDEF], np.uint64).view(np.float64)[0]
    # a negative infinity in a value against a positive x, and -0.0 in x
    vi, xm = val.copy(), np.abs(x) + 0.25
    vi[v["ptr"][bc]] = -np.inf
    xm[(c0 + 1) % n] = -0.0
    # every product -0.0: the sums start at +0.0 and end there
    vm, xz = fc.all_products_negative_zero(val, n)
    for tag, vv, xx in (("inf", vz, xi), ("nan", vn, x), ("-inf", vi, xm), ("-0", vm, xz)):
        ref = vc.matvec(dict(v, value=vv), xx)
        rows = np.arange(v["row"][bi], v["row"][bi + 1])
        if tag == "inf":
            assert np.all(np.isnan(ref[rows]))
        if tag == "nan":
            assert np.isnan(ref[rows[-1]]) and np.count_nonzero(np.isnan(ref)) == 1
        if tag == "-inf":
            assert ref[rows[0]] == -np.inf
        if tag == "-0":
            assert same(ref, np.zeros(n))
        y, _ = product(lib, v, xx, 0, vv)
        y.holds(ref, (m, tag), special=tag in ("inf", "nan"))


def test_the_check_names_every_violation(lib):
    """each array broken at its first, a middle and its last entry gives its own bit and no other kernel runs; arrays that pass give 0"""
    v = model("blockcounts")
    nr, nc, bnnz = v["nr"], v["nc"], v["bnnz"]

    def flags(**changed):
        w = dict(v, **changed)
        arrays = {f: dev(w[f], np.int32) for f in INT_FIELDS}
        return checked(lib, w, arrays)

    def edit(f, at, value):
        a = v[f].copy()
        a[at] = value
        return {f: a}

    assert flags() == 0 and all(checked(lib, model(m), {f: dev(model(m)[f], np.int32) for f in INT_FIELDS}) == 0 for m in ALL)
    for at, value in ((0, 1), (nr, v["n"] - 1), (nr, v["n"] + 1), (2, int(v["row"][1])), (2, int(v["row"][3]))):
        assert flags(**edit("row", at, value)) & BAD_ROW, ("row", at)
    for at, value in ((0, -1), (nc, int(v["col"][-1]) + 1), (5, int(v["col"][4])), (nc - 1, int(v["col"][nc]))):
        assert flags(**edit("col", at, value)) & BAD_COL, ("col", at)
    assert flags(**edit("col", 0, -1)) & BAD_ROW == 0
    for at, value in ((0, 1), (nr, bnnz - 1), (nr, bnnz + 1), (3, int(v["bptr"][2]) - 1)):
        assert flags(**edit("bptr", at, value)) & BAD_BPTR, ("bptr", at)
    for at, value in ((0, -1), (bnnz, v["nnz"] + 1), (7, int(v["ptr"][6]) - 1)):
        assert flags(**edit("ptr", at, value)) & BAD_PTR, ("ptr", at)
    for at, value in ((0, -1), (bnnz - 1, nc), (bnnz // 2, 1 << 30)):
        assert flags(**edit("bindex", at, value)) == BAD_BINDEX, ("bindex", at)
    # a block of another size than its rows x columns: ptr ascends, the size does not fit (also through a bindex of another width)
    assert flags(**edit("ptr", 5, int(v["ptr"][5]) + 1)) == BAD_SIZE
    other = next(bj for bj in range(nc) if v["col"][bj + 1] - v["col"][bj] != v["col"][v["bindex"][0] + 1] - v["col"][v["bindex"][0]])
    assert flags(**edit("bindex", 0, other)) == BAD_SIZE
    # counts that cannot be: no kernel runs
    assert checked(lib, dict(v, nr=0), {f: dev(v[f], np.int32) for f in INT_FIELDS}) == BAD_ROW
    assert checked(lib, dict(v, nc=v["n"] + 1), {f: dev(np.zeros(v["n"] + 3, np.int32), np.int32) for f in INT_FIELDS}) & BAD_COL


@pytest.mark.parametrize("m", ["heights", "blockcounts", "mesh123s", "one"])
def test_transposed_sums_in_chunks_of_block_rows(lib, m):
    """liship_spmv_csr_transposed_bordered_f64 on the transposed rows of the reference's walk: T chunks of BLOCK ROWS, each from +0.0, added in chunk
    order from +0.0; T beyond nr leaves chunks empty"""
    v = model(m)
    n, x = v["n"], vc.xvec(v["n"], 3)
    dst, src, val = [], [], []                                  # the walk: block rows, blocks in stored order, j outer, i inner
    for bi in range(v["nr"]):
        rows = np.arange(v["row"][bi], v["row"][bi + 1])
        for _, c0, blk in vc.blocks_of(v, bi):
            for j in range(blk.shape[0]):
                dst += [c0 + j] * len(rows); src += list(rows); val += list(blk[j])
    order = np.argsort(np.array(dst, np.int64), kind="stable")
    tptr = np.concatenate([[0], np.cumsum(np.bincount(np.array(dst, np.int64), minlength=n))]).astype(np.int32)
    keep = (_, dp), (_, di), (_, dv), (_, dx) = dev(tptr, np.int32), dev(np.array(src, np.int32)[order], np.int32), dev(np.array(val)[order], np.float64), dev(x)
    for T in (1, 2, 8, v["nr"] + 3):
        b = dev(vc.chunk_borders(v, T), np.int32)
        y = Out(n)
        check(lib.liship_spmv_csr_transposed_bordered_f64(n, T, b[1], dp, di, dv, dx, y.ptr, None))
        y.holds(vc.matvech(v, x, T), (m, T))
    assert lib.liship_spmv_csr_transposed_bordered_f64(n, 0, b[1], dp, di, dv, dx, y.ptr, None) == ERR_ARG
    del keep


@pytest.mark.parametrize("m", ["heights", "blockcounts", "mesh123s", "fem3s", "one"])
def test_shift_and_scale_kernels_edit_value_in_place(lib, m):
    """liship_vbr_shift_diagonal_f64 and liship_vbr_scale_f64 on value[] in HBM: the host routines' results in every bit (the reference's diagonal search, right
    or not; value*d[i] and value*d[i]*d[j] in that order), nothing written outside value[0 .. nnz)"""
    v = model(m)
    n, nnz = v["n"], v["nnz"]
    arrays = {f: dev(v[f], np.int32) for f in INT_FIELDS}
    assert checked(lib, v, arrays) == 0
    brow = DA(n + 4, np.int32)
    check(lib.liship_vbr_block_rows(n, v["nr"], arrays["row"][1], brow.ptr, None))
    d = 0.5 + np.random.default_rng(21).uniform(size=n)
    keep = _, dd = dev(d, np.float64, 1)
    pad = np.concatenate([fc.sentinel(1), v["value"], fc.sentinel(fc.Y_PAD)])

    def edited(launch):
        val = DA.from_host(pad)
        check(launch(val.ptr + 8))
        got = val.to_host()
        assert fc.bits(got[:1])[0] == fc.SENTINEL_BITS and np.all(fc.bits(got[1 + nnz:]) == fc.SENTINEL_BITS)
        return got[1:1 + nnz]

    ints = [arrays[f][1] for f in INT_FIELDS]
    assert same(edited(lambda p: lib.liship_vbr_shift_diagonal_f64(n, v["nr"], *ints, p, vc.SHIFT, None)), vc.shift(v, vc.SHIFT))
    for symm in (0, 1):
        assert same(edited(lambda p: lib.liship_vbr_scale_f64(n, *ints, brow.ptr, p, dd, symm, None)), vc.scale(v, d, bool(symm))), symm
    del keep


@pytest.mark.parametrize("m", vc.SCALED)
def test_scaling_a_matrix_whose_copy_lives_in_hbm(lib, m):
    """lis_matrix_scale on a held VBR matrix after its upload: host arrays, b and d as the reference leaves them, and the products that follow run on the scaled
    values -- forward and transposed (the transposed copy is made again from them)"""
    v = model(m)
    n, x = v["n"], vc.xvec(v["n"])
    for action, tag in ((1, "jacobi"), (2, "symm_diag")):
        A = held(lib, m)
        assert lib.dll.lis_amd_matrix_upload(A) == 0 and same(lisdrv.matvech(lib, A, x), G[m + "|yt|T1"])
        err, b, d = drv.scale(lib, A, np.ones(n), action, np.full(n, vc.D_BEFORE))
        assert err == 0 and same(d, G["%s|scale_%s|d" % (m, tag)]) and same(b, G["%s|scale_%s|b" % (m, tag)])
        scaled = G["%s|scale_%s|value" % (m, tag)]
        assert same(drv.arrays(A)["value"], scaled)
        assert lib.dll.lis_amd_matrix_host_written(A) == 0
        w = dict(v, value=scaled)
        assert same(lisdrv.matvec(lib, A, x), vc.matvec(w, x)) and same(lisdrv.matvech(lib, A, x), vc.matvech(w, x))
        lib.lis_matrix_destroy(A)


# ================================================================ API level
def held(lib, m):
    """case m as a VBR matrix from lis_matrix_malloc_vbr + lis_matrix_set_vbr"""
    return drv.make_vbr(lib, model(m))


@pytest.mark.parametrize("m", ALL)
def test_products_through_the_lis_entry_points(lib, m):
    A = held(lib, m)
    v = model(m)
    n = v["n"]
    x = vc.xvec(n)
    assert lib.dll.lis_amd_matrix_device_type(A) == drv.VBR
    assert same(lisdrv.matvec(lib, A, x), G[m + "|y"]) and same(drv.raw_product(lib, A, "vbr", x)[:n], G[m + "|y"])
    for T in (0, 1, 8):
        with mode(lib, T):
            want = G["%s|yt|T%d" % (m, max(T, 1))]
            assert same(lisdrv.matvech(lib, A, x), want), T
            assert same(drv.raw_product(lib, A, "vbr", x, transposed=True), want), T
            assert same(lisdrv.matvec(lib, A, x), G[m + "|y"]), T
    err, d = drv.diagonal(lib, A, np.full(n, 7.0))
    assert err == 0 and same(d, G[m + "|diag"])
    # the shift runs as a kernel on the copy and as the same edit on the host arrays, which the write watch does not take for the program's
    assert lib.lis_matrix_shift_diagonal(A, vc.SHIFT) == 0 and same(drv.arrays(A)["value"], vc.shift(v, vc.SHIFT))
    assert lib.dll.lis_amd_matrix_host_written(A) == 0
    w = dict(v, value=vc.shift(v, vc.SHIFT))
    assert same(lisdrv.matvec(lib, A, x), vc.matvec(w, x)) and same(lisdrv.matvech(lib, A, x), vc.matvech(w, x))
    lib.lis_matrix_destroy(A)


def test_conversion_of_a_source_that_lives_in_hbm(lib):
    """csr2vbr sorts the source in place: its HBM copy, made from the unsorted rows, is rebuilt, and its product carries the sorted rows' bits"""
    csr = vc.found("unsorted")
    n = len(csr[0]) - 1
    x = vc.xvec(n)
    A = lisdrv.make_csr(lib, *csr)
    assert lib.dll.lis_amd_matrix_upload(A) == 0
    import orc
    assert same(lisdrv.matvec(lib, A, x), orc.spmv_csr(*csr, x))
    err, B = drv.to_vbr(lib, A)
    assert err == 0 and same(lisdrv.matrix_arrays(A)["index"], G["unsorted|source|index"])
    assert same(lisdrv.matvec(lib, A, x), orc.spmv_csr(csr[0], G["unsorted|source|index"], G["unsorted|source|value"], x))
    assert same(lisdrv.matvec(lib, B, x), G["unsorted|y"])
    lib.lis_matrix_destroy(B); lib.lis_matrix_destroy(A)


def test_arrays_that_do_not_describe_a_matrix_are_refused_by_name(lib, capfd):
    v = model("mesh123s")
    x = vc.xvec(v["n"])
    for f, at, value, text in (("bindex", 3, v["nc"], "bindex[] holds a block column outside"), ("row", 2, int(v["row"][1]), "row[] must ascend strictly"),
                               ("ptr", 4, int(v["ptr"][4]) + 1, "is not the size of block"), ("bptr", v["nr"], v["bnnz"] + 2, "bptr[] must ascend from 0 to bnnz")):
        a = v[f].copy()
        a[at] = value
        A = drv.make_vbr(lib, dict(v, **{f: a}))
        vx, vy = lisdrv.new_vector(lib, A, x), lisdrv.new_vector(lib, A, np.full(v["n"], 3.0))
        capfd.readouterr()
        assert lib.lis_matvec(A, vx, vy) == ILL_ARG and text in capfd.readouterr().out, f
        assert lib.lis_matvech(A, vx, vy) == ILL_ARG
        assert same(lisdrv.get_vector(lib, vy), np.full(v["n"], 3.0))
        lib.lis_vector_destroy(vx); lib.lis_vector_destroy(vy); lib.lis_matrix_destroy(A)


def solve(lib, m, is_held, opts):
    csr, row, col = vc.source(m)
    A = lisdrv.make_csr(lib, *csr)                  # (-storage converts the caller's matrix for good: a fresh one per solve)
    M = A
    if is_held:
        err, M = drv.to_vbr(lib, A, row, col)
        assert err == 0
    out = lisdrv.solve(lib, M, vc.rhs(csr), opts + " " + vc.COMMON)
    assert out["err"] == 0 and M.contents.matrix_type == drv.VBR
    if is_held:
        lib.lis_matrix_destroy(M)
    lib.lis_matrix_destroy(A)
    return out


@pytest.mark.parametrize("loop", [0, UNFUSED])
@pytest.mark.parametrize("T", vc.THREADS)
@pytest.mark.parametrize("case", vc.SOLVES, ids=lambda c: "%s-%s-%s" % (c[0], "held" if c[1] else "csr", c[2]))
def test_solves_in_the_reference_order_mode_are_the_reference(lib, case, T, loop):
    """count, status, every residual and x in every bit -- from the fused loops and from the unfused ones, which therefore agree in every bit"""
    key = "%s|T%d" % (vc.solve_key(*case), T)
    with mode(lib, T), loops(lib, loop):
        out = solve(lib, *case)
    assert [out["iter"], out["status"]] == G[key + "|meta"].tolist(), (key, out["iter"], out["status"])
    want = G[key + "|rhistory"]
    assert len(out["rhistory"]) == len(want)
    diff = np.flatnonzero(out["rhistory"].view(np.int64) != want.view(np.int64))
    assert diff.size == 0, (key, "first differing history entry", int(diff[0]), out["rhistory"][diff[0]].hex(), want[diff[0]].hex())
    assert same(out["x"], G[key + "|x"]), key


@pytest.mark.parametrize("case", vc.SOLVES, ids=lambda c: "%s-%s-%s" % (c[0], "held" if c[1] else "csr", c[2]))
def test_solves_in_the_default_mode(lib, case):
    """the tree mode: the count inside the reference's own T = 1 / 8 counts widened by 1, x within 1e-8 -- fused and unfused, which agree in every bit
    on VBR storage (its product has no fused dot)"""
    counts = [int(G["%s|T%d|meta" % (vc.solve_key(*case), T)][0]) for T in vc.THREADS]
    runs = []
    for loop in (0, UNFUSED):
        with loops(lib, loop):
            out = solve(lib, *case)
        assert out["status"] == 0 and min(counts) - 1 <= out["iter"] <= max(counts) + 1, (case, loop, out["iter"], counts)
        assert np.allclose(out["x"], G["%s|T1|x" % vc.solve_key(*case)], rtol=0, atol=1e-8), (case, loop)
        runs.append(out)
    assert runs[0]["iter"] == runs[1]["iter"] and same(runs[0]["rhistory"], runs[1]["rhistory"]) and same(runs[0]["x"], runs[1]["x"])


@pytest.mark.parametrize("T", vc.THREADS)
@pytest.mark.parametrize("case", vc.ESOLVES, ids=lambda c: "%s-%s" % ("held" if c[0] else "csr", c[1]))
def test_eigensolves_in_the_reference_order_mode_are_the_reference(lib, case, T):
    is_held, opts = case
    key = "esolve|%s|%s|T%d" % ("held" if is_held else "csr", opts, T)
    csr, row, col = vc.source("sym7b")
    with mode(lib, T):
        A = lisdrv.make_csr(lib, *csr)
        M = A
        if is_held:
            err, M = drv.to_vbr(lib, A, row, col)
            assert err == 0
        if "-ss" in opts:
            res = esolve_multi_drv.esolve(lib, M, opts + " " + vc.ECOMMON)
            assert res["err"] == 0
            got = (list(res["iter"]) + [res["status"]], np.concatenate([res["evalue"], res["resid"]]), res["rhistory"], np.concatenate(res["evector"]))
            esolve_multi_drv.release(lib, res)
        else:
            res = esolve_drv.esolve(lib, M, opts + " " + vc.ECOMMON)
            assert res["err"] == 0
            got = ([res["iter"], res["status"]], np.array([res["evalue"], res["resid"]]), res["rhistory"], res["x"])
        assert M.contents.matrix_type == drv.VBR
        if is_held:
            lib.lis_matrix_destroy(M)
        lib.lis_matrix_destroy(A)
    assert [int(k) for k in got[0]] == G[key + "|meta"].tolist(), key
    assert same(got[1], G[key + "|evalue"]) and same(got[2], G[key + "|rhistory"]) and same(got[3], G[key + "|x"]), key


@pytest.mark.parametrize("is_held", [True, False])
def test_refusals_that_need_a_device(lib, is_held, capfd):
    """-p ilu and -p bjacobi look for a device before they refuse: here, with one, they say why and leave A, b and x alone"""
    csr = vc.found("mesh123s")
    n = len(csr[0]) - 1
    for p, text in (("ilu", "-p ilu is served for"), ("bjacobi", "-p bjacobi on VBR storage is not served")):
        A = held(lib, "mesh123s") if is_held else lisdrv.make_csr(lib, *csr)
        before = drv.arrays(A)
        b, x = lisdrv.new_vector(lib, A, np.ones(n)), lisdrv.new_vector(lib, A, np.full(n, 3.0))
        S = capi.PS()
        assert lib.lis_solver_create(C.byref(S)) == 0 and lib.lis_solver_set_option(("-i cg -p %s%s" % (p, "" if is_held else " -storage vbr")).encode(), S) == 0
        capfd.readouterr()
        assert lib.lis_solve(A, b, x, S) == NOT_IMPLEMENTED
        out = capfd.readouterr().out
        assert text in out and "A is untouched" in out, out
        now = drv.arrays(A)
        assert now["type"] == before["type"] and same(now["value"], before["value"]) and not A.contents.is_splited
        assert same(lisdrv.get_vector(lib, b), np.ones(n)) and same(lisdrv.get_vector(lib, x), np.full(n, 3.0))
        lib.lis_solver_destroy(S); lib.lis_vector_destroy(b); lib.lis_vector_destroy(x); lib.lis_matrix_destroy(A)
