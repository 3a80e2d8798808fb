"""kernels/convert.hip and lisd_convert_csr (host/lis_convert_hbm.c), entry by entry and through lis_matrix_convert, on the matrices of
tests/convert_cases.py: rows out of order and with repeated columns, block rows of exactly 96 and 97 distinct blocks, non-square
blocks and every kind of padding, empty rows, one-row matrices, the borders of the scan (the 1026-tile one included), -0.0 / NaN /
inf / subnormal values, the row forms of constant-coefficient matrices, matrices born in HBM.

Expected arrays are the plain-C oracle's (convert_cases.oracle_arrays; tests/test_convert_cpu.py holds them to the reference on these
matrices), the row forms are the restatements of convert_cases (held there to the oracle's native products).  Every comparison is
integer equality or equality of every bit; there is no tolerance in this file.  Every API-level test asserts WHICH path ran
(lis_amd_matrix_lazy_arrays before the first read: 2 / 3 arrays still in HBM only = built there, 0 = the host routine), so that a quiet
hand-over to the host cannot hide a kernel.

The 1026-tile scan case (4.2 M rows) runs where its size matters: 1 x 1 blocks (bptr is the exclusive scan of the row lengths: 1026
tiles) and DIA (2052 tiles over the offsets, 1026 over the row counts); larger blocks see fewer tiles than the small cases cover."""
import ctypes as C
import time

import numpy as np
import pytest

import convert_cases as cc
import lis_amd
import lisdrv
import orc
from lis_amd import DeviceArray as DA, check
from lis_amd import _capi as capi

pytestmark = pytest.mark.gpu

LISHIP_ERR_ARG = -1
I32, F64 = np.int32, np.float64
SMALL = list(cc.CASES)


@pytest.fixture(scope="module")
def lib():
    if not lis_amd.gpu_available():
        pytest.fail("no HIP device: these tests need the MI355X")
    lib = lis_amd.load()
    assert lib.initialize([]) == 0
    check(lib.liship_set_device(0))
    dll = lib.dll
    for f in (dll.lis_amd_matrix_lazy_arrays, dll.lis_amd_matrix_value_records, dll.lis_amd_matrix_device_type):
        f.argtypes = [capi.PM]
    dll.lis_amd_matrix_poisson3d.argtypes = [capi.PM, C.c_int, C.c_int, C.c_int, C.c_int]
    dll.lis_amd_matrix_set_csr_device.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, capi.PM]
    dll.lis_amd_set_device_convert(1)
    return lib


@pytest.fixture(scope="module")
def big():
    """scan(1025 * 4096 + 7) and its device arrays, made when first asked for and released with the module"""
    keep = {}
    yield keep
    for d in keep.pop("dev", ()):
        d.free()
    keep.clear()


def big_csr(big):
    if "csr" not in big:
        big["csr"] = cc.scan(cc.SCAN_BIG)
        big["dev"] = tuple(DA.from_host(a, t) for a, t in zip(big["csr"], (I32, I32, F64)))
    return big["csr"], big["dev"]


def csr_of(name):
    return cc.CASES[name]


def dev_csr(name):
    ptr, idx, val = cc.CASES[name]
    return DA.from_host(ptr, I32), DA.from_host(idx, I32), DA.from_host(val, F64)


def ints(a, b):
    return np.array_equal(a, b)


# ================================================================ kernel level
@pytest.mark.parametrize("case", cc.EDGES + ["empties", "unsorted", "duplicates"])
def test_csr_row_facts(lib, case):
    ptr, idx, val = csr_of(case)
    n = len(ptr) - 1
    dptr, didx, _ = dev_csr(case)
    facts = DA.from_host(np.array([7, 7, 7, 7], I32), I32)
    want = [cc.max_row(ptr), cc.is_unsorted(ptr, idx)]
    for _ in range(2):
        check(lib.liship_csr_row_facts(n, dptr.ptr, didx.ptr, facts.ptr, None))
        got = facts.to_host()
        assert got[:2].tolist() == want and got[2] == got[3] and got[2] in (7, -12345), (got, want)      # [longest row, out of order?], nothing behind them
        facts.upload(np.array([-12345, 99, -12345, -12345], I32))                         # garbage: the entry zeroes what it accumulates into
    if case == "equal_neighbours":
        assert want[1] == 0 and cc.repeats_a_column(ptr, idx)                             # equal neighbours are in order
    if case == "n513_inversion_last":
        assert want[1] == 1


@pytest.mark.parametrize("case", cc.EDGES + ["empties", "unsorted", "specials"])
def test_csr_to_ell_and_its_row_form(lib, case):
    ptr, idx, val = csr_of(case)
    n = len(ptr) - 1
    mx, eidx, ev = orc.csr2ell(ptr, idx, val)
    rptr, ridx, rval = cc.ell_rows(n, mx, eidx, ev)
    dptr, didx, dval = dev_csr(case)
    oi, ov = DA(n * mx, I32), DA(n * mx, F64)
    qp, qi, qv = DA(n + 1, I32), DA(n * mx, I32), DA(n * mx, F64)
    for _ in range(2):
        check(lib.liship_csr_to_ell(n, mx, dptr.ptr, didx.ptr, dval.ptr, oi.ptr, ov.ptr, None))
        check(lib.liship_csr_to_ell_rows(n, mx, dptr.ptr, didx.ptr, dval.ptr, qp.ptr, qi.ptr, qv.ptr, None))
        assert ints(oi.to_host(), eidx) and cc.same_bits(ov.to_host(), ev)
        assert ints(qp.to_host(), rptr) and ints(qi.to_host(), ridx) and cc.same_bits(qv.to_host(), rval)
    if case == "empties":                                             # row 0 is all padding: +0.0 on its own column
        assert ints(oi.to_host().reshape(mx, n)[:, 0], np.zeros(mx, I32)) and ints(ov.to_host().reshape(mx, n)[:, 0].view(np.uint64), np.zeros(mx, np.uint64))


@pytest.mark.parametrize("case", cc.SORTED + ["scan_big"])
def test_csr_to_dia_and_its_row_form(lib, big, case):
    """offsets, then values, then the row form.  Rows in ascending order; where a row repeats a column (equal_neighbours) the last stored entry wins"""
    t0 = time.time()
    (ptr, idx, val), (dptr, didx, dval) = big_csr(big) if case == "scan_big" else (csr_of(case), dev_csr(case))
    n = len(ptr) - 1
    nnd, off, dv = orc.csr2dia(ptr, idx, val)
    span = 2 * n
    used, slot, scratch = DA(span, I32), DA(span + 1, I32), DA(span // 4096 + 4, np.int64)
    got_nnd, got_rnnz = C.c_int(-7), C.c_int(-7)
    offs, out = DA(max(nnd, 1), I32), DA(max(n * nnd, 1), F64)
    if nnd:
        rptr, ridx, rval = cc.dia_rows(n, n, off, dv)
        count, qp, qi, qv = DA(n, I32), DA(n + 1, I32), DA(max(len(ridx), 1), I32), DA(max(len(ridx), 1), F64)
    for _ in range(2):
        check(lib.liship_csr_dia_offsets(n, n, dptr.ptr, didx.ptr, used.ptr, slot.ptr, scratch.ptr, C.byref(got_nnd), None))
        assert got_nnd.value == nnd
        if nnd == 0:
            continue
        check(lib.liship_csr_to_dia(n, n, nnd, dptr.ptr, didx.ptr, dval.ptr, used.ptr, slot.ptr, offs.ptr, out.ptr, None))
        got_off, got = offs.to_host(), out.to_host()
        assert ints(got_off, off) and np.all(np.diff(got_off) > 0)
        assert cc.same_bits(got, dv)                                  # +0.0 where a diagonal has no entry, -0.0 where the matrix says so
        check(lib.liship_dia_row_counts(n, n, nnd, offs.ptr, count.ptr, qp.ptr, scratch.ptr, C.byref(got_rnnz), None))
        assert got_rnnz.value == rptr[n] == len(ridx)
        check(lib.liship_dia_to_rows(n, n, nnd, offs.ptr, out.ptr, qp.ptr, qi.ptr, qv.ptr, None))
        assert ints(qp.to_host(), rptr) and ints(qi.to_host(len(ridx)), ridx) and cc.same_bits(qv.to_host(len(ridx)), rval)
    if case == "scan_big":
        print("scan_big DIA: %.2f s" % (time.time() - t0))


def _bsr_on_device(lib, name, csr, dev, bnr, bnc):
    """count, then fill, twice; returns (bnnz, bptr, bindex, value) of the second round"""
    ptr, idx, val = csr
    n = len(ptr) - 1
    nr = 1 + (n - 1) // bnr
    dptr, didx, dval = dev
    count, bptr, scratch = DA(nr + 1, I32), DA(nr + 1, I32), DA(nr // 4096 + 4, np.int64)
    out = None
    for _ in range(2):
        bnnz = C.c_int(-7)
        check(lib.liship_csr_bsr_count(n, n, bnr, bnc, dptr.ptr, didx.ptr, count.ptr, bptr.ptr, scratch.ptr, C.byref(bnnz), None))
        if bnnz.value <= 0:
            now = (bnnz.value, bptr.to_host(), None, None)
        else:
            bi, bv = DA(bnnz.value, I32), DA(bnnz.value * bnr * bnc, F64)
            check(lib.liship_csr_to_bsr(n, bnr, bnc, bnnz.value, dptr.ptr, didx.ptr, dval.ptr, bptr.ptr, bi.ptr, bv.ptr, None))
            now = (bnnz.value, bptr.to_host(), bi.to_host(), bv.to_host())
        if out is not None:
            assert out[0] == now[0] and ints(out[1], now[1]) and (now[2] is None or (ints(out[2], now[2]) and cc.same_bits(out[3], now[3])))
        out = now
    return out


@pytest.mark.parametrize("bnr,bnc", cc.BLOCKS, ids=["%dx%d" % b for b in cc.BLOCKS])
@pytest.mark.parametrize("case", SMALL)
def test_csr_to_bsr(lib, case, bnr, bnc):
    csr = csr_of(case)
    nr, bptr, bidx, bval = orc.csr2bsr(*csr, bnr, bnc)
    bnnz, gp, gi, gv = _bsr_on_device(lib, case, csr, dev_csr(case), bnr, bnc)
    assert bnnz == len(bidx) and ints(gp, bptr)
    if bnnz:
        assert ints(gi, bidx) and cc.same_bits(gv, bval)
    if (bnr, bnc) == (1, 1) and case.startswith("scan_"):
        assert ints(gp, csr[0])                                       # the plain exclusive scan of the row lengths


def test_exclusive_scan_over_1026_tiles(lib, big):
    """1 x 1 blocks on scan(1025 * 4096 + 7): bptr is the exclusive scan of 4.2 M row lengths -- 1026 tiles, so every lane of
    scan_tile_offsets but the last ones takes two tiles, the last share is uneven and the last tile ragged"""
    t0 = time.time()
    csr, dev = big_csr(big)
    bnnz, gp, gi, gv = _bsr_on_device(lib, "scan_big", csr, dev, 1, 1)
    assert bnnz == len(csr[1]) and ints(gp, csr[0])                   # row lengths 0, 1, 2, ...: the scan IS ptr
    assert ints(gi, csr[1]) and cc.same_bits(gv, csr[2])              # ... and 1 x 1 blocks in first-seen order are the entries
    print("scan_big BSR 1x1: %.2f s" % (time.time() - t0))


@pytest.mark.parametrize("sorted_", [True, False], ids=["sorted", "unsorted"])
@pytest.mark.parametrize("bnr,bnc", cc.HUB_SHAPES, ids=["%dx%d" % b for b in cc.HUB_SHAPES])
def test_bsr_list_border(lib, bnr, bnc, sorted_):
    """a block row of exactly BSR_LIST distinct blocks converts in HBM; one more raises the overflow flag: *bnnz = -1"""
    for blocks in (cc.BSR_LIST, cc.BSR_LIST + 1):
        csr, br = cc.hub(cc.HUB_N, blocks, bnr, bnc, sorted_)
        assert cc.distinct_blocks(csr[0], csr[1], cc.HUB_N, bnr, bnc, br) == blocks
        dev = tuple(DA.from_host(a, t) for a, t in zip(csr, (I32, I32, F64)))
        bnnz, gp, gi, gv = _bsr_on_device(lib, "hub", csr, dev, bnr, bnc)
        if blocks > cc.BSR_LIST:
            assert bnnz == -1
            continue
        nr, bptr, bidx, bval = orc.csr2bsr(*csr, bnr, bnc)
        assert bnnz == len(bidx) and ints(gp, bptr) and ints(gi, bidx) and cc.same_bits(gv, bval)
        assert gp[br + 1] - gp[br] == cc.BSR_LIST


@pytest.mark.parametrize("case", ["unsorted", "empties"] + cc.EDGES)
def test_csr_to_jad(lib, case):
    ptr, idx, val = csr_of(case)
    n, nnz = len(ptr) - 1, len(idx)
    mx, perm, jptr, jidx, jval = orc.csr2jad(ptr, idx, val)         # the row order is host-made by design: perm and jptr go in
    dptr, didx, dval = dev_csr(case)
    dperm, djptr = DA.from_host(perm, I32), DA.from_host(jptr, I32)
    oi, ov = DA(nnz, I32), DA(nnz, F64)
    for _ in range(2):
        check(lib.liship_csr_to_jad(n, dperm.ptr, djptr.ptr, dptr.ptr, didx.ptr, dval.ptr, oi.ptr, ov.ptr, None))
        assert ints(oi.to_host(), jidx) and cc.same_bits(ov.to_host(), jval)


@pytest.mark.parametrize("bnr,bnc", cc.BLOCKS, ids=["%dx%d" % b for b in cc.BLOCKS])
@pytest.mark.parametrize("case", SMALL)
def test_bsr_to_rows(lib, case, bnr, bnc):
    """on the oracle's BSR arrays: non-square blocks, a padded last block row (rptr[n] leaves its padding rows out), blocks larger than n"""
    ptr, idx, val = csr_of(case)
    n = len(ptr) - 1
    nr, bptr, bidx, bval = orc.csr2bsr(ptr, idx, val, bnr, bnc)
    rptr, ridx, rval = cc.bsr_rows(n, bnr, bnc, bptr, bidx, bval)
    assert len(ridx) <= len(bval)
    dp, di, dv = DA.from_host(bptr, I32), DA.from_host(bidx, I32), DA.from_host(bval, F64)
    qp, qi, qv = DA(n + 1, I32), DA(max(len(bval), 1), I32), DA(max(len(bval), 1), F64)
    for _ in range(2):
        check(lib.liship_bsr_to_rows(n, bnr, bnc, dp.ptr, di.ptr, dv.ptr, qp.ptr, qi.ptr, qv.ptr, None))
        assert ints(qp.to_host(), rptr) and ints(qi.to_host(len(ridx)), ridx) and cc.same_bits(qv.to_host(len(ridx)), rval)


def test_bsr_to_rows_refuses_bad_sizes(lib):
    a = DA.zeros(8, I32)
    v = DA.zeros(8, F64)
    for n, bnr, bnc in ((0, 2, 2), (-1, 2, 2), (4, 0, 2), (4, -1, 2), (4, 2, 0)):
        assert lib.liship_bsr_to_rows(n, bnr, bnc, a.ptr, a.ptr, v.ptr, a.ptr, a.ptr, v.ptr, None) == LISHIP_ERR_ARG


# ================================================================ API level
DEVICE, HOST = {"ell": 2, "dia": 2, "jad": 2, "csc": 3, "bsr": 3}, 0


def _x(n, seed=3):
    return np.random.default_rng(seed).uniform(-1, 1, n)


def _convert_checked(lib, A, csr, fmt, bnr, bnc, path, loose=False):
    """A -> fmt; asserts the path before anything reads an array, then products and arrays against the oracle.  Returns the new matrix."""
    n = len(csr[0]) - 1
    x = _x(n)
    B = lisdrv.convert(lib, A, fmt, bnr or 2, bnc or 2)
    lazy = lib.dll.lis_amd_matrix_lazy_arrays(B)
    assert lazy == (DEVICE[fmt] if path == "device" else HOST), (fmt, path, lazy)
    y, yt = cc.oracle_products(fmt, *csr, x, bnr or 2, bnc or 2)
    assert cc.same_bits(lisdrv.matvec(lib, B, x), y, loose), (fmt, "matvec")
    if path == "device":
        assert lib.dll.lis_amd_matrix_lazy_arrays(B) == lazy         # a product asks for no host array
    assert cc.same_bits(lisdrv.matvech(lib, B, x), yt, loose), (fmt, "matvech")
    ok, key = cc.same_arrays(lisdrv.matrix_arrays(B), cc.oracle_arrays(fmt, *csr, bnr or 2, bnc or 2))
    assert ok, (fmt, bnr, bnc, key)
    assert lib.dll.lis_amd_matrix_lazy_arrays(B) == 0
    assert cc.same_bits(lisdrv.matvec(lib, B, x), y, loose)          # ... and the HBM copy still serves
    return B


def _resident(lib, csr):
    A = lisdrv.make_csr(lib, *csr)
    lisdrv.matvec(lib, A, _x(len(csr[0]) - 1))                       # A's HBM copy exists
    return A


ALL = [("ell", 0, 0), ("dia", 0, 0), ("csc", 0, 0), ("jad", 0, 0), ("bsr", 2, 2), ("bsr", 3, 2)]
# what lisd_convert_csr hands to the host routine, and why
HOST_CASES = [("unsorted", "dia", 0, 0, "rows out of order: csr2dia sorts its input first"),
              ("unsorted", "csc", 0, 0, "rows out of order: the product's row order is the ascending one"),
              ("duplicates", "dia", 0, 0, "rows out of order"), ("duplicates", "csc", 0, 0, "rows out of order"),
              ("n513_inversion_last", "dia", 0, 0, "one inversion, in the last row"), ("n513_inversion_last", "csc", 0, 0, "one inversion, in the last row")]
DEVICE_CASES = [(c, f, r, k) for c in ("unsorted", "duplicates") for f, r, k in ALL if f in ("ell", "bsr", "jad")]
DEVICE_CASES += [(c, f, r, k) for c in ["empties", "specials"] + cc.EDGES for f, r, k in ALL if (c, f, r, k) not in [h[:4] for h in HOST_CASES]]


def _id(t):
    return "%s-%s%s" % (t[0], t[1], "%dx%d" % t[2:4] if t[1] == "bsr" else "")


@pytest.mark.parametrize("case,fmt,bnr,bnc", DEVICE_CASES, ids=[_id(t) for t in DEVICE_CASES])
def test_convert_in_hbm(lib, case, fmt, bnr, bnc):
    csr = csr_of(case)
    A = _resident(lib, csr)
    B = _convert_checked(lib, A, csr, fmt, bnr, bnc, "device", loose=case == "specials")
    lib.lis_matrix_destroy(B); lib.lis_matrix_destroy(A)


@pytest.mark.parametrize("bnr,bnc", cc.BLOCKS, ids=["%dx%d" % b for b in cc.BLOCKS])
def test_convert_in_hbm_every_block_shape_pads(lib, bnr, bnc):
    csr = orc.random_csr(601, 7, seed=9)                              # 601 is prime: every shape pads its last block row and column
    A = _resident(lib, csr)
    B = _convert_checked(lib, A, csr, "bsr", bnr, bnc, "device")
    lib.lis_matrix_destroy(B); lib.lis_matrix_destroy(A)


def _after_a_host_conversion(lib, A, before, x):
    """the source still multiplies (csr2dia may have sorted its rows in place, as the reference does: then as its arrays now say), and a
    conversion to ELL takes the device path again and is right"""
    now = lisdrv.matrix_arrays(A)
    now = (now["ptr"], now["index"], now["value"])
    assert cc.same_bits(lisdrv.matvec(lib, A, x), orc.spmv_csr(*now, x))
    E = _convert_checked(lib, A, now, "ell", 0, 0, "device")
    lib.lis_matrix_destroy(E)
    return now


@pytest.mark.parametrize("case,fmt,bnr,bnc,why", HOST_CASES, ids=[_id(t) for t in HOST_CASES])
def test_hand_over_to_the_host_routine(lib, case, fmt, bnr, bnc, why):
    csr = csr_of(case)
    n = len(csr[0]) - 1
    x = _x(n, 5)
    A = _resident(lib, csr)
    y0 = lisdrv.matvec(lib, A, x)
    assert cc.same_bits(y0, orc.spmv_csr(*csr, x))
    B = _convert_checked(lib, A, csr, fmt, bnr, bnc, "host")
    now = _after_a_host_conversion(lib, A, csr, x)
    if fmt == "dia":                                                  # sorted in place, as the reference sorts its input; equal columns keep their order
        sidx, sval = orc.sort_rows(*csr)
        assert ints(now[1], sidx) and cc.same_bits(now[2], sval)
    else:
        assert ints(now[1], csr[1]) and cc.same_bits(now[2], csr[2]) and cc.same_bits(lisdrv.matvec(lib, A, x), y0)
    lib.lis_matrix_destroy(B); lib.lis_matrix_destroy(A)


@pytest.mark.parametrize("sorted_", [True, False], ids=["sorted", "unsorted"])
@pytest.mark.parametrize("bnr,bnc", cc.HUB_SHAPES, ids=["%dx%d" % b for b in cc.HUB_SHAPES])
def test_bsr_list_border_through_the_api(lib, bnr, bnc, sorted_):
    """96 distinct blocks in a block row: built in HBM; 97: the host routine"""
    for blocks, path in ((cc.BSR_LIST, "device"), (cc.BSR_LIST + 1, "host")):
        csr, br = cc.hub(cc.HUB_N, blocks, bnr, bnc, sorted_)
        x = _x(cc.HUB_N, 5)
        A = _resident(lib, csr)
        y0 = lisdrv.matvec(lib, A, x)
        B = _convert_checked(lib, A, csr, "bsr", bnr, bnc, path)
        if path == "host":
            now = _after_a_host_conversion(lib, A, csr, x)
            assert ints(now[1], csr[1]) and cc.same_bits(lisdrv.matvec(lib, A, x), y0)
        lib.lis_matrix_destroy(B); lib.lis_matrix_destroy(A)


def _born_in_hbm(lib, kind):
    if kind == "poisson3d":
        l, m, n = 6, 5, 4
        csr = orc.poisson3d(l, m, n, sort_cols=True)
        A = capi.PM()
        assert lib.lis_matrix_create(capi.LIS_COMM_WORLD, C.byref(A)) == 0 and lib.lis_matrix_set_size(A, 0, l * m * n) == 0
        assert lib.dll.lis_amd_matrix_poisson3d(A, l, m, n, 1) == 0
        return A, csr
    csr = csr_of("unsorted")
    n = len(csr[0]) - 1
    dev = [DA.from_host(a, t) for a, t in zip(csr, (I32, I32, F64))]
    A = capi.PM()
    assert lib.lis_matrix_create(capi.LIS_COMM_WORLD, C.byref(A)) == 0 and lib.lis_matrix_set_size(A, n, 0) == 0
    assert lib.dll.lis_amd_matrix_set_csr_device(len(csr[1]), n, dev[0].ptr, dev[1].ptr, dev[2].ptr, A) == 0
    for d in dev:
        d.ptr = None                                                  # owned by A now
    return A, csr


BORN = [("poisson3d", f, r, k, "device") for f, r, k in [("ell", 0, 0), ("dia", 0, 0), ("csc", 0, 0), ("bsr", 2, 2), ("bsr", 2, 3)]]
BORN += [("set_csr_device", f, r, k, "device") for f, r, k in [("ell", 0, 0), ("bsr", 2, 2), ("bsr", 2, 3)]]
BORN += [("poisson3d", "jad", 0, 0, "host"), ("set_csr_device", "jad", 0, 0, "host"),          # JAD's row order is the reference's sort, made on host arrays
         ("set_csr_device", "dia", 0, 0, "host"), ("set_csr_device", "csc", 0, 0, "host")]     # rows out of order


@pytest.mark.parametrize("kind,fmt,bnr,bnc,path", BORN, ids=["%s-%s" % (_id(t), t[4]) for t in BORN])
def test_matrices_born_in_hbm(lib, kind, fmt, bnr, bnc, path):
    """no host arrays behind the source: ELL, DIA, CSC and BSR are built in HBM; JAD, and DIA / CSC of rows out of order, run the host routine on a copy brought home"""
    A, csr = _born_in_hbm(lib, kind)
    x = _x(len(csr[0]) - 1, 5)
    y0 = lisdrv.matvec(lib, A, x)
    assert cc.same_bits(y0, orc.spmv_csr(*csr, x))
    B = _convert_checked(lib, A, csr, fmt, bnr, bnc, path)
    assert cc.same_bits(lisdrv.matvec(lib, A, x), y0)                 # the source is untouched, whoever converted
    if path == "host":
        E = _convert_checked(lib, A, csr, "ell", 0, 0, "device")
        lib.lis_matrix_destroy(E)
    lib.lis_matrix_destroy(B); lib.lis_matrix_destroy(A)


@pytest.mark.parametrize("fmt,bnr,bnc", [("ell", 0, 0), ("dia", 0, 0), ("bsr", 2, 2)], ids=["ell", "dia", "bsr2x2"])
@pytest.mark.parametrize("case", ["constant_p3d", "constant_band"])
def test_row_forms_of_constant_matrices(lib, case, fmt, bnr, bnc):
    """constant coefficients: the HBM copy is the row form with value records (built by csr_to_ell_rows / dia_to_rows / bsr_to_rows), the
    product keeps the native format's bits, and the host arrays that come home are the native ones.  lis_amd_matrix_value_records answers 1
    for ELL and DIA (rows of up to 7 terms) and 2, the wide records of lis_amd.h, for the 2 x 2 blocking, whose rows list 8 terms or more"""
    csr = csr_of(case)
    assert (len(csr[0]) - 1) % 2 == 0
    records = 2 if fmt == "bsr" else 1
    A = _resident(lib, csr)
    B = lisdrv.convert(lib, A, fmt, bnr or 2, bnc or 2)
    assert lib.dll.lis_amd_matrix_value_records(B) == records and lib.dll.lis_amd_matrix_device_type(B) == capi.LIS_MATRIX_CSR
    lib.lis_matrix_destroy(B)
    B = _convert_checked(lib, A, csr, fmt, bnr, bnc, "device")
    assert lib.dll.lis_amd_matrix_value_records(B) == records
    lib.lis_matrix_destroy(B); lib.lis_matrix_destroy(A)


@pytest.mark.parametrize("fmt,bnr,bnc", [("ell", 0, 0), ("dia", 0, 0), ("bsr", 2, 2)], ids=["ell", "dia", "bsr2x2"])
@pytest.mark.parametrize("case", ["constant_p3d", "scan_4096"])
def test_both_paths_decide_alike(lib, case, fmt, bnr, bnc):
    """the conversion in HBM and the host routine followed by the upload (LIS_AMD_NO_DEVICE_CONVERT) give the new matrix the same HBM copy: the same kernel
    family, the same value records, the same bits in the product -- constant coefficients (the row form) and values that all differ (the native arrays)"""
    csr = csr_of(case)
    x = _x(len(csr[0]) - 1, 7)
    A = _resident(lib, csr)
    B = lisdrv.convert(lib, A, fmt, bnr or 2, bnc or 2)
    assert lib.dll.lis_amd_matrix_lazy_arrays(B) == DEVICE[fmt]
    lib.dll.lis_amd_set_device_convert(0)
    try:
        H = lisdrv.convert(lib, A, fmt, bnr or 2, bnc or 2)
    finally:
        lib.dll.lis_amd_set_device_convert(1)
    assert lib.dll.lis_amd_matrix_lazy_arrays(H) == HOST
    decided = [(lib.dll.lis_amd_matrix_device_type(M), lib.dll.lis_amd_matrix_value_records(M)) for M in (B, H)]
    assert decided[0] == decided[1], decided
    assert decided[0][0] == (capi.LIS_MATRIX_CSR if case == "constant_p3d" else getattr(capi, "LIS_MATRIX_" + fmt.upper()))
    assert cc.same_bits(lisdrv.matvec(lib, B, x), lisdrv.matvec(lib, H, x))
    lib.lis_matrix_destroy(B); lib.lis_matrix_destroy(H); lib.lis_matrix_destroy(A)
