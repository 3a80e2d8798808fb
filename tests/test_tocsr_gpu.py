"""X -> CSR in HBM: the count and fill kernels of kernels/convert.hip entry by entry, and lis_matrix_convert through lisd_convert_to_csr
(host/lis_convert_tocsr.c), against the numpy models of tests/tocsr_cases.py, which tests/test_tocsr_cpu.py holds to the reference.  Every comparison is integer
equality or equality of every bit; there is no tolerance in this file (a product of a matrix that stores NaN is NaN in the same places, any payload).

Kernel level: n at 1, around the rows of a workgroup and just past a scan tile, widths 1, 2, 7, 33, np around the DNS slab; guard words behind every output; a
second call over outputs filled with garbage.  API level: every source of tocsr_cases in every state its arrays can be in -- made in HBM and still lazy, at home
with a native copy, at home with a row-form copy, at home with no copy -- asserting WHICH path ran (lis_amd_convert_stats, lis_amd_matrix_lazy_arrays) so that a
quiet hand-over to the host cannot hide a kernel."""
import ctypes as C

import numpy as np
import pytest

import convert_cases as cc
import coo_dns_cases as dc
import coo_dns_drv
import lis_amd
import lisdrv
import orc
import shift_model as sm
import tocsr_cases as tc
import tocsr_drv as drv
from lis_amd import DeviceArray as DA, _capi as capi, check

pytestmark = pytest.mark.gpu
I32, F64 = np.int32, np.float64
ERR_ARG = -1
GUARD = 8
GUARD_INT, GARBAGE_INT = -1234567, 0x5A5A5A5A
_info = (C.c_int * 3)()
check(lis_amd.load().liship_tocsr_tile_info(_info))          # (a host-side entry: no device is touched while the tests are collected)
ROWS, SLAB, SCAN = list(_info)            # rows per workgroup, columns per DNS slab, counts per scan tile: the sweeps below move with them


@pytest.fixture(scope="module")
def lib():
    lib = lis_amd.load()
    assert lis_amd.gpu_available(), "no HIP device: these tests need the MI355X"
    assert lib.initialize([]) == 0
    check(lib.liship_set_device(0))
    for f in (lib.dll.lis_amd_matrix_lazy_arrays, lib.dll.lis_amd_matrix_device_type, lib.dll.lis_amd_matrix_upload, lib.dll.lis_amd_matrix_host_modified,
              lib.dll.lis_amd_matrix_protected_arrays):
        f.argtypes = [capi.PM]
    lib.dll.lis_amd_set_device_convert(1)
    A = lisdrv.make_csr(lib, *cc.CASES["n7_full_row"])               # the device is up before the first conversion: the gates ask for that
    lisdrv.matvec(lib, A, np.ones(7))
    lib.lis_matrix_destroy(A)
    return lib


# ================================================================ kernel level
class Guarded:
    """an output of `count` elements in HBM with GUARD more behind it"""

    def __init__(self, count, dtype):
        self.count, self.dtype = count, np.dtype(dtype)
        self.d = DA(count + GUARD, dtype)
        self.fill(GUARD_INT)

    def fill(self, word):
        self.pattern = np.full(self.count + GUARD, word, I32 if self.dtype == I32 else np.int64).view(self.dtype)      # (as a double: 64 bits that no copy of a source value gives)
        self.d.upload(self.pattern)

    def get(self, what):
        host = self.d.to_host()
        assert host[self.count:].tobytes() == self.pattern[self.count:].tobytes(), (what, "guard words written")
        return host[:self.count]

    @property
    def ptr(self):
        return self.d.ptr


def _dev(a, t):
    a = np.ascontiguousarray(a, t)
    return DA.from_host(a if a.size else np.zeros(1, t), t)


def run_kernels(lib, s, passes=2):
    """the count entry and the fill entry of s's format on device arrays, `passes` times over outputs prefilled with a different word each time; every pass is
    held to the model"""
    fmt, n = s["fmt"], s["n"]
    want = tc.model(s)
    nnz = len(want[1])
    keep = {k: _dev(v, v.dtype) for k, v in s.items() if isinstance(v, np.ndarray)}
    p = {k: d.ptr for k, d in keep.items()}
    cells = n
    if fmt == "dns":
        nslab = (s["np"] + SLAB - 1) // SLAB
        cells = n * nslab
        offsets = Guarded(cells + 1, I32)
    if fmt == "vbr":
        flags = C.c_int(-1)
        check(lib.liship_vbr_check(n, n, s["nnz"], s["nr"], s["nc"], s["bnnz"], p["row"], p["col"], p["ptr"], p["bptr"], p["bindex"], C.byref(flags), None))
        assert flags.value == 0
        brow = DA(n + 4, I32)
        check(lib.liship_vbr_block_rows(n, s["nr"], p["row"], brow.ptr, None))
    count, rptr, scratch = Guarded(cells, I32), Guarded(n + 1, I32), DA(cells // 4096 + 4, np.int64)
    ridx, rval = Guarded(nnz, I32), Guarded(nnz, F64)
    for word in (GUARD_INT, GARBAGE_INT)[:passes]:
        for g in (count, rptr, ridx, rval) + ((offsets,) if fmt == "dns" else ()):
            g.fill(word)
        got = C.c_int(-7)
        tail = (count.ptr, rptr.ptr, scratch.ptr, C.byref(got), None)
        if fmt == "ell":
            check(lib.liship_ell_csr_count(n, s["maxnzr"], p["value"], *tail))
        elif fmt == "dia":
            check(lib.liship_dia_csr_count(n, s.get("np", n), s["nnd"], p["index"], p["value"], *tail))
        elif fmt == "bsr":
            check(lib.liship_bsr_csr_count(n, s["bnr"], s["bnc"], p["bptr"], p["bindex"], p["value"], *tail))
        elif fmt == "dns":
            check(lib.liship_dns_csr_count(n, s["np"], p["value"], count.ptr, offsets.ptr, rptr.ptr, scratch.ptr, C.byref(got), None))
        else:
            check(lib.liship_vbr_csr_count(n, p["row"], p["col"], p["ptr"], p["bptr"], p["bindex"], brow.ptr, p["value"], *tail))
        what = (fmt, n, hex(word & 0xFFFFFFFF))
        assert got.value == nnz, what
        if fmt == "dns":
            c = tc.dns_slab_counts(s, SLAB)
            assert np.array_equal(count.get(what), c), what
            assert np.array_equal(offsets.get(what), np.concatenate([[0], np.cumsum(c)])), what
        else:
            assert np.array_equal(count.get(what), tc.counts(s)), what
        assert np.array_equal(rptr.get(what), want[0]), what
        if fmt == "ell":
            check(lib.liship_ell_to_csr(n, s["maxnzr"], p["index"], p["value"], rptr.ptr, ridx.ptr, rval.ptr, None))
        elif fmt == "dia":
            check(lib.liship_dia_to_csr(n, s.get("np", n), s["nnd"], p["index"], p["value"], rptr.ptr, ridx.ptr, rval.ptr, None))
        elif fmt == "bsr":
            check(lib.liship_bsr_to_csr(n, s["bnr"], s["bnc"], p["bptr"], p["bindex"], p["value"], rptr.ptr, ridx.ptr, rval.ptr, None))
        elif fmt == "dns":
            check(lib.liship_dns_to_csr(n, s["np"], p["value"], offsets.ptr, ridx.ptr, rval.ptr, None))
        else:
            check(lib.liship_vbr_to_csr(n, p["row"], p["col"], p["ptr"], p["bptr"], p["bindex"], brow.ptr, p["value"], rptr.ptr, ridx.ptr, rval.ptr, None))
        check(lib.liship_device_synchronize())
        assert np.array_equal(ridx.get(what), want[1]), what
        assert cc.same_bits(rval.get(what), want[2]), what
    del keep


def test_tile_info(lib):
    info = (C.c_int * 3)()
    check(lib.liship_tocsr_tile_info(info))
    assert list(info) == [ROWS, SLAB, SCAN] and min(info) >= 2 and ROWS < SCAN
    assert lib.liship_tocsr_tile_info(None) == ERR_ARG


def test_entry_points_refuse_what_they_cannot_serve(lib):
    a = DA(8, I32)
    v = DA(8, F64)
    n = C.c_int(0)
    assert lib.liship_ell_csr_count(0, 1, v.ptr, a.ptr, a.ptr, a.ptr, C.byref(n), None) == ERR_ARG
    assert lib.liship_ell_csr_count(1, 1, None, a.ptr, a.ptr, a.ptr, C.byref(n), None) == ERR_ARG
    assert lib.liship_ell_to_csr(1, -1, a.ptr, v.ptr, a.ptr, a.ptr, v.ptr, None) == ERR_ARG
    assert lib.liship_dia_csr_count(1, 0, 1, a.ptr, v.ptr, a.ptr, a.ptr, a.ptr, C.byref(n), None) == ERR_ARG
    assert lib.liship_dia_to_csr(1, 1, 1, None, v.ptr, a.ptr, a.ptr, v.ptr, None) == ERR_ARG
    assert lib.liship_bsr_csr_count(4, 0, 2, a.ptr, a.ptr, v.ptr, a.ptr, a.ptr, a.ptr, C.byref(n), None) == ERR_ARG
    assert lib.liship_bsr_to_csr(4, 2, 0, a.ptr, a.ptr, v.ptr, a.ptr, a.ptr, v.ptr, None) == ERR_ARG
    assert lib.liship_dns_csr_count(1, 0, v.ptr, a.ptr, a.ptr, a.ptr, a.ptr, C.byref(n), None) == ERR_ARG
    assert lib.liship_dns_csr_count(1, 65536 * SLAB, v.ptr, a.ptr, a.ptr, a.ptr, a.ptr, C.byref(n), None) == ERR_ARG        # more slabs than a grid has rows
    assert lib.liship_dns_to_csr(0, 1, v.ptr, a.ptr, a.ptr, v.ptr, None) == ERR_ARG
    assert lib.liship_vbr_csr_count(1, a.ptr, a.ptr, a.ptr, a.ptr, a.ptr, None, v.ptr, a.ptr, a.ptr, a.ptr, C.byref(n), None) == ERR_ARG
    assert lib.liship_vbr_to_csr(0, a.ptr, a.ptr, a.ptr, a.ptr, a.ptr, a.ptr, v.ptr, a.ptr, a.ptr, v.ptr, None) == ERR_ARG


NS = [1, ROWS - 1, ROWS, ROWS + 1, SCAN - 1, SCAN, SCAN + 1]
WIDTHS = [1, 2, 7, 33]


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("fmt", ["ell", "dia", "bsr", "vbr"])
def test_kernels_at_the_borders(lib, fmt, n):
    for width in WIDTHS:
        run_kernels(lib, tc.random_source(fmt, n, width, seed=1))


@pytest.mark.parametrize("n", NS + [SLAB - 1, SLAB + 1])
def test_dns_kernels_at_the_borders_of_rows_and_slabs(lib, n):
    for np_ in (1, SLAB - 1, SLAB, SLAB + 1, 2 * SLAB + 3):
        if n >= SCAN - 1 and np_ not in (1, SLAB + 1):
            continue                                               # (the scan border needs one narrow and one two-slab shape, not five)
        run_kernels(lib, tc.random_source("dns", n, np_, seed=2))


def test_dns_scan_runs_over_more_cells_than_a_scan_tile(lib):
    """n * nslab > 4096 with n < 4096: the tiles of the scan cut rows apart"""
    s = tc.random_source("dns", 130, 33 * SLAB + 5, seed=3)
    assert s["n"] * ((s["np"] + SLAB - 1) // SLAB) > SCAN
    run_kernels(lib, s, passes=1)


@pytest.mark.parametrize("key", [k for k in tc.HAND if tc.HAND[k]["fmt"] in tc.KERNEL_FORMATS])
def test_kernels_on_the_hand_written_sources(lib, key):
    s = tc.HAND[key]
    run_kernels(lib, dict(s, np=s["n"]) if s["fmt"] == "dns" else s)


# ================================================================ API level
def _x(n, seed=3):
    return np.random.default_rng(seed).uniform(-1, 1, n)


def _delta(lib, before):
    now = drv.stats(lib)
    return now[0] - before[0], now[1] - before[1]


def _check_to_csr(lib, X, s, path="device"):
    """X -> CSR: the path, B's arrays and product, X untouched.  Returns nothing: B is destroyed."""
    n = s["n"]
    want = tc.model(s)
    lazy_x, prot_x = lib.dll.lis_amd_matrix_lazy_arrays(X), lib.dll.lis_amd_matrix_protected_arrays(X)
    before = drv.stats(lib)
    err, B = drv.to_csr(lib, X)
    assert err == 0
    assert _delta(lib, before) == ((1, 0) if path == "device" else (0, 1)), (s["fmt"], path)
    assert lib.dll.lis_amd_matrix_lazy_arrays(B) == (3 if path == "device" else 0)
    assert lib.dll.lis_amd_matrix_lazy_arrays(X) == lazy_x              # the source's arrays stayed where they were
    if s["fmt"] not in ("csc", "jad"):                                  # (CSC and JAD are read FROM their copy, which is made if it is not there)
        assert lib.dll.lis_amd_matrix_protected_arrays(X) == prot_x     # ... and no copy of the source was built for the conversion's sake
    x = _x(n)
    y = lisdrv.matvec(lib, B, x)
    assert cc.same_bits(y, orc.spmv_csr(*want, x), nan_payload_free=True)
    if path == "device":
        assert lib.dll.lis_amd_matrix_lazy_arrays(B) == 3               # a product asks for no host array
    ok, which = tc.same_csr(drv.csr_arrays(B), want)
    assert ok, (s["fmt"], which)
    assert B.contents.nnz == len(want[1]) and lib.dll.lis_amd_matrix_lazy_arrays(B) == 0
    assert cc.same_bits(lisdrv.matvec(lib, B, x), y, nan_payload_free=True)      # the HBM copy still serves
    lib.lis_matrix_destroy(B)
    assert drv.unchanged(X, s)                                           # (reads X's arrays: last)


def _kept(s):
    return len(tc.model(s)[1])


HOME = [k for k in tc.ALL]


@pytest.mark.parametrize("state", ["native_copy", "no_copy"])
@pytest.mark.parametrize("key", HOME)
def test_sources_whose_arrays_are_at_home(lib, key, state):
    """host arrays at home; the HBM copy is the one an upload makes (the native arrays, CSC / JAD: their rows) or there is none"""
    s = tc.source(key)
    X = drv.make(lib, s)
    if state == "native_copy":
        assert lib.dll.lis_amd_matrix_upload(X) == 0
    else:
        assert lib.dll.lis_amd_matrix_host_modified(X) == 0              # the copy assemble made is dropped
        assert lib.dll.lis_amd_matrix_protected_arrays(X) == 0
    assert lib.dll.lis_amd_matrix_lazy_arrays(X) == 0
    _check_to_csr(lib, X, s)
    lib.lis_matrix_destroy(X)


LAZY_CASES = ["specials", "empties", "n257_longest_last", "n1", "constant_p3d", "constant_band"]
LAZY_FORMATS = [("ell", 0, 0), ("dia", 0, 0), ("bsr", 2, 2), ("bsr", 3, 2), ("csc", 0, 0), ("jad", 0, 0), ("dns", 0, 0)]


@pytest.mark.parametrize("fmt,bnr,bnc", LAZY_FORMATS, ids=["%s%s" % (f, "%dx%d" % (r, c) if r else "") for f, r, c in LAZY_FORMATS])
@pytest.mark.parametrize("case", LAZY_CASES)
def test_sources_made_in_hbm_and_still_lazy(lib, case, fmt, bnr, bnc):
    """X was itself made by a conversion in HBM: its host arrays are address space bound to device buffers and stay that.  Constant coefficients: X's copy is the
    row form and only the buffers behind the lazy arrays hold the native layout"""
    csr = cc.CASES[case]
    s = tc.from_csr(fmt, csr, bnr or 2, bnc or 2)
    A = lisdrv.make_csr(lib, *csr)
    assert lib.dll.lis_amd_matrix_upload(A) == 0
    X = lisdrv.convert(lib, A, fmt, bnr or 2, bnc or 2)
    assert lib.dll.lis_amd_matrix_lazy_arrays(X) >= 1, "the source was to be made in HBM"
    if case.startswith("constant") and fmt in ("ell", "dia") or (case.startswith("constant") and (fmt, bnr, bnc) == ("bsr", 2, 2)):
        assert lib.dll.lis_amd_matrix_device_type(X) == capi.LIS_MATRIX_CSR     # the row form
    _check_to_csr(lib, X, s)
    lib.lis_matrix_destroy(X); lib.lis_matrix_destroy(A)


@pytest.mark.parametrize("fmt,bnr,bnc", [("ell", 0, 0), ("dia", 0, 0), ("bsr", 2, 2)], ids=["ell", "dia", "bsr2x2"])
@pytest.mark.parametrize("case", ["constant_p3d", "constant_band"])
def test_sources_at_home_with_a_row_form_copy(lib, case, fmt, bnr, bnc):
    s = tc.from_csr(fmt, cc.CASES[case], bnr or 2, bnc or 2)
    X = drv.make(lib, s)
    assert lib.dll.lis_amd_matrix_upload(X) == 0
    assert lib.dll.lis_amd_matrix_device_type(X) == capi.LIS_MATRIX_CSR and lib.dll.lis_amd_matrix_lazy_arrays(X) == 0
    _check_to_csr(lib, X, s)
    lib.lis_matrix_destroy(X)


@pytest.mark.parametrize("key", ["specials-ell", "specials-dia", "specials-bsr3x2", "specials-dns", "specials-vbr", "specials-csc", "specials-jad", "vbr_1to3"])
def test_switched_off_the_host_routine_serves(lib, key):
    s = tc.source(key)
    X = drv.make(lib, s)
    lib.dll.lis_amd_set_device_convert(0)
    try:
        _check_to_csr(lib, X, s, path="host")
    finally:
        lib.dll.lis_amd_set_device_convert(1)
    _check_to_csr(lib, X, s)                                             # ... and switched back on
    lib.lis_matrix_destroy(X)


@pytest.mark.parametrize("t", dc.TRIPLETS)
def test_coo_stays_on_the_host_and_is_sorted_in_place(lib, t):
    n, row, col, val = dc.triplets(t)
    A = coo_dns_drv.make_coo(lib, n, row, col, val)
    before = drv.stats(lib)
    err, B = drv.to_csr(lib, A)
    assert err == 0 and _delta(lib, before) == (0, 1) and lib.dll.lis_amd_matrix_lazy_arrays(B) == 0
    want, (srow, scol, sval) = dc.coo2csr(n, row, col, val)
    a = coo_dns_drv.arrays(A)
    assert np.array_equal(a["row"], srow) and np.array_equal(a["col"], scol) and cc.same_bits(a["value"], sval)
    ok, which = tc.same_csr(drv.csr_arrays(B), want)
    assert ok, which
    lib.lis_matrix_destroy(B); lib.lis_matrix_destroy(A)


def tridiagonal(n=301):
    """rows in ascending column order whose 2 x 2 blocking lists its blocks in ascending order too, so that every conversion out of it is built in HBM"""
    rows = [[c for c in (r - 1, r, r + 1) if 0 <= c < n] for r in range(n)]
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(I32)
    idx = np.array([c for r in rows for c in r], I32)
    val = np.random.default_rng(12).uniform(0.5, 2, len(idx)) * np.where(np.arange(len(idx)) % 2, 1, -1)
    return ptr, idx, val


CHAINS = [("ell", "bsr"), ("dia", "ell"), ("bsr", "dia"), ("jad", "csc")]


@pytest.mark.parametrize("xf,yf", CHAINS, ids=["%s-%s" % c for c in CHAINS])
def test_chains_between_two_formats_stay_in_hbm(lib, xf, yf):
    csr = tridiagonal()
    A = lisdrv.make_csr(lib, *csr)
    assert lib.dll.lis_amd_matrix_upload(A) == 0
    X = lisdrv.convert(lib, A, xf)
    lazy_x = lib.dll.lis_amd_matrix_lazy_arrays(X)
    assert lazy_x >= 2
    middle = tc.model(tc.from_csr(xf, csr))
    want = cc.oracle_arrays(yf, *middle)
    before = drv.stats(lib)
    Y = lisdrv.convert(lib, X, yf)
    assert _delta(lib, before) == (2, 0)
    assert lib.dll.lis_amd_matrix_lazy_arrays(X) == lazy_x and lib.dll.lis_amd_matrix_lazy_arrays(Y) >= 2
    ok, which = cc.same_arrays(lisdrv.matrix_arrays(Y), want)
    assert ok, (xf, yf, which)
    for M in (Y, X, A):
        lib.lis_matrix_destroy(M)


@pytest.mark.parametrize("fmt", ["ell", "bsr"])
def test_shift_matrix_of_a_matrix_made_in_hbm_converts_nothing_on_the_host(lib, fmt):
    """lis_matrix_shift_matrix on X: X -> CSR -> shift -> X, every step in HBM; the arrays afterwards are csr2X of tests/shift_model.py's rows"""
    a = tridiagonal(300)
    n = len(a[0]) - 1
    b = (np.arange(n + 1, dtype=I32), np.arange(n, dtype=I32), np.full(n, 1.0))
    fn = lib.dll.lis_matrix_shift_matrix
    fn.restype, fn.argtypes = capi.LIS_INT, [capi.PM, capi.PM, C.c_double]
    A0 = lisdrv.make_csr(lib, *a)
    assert lib.dll.lis_amd_matrix_upload(A0) == 0
    X = lisdrv.convert(lib, A0, fmt)
    B = lisdrv.make_csr(lib, *b)
    seen = tc.model(tc.from_csr(fmt, a))                                 # the rows the shift sees: X -> CSR
    ptr, idx, val = sm.shift_matrix(*seen, *b, 0.375)
    before = drv.stats(lib)
    assert fn(X, B, 0.375) == 0
    assert _delta(lib, before) == (2, 0)
    got = lisdrv.matrix_arrays(X)
    x = _x(n)
    if fmt == "ell":
        mx, eidx, ev = orc.csr2ell(ptr, idx, val)
        assert got["type"] == capi.LIS_MATRIX_ELL and got["maxnzr"] == mx and np.array_equal(got["index"], eidx) and cc.same_bits(got["value"], ev)
        assert cc.same_bits(lisdrv.matvec(lib, X, x), orc.spmv_ell(n, mx, eidx, ev, x))
    else:
        nr, bptr, bidx, bval = orc.csr2bsr(ptr, idx, val)
        assert got["type"] == capi.LIS_MATRIX_BSR and (got["bnr"], got["bnc"], got["nr"]) == (2, 2, nr)
        assert np.array_equal(got["bptr"], bptr) and np.array_equal(got["bindex"], bidx) and cc.same_bits(got["value"], bval)
        assert cc.same_bits(lisdrv.matvec(lib, X, x), orc.spmv_bsr(n, nr, 2, 2, bptr, bidx, bval, x))
    for M in (X, B, A0):
        lib.lis_matrix_destroy(M)
