"""COO and DNS storage on the device, bit for bit.

Kernel level (include/liship.h through lis_amd.load()): the two dense kernels of kernels/dns.hip at the borders of their tiles and slabs, with unaligned
arrays, special values and a sentinel behind y; the stable grouping of kernels/transpose.hip and the row form of kernels/coo.hip at the borders of the
ordering kernels, on both of its paths.  Expectations come from the numpy models of tests/coo_dns_cases.py, which tests/test_coo_dns_cpu.py holds to the
reference's own results.

API level: products through lis_matvec / lis_matvech and the raw entry points, conversions in HBM, whole solves and eigensolves against
tests/golden/coo_dns_bits.npz -- in the reference-order mode every count, status, residual history and solution in every bit; in the default mode the
count inside the reference's own spread over T = 1 / 8 widened by 1 and x within 1e-8 (the bar of tests/test_more_solvers_gpu.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import coo_dns_cases as cc
import coo_dns_drv as drv
import esolve_drv
import format_cases as fc
import lis_amd
import lisdrv
from gpu_arrays import Out, dev
from lis_amd import DeviceArray as DA, _capi as capi, check

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", cc.FIXTURE))
ERR_ARG = -1                                    # LISHIP_ERR_ARG
ROWS, SLAB, TCOLS, TSLAB = 32, 64, 32, 64       # the tiles of kernels/dns.hip (liship_dns_tile_info)
NOT_IMPLEMENTED = capi.LIS_ERR_NOT_IMPLEMENTED


@pytest.fixture(scope="module")
def lib():
    lib = lis_amd.load()
    assert lis_amd.gpu_available(), "no HIP device: the product path has no CPU fallback"
    assert lib.initialize([]) == 0
    for f in (lib.dll.lis_amd_matrix_lazy_arrays, lib.dll.lis_amd_matrix_device_type, lib.dll.lis_amd_matrix_upload):
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


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def dense(n, np_, seed):
    rng = np.random.default_rng(seed)
    d = rng.uniform(-1, 1, n * np_)
    d[rng.uniform(size=n * np_) < 0.2] = 0.0            # zeros are multiplied like any other entry
    return d


# ================================================================ kernel level: DNS
def test_tile_constants(lib):
    info = (C.c_int * 4)()
    check(lib.liship_dns_tile_info(info))
    assert list(info) == [ROWS, SLAB, TCOLS, TSLAB]
    assert lib.liship_dns_tile_info(None) == ERR_ARG
    assert lib.liship_spmv_dns_f64(-1, 1, None, None, None, None) == ERR_ARG and lib.liship_spmv_dns_t_f64(1, 1, 0, None, None, None, None) == ERR_ARG


@pytest.mark.parametrize("n", [1, ROWS - 1, ROWS, ROWS + 1, 63, 64, 65])
def test_dns_forward_at_the_borders_of_tile_and_slab(lib, n):
    """every row's sum is the chain over the columns from +0.0; value and x one element behind an aligned address; Y_PAD elements behind y keep the sentinel"""
    for np_ in (1, SLAB - 1, SLAB, SLAB + 1, 2 * SLAB + 3):
        d, x = dense(n, np_, 100 * n + np_), cc.xvec(np_, np_)
        keep = (_, dv), (_, dx) = dev(d, shift=1), dev(x, shift=1)
        y = Out(n, shift=1)
        check(lib.liship_spmv_dns_f64(n, np_, dv, dx, y.ptr, None))
        y.holds(cc.dns_matvec(n, np_, d, x), ("dns", n, np_))
        del keep


def test_dns_forward_special_values(lib):
    n, np_ = ROWS + 5, SLAB + 7
    d, x = dense(n, np_, 7), cc.xvec(np_, 8)
    # an infinity in x against a column of zeros: 0 * inf is NaN in every row
    dz, xi = d.copy(), x.copy()
    dz.reshape(np_, n)[SLAB + 2] = 0.0
    xi[SLAB + 2] = np.inf
    # a NaN with a payload in one entry: its row is NaN, the others are not
    dn = d.copy()
    dn.reshape(np_, n)[3, 5] = np.array([0x7FF8000000ABCDEF], np.uint64).view(np.float64)[0]
    # every product -0.0: the sums start at +0.0 and end there
    dm, xz = fc.all_products_negative_zero(d, np_)
    for tag, dd, xx in (("inf", dz, xi), ("nan", dn, x), ("-0", dm, xz)):
        keep = (_, dv), (_, dx) = dev(dd), dev(xx)
        y = Out(n)
        check(lib.liship_spmv_dns_f64(n, np_, dv, dx, y.ptr, None))
        ref = cc.dns_matvec(n, np_, dd, xx)
        if tag == "inf":
            assert np.all(np.isnan(ref))
        if tag == "nan":
            assert np.isnan(ref[5]) and np.count_nonzero(np.isnan(ref)) == 1
        if tag == "-0":
            assert same(ref, np.zeros(n))
        y.holds(ref, ("dns", tag), special=tag != "-0")
        del keep


@pytest.mark.parametrize("np_", [1, TCOLS - 1, TCOLS, TCOLS + 1, 63, 64, 65])
def test_dns_transposed_at_the_borders_and_in_row_chunks(lib, np_):
    """column j's sum is over T row chunks, each from +0.0, the chunk sums added in chunk order from +0.0; T > n leaves chunks empty"""
    for n in (1, TSLAB - 1, TSLAB, TSLAB + 1, 2 * TSLAB + 3):
        d, x = dense(n, np_, 200 * np_ + n), cc.xvec(n, n)
        keep = (_, dv), (_, dx) = dev(d, shift=1), dev(x, shift=1)
        for T in (1, 2, 8, n + 3):
            y = Out(np_, shift=1)
            check(lib.liship_spmv_dns_t_f64(n, np_, T, dv, dx, y.ptr, None))
            y.holds(cc.dns_matvech(n, np_, d, x, T), ("dns_t", n, np_, T))
        del keep


def test_dns_transposed_special_values(lib):
    n, np_ = 2 * TSLAB + 9, TCOLS + 3
    d, x = dense(n, np_, 17), cc.xvec(n, 18)
    dz, xi = d.copy(), x.copy()
    dz.reshape(np_, n)[:, TSLAB + 1] = 0.0                # a ROW of zeros against an infinity in x: NaN in every column
    xi[TSLAB + 1] = np.inf
    dm, xz = fc.all_products_negative_zero(d, n)
    for tag, dd, xx in (("inf", dz, xi), ("-0", dm, xz)):
        keep = (_, dv), (_, dx) = dev(dd), dev(xx)
        for T in (1, 8):
            y = Out(np_)
            check(lib.liship_spmv_dns_t_f64(n, np_, T, dv, dx, y.ptr, None))
            ref = cc.dns_matvech(n, np_, dd, xx, T)
            assert np.all(np.isnan(ref)) if tag == "inf" else same(ref, np.zeros(np_))
            y.holds(ref, ("dns_t", tag, T), special=tag == "inf")
        del keep


# ================================================================ kernel level: the grouping and the COO row form
def grouped(lib, nkeys, key, src, val):
    """liship_group_by_key_f64 -> (ptr, index, value)"""
    nnz = len(key)
    keep = (_, dk), (_, ds), (_, dv) = dev(key, np.int32), dev(src, np.int32), dev(val, np.float64)
    tp, ti, tv = DA(nkeys + 1, np.int32), DA(max(nnz, 1), np.int32), DA(max(nnz, 1), np.float64)
    check(lib.liship_group_by_key_f64(nkeys, nnz, dk, ds, dv, tp.ptr, ti.ptr, tv.ptr, None))
    del keep
    return tp.to_host(), ti.to_host(nnz), tv.to_host(nnz)


def row_form(lib, n, row, col, val):
    """liship_coo_rows_f64 -> (ptr, index, value, in_place)"""
    nnz = len(row)
    keep = (_, dr), (_, dc), (_, dv) = dev(row, np.int32), dev(col, np.int32), dev(val, np.float64)
    ptr, pi, pv = DA(n + 1, np.int32), C.c_void_p(), C.c_void_p()
    check(lib.liship_coo_rows_f64(n, nnz, dr, dc, dv, ptr.ptr, C.byref(pi), C.byref(pv), None))
    in_place = pi.value == dc and pv.value == dv
    assert in_place or (pi.value not in (None, dc) and pv.value not in (None, dv))
    idx, v = np.empty(nnz, np.int32), np.empty(nnz, np.float64)
    if nnz:
        check(lib.liship_memcpy_d2h(idx.ctypes.data, pi, idx.nbytes, None))
        check(lib.liship_memcpy_d2h(v.ctypes.data, pv, v.nbytes, None))
        check(lib.liship_device_synchronize())
    if not in_place:
        check(lib.liship_free(pi))
        check(lib.liship_free(pv))
    del keep
    return ptr.to_host(), idx, v, in_place


def segments(lengths, nkeys, seed, order):
    """triplets whose key c occurs lengths[c] times (keys beyond len(lengths): never), in the given order"""
    rng = np.random.default_rng(seed)
    key = np.repeat(np.arange(len(lengths), dtype=np.int32), lengths)
    if order == "shuffled":
        key = key[rng.permutation(len(key))]
    elif order == "descending":
        key = key[::-1].copy()
    src = rng.integers(0, nkeys, len(key)).astype(np.int32)
    return key, src, rng.uniform(-1, 1, len(key))


def test_the_borders_are_the_ones_the_cases_aim_at(lib):
    out = (C.c_int * 3)()
    check(lib.liship_group_by_key_borders(out))
    assert list(out) == [32, 33, 2048]


BORDERS = [31, 32, 33, 34, 2047, 2048, 2049]


@pytest.mark.parametrize("order", ["sorted", "shuffled", "descending"])
@pytest.mark.parametrize("nkeys", [len(BORDERS) + 1, 4096])
def test_grouping_at_the_borders_of_the_ordering_kernels(lib, nkeys, order):
    """segment lengths around 32 | 33 and 2048 | 2049, an empty segment among them; few keys (nnz > 8 nkeys: a wavefront ranks the segments of 33 .. 2048
    in LDS) and many (every segment by the lane-per-segment sorts)"""
    lengths = [BORDERS[0], 0] + BORDERS[1:]
    key, src, val = segments(lengths, nkeys, 5, order)
    assert (len(key) > 8 * nkeys) == (nkeys < 4096)
    got, want = grouped(lib, nkeys, key, src, val), cc.group_by_key(nkeys, key, src, val)
    for g, w, f in zip(got, want, ("ptr", "index", "value")):
        assert same(g, w), (f, nkeys, order)
    # the row form: in place exactly when the rows are grouped already
    ptr, idx, v, in_place = row_form(lib, nkeys, key, src, val)
    assert in_place == (order == "sorted")
    assert same(ptr, want[0]) and same(idx, want[1]) and same(v, want[2])


def test_grouping_edges(lib):
    # no entries
    for got in (grouped(lib, 5, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0)), row_form(lib, 5, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0))[:3]):
        assert same(got[0], np.zeros(6, np.int32)) and len(got[1]) == 0 and len(got[2]) == 0
    assert row_form(lib, 5, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0))[3]
    # one row holding everything, first, middle and last
    for r in (0, 3, 6):
        key, src, val = segments([0] * r + [5000], 7, r, "sorted")
        for got in (grouped(lib, 7, key, src, val), row_form(lib, 7, key, src, val)[:3]):
            for g, w in zip(got, cc.group_by_key(7, key, src, val)):
                assert same(g, w), r
    # duplicate (key, src) pairs stay apart and in stored order
    key = np.array([2, 0, 2, 2, 0, 1, 2], np.int32)
    src = np.array([1, 1, 1, 1, 1, 0, 1], np.int32)
    val = np.arange(7, dtype=np.float64)
    ptr, idx, v, in_place = row_form(lib, 3, key, src, val)
    assert not in_place and same(ptr, np.array([0, 2, 3, 7], np.int32)) and same(v, np.array([1., 4., 5., 0., 2., 3., 6.]))
    # a row outside [0, n): refused, nothing built
    keep = (_, dr), (_, dc), (_, dv) = dev(np.array([0, 3], np.int32)), dev(np.array([0, 0], np.int32)), dev(np.ones(2))
    ptr, pi, pv = DA(4, np.int32), C.c_void_p(), C.c_void_p()
    assert lib.liship_coo_rows_f64(3, 2, dr, dc, dv, ptr.ptr, C.byref(pi), C.byref(pv), None) == ERR_ARG and not pi.value and not pv.value
    flags = C.c_int(-1)
    check(lib.liship_key_facts(3, 2, dr, C.byref(flags), None))
    assert flags.value == 2
    del keep


# ================================================================ API level
def build(lib, m, fmt):
    n = len(cc.matrix(m)[0]) - 1
    if fmt == "coo":
        return drv.make_coo(lib, n, G[m + "|coo|row"], G[m + "|coo|col"], G[m + "|coo|value"])
    return drv.make_dns(lib, n, G[m + "|dns|value"])


@pytest.mark.parametrize("fmt", ["coo", "dns"])
@pytest.mark.parametrize("m", cc.MATRICES)
def test_products_through_the_lis_entry_points(lib, m, fmt):
    A = build(lib, m, fmt)
    n = A.contents.n
    x = cc.xvec(n)
    assert lib.dll.lis_amd_matrix_device_type(A) == (capi.LIS_MATRIX_CSR if fmt == "coo" else drv.DNS)
    assert same(lisdrv.matvec(lib, A, x), G["%s|%s|y" % (m, fmt)]) and same(drv.raw_product(lib, A, fmt, x)[:n], G["%s|%s|y" % (m, fmt)])
    for T in (0, 1, 8):
        with mode(lib, T):
            want = G["%s|%s|yt|T%d" % (m, fmt, max(T, 1))]
            assert same(lisdrv.matvech(lib, A, x), want), T
            assert same(drv.raw_product(lib, A, fmt, x, transposed=True), want), T
            assert same(lisdrv.matvec(lib, A, x), G["%s|%s|y" % (m, fmt)]), T
    err, d = drv.diagonal(lib, A, np.full(n, 7.0))
    assert err == 0 and same(d, G["%s|%s|diag" % (m, fmt)])
    if m != "rand301":                                            # the shift goes the way of the host-edited formats: the next product uploads the edited arrays
        assert lib.lis_matrix_shift_diagonal(A, cc.SHIFT) == 0 and same(drv.arrays(A)["value"], G["%s|%s|shift|value" % (m, fmt)])
        ptr, idx, val = cc.matrix(m)
        a = drv.arrays(A)
        want = cc.coo_matvec(n, a["row"], a["col"], a["value"], x) if fmt == "coo" else cc.dns_matvec(n, n, a["value"], x)
        assert same(lisdrv.matvec(lib, A, x), want)
    lib.lis_matrix_destroy(A)


@pytest.mark.parametrize("t", cc.TRIPLETS)
def test_a_coo_source_changes_its_bits_when_it_is_converted(lib, t):
    n, row, col, val = cc.triplets(t)
    x = cc.xvec(n)
    A = drv.make_coo(lib, n, row, col, val)
    assert same(lisdrv.matvec(lib, A, x), G[t + "|y_before"])
    assert same(lisdrv.matvech(lib, A, x), cc.coo_matvech(n, row, col, val, x))
    err, B = drv.convert(lib, A, "csr")
    assert err == 0
    for f in ("row", "col", "value"):
        assert same(drv.arrays(A)[f], G["%s|after|%s" % (t, f)]), f
    assert same(lisdrv.matvec(lib, A, x), G[t + "|y_after"]) and not same(G[t + "|y_after"], G[t + "|y_before"])
    a = drv.arrays(A)
    assert same(lisdrv.matvech(lib, A, x), cc.coo_matvech(n, a["row"], a["col"], a["value"], x))
    assert same(lisdrv.matvec(lib, B, x), G[t + "|y_after"])      # the CSR matrix lists the sorted triplets
    lib.lis_matrix_destroy(B)
    lib.lis_matrix_destroy(A)


@pytest.mark.parametrize("m", cc.MATRICES)
def test_conversions_in_hbm(lib, m):
    """a CSR source with an HBM copy: csr2coo and csr2dns are built there, the host arrays come home on their first touch"""
    ptr, idx, val = cc.matrix(m)
    n = len(ptr) - 1
    x = cc.xvec(n)
    A = lisdrv.make_csr(lib, ptr, idx, val)
    assert lib.dll.lis_amd_matrix_upload(A) == 0
    for fmt, arrays in (("coo", 3), ("dns", 1)):
        err, B = drv.convert(lib, A, fmt)
        assert err == 0 and B.contents.matrix_type == capi.FORMAT_ID[fmt]
        lazy = lib.dll.lis_amd_matrix_lazy_arrays(B)
        assert lazy == arrays, (fmt, lazy)
        assert lib.dll.lis_amd_matrix_device_type(B) == (capi.LIS_MATRIX_CSR if fmt == "coo" else drv.DNS)
        assert same(lisdrv.matvec(lib, B, x), G["%s|%s|y" % (m, fmt)]) and same(lisdrv.matvech(lib, B, x), G["%s|%s|yt|T1" % (m, fmt)])
        assert lib.dll.lis_amd_matrix_lazy_arrays(B) == lazy      # a product asks for no host array
        a = drv.arrays(B)
        assert a["nnz"] == int(G["%s|%s|nnz" % (m, fmt)][0])
        for f in ("row", "col", "value"):
            if f in a:
                assert same(a[f], G["%s|%s|%s" % (m, fmt, f)]), (fmt, f)
        assert lib.dll.lis_amd_matrix_lazy_arrays(B) == 0
        lib.lis_matrix_destroy(B)
    lib.lis_matrix_destroy(A)


def solve(lib, opts):
    ptr, idx, val = cc.matrix("stencil")
    A = lisdrv.make_csr(lib, ptr, idx, val)                       # (-storage converts the caller's matrix for good: a fresh one per solve)
    out = lisdrv.solve(lib, A, cc.rhs(ptr, idx, val), opts + " " + cc.COMMON)
    assert out["err"] == 0 and A.contents.matrix_type == capi.FORMAT_ID[opts.split()[-1]]
    lib.lis_matrix_destroy(A)
    return out


UNFUSED = 2                                     # LIS_AMD_LOOP_UNFUSED: one kernel per reference call (LIS_AMD_NO_FUSION=1)


class loops:
    """lis_amd_set_loop_mode(mode) for the duration of a with block"""
    def __init__(self, lib, mode):
        self.lib, self.mode = lib, mode

    def __enter__(self):
        assert self.lib.dll.lis_amd_set_loop_mode(self.mode) == 0

    def __exit__(self, *a):
        self.lib.dll.lis_amd_set_loop_mode(0)


@pytest.mark.parametrize("loop", [0, UNFUSED])
@pytest.mark.parametrize("T", cc.THREADS)
@pytest.mark.parametrize("opts", cc.SOLVES)
def test_solves_in_the_reference_order_mode_are_the_reference(lib, opts, T, loop):
    """count, status, every residual and x in every bit -- from the fused loops and from the unfused ones, which therefore agree in every bit"""
    key = "solve|%s|T%d" % (opts, T)
    with mode(lib, T), loops(lib, loop):
        out = solve(lib, opts)
    assert [out["iter"], out["status"]] == G[key + "|meta"].tolist(), (key, out["iter"], out["status"])
    want = G[key + "|rhistory"]
    assert len(out["rhistory"]) == len(want)
    diff = np.flatnonzero(out["rhistory"].view(np.int64) != want.view(np.int64))
    assert diff.size == 0, (key, "first differing history entry", int(diff[0]), out["rhistory"][diff[0]].hex(), want[diff[0]].hex())
    assert same(out["x"], G[key + "|x"]), key


@pytest.mark.parametrize("opts", cc.SOLVES)
def test_solves_in_the_default_mode(lib, opts):
    """the tree mode: the count inside the reference's own T = 1 / 8 counts widened by 1, x within 1e-8 -- fused and unfused.  The unfused loops group the
    reductions of a CSR copy differently from the fused product + dot (tests/test_device_loops_gpu.py), so on COO storage the two are held to the same bar
    each; on DNS storage, whose product has no fused dot, they agree in every bit"""
    counts = [int(G["solve|%s|T%d|meta" % (opts, T)][0]) for T in cc.THREADS]
    runs = []
    for loop in (0, UNFUSED):
        with loops(lib, loop):
            out = solve(lib, opts)
        assert out["status"] == 0 and min(counts) - 1 <= out["iter"] <= max(counts) + 1, (opts, loop, out["iter"], counts)
        assert np.allclose(out["x"], G["solve|%s|T1|x" % opts], rtol=0, atol=1e-8), (opts, loop)
        runs.append(out)
    if opts.endswith("dns"):
        assert runs[0]["iter"] == runs[1]["iter"] and same(runs[0]["rhistory"], runs[1]["rhistory"]) and same(runs[0]["x"], runs[1]["x"])


@pytest.mark.parametrize("T", cc.THREADS)
@pytest.mark.parametrize("opts", cc.ESOLVES)
def test_eigensolves_in_the_reference_order_mode_are_the_reference(lib, opts, T):
    key = "esolve|%s|T%d" % (opts, T)
    with mode(lib, T):
        A = esolve_drv.make_matrix(lib, "sym7")
        out = esolve_drv.esolve(lib, A, opts + " " + cc.ECOMMON)
        assert out["err"] == 0 and A.contents.matrix_type == capi.FORMAT_ID[opts.split()[-1]]
        lib.lis_matrix_destroy(A)
    assert [out["iter"], out["status"]] == G[key + "|meta"].tolist()
    assert same(np.array([out["evalue"], out["resid"]]), G[key + "|evalue"]) and same(out["rhistory"], G[key + "|rhistory"]) and same(out["x"], G[key + "|x"])


@pytest.mark.parametrize("fmt", ["coo", "dns"])
def test_refusals_that_need_a_device(lib, fmt, capfd):
    """-p ilu and -p bjacobi look for a device before they refuse: here, with one, they say why and leave A, b and x alone"""
    ptr, idx, val = cc.matrix("dups")
    n = len(ptr) - 1
    for p, text in (("ilu", "-p ilu is served for"), ("bjacobi", "-p bjacobi on %s storage is not served" % fmt.upper())):
        A = lisdrv.make_csr(lib, ptr, idx, val)
        b, x = lisdrv.new_vector(lib, A, np.ones(n)), lisdrv.new_vector(lib, A, np.full(n, 3.0))
        S = capi.PS()
        assert lib.lis_solver_create(C.byref(S)) == 0 and lib.lis_solver_set_option(("-i cg -p %s -storage %s" % (p, fmt)).encode(), S) == 0
        capfd.readouterr()
        assert lib.lis_solve(A, b, x, S) == NOT_IMPLEMENTED
        out = capfd.readouterr().out
        assert text in out and "A is untouched" in out, out
        assert A.contents.matrix_type == capi.LIS_MATRIX_CSR and same(lisdrv.matrix_arrays(A)["value"], val)
        assert same(lisdrv.get_vector(lib, b), np.ones(n)) and same(lisdrv.get_vector(lib, x), np.full(n, 3.0))
        lib.lis_solver_destroy(S); lib.lis_vector_destroy(b); lib.lis_vector_destroy(x); lib.lis_matrix_destroy(A)
