"""lis_matrix_shift_diagonal on a matrix that lives in HBM (host/lis_shift.c, kernels/eigen.hip liship_csr_shift_diagonal_f64) against tests/esolve_model.py,
in every bit of the HBM values and of the next product; that everything derived from the old values is gone (the plan, the transposed copy, the ILU
factor); that the write watch does not take the library's own host edit for the program's; the five other formats through their host path."""
import ctypes as C

import numpy as np
import pytest

import esolve_drv
import esolve_model as em
import lis_amd
import lisdrv
import orc
from lis_amd import DeviceArray as DA, check
from lis_amd import _capi as capi

pytestmark = pytest.mark.gpu
SIGMAS = [0.0, -0.0, 1.5, 5e-324, float("inf")]


@pytest.fixture(scope="module")
def lib():
    lib = lis_amd.load()
    assert lis_amd.gpu_available(), "no HIP device: the product path has no CPU fallback"
    assert lib.initialize([]) == 0
    lib.dll.lis_amd_set_residency(0)
    lib.dll.lis_amd_matrix_set_csr_device.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, capi.PM]
    return lib


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.int64), np.ascontiguousarray(b, np.float64).view(np.int64))


def long_rows():
    """rows of 1, 64, 65 and 1025 entries with the diagonal stored first, and the same lengths with it stored last (n = 1100, columns otherwise ascending)"""
    n = 1100
    rows = []
    for first in (True, False):
        for length in (1, 64, 65, 1025):
            i = len(rows)
            others = [c for c in range(n) if c != i][:length - 1]
            cols = ([i] + others) if first else (others + [i])
            rows.append([(c, 0.5 + 0.001 * c) for c in cols])
    while len(rows) < n:
        rows.append([])
    ptr = np.zeros(n + 1, np.int32)
    idx, val = [], []
    for i, r in enumerate(rows):
        idx += [c for c, _ in r]
        val += [v for _, v in r]
        ptr[i + 1] = len(idx)
    return ptr, np.array(idx, np.int32), np.array(val, np.float64)


KERNEL_MATRICES = {
    "n1": lambda: (np.array([0, 1], np.int32), np.array([0], np.int32), np.array([3.0])),
    "n1_no_diagonal": lambda: (np.array([0, 0], np.int32), np.zeros(0, np.int32), np.zeros(0)),
    "edges": em.shift_matrix,                        # empty rows, rows without a diagonal, the diagonal stored twice, unsorted columns
    "long_rows": long_rows,
    "blocks": lambda: orc.poisson3d(9, 8, 7),        # more than one workgroup of rows (504)
}


@pytest.mark.parametrize("name", sorted(KERNEL_MATRICES))
def test_kernel_moves_the_first_diagonal_entry_of_every_row(lib, name):
    ptr, idx, val = KERNEL_MATRICES[name]()
    n = len(ptr) - 1
    dptr, didx = DA.from_host(ptr, np.int32), DA.from_host(idx if len(idx) else np.zeros(1, np.int32), np.int32)
    bad = {}
    for sigma in SIGMAS + [-1.5]:
        dval = DA.from_host(np.concatenate([val, [7.25]]), np.float64)        # one double behind the last entry: must stay
        check(lib.liship_csr_shift_diagonal_f64(n, dptr.ptr, didx.ptr, dval.ptr, sigma, None))
        check(lib.liship_device_synchronize())
        got = dval.to_host()
        want = em.shift_csr_values(ptr, idx, val, sigma)
        if not same_bits(got[:-1], want) or got[-1] != 7.25:
            bad[sigma] = np.flatnonzero(got[:-1].view(np.int64) != want.view(np.int64))[:8].tolist()
    assert bad == {}
    assert lib.liship_csr_shift_diagonal_f64(-1, dptr.ptr, didx.ptr, dptr.ptr, 1.0, None) == -1
    assert lib.liship_csr_shift_diagonal_f64(0, None, None, None, 1.0, None) == 0


def test_shift_then_unshift_keeps_the_reference_drift(lib):
    ptr, idx, val = orc.poisson3d(9, 8, 7)
    val = val * (1.0 + 1e-3 * np.cos(np.arange(len(val))))
    dptr, didx, dval = DA.from_host(ptr, np.int32), DA.from_host(idx, np.int32), DA.from_host(val, np.float64)
    bad = []
    for s in (0.1, 1.0 / 3.0, 1e17):
        dval.upload(val)
        check(lib.liship_csr_shift_diagonal_f64(len(ptr) - 1, dptr.ptr, didx.ptr, dval.ptr, s, None))
        check(lib.liship_csr_shift_diagonal_f64(len(ptr) - 1, dptr.ptr, didx.ptr, dval.ptr, -s, None))
        want = em.shift_csr_values(ptr, idx, em.shift_csr_values(ptr, idx, val, s), -s)
        if not same_bits(dval.to_host(), want):
            bad.append(s)
    assert bad == []
    assert not same_bits(want, val)                 # (1e17 swallows the diagonal: the drift is there, and the kernel has it)


def _x(n):
    return np.sin(np.arange(n) * 0.7) + 0.25


@pytest.mark.parametrize("sigma", SIGMAS)
def test_resident_host_backed_matrix(lib, sigma):
    """The copy exists (a product ran): the HBM values are edited in place, the host arrays on the host, the watch stays quiet, the next product is the
    product of the shifted matrix -- of a matrix built shifted from the start, and of the oracle."""
    ptr, idx, val = esolve_drv.sym_csr()
    n = len(ptr) - 1
    x = _x(n)
    A = lisdrv.make_csr(lib, ptr, idx, val)
    assert same_bits(lisdrv.matvec(lib, A, x), orc.spmv_csr(ptr, idx, val, x))
    assert lib.dll.lis_amd_matrix_host_written(A) == 0
    assert lib.lis_matrix_shift_diagonal(A, sigma) == 0
    assert lib.dll.lis_amd_matrix_host_written(A) == 0
    want = em.shift_csr_values(ptr, idx, val, sigma)
    with np.errstate(all="ignore"):
        y = lisdrv.matvec(lib, A, x)
        assert same_bits(np.nan_to_num(y, nan=7.0), np.nan_to_num(orc.spmv_csr(ptr, idx, want, x), nan=7.0))
    assert lib.dll.lis_amd_matrix_host_written(A) == 0
    assert same_bits(lisdrv.matrix_arrays(A)["value"], want)                     # the host arrays got the same edit (reading them is free)
    assert lib.dll.lis_amd_matrix_host_written(A) == 0
    if np.isfinite(sigma):
        B = lisdrv.make_csr(lib, ptr, idx, want)
        assert same_bits(y, lisdrv.matvec(lib, B, x))
        assert same_bits(lisdrv.matvech(lib, A, x), lisdrv.matvech(lib, B, x))   # the transposed copy is made from the shifted values
        lib.lis_matrix_destroy(B)
    lib.lis_matrix_destroy(A)


def test_program_writes_are_still_seen_after_a_shift(lib):
    """The library's own edit is not the program's; a write of the program's after it still is."""
    ptr, idx, val = esolve_drv.sym_csr()
    n = len(ptr) - 1
    x = _x(n)
    A = lisdrv.make_csr(lib, ptr, idx, val)
    lisdrv.matvec(lib, A, x)
    assert lib.lis_matrix_shift_diagonal(A, 1.5) == 0 and lib.dll.lis_amd_matrix_host_written(A) == 0
    want = em.shift_csr_values(ptr, idx, val, 1.5)
    A.contents.value[3] = 42.0
    want[3] = 42.0
    assert same_bits(lisdrv.matvec(lib, A, x), orc.spmv_csr(ptr, idx, want, x))
    lib.lis_matrix_destroy(A)


def test_stale_caches_and_the_transposed_copy_go(lib):
    """lis_solve with -p ilu and with -i bicg on the shifted matrix equals the same solves on a matrix built shifted from the start: the ILU factor and
    A^T cached on the copy before the shift must not come back."""
    ptr, idx, val = esolve_drv.sym_csr()
    n = len(ptr) - 1
    b = orc.spmv_csr(ptr, idx, val, np.ones(n))
    A = lisdrv.make_csr(lib, ptr, idx, val)
    opts = ("-i cg -p ilu -tol 1e-12 -maxiter 300 -print mem", "-i bicg -p none -tol 1e-12 -maxiter 300 -print mem")
    before = [lisdrv.solve(lib, A, b, o) for o in opts]                      # caches the factor and the transposed copy
    assert all(r["err"] == 0 and r["status"] == 0 for r in before)
    assert lib.lis_matrix_shift_diagonal(A, 0.8) == 0
    B = lisdrv.make_csr(lib, ptr, idx, em.shift_csr_values(ptr, idx, val, 0.8))
    for o, old in zip(opts, before):
        ra, rb = lisdrv.solve(lib, A, b, o), lisdrv.solve(lib, B, b, o)
        assert (ra["iter"], ra["status"]) == (rb["iter"], rb["status"]) and ra["status"] == 0
        assert same_bits(ra["rhistory"], rb["rhistory"]) and same_bits(ra["x"], rb["x"])
        assert not same_bits(ra["x"], old["x"])
    lib.lis_matrix_destroy(A)
    lib.lis_matrix_destroy(B)


@pytest.mark.parametrize("sigma", [1.5, 5e-324])
def test_split_matrix_shifts_D(lib, sigma):
    ptr, idx, val = orc.poisson3d(5, 4, 3)
    val = val * (1.0 + 1e-3 * np.cos(np.arange(len(val))))
    n = len(ptr) - 1
    x = _x(n)
    A = lisdrv.make_csr(lib, ptr, idx, val)
    assert lib.lis_matrix_split(A) == 0
    assert same_bits(lisdrv.matvec(lib, A, x), orc.spmv_split_csr(ptr, idx, val, x))
    d0 = lisdrv.split_arrays(A)["D"]
    assert lib.lis_matrix_shift_diagonal(A, sigma) == 0
    want = em.shift_csr_values(ptr, idx, val, sigma)                         # (every row stores its diagonal: D - sigma is the shifted matrix's D)
    assert same_bits(lisdrv.matvec(lib, A, x), orc.spmv_split_csr(ptr, idx, want, x))
    assert same_bits(lisdrv.split_arrays(A)["D"], d0 - sigma)
    B = lisdrv.make_csr(lib, ptr, idx, want)
    assert lib.lis_matrix_split(B) == 0
    assert same_bits(lisdrv.matvech(lib, A, x), lisdrv.matvech(lib, B, x))
    lib.lis_matrix_destroy(A)
    lib.lis_matrix_destroy(B)


@pytest.mark.parametrize("sigma", SIGMAS)
def test_matrix_that_lives_in_hbm_only(lib, sigma):
    ptr, idx, val = em.shift_matrix()
    n = len(ptr) - 1
    x = _x(n)
    dptr, didx, dval = DA.from_host(ptr, np.int32), DA.from_host(idx, np.int32), DA.from_host(val, np.float64)
    A = capi.PM()
    assert lib.lis_matrix_create(0, C.byref(A)) == 0 and lib.lis_matrix_set_size(A, n, 0) == 0
    assert lib.dll.lis_amd_matrix_set_csr_device(len(idx), n, dptr.ptr, didx.ptr, dval.ptr, A) == 0
    value_at = dval.ptr
    dptr.ptr = didx.ptr = dval.ptr = None                                    # owned by A now
    assert same_bits(lisdrv.matvec(lib, A, x), orc.spmv_csr(ptr, idx, val, x))
    assert lib.lis_matrix_shift_diagonal(A, sigma) == 0
    want = em.shift_csr_values(ptr, idx, val, sigma)
    got = np.empty(len(val))
    check(lib.liship_memcpy_d2h(got.ctypes.data, value_at, got.nbytes, None))
    check(lib.liship_device_synchronize())
    assert same_bits(got, want)                                               # edited where it lies
    with np.errstate(all="ignore"):
        assert same_bits(np.nan_to_num(lisdrv.matvec(lib, A, x), nan=7.0), np.nan_to_num(orc.spmv_csr(ptr, idx, want, x), nan=7.0))
    lib.lis_matrix_destroy(A)


def test_hbm_only_matrix_with_value_records_keeps_the_right_product(lib):
    """A constant-coefficient stencil born in HBM: the plan's value records of the unshifted matrix are gone with the shift."""
    N = 12
    P = capi.PM()
    assert lib.lis_matrix_create(0, C.byref(P)) == 0 and lib.lis_matrix_set_size(P, 0, N ** 3) == 0
    lib.dll.lis_amd_matrix_poisson3d.argtypes = [capi.PM, C.c_int, C.c_int, C.c_int, C.c_int]
    assert lib.dll.lis_amd_matrix_poisson3d(P, N, N, N, 0) == 0
    ptr, idx, val = orc.poisson3d(N, N, N)
    x = _x(N ** 3)
    assert same_bits(lisdrv.matvec(lib, P, x), orc.spmv_csr(ptr, idx, val, x))
    for sigma in (0.37, -0.37):
        assert lib.lis_matrix_shift_diagonal(P, sigma) == 0
        val = em.shift_csr_values(ptr, idx, val, sigma)
        assert same_bits(lisdrv.matvec(lib, P, x), orc.spmv_csr(ptr, idx, val, x))
    lib.lis_matrix_destroy(P)


@pytest.mark.parametrize("fmt", ["csc", "ell", "dia", "jad", "bsr"])
def test_other_formats_take_the_host_path_and_drop_the_copy(lib, fmt):
    ptr, idx, val = em.shift_matrix(twice=False)
    n = len(ptr) - 1
    x = _x(n)
    A0 = lisdrv.make_csr(lib, ptr, idx, val)
    A = lisdrv.convert(lib, A0, fmt)
    y0 = lisdrv.matvec(lib, A, x)                                             # the copy exists
    before = lisdrv.matrix_arrays(A)
    assert lib.lis_matrix_shift_diagonal(A, 1.5) == 0
    want = em.shift(fmt, before, before["value"], 1.5)
    assert same_bits(lisdrv.matrix_arrays(A)["value"], want)
    B0 = lisdrv.make_csr(lib, ptr, idx, val)
    B = lisdrv.convert(lib, B0, fmt)
    C.memmove(B.contents.value, want.ctypes.data, want.nbytes)               # a matrix holding the shifted arrays from the start
    assert lib.dll.lis_amd_matrix_host_modified(B) == 0
    y = lisdrv.matvec(lib, A, x)
    assert same_bits(y, lisdrv.matvec(lib, B, x)) and not same_bits(y, y0)
    for m in (A, A0, B, B0):
        lib.lis_matrix_destroy(m)


def test_ell_made_in_hbm_from_an_hbm_only_matrix_shifts_through_its_host_arrays(lib):
    """lis_matrix_convert builds the ELL arrays in HBM and leaves the host arrays to their first touch: the shift is that touch, once, and the copy is dropped.
    (A matrix that lives in HBM only and is not CSR cannot be made through the API; lis_matrix_shift_diagonal refuses it all the same.)"""
    ptr, idx, val = orc.poisson3d(4, 4, 4)
    n = len(ptr) - 1
    x = _x(n)
    dptr, didx, dval = DA.from_host(ptr, np.int32), DA.from_host(idx, np.int32), DA.from_host(val, np.float64)
    A = capi.PM()
    assert lib.lis_matrix_create(0, C.byref(A)) == 0 and lib.lis_matrix_set_size(A, n, 0) == 0
    assert lib.dll.lis_amd_matrix_set_csr_device(len(idx), n, dptr.ptr, didx.ptr, dval.ptr, A) == 0
    dptr.ptr = didx.ptr = dval.ptr = None
    E = lisdrv.convert(lib, A, "ell")
    lisdrv.matvec(lib, E, x)
    assert lib.lis_matrix_shift_diagonal(E, 0.5) == 0
    B0 = lisdrv.make_csr(lib, ptr, idx, em.shift_csr_values(ptr, idx, val, 0.5))
    B = lisdrv.convert(lib, B0, "ell")
    assert same_bits(lisdrv.matvec(lib, E, x), lisdrv.matvec(lib, B, x))
    assert same_bits(lisdrv.matrix_arrays(E)["value"], lisdrv.matrix_arrays(B)["value"])
    for m in (E, A, B, B0):
        lib.lis_matrix_destroy(m)
