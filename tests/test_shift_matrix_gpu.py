"""lis_matrix_shift_matrix on the GPU (host/lis_shift.c, kernels/spgeam.hip) against the numpy model of tests/shift_model.py, which tests/test_gesolve_cpu.py
holds to the reference in every bit.  Every case of gesolve_cases.SHIFTS, shift after shift of its sequence:
  - the arrays read back (A's host arrays, filled from HBM on this first touch; for a matrix that lives in HBM only the copy's own arrays) equal the model's bits;
  - lis_matvec of the shifted A equals the CPU oracle's product of the model's arrays: the HBM copy and its plan followed;
  - lis_amd_last_shift_matrix reports the path the model's rule names (in place or rebuilt) and the nnz before and after.
A in ELL and in BSR 2 x 2 goes X -> CSR -> shift -> X: the expected arrays are the model's rows converted by the oracle (the reference itself leaves such an A
untouched and says LIS_SUCCESS: tests/golden/make_golden_gesolve.py)."""
import ctypes as C

import numpy as np
import pytest

import gesolve_cases as gc
import gesolve_drv as gd
import lis_amd
import lisdrv
import orc
import shift_model as sm
from lis_amd import _capi as capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    lib = lis_amd.load()
    assert lis_amd.gpu_available(), "no HIP device: the product path has no CPU fallback"
    assert lib.initialize([]) == 0
    return lib


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.int64), np.ascontiguousarray(b, np.float64).view(np.int64))


def _x(n):
    return np.sin(np.arange(n) * 0.7) + 0.25


def _check_csr(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, "ptr")
    assert np.array_equal(got[1], want[1]), (what, "index")
    assert same_bits(got[2], want[2]), (what, "value")


@pytest.mark.parametrize("name", sorted(gc.SHIFTS))
def test_every_shift_case_equals_the_model(lib, name):
    maker, sigmas, storage = gc.SHIFTS[name]
    a, b = maker()
    n = len(a[0]) - 1
    x = _x(n)
    B = gd.make(lib, b)
    if storage == "hbm":
        A = gd.make_hbm(lib, a)
    else:
        A = gd.make(lib, a)
        if storage in ("ell", "bsr"):
            X = lisdrv.convert(lib, A, storage)
            lib.lis_matrix_destroy(A)
            A = X
            back = lisdrv.convert(lib, A, "csr")                       # the rows the shift will see: X -> CSR by the library's converter
            a = gd.csr_arrays(back)
            lib.lis_matrix_destroy(back)
    lisdrv.matvec(lib, A, x)                                           # the HBM copy and its plan exist before the first shift
    nnz = len(a[1])
    for step, (ptr, idx, val, in_place) in enumerate(sm.apply(a, b, sigmas)):
        assert gd.shift(lib, A, B, sigmas[step]) == 0
        info = gd.last_shift(lib)
        print(name, step, "sigma", sigmas[step], "info", info, "model", [int(in_place), nnz, len(idx)])
        assert info == [int(in_place), nnz, len(idx)], (name, step)
        nnz = len(idx)
        want_y = orc.spmv_csr(ptr, idx, val, x)
        if storage == "ell":
            mx, eidx, eval_ = orc.csr2ell(ptr, idx, val)
            got = lisdrv.matrix_arrays(A)
            assert got["type"] == capi.LIS_MATRIX_ELL and got["maxnzr"] == mx
            assert np.array_equal(got["index"], eidx) and same_bits(got["value"], eval_)
            want_y = orc.spmv_ell(n, mx, eidx, eval_, x)
        elif storage == "bsr":
            nr, bptr, bidx, bval = orc.csr2bsr(ptr, idx, val)
            got = lisdrv.matrix_arrays(A)
            assert got["type"] == capi.LIS_MATRIX_BSR and (got["bnr"], got["bnc"], got["nr"]) == (2, 2, nr)
            assert np.array_equal(got["bptr"], bptr) and np.array_equal(got["bindex"], bidx) and same_bits(got["value"], bval)
            want_y = orc.spmv_bsr(n, nr, 2, 2, bptr, bidx, bval, x)
        elif storage == "hbm":
            assert A.contents.nnz == len(idx)
            _check_csr(gd.hbm_csr_arrays(lib, A), (ptr, idx, val), (name, step))
        else:
            assert A.contents.nnz == len(idx) and A.contents.matrix_type == capi.LIS_MATRIX_CSR
            _check_csr(gd.csr_arrays(A), (ptr, idx, val), (name, step))          # (a first touch: the arrays come home from HBM)
        assert same_bits(lisdrv.matvec(lib, A, x), want_y), (name, step, "product")
    lib.lis_matrix_destroy(A)
    lib.lis_matrix_destroy(B)


def test_host_arrays_stay_in_hbm_until_they_are_read_and_writes_are_still_seen(lib):
    """After a shift A's host arrays are address space bound to the copy's buffers: nothing crosses the bus until the program reads them; a program's write
    after that is seen by the write watch, and the next product is the product of what the program wrote."""
    a, b = gc.P3()
    n = len(a[0]) - 1
    x = _x(n)
    A, B = gd.make(lib, a), gd.make(lib, b)
    assert gd.shift(lib, A, B, 0.3) == 0
    ptr, idx, val, _ = sm.apply(a, b, (0.3,))[0]
    assert lib.dll.lis_amd_matrix_lazy_arrays(A) == 3
    assert same_bits(lisdrv.matvec(lib, A, x), orc.spmv_csr(ptr, idx, val, x))
    assert lib.dll.lis_amd_matrix_lazy_arrays(A) == 3                   # a product reads none of them
    _check_csr(gd.csr_arrays(A), (ptr, idx, val), "read back")
    assert lib.dll.lis_amd_matrix_lazy_arrays(A) == 0 and lib.dll.lis_amd_matrix_host_written(A) == 0
    A.contents.value[3] = 1.75                                          # the program edits the matrix
    assert lib.dll.lis_amd_matrix_host_written(A) == 1
    val = val.copy()
    val[3] = 1.75
    assert same_bits(lisdrv.matvec(lib, A, x), orc.spmv_csr(ptr, idx, val, x))
    assert gd.shift(lib, A, B, -0.3) == 0                               # ... and a shift after that starts from the edited matrix
    ptr2, idx2, val2, _ = sm.apply((ptr, idx, val), b, (-0.3,))[0]
    _check_csr(gd.csr_arrays(A), (ptr2, idx2, val2), "after the edit")
    lib.lis_matrix_destroy(A)
    lib.lis_matrix_destroy(B)


def test_solves_after_a_shift_run_on_the_shifted_matrix(lib):
    """lis_solve -i bicg (which builds A^T on the copy) before and after a rebuilding shift: the transposed copy of the old matrix must not come back"""
    a, b = gc.P4()
    n = len(a[0]) - 1
    rhs = _x(n)
    A, B = gd.make(lib, a), gd.make(lib, b)
    lisdrv.solve(lib, A, rhs, "-i bicg -p none -tol 1e-12 -maxiter 200")
    assert gd.shift(lib, A, B, 0.005) == 0 and gd.last_shift(lib)[0] == 0
    ptr, idx, val, _ = sm.apply(a, b, (0.005,))[0]
    fresh = gd.make(lib, (ptr, idx, val))
    got = lisdrv.solve(lib, A, rhs, "-i bicg -p none -tol 1e-12 -maxiter 200")
    want = lisdrv.solve(lib, fresh, rhs, "-i bicg -p none -tol 1e-12 -maxiter 200")
    assert got["iter"] == want["iter"] and same_bits(got["x"], want["x"])
    for M in (A, B, fresh):
        lib.lis_matrix_destroy(M)


def test_B_in_another_storage_and_A_shifted_by_itself(lib):
    a, b = gc.P3()
    n = len(a[0]) - 1
    x = _x(n)
    A, B0 = gd.make(lib, a), gd.make(lib, b)
    B = lisdrv.convert(lib, B0, "ell")
    assert gd.shift(lib, A, B, 0.3) == 0
    ptr, idx, val, _ = sm.apply(a, b, (0.3,))[0]
    _check_csr(gd.csr_arrays(A), (ptr, idx, val), "B in ELL")
    assert gd.shift(lib, A, A, 0.25) == 0                               # A <- A - 0.25 A
    ptr2, idx2, val2, _ = sm.apply((ptr, idx, val), (ptr, idx, val), (0.25,))[0]
    _check_csr(gd.csr_arrays(A), (ptr2, idx2, val2), "A by itself")
    assert same_bits(lisdrv.matvec(lib, A, x), orc.spmv_csr(ptr2, idx2, val2, x))
    for M in (A, B, B0):
        lib.lis_matrix_destroy(M)


def test_launcher_argument_checks(lib):
    flag = lis_amd.DeviceArray.zeros(4, np.int32)
    nnz = C.c_int(-1)
    assert lib.liship_csr_shift_matrix_try_f64(-1, None, None, None, None, None, None, 1.0, None, None, flag.ptr, None) == -1
    assert lib.liship_csr_shift_matrix_try_f64(3, None, None, None, None, None, None, 1.0, None, None, flag.ptr, None) == -1
    assert lib.liship_csr_shift_matrix_try_f64(0, None, None, None, None, None, None, 1.0, None, None, None, None) == -1
    assert lib.liship_csr_shift_matrix_try_f64(0, None, None, None, None, None, None, 1.0, None, None, flag.ptr, None) == 0
    assert lib.liship_csr_shift_matrix_scan(-1, None, flag.ptr, None, C.byref(nnz), None) == -1
    assert lib.liship_csr_shift_matrix_scan(0, None, flag.ptr, None, C.byref(nnz), None) == 0 and nnz.value == 0
    assert lib.liship_csr_shift_matrix_fill_f64(-1, None, None, None, None, None, None, 1.0, None, None, None, None, None) == -1
    assert lib.liship_csr_shift_matrix_fill_f64(0, None, None, None, None, None, None, 1.0, None, None, None, None, None) == 0
