"""Drive the COO / DNS entry points of a library exporting the Lis C API (the reference build or this repo's liblis_amd.so) from numpy:
lis_matrix_malloc_coo / _set_coo / _malloc_dns / _set_dns, the raw products lis_matvec[h]_coo / _dns, and readers of the two layouts.
lisdrv's idioms otherwise (create -> set_size -> set_<fmt> -> assemble)."""
import ctypes as C

import numpy as np

import lisdrv
from lis_amd import _capi as capi

COO, DNS = capi.FORMAT_ID["coo"], capi.FORMAT_ID["dns"]


def _new(lib, n):
    A = capi.PM()
    assert lib.lis_matrix_create(capi.LIS_COMM_WORLD, C.byref(A)) == 0
    assert lib.lis_matrix_set_size(A, n, 0) == 0
    return A


def make_coo(lib, n, row, col, val, assemble=True):
    """a COO matrix whose arrays come from lis_matrix_malloc_coo"""
    A = _new(lib, n)
    nnz = len(row)
    r, c, v = capi.P_INT(), capi.P_INT(), capi.P_DBL()
    assert lib.lis_matrix_malloc_coo(max(nnz, 1), C.byref(r), C.byref(c), C.byref(v)) == 0
    if nnz:
        lisdrv._copy_in(r, np.ascontiguousarray(row, np.int32))
        lisdrv._copy_in(c, np.ascontiguousarray(col, np.int32))
        lisdrv._copy_in(v, np.ascontiguousarray(val, np.float64))
    assert lib.lis_matrix_set_coo(nnz, r, c, v, A) == 0
    if assemble:
        assert lib.lis_matrix_assemble(A) == 0
    return A


def make_dns(lib, n, dns, assemble=True):
    """a DNS matrix (n x n, column-major values) whose array comes from lis_matrix_malloc_dns"""
    A = _new(lib, n)
    v = capi.P_DBL()
    assert lib.lis_matrix_malloc_dns(n, n, C.byref(v)) == 0
    lisdrv._copy_in(v, np.ascontiguousarray(dns, np.float64))
    assert lib.lis_matrix_set_dns(v, A) == 0
    if assemble:
        assert lib.lis_matrix_assemble(A) == 0
    return A


def arrays(A):
    """host arrays of an assembled matrix: lisdrv.matrix_arrays plus the two layouts it does not know"""
    a = A.contents
    if a.matrix_type == COO:
        return dict(type=COO, n=a.n, np=a.np, nnz=a.nnz, row=lisdrv._arr(a.row, a.nnz, np.int32), col=lisdrv._arr(a.col, a.nnz, np.int32),
                    value=lisdrv._arr(a.value, a.nnz, np.float64))
    if a.matrix_type == DNS:
        return dict(type=DNS, n=a.n, np=a.np, nnz=a.nnz, value=lisdrv._arr(a.value, a.n * a.np, np.float64))
    return lisdrv.matrix_arrays(A)


def duplicate_as(lib, A, fmt):
    """lis_matrix_duplicate + set_type: the target of a conversion or copy"""
    B = capi.PM()
    assert lib.lis_matrix_duplicate(A, C.byref(B)) == 0
    assert lib.lis_matrix_set_type(B, capi.FORMAT_ID[fmt]) == 0
    return B


def convert(lib, A, fmt):
    """(err, B): lis_matrix_convert into a duplicate of type fmt"""
    B = duplicate_as(lib, A, fmt)
    return lib.lis_matrix_convert(A, B), B


def raw_product(lib, A, fmt, x, transposed=False):
    """lis_matvec_<fmt> / lis_matvech_<fmt> on raw host arrays"""
    fn = getattr(lib.dll, "lis_matvec%s_%s" % ("h" if transposed else "", fmt))
    fn.restype, fn.argtypes = None, [capi.PM, capi.P_DBL, capi.P_DBL]
    x = np.ascontiguousarray(x, np.float64)
    y = np.full(A.contents.np, np.nan)
    fn(A, x.ctypes.data_as(capi.P_DBL), y.ctypes.data_as(capi.P_DBL))
    return y


def diagonal(lib, A, before=None):
    """lis_matrix_get_diagonal into a vector that held `before`"""
    d = lisdrv.new_vector(lib, A, before)
    err = lib.lis_matrix_get_diagonal(A, d)
    out = lisdrv.get_vector(lib, d, A.contents.n)
    lib.lis_vector_destroy(d)
    return err, out


def scale(lib, A, b, action):
    """lis_matrix_scale(A, B, D, action) -> (err, b after, d)"""
    vb = lisdrv.new_vector(lib, A, b)
    vd = lisdrv.new_vector(lib, A)
    err = lib.lis_matrix_scale(A, vb, vd, action)
    out = (err, lisdrv.get_vector(lib, vb, A.contents.n), lisdrv.get_vector(lib, vd, A.contents.n))
    lib.lis_vector_destroy(vb)
    lib.lis_vector_destroy(vd)
    return out
