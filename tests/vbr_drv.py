"""Drive the VBR entry points of a library exporting the Lis C API (the reference build or this repo's liblis_amd.so) from numpy: lis_matrix_malloc_vbr /
_set_vbr, lis_matrix_set_blocksize with arrays, the raw products lis_matvec[h]_vbr and a reader of the six arrays.  lisdrv's idioms otherwise."""
import ctypes as C

import numpy as np

import coo_dns_drv as drv
import lisdrv
from lis_amd import _capi as capi

VBR = capi.FORMAT_ID["vbr"]
diagonal, raw_product, duplicate_as = drv.diagonal, drv.raw_product, drv.duplicate_as


def make_vbr(lib, v, assemble=True):
    """a VBR matrix (tests/vbr_cases.py dict) whose arrays come from lis_matrix_malloc_vbr"""
    A = capi.PM()
    assert lib.lis_matrix_create(capi.LIS_COMM_WORLD, C.byref(A)) == 0
    assert lib.lis_matrix_set_size(A, v["n"], 0) == 0
    p = [capi.P_INT() for _ in range(5)] + [capi.P_DBL()]
    assert lib.lis_matrix_malloc_vbr(v["n"], max(v["nnz"], 1), v["nr"], v["nc"], max(v["bnnz"], 1), *[C.byref(q) for q in p]) == 0
    for q, f in zip(p, ("row", "col", "ptr", "bptr", "bindex", "value")):
        a = np.ascontiguousarray(v[f], np.float64 if f == "value" else np.int32)
        if a.size:
            lisdrv._copy_in(q, a)
    assert lib.lis_matrix_set_vbr(v["nnz"], v["nr"], v["nc"], v["bnnz"], *p, A) == 0
    if assemble:
        assert lib.lis_matrix_assemble(A) == 0
    return A


def arrays(A):
    """host arrays of an assembled matrix: a tests/vbr_cases.py dict for VBR, lisdrv.matrix_arrays otherwise"""
    a = A.contents
    if a.matrix_type != VBR:
        return lisdrv.matrix_arrays(A)
    i32 = lambda p, count: lisdrv._arr(p, count, np.int32)
    return dict(type=VBR, n=a.n, nr=a.nr, nc=a.nc, bnnz=a.bnnz, nnz=a.nnz, row=i32(a.row, a.nr + 1), col=i32(a.col, a.nc + 1), ptr=i32(a.ptr, a.bnnz + 1),
                bptr=i32(a.bptr, a.nr + 1), bindex=i32(a.bindex, a.bnnz), value=lisdrv._arr(a.value, a.nnz, np.float64))


def set_blocks(lib, B, row, col):
    """lis_matrix_set_blocksize with arrays: the counts first (the reference stores them only in a call without arrays), then the arrays, handed over at
    a length of n entries at least (the reference copies n of each, whatever their length)"""
    nr, nc, n = len(row) - 1, len(col) - 1, B.contents.n
    assert nr + 1 <= n and nc + 1 <= n
    r, c = np.zeros(n, np.int32), np.zeros(n, np.int32)
    r[:nr + 1], c[:nc + 1] = row, col
    assert lib.lis_matrix_set_blocksize(B, nr, nc, None, None) == 0
    return lib.lis_matrix_set_blocksize(B, nr, nc, r.ctypes.data_as(capi.P_INT), c.ctypes.data_as(capi.P_INT))


def to_vbr(lib, A, row=None, col=None):
    """(err, B): lis_matrix_convert of A into a VBR duplicate, with the partition row / col or the one the conversion finds"""
    B = duplicate_as(lib, A, "vbr")
    if row is not None:
        assert set_blocks(lib, B, row, col) == 0
    return lib.lis_matrix_convert(A, B), B


def scale(lib, A, b, action, before):
    """lis_matrix_scale(A, B, D, action) with D holding `before` (VBR leaves the rows its diagonal search misses as they were) -> (err, b after, d)"""
    vb, vd = lisdrv.new_vector(lib, A, b), lisdrv.new_vector(lib, A, before)
    err = lib.lis_matrix_scale(A, vb, vd, action)
    out = (err, lisdrv.get_vector(lib, vb, A.contents.n), lisdrv.get_vector(lib, vd, A.contents.n))
    lib.lis_vector_destroy(vb)
    lib.lis_vector_destroy(vd)
    return out


def convert(lib, A, fmt):
    return drv.convert(lib, A, fmt)
