"""Sources of tests/tocsr_cases.py as matrices of a library exporting the Lis C API (the reference build or liblis_amd.so): made from their arrays through
lis_matrix_malloc_<fmt> / lis_matrix_set_<fmt>, read back under the same names, converted to CSR.  lisdrv's idioms otherwise."""
import ctypes as C

import numpy as np

import coo_dns_drv
import lisdrv
import vbr_drv
from lis_amd import _capi as capi


def _new(lib, n):
    A = capi.PM()
    assert lib.lis_matrix_create(capi.LIS_COMM_WORLD, C.byref(A)) == 0
    assert lib.lis_matrix_set_size(A, n, 0) == 0
    return A


def _fill(pairs):
    for p, a, t in pairs:
        a = np.ascontiguousarray(a, t)
        if a.size:
            lisdrv._copy_in(p, a)


def make(lib, s):
    """the source as an assembled matrix whose arrays are the library's own"""
    fmt, n = s["fmt"], s["n"]
    if fmt == "vbr":
        return vbr_drv.make_vbr(lib, s)
    if fmt == "dns":
        return coo_dns_drv.make_dns(lib, n, s["value"])
    A = _new(lib, n)
    i, j, k, v = capi.P_INT(), capi.P_INT(), capi.P_INT(), capi.P_DBL()
    if fmt == "ell":
        assert lib.lis_matrix_malloc_ell(n, max(s["maxnzr"], 1), C.byref(i), C.byref(v)) == 0
        _fill([(i, s["index"], np.int32), (v, s["value"], np.float64)])
        assert lib.lis_matrix_set_ell(s["maxnzr"], i, v, A) == 0
    elif fmt == "dia":
        assert lib.lis_matrix_malloc_dia(n, max(s["nnd"], 1), C.byref(i), C.byref(v)) == 0
        _fill([(i, s["index"], np.int32), (v, s["value"], np.float64)])
        assert lib.lis_matrix_set_dia(s["nnd"], i, v, A) == 0
    elif fmt == "bsr":
        assert lib.lis_matrix_malloc_bsr(n, s["bnr"], s["bnc"], max(s["bnnz"], 1), C.byref(i), C.byref(j), C.byref(v)) == 0
        _fill([(i, s["bptr"], np.int32), (j, s["bindex"], np.int32), (v, s["value"], np.float64)])
        assert lib.lis_matrix_set_bsr(s["bnr"], s["bnc"], s["bnnz"], i, j, v, A) == 0
    elif fmt == "csc":
        nnz = len(s["index"])
        assert lib.lis_matrix_malloc_csc(n, max(nnz, 1), C.byref(i), C.byref(j), C.byref(v)) == 0
        _fill([(i, s["ptr"], np.int32), (j, s["index"], np.int32), (v, s["value"], np.float64)])
        assert lib.lis_matrix_set_csc(nnz, i, j, v, A) == 0
    else:
        assert fmt == "jad"
        nnz = len(s["index"])
        assert lib.lis_matrix_malloc_jad(n, max(nnz, 1), max(s["maxnzr"], 1), C.byref(i), C.byref(j), C.byref(k), C.byref(v)) == 0
        _fill([(i, s["row"], np.int32), (j, s["ptr"], np.int32), (k, s["index"], np.int32), (v, s["value"], np.float64)])
        assert lib.lis_matrix_set_jad(nnz, s["maxnzr"], i, j, k, v, A) == 0
    assert lib.lis_matrix_assemble(A) == 0
    return A


def arrays(A):
    """host arrays of an assembled matrix of any of the nine formats (reads them: arrays held in HBM come home)"""
    return vbr_drv.arrays(A) if A.contents.matrix_type == vbr_drv.VBR else coo_dns_drv.arrays(A)


def unchanged(A, s):
    """A still holds the source's arrays, every integer and every bit"""
    got = arrays(A)
    for key, want in s.items():
        if not isinstance(want, np.ndarray):
            continue
        g = got[key]
        if want.dtype == np.float64:
            if np.ascontiguousarray(g, np.float64).tobytes() != np.ascontiguousarray(want).tobytes():
                return False
        elif not np.array_equal(g, want):
            return False
    return True


def to_csr(lib, A):
    """(err, B): lis_matrix_convert into a CSR duplicate"""
    return coo_dns_drv.convert(lib, A, "csr")


def csr_arrays(B):
    a = lisdrv.matrix_arrays(B)
    assert a["type"] == capi.LIS_MATRIX_CSR
    return a["ptr"], a["index"], a["value"]


def stats(lib):
    out = (C.c_int * 2)()
    assert lib.dll.lis_amd_convert_stats(out) == 0
    return out[0], out[1]
