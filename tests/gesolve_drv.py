"""Drive lis_gesolve and lis_matrix_shift_matrix of a library exporting the Lis C API (the reference build or this repo's liblis_amd.so) from numpy.

The calls are those of the reference's test/getest1.c: lis_esolver_create -> lis_esolver_set_option -> lis_gesolve -> the getters.  lis_matrix_shift_matrix is
exported by both libraries (the reference declares it in its internal header only).  open_lib and the matrix helpers are lisdrv's."""
import ctypes as C

import numpy as np

import lisdrv
from lis_amd import _capi as capi

open_lib = lisdrv.open_lib


def _bind(lib):
    fn = lib.dll.lis_matrix_shift_matrix
    fn.restype, fn.argtypes = capi.LIS_INT, [capi.PM, capi.PM, capi.LIS_SCALAR]
    return fn


def make(lib, m):
    return lisdrv.make_csr(lib, *m)


def gesolve(lib, A, B, options, x0=None):
    """lis_gesolve with `options` text -> dict(err, evalue, x, iter, status, resid, rhistory)"""
    vx = lisdrv.new_vector(lib, A, x0)
    E = capi.PE()
    assert lib.lis_esolver_create(C.byref(E)) == 0
    err = lib.lis_esolver_set_option(options.encode(), E)
    ev = C.c_double(-7.0)
    out = dict(err=err)
    if err == 0:
        err = lib.lis_gesolve(A, B, vx, C.byref(ev), E)
        out["err"] = err
    e = E.contents
    out.update(status=e.retcode, evalue=ev.value, x=lisdrv.get_vector(lib, vx, A.contents.n))
    if err == 0:
        it, res, st = C.c_int(), C.c_double(), C.c_int()
        lib.lis_esolver_get_iter(E, C.byref(it))
        lib.lis_esolver_get_residualnorm(E, C.byref(res))
        lib.lis_esolver_get_status(E, C.byref(st))
        count = it.value + 1 - (1 if st.value != 0 else 0)          # lis_esolver_get_rhistory's length (lis_esolver.c:1138-1142)
        out.update(iter=it.value, status=st.value, resid=res.value, rhistory=lisdrv._arr(e.rhistory, count, np.float64))
    lib.lis_esolver_destroy(E)
    lib.lis_vector_destroy(vx)
    return out


def shift(lib, A, B, sigma):
    return _bind(lib)(A, B, float(sigma))


def csr_arrays(A):
    """(ptr, index, value) of a CSR matrix with host arrays, as numpy copies (a first touch brings arrays held in HBM home)"""
    a = lisdrv.matrix_arrays(A)
    assert a["type"] == capi.LIS_MATRIX_CSR
    return a["ptr"], a["index"], a["value"]


def last_shift(lib):
    info = (C.c_int * 3)()
    assert lib.dll.lis_amd_last_shift_matrix(info) == 0
    return list(info)


# ---------------------------------------------------------------------------------------------- matrices that live in HBM only (liblis_amd.so)
def make_hbm(lib, m):
    """A CSR matrix adopted from arrays in HBM: no host copy exists"""
    from lis_amd import DeviceArray as DA
    ptr, idx, val = m
    n = len(ptr) - 1
    A = capi.PM()
    assert lib.lis_matrix_create(capi.LIS_COMM_WORLD, C.byref(A)) == 0 and lib.lis_matrix_set_size(A, n, 0) == 0
    d = [DA.from_host(ptr, np.int32), DA.from_host(idx if len(idx) else np.zeros(1, np.int32), np.int32), DA.from_host(val if len(val) else np.zeros(1), np.float64)]
    fn = lib.dll.lis_amd_matrix_set_csr_device
    fn.restype, fn.argtypes = capi.LIS_INT, [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, capi.PM]
    assert fn(len(idx), n, d[0].ptr, d[1].ptr, d[2].ptr, A) == 0
    for a in d:
        a.ptr = None                                                 # owned by A now
    return A


def hbm_csr_arrays(lib, A):
    """(ptr, index, value) of the HBM copy of a CSR matrix, read back"""
    import lis_amd
    fn = lib.dll.lis_amd_matrix_device_csr
    fn.restype, fn.argtypes = capi.LIS_INT, [capi.PM, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    p, i, v = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert fn(A, C.byref(p), C.byref(i), C.byref(v)) == 0
    n, nnz = A.contents.n, A.contents.nnz
    ptr, idx, val = np.empty(n + 1, np.int32), np.empty(nnz, np.int32), np.empty(nnz, np.float64)
    for host, dev in ((ptr, p), (idx, i), (val, v)):
        if host.nbytes:
            lis_amd.check(lib.liship_memcpy_d2h(host.ctypes.data, dev.value, host.nbytes, None))
    lis_amd.check(lib.liship_device_synchronize())
    return ptr, idx, val
