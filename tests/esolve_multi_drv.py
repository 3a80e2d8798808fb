"""Drive the eigensolvers of several pairs (-e si | li | ai) of a library exporting the Lis C API -- the reference build or liblis_amd.so -- from numpy.

The calls are those of the reference's test/etest5.c: lis_esolver_create -> lis_esolver_set_option -> lis_esolve, then everything the solve left is read from
LIS_ESOLVER_STRUCT itself before lis_esolver_destroy (evalue[], resid[], iter[] of ss entries, evector[], rhistory), so that the reference's bits and this
library's come through one path.  The cases the goldens, the CPU and the GPU tests share are listed here as well."""
import ctypes as C

import numpy as np

import esolve_drv
import lisdrv
from lis_amd import _capi as capi

ETOL = 1e-10
BIT_COMMON = " -etol 1e-10 -emaxiter 60 -eprint mem"
TREE_COMMON = " -etol 1e-10 -emaxiter 150"
# (matrix, options): compared in every bit at T = 1 and 8
BIT_CASES = [
    ("sym7", "-e si -ss 3 -ie pi"),
    ("sym7", "-e si -ss 3 -ie ii"),
    ("sym7", "-e si -ss 3 -ie ii -shift 0.75"),
    ("sym7", "-e li -ss 4"),
    ("sym7", "-e li -ss 4 -ie cg"),
    ("sym7", "-e li -ss 3 -rval true"),
    ("sym7", "-e ai -ss 4"),
    ("sym7", "-e ai -ss 4 -ie rqi"),
    ("sym7", "-e li -ss 4 -estorage ell"),
    ("nonsym7", "-e si -ss 3 -ie pi"),
    ("nonsym7", "-e ai -ss 4"),
]
# compared in the tree mode, mode by mode, where the reference converges at T = 1, 2, 4 and 8: (matrix, options, modes that must be admitted)
TREE_CASES = [
    ("sym7", "-e li -ss 4", (0, 1, 2, 3)),
    ("sym7", "-e ai -ss 4", 3),              # a count: at least that many modes
    ("sym7", "-e si -ss 3 -ie pi", (0,)),
]


def subspace(options):
    words = options.split()
    return int(words[words.index("-ss") + 1])


def esolve(lib, A, options):
    """lis_esolve with `options` -> dict(err, status, evalue0, ss, x, evalue[ss]) and, unless the options hold -rval true (the reference leaves heap contents in
    them then), resid[ss], iter[ss], rhistory, evector[ss]; E and vx stay alive for the getters until release()."""
    n = A.contents.n
    ss = subspace(options)
    rval = "-rval true" in options
    vx = lisdrv.new_vector(lib, A)
    E = capi.PE()
    assert lib.lis_esolver_create(C.byref(E)) == 0
    assert lib.lis_esolver_set_option(options.encode(), E) == 0
    ev = C.c_double(-7.0)
    err = lib.lis_esolve(A, vx, C.byref(ev), E)
    e = E.contents
    out = dict(err=err, status=e.retcode, evalue0=ev.value, ss=ss, rval=rval, E=E, vx=vx)
    if err == 0:
        out.update(x=lisdrv.get_vector(lib, vx, n), evalue=lisdrv._arr(e.evalue, ss, np.float64))
    if err == 0 and not rval:
        count = e.iter[0] + 1 - (1 if e.retcode != 0 else 0)
        vecs = C.cast(e.evector, C.POINTER(capi.PV))
        out.update(resid=lisdrv._arr(e.resid, ss, np.float64), iter=lisdrv._arr(e.iter, ss, np.int32), rhistory=lisdrv._arr(e.rhistory, count, np.float64),
                   evector=[lisdrv.get_vector(lib, vecs[i], n) for i in range(ss)])
    return out


def release(lib, res):
    lib.lis_esolver_destroy(res.pop("E"))
    lib.lis_vector_destroy(res.pop("vx"))


def make_matrix(lib, name):
    return esolve_drv.make_matrix(lib, name)
