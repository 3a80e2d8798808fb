"""Drive lis_esolve of a library exporting the Lis C API (the reference build or this repo's liblis_amd.so) from numpy.

The calls are those of the reference's test/etest1.c: lis_esolver_create -> lis_esolver_set_option -> lis_esolve -> the getters.
open_lib is lisdrv's idiom (load + lis_initialize once per path; threads only matters for the OpenMP reference build), and the
matrices are lisdrv's.  The matrices the goldens, the model and the GPU tests share are built here too, so that all three see the
same bits."""
import ctypes as C
import os

import numpy as np

import lisdrv
import orc
from lis_amd import _capi as capi

HERE = os.path.dirname(os.path.abspath(__file__))
open_lib = lisdrv.open_lib


def esolve(lib, A, options, x0=None):
    """lis_esolve with `options` text -> dict(err, evalue, x, iter, status, resid, rhistory); x0: the caller's x (-initx_ones false reads it)."""
    vx = lisdrv.new_vector(lib, A, x0)
    E = capi.PE()
    assert lib.lis_esolver_create(C.byref(E)) == 0
    err = lib.lis_esolver_set_option(options.encode(), E)
    ev = C.c_double(0.0)
    out = dict(err=err)
    if err == 0:
        err = lib.lis_esolve(A, vx, C.byref(ev), E)
        out["err"] = err
    e = E.contents
    out.update(status=e.retcode, options=list(e.options), params=list(e.params))
    if err == 0:
        it, res, st = C.c_int(), C.c_double(), C.c_int()
        lib.lis_esolver_get_iter(E, C.byref(it))
        lib.lis_esolver_get_residualnorm(E, C.byref(res))
        lib.lis_esolver_get_status(E, C.byref(st))
        count = it.value + 1 - (1 if st.value != 0 else 0)          # lis_esolver_get_rhistory's length (lis_esolver.c:1138-1142)
        out.update(evalue=ev.value, x=lisdrv.get_vector(lib, vx, A.contents.n), iter=it.value, status=st.value, resid=res.value,
                   rhistory=lisdrv._arr(e.rhistory, count, np.float64))
    lib.lis_esolver_destroy(E)
    lib.lis_vector_destroy(vx)
    return out


def parsed(lib, options):
    """(err, options[], params[]) of a fresh esolver after lis_esolver_set_option(options)."""
    E = capi.PE()
    assert lib.lis_esolver_create(C.byref(E)) == 0
    err = lib.lis_esolver_set_option(options.encode(), E)
    options = list(E.contents.options)
    options[11] = 0       # LIS_EOPTIONS_SWITCH_MAXITER: lis_esolver_init (lis_esolver.c:143-187) never sets it and no option names it -- heap contents in the reference
    got = (err, options, list(E.contents.params))
    lib.lis_esolver_destroy(E)
    return got


# option strings whose parse the tests hold to the reference's tables (lis_esolver.c:103-122): every option, -e by name and by number, values out of range,
# names that do not exist (an error), unknown options (ignored), upper case (folded), a number where a name may stand
OPTION_TEXTS = [
    "", "-e pi", "-e ii", "-e rqi", "-e cg", "-e cr", "-e si", "-e li", "-e ai", "-e gpi", "-e gai", "-e 1", "-e 5", "-e 16", "-e 17", "-e 0", "-e 99", "-e CG",
    "-e nosuch", "-emaxiter 37", "-emaxiter -3", "-emaxiter abc", "-etol 1e-6", "-etol 2.5E-3", "-ss 4", "-m 2", "-shift 0.75", "-shift -1.25e2",
    "-shift_im 3", "-eprint none", "-eprint mem", "-eprint out", "-eprint all", "-eprint 2", "-eprint 3", "-eprint 7", "-eprint loud", "-initx_ones false",
    "-initx_ones true", "-initx_ones 0", "-initx_ones 1", "-initx_ones 2", "-initx_ones maybe", "-ie pi", "-ie ii", "-ie 3", "-ie nosuch", "-ige gii", "-ige 12",
    "-estorage csr", "-estorage ell", "-estorage dns", "-estorage 7", "-estorage 42", "-estorage xyz", "-estorage_block 3", "-ef double", "-ef quad", "-ef switch",
    "-ef 0", "-ef 1", "-ef 2", "-ef half", "-rval true", "-rval false", "-rval 1", "-rval 2", "-nosuch 5", "-i cg -p jacobi", "-tol 1e-3 -maxiter 7",
    "-e ii -shift 0.5 -etol 1e-9 -emaxiter 200 -eprint mem -initx_ones false -estorage bsr -estorage_block 3", "-e pi -e cr", "-e nosuch -emaxiter 5",
    "-emaxiter 5 -e nosuch", "-shift", "-e", "-E PI -ETOL 1E-3",
]


def from_file(lib, path):
    A, b, x = capi.PM(), capi.PV(), capi.PV()
    assert lib.lis_matrix_create(capi.LIS_COMM_WORLD, C.byref(A)) == 0
    assert lib.lis_vector_create(capi.LIS_COMM_WORLD, C.byref(b)) == 0 and lib.lis_vector_create(capi.LIS_COMM_WORLD, C.byref(x)) == 0
    assert lib.lis_input(A, b, x, path.encode()) == 0
    lib.lis_vector_destroy(b)
    lib.lis_vector_destroy(x)
    return A


# ---------------------------------------------------------------------------------------------- the shared matrices
def sym_csr():
    """7-point Poisson on 7^3 (an odd side: the all-ones start vector is not orthogonal to the extreme modes) with a varied diagonal -- 6 + 3 i / n, and
    20 in the centre row, which lifts one eigenvalue clear of the rest -- so that both ends of the spectrum are well separated."""
    ptr, idx, val = orc.poisson3d(7, 7, 7)
    val = val.copy()
    n = len(ptr) - 1
    for i in range(n):
        for k in range(ptr[i], ptr[i + 1]):
            if idx[k] == i:
                val[k] = 20.0 if i == n // 2 else 6.0 + 3.0 * i / n
    return ptr, idx, val


def nonsym_csr():
    """The same grid with the couplings to lower-numbered neighbours weakened (-0.5 instead of -1): nonsymmetric, real dominant eigenvalue (power iteration only)."""
    ptr, idx, val = sym_csr()
    val = val.copy()
    for i in range(len(ptr) - 1):
        for k in range(ptr[i], ptr[i + 1]):
            if idx[k] < i:
                val[k] = -0.5
    return ptr, idx, val


_START = {}


def start_vector(n):
    """The caller's x for -initx_ones false on sym_csr's grid (n = s^3): close to the lowest eigenvector (overlap 1 - 1e-4, Rayleigh quotient within
    3e-4 of the eigenvalue 1.377, the next one is 1.802).  Why so close: Rayleigh quotient iteration solves (A - rho I) y = v with rho = <v, A v>, and
    the first step of the reference's inner BiCG divides by <v, (A - rho I) v> -- zero but for rounding -- so which eigenpair the iteration ends at from
    a start BETWEEN two of them hangs on the last bits of its sums.  From here every order of summation ends at the same pair; make_golden_esolve.py
    asserts that of the reference at T = 1, 2, 4, 8.
    Made by a Chebyshev filter of degree 16 that damps the eigenvalues in [1.78, 20.6], applied to a parabola g (s + 1 - g) along each axis (the shape
    of the Dirichlet grid's lowest mode): products by the CPU oracle and element-wise passes only, the same bits wherever it runs."""
    if n not in _START:
        s = int(round(n ** (1.0 / 3.0)))
        assert s ** 3 == n, n
        ptr, idx, val = sym_csr()
        g = np.arange(1.0, s + 1.0)
        p = g * (s + 1.0 - g)
        lo, hi = 1.78, 20.6

        def b(x):                                        # B x, B = (2 A - (lo + hi) I) / (hi - lo): [lo, hi] -> [-1, 1]
            return (2.0 * orc.spmv_csr(ptr, idx, val, x) - (lo + hi) * x) / (hi - lo)
        x0 = (p[:, None, None] * p[None, :, None] * p[None, None, :]).reshape(-1) / float(p.max() ** 3)
        x1 = b(x0)
        for _ in range(15):
            x0, x1 = x1, 2.0 * b(x1) - x0
        _START[n] = x1 / np.abs(x1).max()
    return _START[n].copy()


MATRICES = {"sym7": sym_csr, "nonsym7": nonsym_csr}


def make_matrix(lib, name):
    if name.startswith("mm/"):
        return from_file(lib, os.path.join(HERE, "golden", name))
    ptr, idx, val = MATRICES[name]()
    return lisdrv.make_csr(lib, ptr, idx, val)
