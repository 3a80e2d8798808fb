"""What tests/test_ilu_cpu.py (oracle against the reference library) and tests/test_ilu_gpu.py (liblis_amd against the oracle) share:
the matrices, the reference's ILU structures seen through ctypes, and the comparison of two factors.

Matrices: poisson3d(8, 7, 6), the non-symmetric system of the other solver tests, tests/golden/mm/testmat0.mtx and one hand-made
matrix with unsorted rows, a row without a stored diagonal entry and columns stored twice (in L, in U and on the diagonal)."""
import ctypes as C
import os
import sys

import numpy as np

import orc
from lis_amd import _capi as capi

HERE = os.path.dirname(os.path.abspath(__file__))
FILLS = (0, 1, 2)
THREADS = (1, 3, 8)


def read_mtx(path):
    """a MatrixMarket coordinate file (general or symmetric) as CSR, entries of a row in file order"""
    rows = None
    with open(path) as f:
        head = f.readline().lower()
        sym = "symmetric" in head
        for line in f:
            if line.startswith("%") or not line.strip():
                continue
            t = line.split()
            if rows is None:
                n = int(t[0])
                rows = [[] for _ in range(n)]
                continue
            if len(t) < 3:
                continue
            i, j, v = int(t[0]) - 1, int(t[1]) - 1, float(t[2])
            rows[i].append((j, v))
            if sym and i != j:
                rows[j].append((i, v))
    ptr = np.zeros(len(rows) + 1, np.int32)
    for i, r in enumerate(rows):
        ptr[i + 1] = ptr[i] + len(r)
    return ptr, np.array([c for r in rows for c, _ in r], np.int32), np.array([v for r in rows for _, v in r], np.float64)


def handmade():
    """12 rows; row 4 has no stored diagonal entry (its pivot comes from the updates alone), row 6 stores column 2 twice (L), row 3
    column 9 twice (U), row 7 its diagonal twice; every row unsorted"""
    rows = {
        0: [(3, -1.0), (0, 4.0), (1, -0.5)],
        1: [(1, 5.0), (0, -1.25), (5, 0.75), (2, -1.0)],
        2: [(6, -0.5), (2, 6.0), (1, -1.0), (0, 0.25)],
        3: [(9, -0.75), (3, 5.5), (0, -1.0), (9, 0.5), (4, -1.5)],
        4: [(3, -2.0), (8, -1.0), (1, 0.5)],
        5: [(5, 7.0), (1, 1.0), (10, -1.0), (4, -0.5)],
        6: [(2, -1.0), (7, -0.25), (6, 4.5), (2, 0.5), (11, -1.0)],
        7: [(7, 1.0), (6, -0.5), (8, -1.0), (7, 5.0), (3, 0.125)],
        8: [(11, -1.5), (4, -1.0), (8, 6.0), (7, -1.0)],
        9: [(3, -0.75), (9, 4.0), (10, -1.0), (0, 0.5)],
        10: [(10, 5.0), (9, -1.0), (5, -1.0)],
        11: [(8, -1.5), (11, 6.5), (6, -1.0), (10, 0.25)],
    }
    ptr, idx, val = [0], [], []
    for i in range(12):
        idx += [c for c, _ in rows[i]]
        val += [v for _, v in rows[i]]
        ptr.append(len(idx))
    return np.array(ptr, np.int32), np.array(idx, np.int32), np.array(val, np.float64)


_cache = {}


def system(name):
    """(ptr, idx, val) of a named matrix"""
    if name not in _cache:
        if name == "p3d":
            _cache[name] = orc.poisson3d(8, 7, 6)
        elif name == "nonsym":
            sys.path.insert(0, os.path.join(HERE, "golden"))
            from make_golden_scale import test_matrix
            _cache[name] = test_matrix(n=120, seed=9)
        elif name == "testmat0":
            _cache[name] = read_mtx(os.path.join(HERE, "golden", "mm", "testmat0.mtx"))
        elif name == "handmade":
            _cache[name] = handmade()
        else:
            raise KeyError(name)
    return _cache[name]


NAMED = ("p3d", "nonsym", "testmat0", "handmade")


def rhs(n):
    return np.arange(1, n + 1, dtype=np.float64) / max(n, 1)


# ---------------------------------------------------------------- the reference's structures (its include/lis.h: LIS_MATRIX_ILU_STRUCT, LIS_PRECON_STRUCT)
class MatrixILU(C.Structure):
    _fields_ = [("n", C.c_int), ("bs", C.c_int), ("nnz_ma", capi.P_INT), ("nnz", capi.P_INT), ("bsz", capi.P_INT),
                ("index", C.POINTER(capi.P_INT)), ("value", C.POINTER(capi.P_DBL)), ("values", C.c_void_p)]


class Precon(C.Structure):
    _fields_ = [("precon_type", C.c_int), ("A", C.c_void_p), ("Ah", C.c_void_p), ("L", C.POINTER(MatrixILU)), ("U", C.POINTER(MatrixILU)),
                ("WD", C.c_void_p), ("D", capi.PV)]


def _ilu_rows(m, n):
    ptr = np.zeros(n + 1, np.int32)
    idx, val = [], []
    for i in range(n):
        k = m.nnz[i]
        ptr[i + 1] = ptr[i] + k
        if k:
            idx.append(np.ctypeslib.as_array(m.index[i], shape=(k,)).copy())
            val.append(np.ctypeslib.as_array(m.value[i], shape=(k,)).copy())
    return (ptr, np.concatenate(idx).astype(np.int32) if idx else np.zeros(0, np.int32), np.concatenate(val) if val else np.zeros(0))


def reference_ilu(ref, ptr, idx, val, fill, b):
    """{"L", "U", "D", "psolve", "psolveh"} from the reference library: its lis_precon_create, its two psolves (separate B and X)"""
    import lisdrv
    A = lisdrv.make_csr(ref, ptr, idx, val)
    n = A.contents.n
    S = capi.PS()
    assert ref.lis_solver_create(C.byref(S)) == 0
    assert ref.lis_solver_set_option(("-p ilu -ilu_fill %d" % fill).encode(), S) == 0
    S.contents.A = A
    create = ref.dll.lis_precon_create
    create.restype, create.argtypes = C.c_int, [capi.PS, C.POINTER(C.c_void_p)]
    pp = C.c_void_p()
    assert create(S, C.byref(pp)) == 0
    P = C.cast(pp, C.POINTER(Precon)).contents
    out = {"L": _ilu_rows(P.L.contents, n), "U": _ilu_rows(P.U.contents, n), "D": lisdrv.get_vector(ref, P.D, n)}
    S.contents.precon = pp
    for name in ("psolve", "psolveh"):
        fn = getattr(ref.dll, "lis_%s_iluk_csr" % name)
        fn.restype, fn.argtypes = C.c_int, [capi.PS, capi.PV, capi.PV]
        vb, vx = lisdrv.new_vector(ref, A, b), lisdrv.new_vector(ref, A, np.full(n, 7.0))
        assert fn(S, vb, vx) == 0
        out[name] = lisdrv.get_vector(ref, vx, n)
        ref.lis_vector_destroy(vb)
        ref.lis_vector_destroy(vx)
    S.contents.precon = None
    destroy = ref.dll.lis_precon_destroy
    destroy.restype, destroy.argtypes = C.c_int, [C.c_void_p]
    destroy(pp)
    ref.lis_solver_destroy(S)
    ref.lis_matrix_destroy(A)
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def same_bits(got, want, nan_payload=True):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape:
        return False
    same = bits(got) == bits(want)
    if not nan_payload:
        same |= np.isnan(got) & np.isnan(want)
    return bool(same.all())


def factor_differences(got, want, nan_payload=True):
    """[] when the two factors agree in pattern, term order and every bit of L, U and D"""
    bad = []
    for part in ("L", "U"):
        for k, what in enumerate(("ptr", "index")):
            if not np.array_equal(np.asarray(got[part][k]), np.asarray(want[part][k])):
                bad.append(part + " " + what)
        if not bad and not same_bits(got[part][2], want[part][2], nan_payload):
            bad.append(part + " value")
    if not same_bits(got["D"], want["D"], nan_payload):
        bad.append("D")
    return bad
