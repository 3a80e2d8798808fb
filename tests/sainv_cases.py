"""What the SAINV and I+S tests share: the matrices of the issue's table, the input vectors, the reference's structures seen through
ctypes (tests/ilu_cases.py: precon->L / U / D hold W / Z / d for SAINV) and the comparison of two factors."""
import ctypes as C

import numpy as np

import ilu_cases
import lisdrv
import orc
import reduction_cases
from lis_amd import _capi as capi

DROP = 0.05
THREADS = (1, 3, 8)
same_bits = ilu_cases.same_bits


def tridiagonal(n):
    ptr, idx, val = [0], [], []
    for i in range(n):
        for c, v in ((i - 1, -1.0), (i, 2.5 + 0.01 * i), (i + 1, -1.25)):
            if 0 <= c < n:
                idx.append(c)
                val.append(v)
        ptr.append(len(idx))
    return np.array(ptr, np.int32), np.array(idx, np.int32), np.array(val, np.float64)


def dominant(n=257, per_row=5, seed=3):
    """random pattern, diagonally dominant, the diagonal stored wherever it falls, rows unsorted"""
    rng = np.random.default_rng(seed)
    ptr, idx, val = [0], [], []
    for i in range(n):
        cols = [int(c) for c in rng.choice(n, per_row, replace=False) if c != i][:per_row - 1]
        vals = list(rng.uniform(-1.0, 1.0, len(cols)))
        at = int(rng.integers(0, len(cols) + 1))
        cols.insert(at, i)
        vals.insert(at, float(np.abs(vals).sum() + 1.0) * (1 if i % 4 else -1))
        idx += cols
        val += vals
        ptr.append(len(idx))
    return np.array(ptr, np.int32), np.array(idx, np.int32), np.array(val, np.float64)


def twice():
    """12 rows (the reference preallocates n / 10 entries per row and cannot grow a row from none); row 2 stores column 5 twice (right of the diagonal), row 6 column 1 twice (left of it), row 4 its diagonal twice"""
    rows = {
        0: [(0, 4.0), (1, -1.0), (3, 0.5)],
        1: [(0, -1.0), (1, 5.0), (2, -1.5)],
        2: [(5, -0.75), (2, 6.0), (1, -1.0), (5, 0.5), (3, -0.25)],
        3: [(3, 4.5), (2, -1.0), (4, -1.0)],
        4: [(4, 2.0), (3, -1.0), (4, 3.0), (7, -0.5)],
        5: [(2, -0.5), (5, 5.0), (6, -1.0)],
        6: [(1, 0.25), (6, 4.0), (1, -0.75), (7, -1.0), (5, -1.0)],
        7: [(6, -1.0), (7, 3.5), (4, -0.5), (9, 0.5)],
        8: [(8, 4.0), (0, -1.0), (11, -0.5)],
        9: [(7, 0.5), (9, 3.0), (10, -1.0)],
        10: [(10, 5.0), (9, -1.0), (2, 0.75)],
        11: [(8, -0.5), (11, 4.5), (10, -1.5)],
    }
    ptr, idx, val = [0], [], []
    for i in range(12):
        idx += [c for c, _ in rows[i]]
        val += [v for _, v in rows[i]]
        ptr.append(len(idx))
    return np.array(ptr, np.int32), np.array(idx, np.int32), np.array(val, np.float64)


def empty_upper():
    """for I+S, 12 rows: rows 0, 3, 4, 7, 9 and the last row have nothing right of the diagonal; row 1 has 6 entries there, row 2 stores column 5 twice"""
    rows = {
        0: [(0, 3.0)],
        1: [(7, -0.5), (1, 4.0), (2, -1.0), (3, 0.25), (6, -0.75), (5, 1.5), (0, -1.0), (4, -0.125)],
        2: [(5, -0.75), (2, 6.0), (1, -1.0), (5, 0.5)],
        3: [(0, -1.0), (3, 2.0), (1, 0.5)],
        4: [(4, 5.0)],
        5: [(5, 4.0), (6, -2.0), (0, 1.0)],
        6: [(7, 0.5), (6, 3.0)],
        7: [(7, 2.0), (3, -1.0)],
        8: [(8, 3.0), (10, -1.0), (9, 0.5)],
        9: [(9, 4.0), (8, -1.0)],
        10: [(11, -0.25), (10, 2.5)],
        11: [(11, 3.0), (0, 0.5)],
    }
    ptr, idx, val = [0], [], []
    for i in range(12):
        idx += [c for c, _ in rows[i]]
        val += [v for _, v in rows[i]]
        ptr.append(len(idx))
    return np.array(ptr, np.int32), np.array(idx, np.int32), np.array(val, np.float64)


_cache = {}


def system(name):
    if name not in _cache:
        if name == "one":
            _cache[name] = (np.array([0, 1], np.int32), np.array([0], np.int32), np.array([-2.5]))
        elif name == "tri65":
            _cache[name] = tridiagonal(65)
        elif name == "p654":
            _cache[name] = orc.poisson3d(6, 5, 4)
        elif name == "nonsym":
            _cache[name] = ilu_cases.system("nonsym")
        elif name == "dom257":
            _cache[name] = dominant()
        elif name == "twice":
            _cache[name] = twice()
        elif name == "empty_upper":
            _cache[name] = empty_upper()
        else:
            raise KeyError(name)
    return _cache[name]


# (case name, matrix, drop tolerance): the issue's table; the storage-format rows reuse p654
SAINV_CASES = (("one", "one", DROP), ("tri65_full", "tri65", 0.0), ("tri65_identity", "tri65", 10.0), ("p654", "p654", DROP),
               ("nonsym", "nonsym", DROP), ("dom257", "dom257", DROP), ("twice", "twice", DROP))
IS_MATRICES = ("p654", "nonsym", "twice", "empty_upper")
IS_PARAMS = ((1.0, 3), (0.7, 3), (1.0, 0), (0.7, 1000))
WHOLE = (("p654", "-i cg -p sainv"), ("p654", "-i bicg -p sainv"), ("p654", "-i bicgstab -p sainv"), ("p654", "-i gmres -restart 30 -p sainv"),
         # (CG on the non-symmetric matrix: the reference itself ends with LIS_MAXITER, no fixture)
         ("nonsym", "-i bicg -p sainv"), ("nonsym", "-i bicgstab -p sainv"), ("nonsym", "-i gmres -restart 30 -p sainv"),
         # (CG under -p is: I - alpha S is no symmetric preconditioner and the reference's CG ends with LIS_MAXITER on both matrices; BiCGSTAB stands in)
         ("p654", "-i bicg -p is"), ("p654", "-i bicgstab -p is"), ("nonsym", "-i bicg -p is"), ("nonsym", "-i bicgstab -p is"))
COMMON = "-tol 1e-10 -maxiter 400 -print mem"


def inputs(n):
    """a wide-exponent vector, and one with -0.0 and zeros among wide entries"""
    rng = np.random.default_rng([n, 17])
    a = reduction_cases.wide(rng, n)
    b = reduction_cases.wide(rng, n)
    b[::3] = -0.0
    b[1::5] = 0.0
    return {"wide": a, "zeros": b}


def rhs(ptr, idx, val):
    return orc.spmv_csr(ptr, idx, val, np.ones(len(ptr) - 1))


def factor_differences(got, want):
    bad = []
    for part in ("W", "Z"):
        for k, what in enumerate(("ptr", "index")):
            if not np.array_equal(np.asarray(got[part][k]), np.asarray(want[part][k])):
                bad.append(part + " " + what)
        if not bad and not same_bits(got[part][2], want[part][2]):
            bad.append(part + " value")
    if not same_bits(got["D"], want["D"]):
        bad.append("D")
    return bad


# ---------------------------------------------------------------- the reference library
def _precon(ref, A, options):
    S = capi.PS()
    assert ref.lis_solver_create(C.byref(S)) == 0
    assert ref.lis_solver_set_option(options.encode(), S) == 0
    S.contents.A = A
    create = ref.dll.lis_precon_create
    create.restype, create.argtypes = C.c_int, [capi.PS, C.POINTER(C.c_void_p)]
    pp = C.c_void_p()
    assert create(S, C.byref(pp)) == 0
    S.contents.precon = pp
    return S, pp


def _release(ref, S, pp, A):
    S.contents.precon = None
    destroy = ref.dll.lis_precon_destroy
    destroy.restype, destroy.argtypes = C.c_int, [C.c_void_p]
    destroy(pp)
    ref.lis_solver_destroy(S)
    ref.lis_matrix_destroy(A)


def _apply(ref, fname, S, A, b):
    fn = getattr(ref.dll, fname)
    fn.restype, fn.argtypes = C.c_int, [capi.PS, capi.PV, capi.PV]
    n = A.contents.n
    vb, vx = lisdrv.new_vector(ref, A, b), lisdrv.new_vector(ref, A, np.full(n, 7.0))
    assert fn(S, vb, vx) == 0
    out = lisdrv.get_vector(ref, vx, n)
    ref.lis_vector_destroy(vb)
    ref.lis_vector_destroy(vx)
    return out


def reference_sainv(ref, ptr, idx, val, tol, vectors):
    """{"W", "Z", "D", "psolve": {tag: x}, "psolveh": {tag: x}} from the reference library at the thread count it was initialised with"""
    A = lisdrv.make_csr(ref, ptr, idx, val)
    n = A.contents.n
    S, pp = _precon(ref, A, "-p sainv -sainv_drop %r" % float(tol))
    P = C.cast(pp, C.POINTER(ilu_cases.Precon)).contents
    out = {"W": ilu_cases._ilu_rows(P.L.contents, n), "Z": ilu_cases._ilu_rows(P.U.contents, n), "D": lisdrv.get_vector(ref, P.D, n)}
    for name in ("psolve", "psolveh"):
        out[name] = {tag: _apply(ref, "lis_%s_sainv" % name, S, A, b) for tag, b in vectors.items()}
    _release(ref, S, pp, A)
    return out


def reference_is(ref, ptr, idx, val, alpha, m, vectors):
    """{"psolve": {tag: y}, "psolveh": {tag: y}} of -p is (level 1) from the reference library"""
    A = lisdrv.make_csr(ref, ptr, idx, val)
    S, pp = _precon(ref, A, "-i bicg -p is -is_alpha %r -is_m %d" % (float(alpha), m))
    out = {name: {tag: _apply(ref, "lis_%s_is" % name, S, A, b) for tag, b in vectors.items()} for name in ("psolve", "psolveh")}
    _release(ref, S, pp, A)
    return out
