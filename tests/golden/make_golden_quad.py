"""Goldens of -f quad: the reference's quad build, bit for bit (tests/golden/quad_bits.npz).

    python tests/golden/make_golden_quad.py          (needs the reference's sources; no GPU)

The reference is compiled in place from its sources with what its configure picks for --enable-quad on x86-64
(-DUSE_QUAD_PRECISION -DUSE_FAST_QUAD_ADD -DUSE_SSE2 -DUSE_FMA2_SSE2 -msse2 on top of the flags of oracle/Makefile) into a temporary directory
outside the repository; nothing compiled is kept.  It is then driven through its C API at 1, 2, 4 and 8 OpenMP threads, one process per
thread count, on the inputs of tests/quad_cases.py, and every bit of hi and lo is recorded:
  scalar/<op>            lis_quad_add, _mul, _mul_dd_d, _div on a few hundred pairs
  vec/<op>/T<t>          lis_vector_axpyex_mmm, xpayex_mmm, axpyzex_mmmm; vec/muld: lis_quad_mul_dd_d element by element (Jacobi's psolve)
  dot/<n>/T<t>           lis_vector_dotex_mmm
  rows/T<t>              lis_matvec on quad vectors (the row sums do not depend on T: asserted)
  rows_t/T1              lis_matvech at one thread (beyond, the reference's A^T x has no defined bits)
  solve/<matrix>/<solver>/<precon>/<zeros|x0>/T<t>/{iter,status,resid,rhistory,x}      bicg at T = 1 only
  spread/<matrix>/<solver>/<precon>/<zeros|x0>    max over T of max|x_T - x_1|, what the default mode's x is held to
The script asserts that the build really is quad (quad CG ends in fewer iterations than double CG at -tol 1e-25 on the symmetric fixture) and that
every recorded solve converges."""
import ctypes as C
import glob
import os
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import lisdrv  # noqa: E402
import quad_cases as qc  # noqa: E402
from lis_amd import _capi as capi  # noqa: E402

REF = os.environ.get("LIS_REFERENCE", "/root/reference")
QUAD_FLAGS = ["-DUSE_QUAD_PRECISION", "-DUSE_FAST_QUAD_ADD", "-DUSE_SSE2", "-DUSE_FMA2_SSE2", "-msse2"]
BASE_FLAGS = ["-O3", "-fomit-frame-pointer", "-fopenmp", "-fPIC", "-w", "-I" + os.path.join(REF, "include")]
DIRS = ["system", "matrix", "vector", "matvec", "precon", "solver", "esolver", "precision", "array"]


class QuadPtr(C.Structure):
    _fields_ = [("hi", capi.P_DBL), ("lo", capi.P_DBL)]


class Quad(C.Structure):
    _fields_ = [("hi", C.c_double), ("lo", C.c_double)]


def build(tmp):
    srcs = [s for d in DIRS for s in sorted(glob.glob(os.path.join(REF, "src", d, "*.c")))]
    objs = [os.path.join(tmp, f"{i}.o") for i in range(len(srcs))]

    def cc(job):
        subprocess.run(["gcc"] + BASE_FLAGS + QUAD_FLAGS + ["-c", job[0], "-o", job[1]], check=True)
    with ThreadPoolExecutor(8) as ex:
        list(ex.map(cc, zip(srcs, objs)))
    so = os.path.join(tmp, "liblis_refquad.so")
    subprocess.run(["gcc", "-shared", "-fopenmp", "-Wl,-Bsymbolic", "-o", so] + objs + ["-lm"], check=True)
    return so


def qvec(lib, A, pair=None):
    v = capi.PV()
    assert lib.dll.lis_vector_duplicateex(1, C.cast(A, C.c_void_p), C.byref(v)) == 0
    n = v.contents.n
    if pair is not None:
        C.memmove(v.contents.value, np.ascontiguousarray(pair[0]).ctypes.data, 8 * n)
        C.memmove(v.contents.value_lo, np.ascontiguousarray(pair[1]).ctypes.data, 8 * n)
    return v


def qget(v, n=None):
    n = v.contents.n if n is None else n
    if n == 0:
        return np.zeros(0), np.zeros(0)
    return (np.ctypeslib.as_array(v.contents.value, shape=(n,)).copy(), np.ctypeslib.as_array(v.contents.value_lo, shape=(n,)).copy())


def put(out, key, pair):
    out[key + "/hi"] = np.atleast_1d(np.asarray(pair[0], np.float64)).view(np.uint64)
    out[key + "/lo"] = np.atleast_1d(np.asarray(pair[1], np.float64)).view(np.uint64)


def identity(lib, n):
    """an n x n matrix to duplicate vectors of length n from"""
    n1 = max(n, 1)
    ptr = np.arange(n1 + 1, dtype=np.int32)
    return lisdrv.make_csr(lib, ptr, np.arange(n1, dtype=np.int32), np.ones(n1))


def scalar_part(lib, out):
    a, b = qc.scalar_pairs()
    d = lib.dll
    for f in (d.lis_quad_add, d.lis_quad_mul, d.lis_quad_div):
        f.restype, f.argtypes = None, [C.POINTER(Quad)] * 3
    d.lis_quad_mul_dd_d.restype, d.lis_quad_mul_dd_d.argtypes = None, [C.POINTER(Quad), C.POINTER(Quad), C.c_double]
    res = {k: (np.zeros(len(a[0])), np.zeros(len(a[0]))) for k in ("add", "mul", "muld", "div")}
    for i in range(len(a[0])):
        qa, qb, r = Quad(a[0][i], a[1][i]), Quad(b[0][i], b[1][i]), Quad()
        for k, call in (("add", lambda: d.lis_quad_add(r, qa, qb)), ("mul", lambda: d.lis_quad_mul(r, qa, qb)),
                        ("muld", lambda: d.lis_quad_mul_dd_d(r, qa, b[0][i])), ("div", lambda: d.lis_quad_div(r, qa, qb))):
            call()
            res[k][0][i], res[k][1][i] = r.hi, r.lo
    for k, v in res.items():
        put(out, "scalar/" + k, v)
    # Jacobi's psolve: x = b * d element by element
    bb, dd = qc.dd_vector(qc.VEC_N, 31), qc.dd_vector(qc.VEC_N, 32)[0]
    xh, xl = np.zeros(qc.VEC_N), np.zeros(qc.VEC_N)
    for i in range(qc.VEC_N):
        r = Quad()
        d.lis_quad_mul_dd_d(r, Quad(bb[0][i], bb[1][i]), dd[i])
        xh[i], xl[i] = r.hi, r.lo
    put(out, "vec/muld", (xh, xl))


def vector_part(lib, out, T):
    d = lib.dll
    d.lis_vector_axpyex_mmm.argtypes = [QuadPtr, capi.PV, capi.PV]
    d.lis_vector_xpayex_mmm.argtypes = [capi.PV, QuadPtr, capi.PV]
    d.lis_vector_axpyzex_mmmm.argtypes = [QuadPtr, capi.PV, capi.PV, capi.PV]
    d.lis_vector_dotex_mmm.argtypes = [capi.PV, capi.PV, C.POINTER(QuadPtr)]
    n = qc.VEC_N
    A = identity(lib, n)
    x, y = qc.dd_vector(n, 21), qc.dd_vector(n, 22)
    al = qc.dd_vector(1, 23, -2, 2)
    ahi, alo = (C.c_double * 2)(al[0][0], 0.0), (C.c_double * 2)(al[1][0], 0.0)
    alpha = QuadPtr(C.cast(ahi, capi.P_DBL), C.cast(alo, capi.P_DBL))
    vx, vy, vz = qvec(lib, A, x), qvec(lib, A, y), qvec(lib, A)
    assert d.lis_vector_axpyzex_mmmm(alpha, vx, vy, vz) == 0
    put(out, f"vec/axpyz/T{T}", qget(vz))
    assert d.lis_vector_axpyex_mmm(alpha, vx, vy) == 0
    put(out, f"vec/axpy/T{T}", qget(vy))
    vy = qvec(lib, A, y)
    assert d.lis_vector_xpayex_mmm(vx, alpha, vy) == 0
    put(out, f"vec/xpay/T{T}", qget(vy))
    for n in qc.DOT_SIZES:
        A = identity(lib, n)
        x, y = qc.dot_vectors(n)
        vx, vy = qvec(lib, A), qvec(lib, A)
        if n:
            for v, p in ((vx, x), (vy, y)):
                C.memmove(v.contents.value, p[0].ctypes.data, 8 * n)
                C.memmove(v.contents.value_lo, p[1].ctypes.data, 8 * n)
        else:            # the library has no vector of length 0: one of length 1 whose n is set to 0 for the call
            vx.contents.n = 0
            vy.contents.n = 0
        rh, rl = (C.c_double * 2)(), (C.c_double * 2)()
        res = QuadPtr(C.cast(rh, capi.P_DBL), C.cast(rl, capi.P_DBL))
        assert d.lis_vector_dotex_mmm(vx, vy, C.byref(res)) == 0
        put(out, f"dot/{n}/T{T}", (rh[0], rl[0]))


def product_part(lib, out, T):
    ptr, idx, val, x, ncols = qc.rows_matrix()
    rows = len(ptr) - 1
    # a square matrix of ncols rows: the rows behind the listed ones are empty
    sq = np.concatenate([ptr, np.full(ncols - rows, ptr[-1], np.int32)])
    A = lisdrv.make_csr(lib, sq, idx, val)
    vx, vy = qvec(lib, A, x), qvec(lib, A)
    assert lib.lis_matvec(A, vx, vy) == 0
    put(out, f"rows/T{T}", qget(vy, rows))
    if T == 1:
        xt = qc.transposed_input()
        full = (np.concatenate([xt[0], np.zeros(ncols - rows)]), np.concatenate([xt[1], np.zeros(ncols - rows)]))
        vx, vy = qvec(lib, A, full), qvec(lib, A)
        assert lib.lis_matvech(A, vx, vy) == 0
        put(out, "rows_t/T1", qget(vy))


def solve_part(lib, out, T):
    for mat, (ptr, idx, val) in qc.solve_matrices().items():
        A = lisdrv.make_csr(lib, ptr, idx, val)
        n = len(ptr) - 1
        b = qc.solve_rhs(mat, ptr, idx, val)
        if T == 1 and mat == "poisson1d":
            q = lisdrv.solve(lib, A, b, qc.solve_options("cg", "none", True))
            dbl = lisdrv.solve(lib, A, b, qc.solve_options("cg", "none", True).replace("-f quad", "-f double"))
            print(f"quad CG: {q['iter']} iterations (status {q['status']}), double CG: {dbl['iter']} (status {dbl['status']})")
            assert q["status"] == 0 and q["iter"] < dbl["iter"], "the build is not quad"
        for solver in qc.SOLVERS:
            if T not in qc.solve_threads(solver):
                continue
            for precon in qc.PRECONS:
                for zeros in (True, False):
                    r = lisdrv.solve(lib, A, b, qc.solve_options(solver, precon, zeros), x0=None if zeros else qc.solve_x0(n))
                    key = qc.solve_key(mat, solver, precon, zeros, T)
                    assert r["err"] == 0 and r["status"] == 0, (key, r["err"], r["status"], r["iter"], r["resid"])
                    out[key + "/iter"] = np.array([r["iter"]], np.int64)
                    out[key + "/status"] = np.array([r["status"]], np.int64)
                    out[key + "/resid"] = np.array([r["resid"]]).view(np.uint64)
                    out[key + "/rhistory"] = r["rhistory"].view(np.uint64)
                    out[key + "/x"] = r["x"].view(np.uint64)
                    print(f"{key}: iter {r['iter']} resid {r['resid']:.3e}")


def worker(so, T, path):
    lib = lisdrv.open_lib(so, threads=T)
    out = {}
    if T == 1:
        scalar_part(lib, out)
    vector_part(lib, out, T)
    product_part(lib, out, T)
    solve_part(lib, out, T)
    np.savez(path, **out)


def main():
    tmp = tempfile.mkdtemp(prefix="lis_refquad_")
    try:
        so = build(tmp)
        merged = {}
        for T in qc.THREADS:
            part = os.path.join(tmp, f"part{T}.npz")
            env = dict(os.environ, OMP_NUM_THREADS=str(T))
            subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", so, str(T), part], check=True, env=env)
            with np.load(part) as z:
                merged.update({k: z[k] for k in z.files})
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    for T in qc.THREADS[1:]:
        for part in ("hi", "lo"):
            assert np.array_equal(merged[f"rows/T{T}/{part}"], merged[f"rows/T1/{part}"]), "the reference's row sums depend on the thread count"
    # the reference's own spread over the thread counts: what the default mode's x is held to (tests/test_quad_gpu.py)
    for mat in qc.solve_matrices():
        for solver in qc.SOLVERS:
            for precon in qc.PRECONS:
                for zeros in (True, False):
                    x1 = merged[qc.solve_key(mat, solver, precon, zeros, 1) + "/x"].view(np.float64)
                    sp = max([float(np.max(np.abs(merged[qc.solve_key(mat, solver, precon, zeros, T) + "/x"].view(np.float64) - x1)))
                              for T in qc.solve_threads(solver)[1:]] or [0.0])
                    key = f"spread/{mat}/{solver}/{precon}/{'zeros' if zeros else 'x0'}"
                    merged[key] = np.array([sp])
                    print(f"{key}: {sp:.3e}")
    np.savez_compressed(os.path.join(HERE, "quad_bits.npz"), **merged)
    print("wrote quad_bits.npz,", os.path.getsize(os.path.join(HERE, "quad_bits.npz")), "bytes")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--worker":
        worker(sys.argv[2], int(sys.argv[3]), sys.argv[4])
    else:
        main()
