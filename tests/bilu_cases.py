"""What tests/test_bilu_cpu.py (the model of tests/bilu_oracle.py against the reference library) and the GPU tests of the block ILU
(liblis_amd against the model and the reference) share: the BSR matrices, the reference's block ILU seen through ctypes, and the child
process the reference runs in.

The reference's block ILU is run at ONE thread only, with blocks of 1, 2 or 3 only, and always in a child process of its own: with
more threads its factorisation calls lis_array_ge inside the parallel region, which registers a buffer in lis_malloc's unlocked list
and leaves that list damaged for the rest of the process; with larger blocks its sweeps overrun LIS_SCALAR w[3].

Matrices (name -> CSR, blocked bn x bn by bilu_oracle.csr_to_bsr): the 7-point Poisson matrix on 5x5x4, 5x5x5 and 8x7x6 (n % bn takes
every residue), the non-symmetric system of the other solver tests, tests/golden/mm/testmat0.mtx; and "twice", built block by block:
block rows that store a block column twice in L, in U and on the diagonal, unsorted, one block row without a stored diagonal block."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

import bilu_oracle
import ilu_cases
import orc
from lis_amd import _capi as capi

HERE = os.path.dirname(os.path.abspath(__file__))
BNS = (1, 2, 3)
FILLS = (0, 1, 2)
THREADS = (1, 3, 8)
NAMED = ("p100", "p125", "p336", "nonsym", "testmat0", "twice")
bits, same_bits, factor_differences = ilu_cases.bits, ilu_cases.same_bits, ilu_cases.factor_differences

_cache = {}


def csr_system(name):
    if name == "p100":
        return orc.poisson3d(5, 5, 4)
    if name == "p125":
        return orc.poisson3d(5, 5, 5)
    if name == "p336":
        return orc.poisson3d(8, 7, 6)
    return ilu_cases.system(name)


def twice(bn):
    """9 block rows, n = 9*bn - (bn - 1) (one scalar row in the last block when bn > 1).  Block row 6 stores block column 2 twice (L),
    block row 3 column 7 twice (U), block row 5 its diagonal block twice, block row 4 none; every block row unsorted"""
    pattern = {0: [3, 0, 1], 1: [1, 0, 5, 2], 2: [6, 2, 1, 0], 3: [7, 3, 0, 7, 4], 4: [3, 8, 1], 5: [5, 1, 5, 4, 8],
               6: [2, 7, 6, 2], 7: [7, 6, 8, 3], 8: [4, 8, 7, 2]}
    nr, bs = 9, bn * bn
    n = nr * bn - (bn - 1)
    rng = np.random.default_rng(100 + bn)
    bptr, bindex, value = [0], [], []
    for i in range(nr):
        for c in pattern[i]:
            blk = rng.uniform(-1.0, 1.0, bs)
            if c == i:
                for r in range(bn):
                    blk[r * (bn + 1)] = 6.0 + rng.uniform(0.0, 1.0)
            for r in range(bn):
                for q in range(bn):
                    if i * bn + r >= n or c * bn + q >= n:
                        blk[r + q * bn] = 0.0
            bindex.append(c)
            value += blk.tolist()
        bptr.append(len(bindex))
    return np.array(bptr, np.int32), np.array(bindex, np.int32), np.array(value, np.float64), bn, n


def system(name, bn):
    """(bptr, bindex, value, bn, n) of a named matrix in bn x bn blocks"""
    key = (name, bn)
    if key not in _cache:
        if name == "twice":
            _cache[key] = twice(bn)
        else:
            ptr, idx, val = csr_system(name)
            _cache[key] = bilu_oracle.csr_to_bsr(ptr, idx, val, bn) + (bn, len(ptr) - 1)
    return _cache[key]


def rhs(n):
    """mixed signs, no zero"""
    i = np.arange(1, n + 1, dtype=np.float64)
    return np.where(i % 3 == 0, -i, i) / max(n, 1)


def spmv(bsr, x):
    """A x of a BSR matrix, in float64 (the right-hand sides of the solves: any b serves, this one has a known answer)"""
    bptr, bindex, value, bn, n = bsr
    nr = len(bptr) - 1
    xp = np.zeros(nr * bn)
    xp[:n] = x
    y = np.zeros(nr * bn)
    for i in range(nr):
        for k in range(bptr[i], bptr[i + 1]):
            blk = value[k * bn * bn:(k + 1) * bn * bn].reshape(bn, bn).T
            y[i * bn:(i + 1) * bn] += blk @ xp[bindex[k] * bn:(bindex[k] + 1) * bn]
    return y[:n]


def make_bsr(lib, bsr):
    """an assembled LIS_MATRIX_BSR from the arrays, through lis_matrix_malloc_bsr + lis_matrix_set_bsr"""
    bptr, bindex, value, bn, n = bsr
    bnnz = int(bptr[-1])
    A = capi.PM()
    assert lib.lis_matrix_create(capi.LIS_COMM_WORLD, C.byref(A)) == 0
    assert lib.lis_matrix_set_size(A, n, 0) == 0
    p, i, v = capi.P_INT(), capi.P_INT(), capi.P_DBL()
    assert lib.lis_matrix_malloc_bsr(n, bn, bn, max(bnnz, 1), C.byref(p), C.byref(i), C.byref(v)) == 0
    C.memmove(p, np.ascontiguousarray(bptr, np.int32).ctypes.data, 4 * len(bptr))
    if bnnz:
        C.memmove(i, np.ascontiguousarray(bindex, np.int32).ctypes.data, 4 * bnnz)
        C.memmove(v, np.ascontiguousarray(value, np.float64).ctypes.data, 8 * bnnz * bn * bn)
    assert lib.lis_matrix_set_bsr(bn, bn, bnnz, p, i, v, A) == 0
    assert lib.lis_matrix_assemble(A) == 0
    return A


# ---------------------------------------------------------------- the library's factor and psolve (GPU)
def library_factor(lib, A, fill):
    """the factor of liblis_amd in the shape of bilu_oracle.factor"""
    a = A.contents
    bn, nr = a.bnr, a.nr
    bs = bn * bn
    sizes = (C.c_int * 3)()
    err = lib.dll.lis_amd_ilu_factor(A, fill, sizes)
    assert err == 0, err
    assert sizes[0] == nr
    lp, up = np.zeros(nr + 1, np.int32), np.zeros(nr + 1, np.int32)
    li, ui = np.zeros(max(sizes[1], 1), np.int32), np.zeros(max(sizes[2], 1), np.int32)
    lv, uv, d = np.zeros(max(sizes[1] * bs, 1)), np.zeros(max(sizes[2] * bs, 1)), np.zeros(max(nr * bs, 1))
    P = lambda x, t: x.ctypes.data_as(t)
    err = lib.dll.lis_amd_ilu_copy(A, fill, P(lp, capi.P_INT), P(li, capi.P_INT), P(lv, capi.P_DBL), P(up, capi.P_INT), P(ui, capi.P_INT), P(uv, capi.P_DBL), P(d, capi.P_DBL))
    assert err == 0, err
    return {"L": (lp, li[:sizes[1]], lv[:sizes[1] * bs]), "U": (up, ui[:sizes[2]], uv[:sizes[2] * bs]), "D": d[:nr * bs], "bn": bn, "n": a.n}


def library_psolve(lib, A, fill, b, alias=False, transposed=0):
    import lisdrv
    vb = lisdrv.new_vector(lib, A, b)
    vx = vb if alias else lisdrv.new_vector(lib, A, np.full(len(b), 7.0))
    err = lib.dll.lis_amd_ilu_psolve(A, fill, vb, vx, transposed)
    x = lisdrv.get_vector(lib, vx, len(b)) if not err else None
    lib.lis_vector_destroy(vb)
    if not alias:
        lib.lis_vector_destroy(vx)
    return err, x


# ---------------------------------------------------------------- the reference's structures (its include/lis.h)
class Precon(C.Structure):
    _fields_ = [("precon_type", C.c_int), ("A", C.c_void_p), ("Ah", C.c_void_p), ("L", C.POINTER(ilu_cases.MatrixILU)), ("U", C.POINTER(ilu_cases.MatrixILU)),
                ("WD", C.POINTER(capi.MatrixDiag)), ("D", capi.PV)]


def _ilu_block_rows(m, nr, bs):
    ptr = np.zeros(nr + 1, np.int32)
    idx, val = [], []
    for i in range(nr):
        k = m.nnz[i]
        ptr[i + 1] = ptr[i] + k
        if k:
            idx.append(np.ctypeslib.as_array(m.index[i], shape=(k,)).copy())
            val.append(np.ctypeslib.as_array(m.value[i], shape=(k * bs,)).copy())
    return (ptr, np.concatenate(idx).astype(np.int32) if idx else np.zeros(0, np.int32), np.concatenate(val) if val else np.zeros(0))


def reference_bilu(ref, bsr, fill, b):
    """{"L", "U", "D", "psolve"} from the reference library (one thread, bn <= 3): its lis_precon_create on the BSR matrix, its psolve"""
    import lisdrv
    bn, n = bsr[3], bsr[4]
    assert bn <= 3
    ref.dll.omp_get_max_threads.restype = C.c_int
    assert ref.dll.omp_get_max_threads() == 1
    A = make_bsr(ref, bsr)
    nr, bs = A.contents.nr, bn * bn
    S = capi.PS()
    assert ref.lis_solver_create(C.byref(S)) == 0
    assert ref.lis_solver_set_option(("-p ilu -ilu_fill %d" % fill).encode(), S) == 0
    S.contents.A = A
    create = ref.dll.lis_precon_create
    create.restype, create.argtypes = C.c_int, [capi.PS, C.POINTER(C.c_void_p)]
    pp = C.c_void_p()
    assert create(S, C.byref(pp)) == 0
    P = C.cast(pp, C.POINTER(Precon)).contents
    WD = P.WD.contents
    out = {"L": _ilu_block_rows(P.L.contents, nr, bs), "U": _ilu_block_rows(P.U.contents, nr, bs),
           "D": np.ctypeslib.as_array(WD.value, shape=(nr * bs,)).copy()}
    S.contents.precon = pp
    fn = ref.dll.lis_psolve_iluk_bsr
    fn.restype, fn.argtypes = C.c_int, [capi.PS, capi.PV, capi.PV]
    vb, vx = lisdrv.new_vector(ref, A, b), lisdrv.new_vector(ref, A, np.full(n, 7.0))
    assert fn(S, vb, vx) == 0
    out["psolve"] = lisdrv.get_vector(ref, vx, n)
    ref.lis_vector_destroy(vb)
    ref.lis_vector_destroy(vx)
    S.contents.precon = None
    destroy = ref.dll.lis_precon_destroy
    destroy.restype, destroy.argtypes = C.c_int, [C.c_void_p]
    destroy(pp)
    ref.lis_solver_destroy(S)
    ref.lis_matrix_destroy(A)
    return out


# ---------------------------------------------------------------- the reference in a child process, at one thread
def queen_mini_bsr():
    """queen_class "mini" (tests/golden/gen_queen_class.c) as BSR 3 x 3"""
    if "queen" not in _cache:
        import queen_class
        path, rows, _ = queen_class.generate("mini")
        try:
            ptr, idx, val = ilu_cases.read_mtx(path)
        finally:
            os.unlink(path)
        assert len(ptr) - 1 == rows
        _cache["queen"] = bilu_oracle.csr_to_bsr(ptr, idx, val, 3) + (3, rows)
    return _cache["queen"]


def job_system(job):
    return queen_mini_bsr() if job["name"] == "queen_mini" else system(job["name"], job["bn"])


def job_rhs(job, bsr):
    return spmv(bsr, np.ones(bsr[4])) if job["kind"] == "solve" else rhs(bsr[4])


def child_main(jobs_json, out_path):
    """runs in the child: every job on the reference library, results into one .npz"""
    import lisdrv
    assert os.environ.get("OMP_NUM_THREADS") == "1"
    ref = lisdrv.open_lib(orc.REF_SO, threads=1)
    out = {}
    for k, job in enumerate(json.loads(jobs_json)):
        bsr = job_system(job)
        assert bsr[3] <= 3
        b = job_rhs(job, bsr)
        if job["kind"] == "factor":
            f = reference_bilu(ref, bsr, job["fill"], b)
            for part in ("L", "U"):
                for q, what in enumerate(("ptr", "index", "value")):
                    out["%d_%s_%s" % (k, part, what)] = f[part][q]
            out["%d_D" % k], out["%d_psolve" % k] = f["D"], f["psolve"]
        else:
            A = make_bsr(ref, bsr)
            r = lisdrv.solve(ref, A, b, job["opts"])
            ref.lis_matrix_destroy(A)
            out["%d_x" % k], out["%d_rhistory" % k] = r["x"], r["rhistory"]
            out["%d_meta" % k] = np.array([r["err"], r["iter"], r["status"]], np.int64)
    np.savez(out_path, **out)


def reference_jobs(jobs):
    """the jobs' results from the reference at one thread, in a child process of its own: a list of dicts, one per job"""
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "out.npz")
        code = "import sys; sys.path[:0] = %r; import bilu_cases; bilu_cases.child_main(sys.argv[1], sys.argv[2])" % ([os.path.dirname(HERE), HERE],)
        res = subprocess.run([sys.executable, "-c", code, json.dumps(jobs), path], capture_output=True, text=True,
                             env=dict(os.environ, OMP_NUM_THREADS="1"), timeout=900)
        assert res.returncode == 0, res.stderr[-3000:]
        Z = np.load(path)
        out = []
        for k, job in enumerate(jobs):
            if job["kind"] == "factor":
                out.append({"L": tuple(Z["%d_L_%s" % (k, w)] for w in ("ptr", "index", "value")), "U": tuple(Z["%d_U_%s" % (k, w)] for w in ("ptr", "index", "value")),
                            "D": Z["%d_D" % k], "psolve": Z["%d_psolve" % k]})
            else:
                meta = Z["%d_meta" % k]
                out.append({"err": int(meta[0]), "iter": int(meta[1]), "status": int(meta[2]), "x": Z["%d_x" % k], "rhistory": Z["%d_rhistory" % k]})
        return out
