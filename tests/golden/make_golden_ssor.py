"""Bit-level goldens of whole solves with the SSOR preconditioner: iteration count, status, the FULL residual history and the solution
of the reference (oracle/_ref = Lis compiled from the reference sources by oracle/Makefile) at T = 1 and T = 8 OpenMP threads.

The reference's SSOR sweeps run one row block per thread (LIS_GET_ISIE, src/matrix/lis_matrix_csr.c:1572-1627): at T = 8 the
preconditioner itself is block-Jacobi SSOR with 8 blocks.  liblis_amd reproduces both under lis_amd_set_reference_reductions(T);
tests/test_ssor_gpu.py demands the same count, status, history bits and solution bits.  Also kept: the bits of A->WD after
"-p ssor -ssor_omega 1.3" and of lis_matrix_solve / lis_matrix_solveh (flag SSOR) on b = 1..n scaled, at both T.

Cases: poisson32 (7-point Poisson 32^3, orc.poisson3d, b = A*1) and mm/testmat0.mtx (lis_input, b = A*1), each with CG, BiCGSTAB,
GMRES(30) and BiCG under -p ssor -ssor_omega 1.2, tol 1e-12.

    python tests/golden/make_golden_ssor.py      (needs oracle/_ref; rewrites ssor_bits.npz / .json)
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

SOLVES = ("-i cg", "-i bicgstab", "-i gmres -restart 30", "-i bicg")
THREADS = (1, 8)
COMMON = " -p ssor -ssor_omega 1.2 -tol 1e-12 -maxiter 2000 -print mem"

WORKER = r'''
import ctypes as C, hashlib, json, os, sys
import numpy as np
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
import lisdrv, orc
from lis_amd import _capi as capi
threads = int(sys.argv[1])
ref = lisdrv.open_lib(orc.REF_SO, threads=threads)
out, arrays = {}, {}

def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()

def matrix(case):
    if case == "poisson32":
        ptr, idx, val = orc.poisson3d(32, 32, 32)
        return lisdrv.make_csr(ref, ptr, idx, val)
    A, b, x = capi.PM(), capi.PV(), capi.PV()
    assert ref.lis_matrix_create(capi.LIS_COMM_WORLD, C.byref(A)) == 0
    assert ref.lis_vector_create(capi.LIS_COMM_WORLD, C.byref(b)) == 0 and ref.lis_vector_create(capi.LIS_COMM_WORLD, C.byref(x)) == 0
    assert ref.lis_input(A, b, x, os.path.join(%(here)r, "mm", "testmat0.mtx").encode()) == 0
    return A

for case in ("poisson32", "mm/testmat0.mtx"):
    for opts in %(solves)r:
        A = matrix(case)
        n = A.contents.n
        rhs = lisdrv.matvec(ref, A, np.ones(n))
        res = lisdrv.solve(ref, A, rhs, opts + %(common)r)
        key = "%%s|%%s|T%%d" %% (case, opts, threads)
        out[key] = {"iter": int(res["iter"]), "status": int(res["status"]), "resid_hex": float(res["resid"]).hex(), "x_sha256": sha(res["x"]), "n": int(n)}
        arrays[key] = res["rhistory"]
        ref.lis_matrix_destroy(A)
    # WD and the two SSOR solves after one -p ssor -ssor_omega 1.3 solve
    A = matrix(case)
    n = A.contents.n
    rhs = lisdrv.matvec(ref, A, np.ones(n))
    lisdrv.solve(ref, A, rhs, "-i cg -p ssor -ssor_omega 1.3 -maxiter 1")
    wd = np.ctypeslib.as_array(C.cast(A.contents.WD, C.POINTER(capi.MatrixDiag)).contents.value, shape=(n,)).copy()
    b = np.arange(1, n + 1, dtype=np.float64) / n
    for tag, fn in (("solve", ref.lis_matrix_solve), ("solveh", ref.lis_matrix_solveh)):
        vb, vx = lisdrv.new_vector(ref, A, b), lisdrv.new_vector(ref, A)
        assert fn(A, vb, vx, capi.LIS_MATRIX_SSOR) == 0
        out["%%s|%%s|T%%d" %% (case, tag, threads)] = {"sha256": sha(lisdrv.get_vector(ref, vx, n))}
        ref.lis_vector_destroy(vb); ref.lis_vector_destroy(vx)
    out["%%s|wd|T%%d" %% (case, threads)] = {"sha256": sha(wd)}
    ref.lis_matrix_destroy(A)
np.savez(sys.argv[2], **arrays)
json.dump(out, open(sys.argv[2] + ".json", "w"))
'''


def main():
    meta, arrays = {}, {}
    for T in THREADS:
        tmp = os.path.join(HERE, "_ssor_T%d.npz" % T)
        env = dict(os.environ, OMP_NUM_THREADS=str(T))
        src = WORKER % {"root": ROOT, "here": HERE, "solves": SOLVES, "common": COMMON}
        txt = subprocess.run([sys.executable, "-c", src, str(T), tmp], capture_output=True, text=True, env=env)
        sys.stderr.write(txt.stderr[-4000:])
        txt.check_returncode()
        meta.update(json.load(open(tmp + ".json")))
        os.unlink(tmp + ".json")
        with np.load(tmp) as z:
            for k in z.files:
                arrays[k] = z[k]
        os.unlink(tmp)
    np.savez_compressed(os.path.join(HERE, "ssor_bits.npz"), **arrays)
    doc = {"_source": "Lis (oracle/_ref, gcc -O3 -fopenmp, no FMA) at OMP_NUM_THREADS = 1 and 8; rhistory arrays (f64, every bit) in ssor_bits.npz "
                      "under the keys 'case|options|T<threads>'; x_sha256 / sha256 = sha256 of the bytes of x, of A->WD ('case|wd|T') and of "
                      "lis_matrix_solve / _solveh with flag SSOR on b[i] = (i+1)/n ('case|solve|T', 'case|solveh|T')",
           "common_options": COMMON.strip(), "solves": meta}
    json.dump(doc, open(os.path.join(HERE, "ssor_bits.json"), "w"), indent=1, sort_keys=True)
    print(len(meta), "solves written")


if __name__ == "__main__":
    main()
