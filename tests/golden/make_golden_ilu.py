"""Bit-level goldens of the ILU(k) preconditioner: whole solves (iteration count, status, the FULL residual history, the solution)
and the factor itself, from the reference (oracle/_ref = Lis compiled from the reference sources by oracle/Makefile) at T = 1 and
T = 8 OpenMP threads.

The reference factorises and sweeps one row block per thread (LIS_GET_ISIE, src/precon/lis_precon_iluk.c): at T = 8 the
preconditioner is block-Jacobi ILU with 8 blocks.  liblis_amd reproduces both under lis_amd_set_reference_reductions(T);
tests/test_ilu_gpu.py demands the same count, status, history bits and solution bits.  Also kept, per fill level 0, 1, 2 and T: the
sha256 of the values of L and U (in the pattern's term order), of D, and of M^-1 b and M^-H b on b[i] = (i + 1) / n.

Cases: poisson32 (7-point Poisson 32^3, orc.poisson3d, b = A*1) and mm/testmat0.mtx (lis_input, b = A*1), each with CG, BiCGSTAB,
GMRES(30) and BiCG under -p ilu, and CG under -p ilu -ilu_fill 1 and 2, tol 1e-12.  Every solve must reach status 0.

    python tests/golden/make_golden_ilu.py      (needs oracle/_ref; rewrites ilu_bits.npz / .json)
"""
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

SOLVES = ("-i cg", "-i bicgstab", "-i gmres -restart 30", "-i bicg", "-i cg -ilu_fill 1", "-i cg -ilu_fill 2")
THREADS = (1, 8)
COMMON = " -p ilu -tol 1e-12 -maxiter 2000 -print mem"

WORKER = r'''
import ctypes as C, hashlib, json, os, sys
import numpy as np
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
import lisdrv, orc, ilu_cases
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
        assert res["err"] == 0 and res["status"] == 0, (key, res["err"], res["status"])
        out[key] = {"iter": int(res["iter"]), "status": int(res["status"]), "resid_hex": float(res["resid"]).hex(), "x_sha256": sha(res["x"]), "n": int(n)}
        arrays[key] = res["rhistory"]
        ref.lis_matrix_destroy(A)
    # the factor and the two psolves, from the arrays the library holds for the case
    A = matrix(case)
    arr = lisdrv.matrix_arrays(A)
    ref.lis_matrix_destroy(A)
    n = arr["n"]
    for fill in (0, 1, 2):
        f = ilu_cases.reference_ilu(ref, arr["ptr"], arr["index"], arr["value"], fill, ilu_cases.rhs(n))
        for tag, a in (("L", f["L"][2]), ("U", f["U"][2]), ("D", f["D"]), ("psolve", f["psolve"]), ("psolveh", f["psolveh"])):
            out["%%s|%%s|fill%%d|T%%d" %% (case, tag, fill, threads)] = {"sha256": sha(a), "count": int(len(a))}
np.savez(sys.argv[2], **arrays)
json.dump(out, open(sys.argv[2] + ".json", "w"))
'''


def main():
    meta, arrays = {}, {}
    for T in THREADS:
        tmp = os.path.join(HERE, "_ilu_T%d.npz" % T)
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
    for k, v in meta.items():
        assert v.get("status", 0) == 0, k
    np.savez_compressed(os.path.join(HERE, "ilu_bits.npz"), **arrays)
    doc = {"_source": "Lis (oracle/_ref, gcc -O3 -fopenmp, no FMA) at OMP_NUM_THREADS = 1 and 8; rhistory arrays (f64, every bit) in ilu_bits.npz "
                      "under the keys 'case|options|T<threads>'; x_sha256 / sha256 = sha256 of the bytes of x, of the values of L and U in term "
                      "order ('case|L|fill<k>|T', 'case|U|...'), of D = 1 / pivot ('case|D|...') and of lis_psolve_iluk_csr / lis_psolveh_iluk_csr "
                      "on b[i] = (i+1)/n ('case|psolve|...', 'case|psolveh|...')",
           "common_options": COMMON.strip(), "solves": meta}
    json.dump(doc, open(os.path.join(HERE, "ilu_bits.json"), "w"), indent=1, sort_keys=True)
    print(len(meta), "entries written")


if __name__ == "__main__":
    main()
