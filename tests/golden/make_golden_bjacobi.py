"""Bit-level goldens of the block Jacobi preconditioner: whole solves (iteration count, status, the FULL residual history, the solution)
and WD itself, from the reference (oracle/_ref = Lis compiled from the reference sources by oracle/Makefile) at T = 1 and T = 8
OpenMP threads.

The preconditioner does not depend on T (one thread inverts and applies a block); the Krylov loops' sums do.  liblis_amd
reproduces both under lis_amd_set_reference_reductions(T); tests/test_bjacobi_gpu.py demands the same count, status, history bits
and solution bits.  Also kept, per block size and T: the sha256 of WD (nr * k * k values, the last block padded).

Cases: poisson7x5x3 and poisson16 (7-point Poisson, orc.poisson3d, b = A*1) and mm/testmat0.mtx (read as CSR, b = A*1), each with
CG, BiCGSTAB, GMRES(30) and BiCG under -p bjacobi -storage bsr -storage_block k, k = 2, 3, 4, 5, tol 1e-12.  Block sizes 2 and 4 leave
a partial last block on 7 x 5 x 3 (n = 105), 3 and 5 on 16^3 (n = 4096), 3 on testmat0 (n = 100).  Every kept solve reaches status 0;
a solve that does not in the reference is dropped and listed under "dropped" in the .json -- with the matrices as they are: none.

The reference's lis_precon_create runs at one thread in every case (tests/bjacobi_cases.py, class one_thread: its block inversion
is not safe to run in parallel); everything else runs at T threads.

    python tests/golden/make_golden_bjacobi.py      (needs oracle/_ref; rewrites bjacobi_bits.npz / .json)
"""
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

SOLVES = ("-i cg", "-i bicgstab", "-i gmres -restart 30", "-i bicg")
BLOCKS = (2, 3, 4, 5)
CASES = ("poisson7x5x3", "poisson16", "mm/testmat0.mtx")
THREADS = (1, 8)
COMMON = "-p bjacobi -storage bsr -tol 1e-12 -maxiter 2000 -print mem"

WORKER = r'''
import hashlib, json, os, sys
import numpy as np
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
import lisdrv, orc, bjacobi_cases as cases
threads = int(sys.argv[1])
ref = lisdrv.open_lib(orc.REF_SO, threads=threads)
out, dropped, arrays = {}, [], {}

def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()

for case in %(cases)r:
    ptr, idx, val = cases.golden_system(case)
    n = len(ptr) - 1
    for k in %(blocks)r:
        for opts in %(solves)r:
            A = lisdrv.make_csr(ref, ptr, idx, val)
            rhs = lisdrv.matvec(ref, A, np.ones(n))
            res = cases.reference_solve(ref, A, rhs, "%%s -storage_block %%d %%s" %% (opts, k, %(common)r))
            key = "%%s|%%s|k%%d|T%%d" %% (case, opts, k, threads)
            ok = res["err"] == 0 and res["status"] == 0 and A.contents.matrix_type == 7 and A.contents.is_splited
            ref.lis_matrix_destroy(A)
            if not ok:
                dropped.append(key)
                continue
            out[key] = {"iter": int(res["iter"]), "status": int(res["status"]), "resid_hex": float(res["resid"]).hex(), "x_sha256": sha(res["x"]), "n": int(n)}
            arrays[key] = res["rhistory"]
        wd = cases.reference_bjacobi(ref, ptr, idx, val, k, cases.rhs(n))["WD"]
        out["%%s|WD|k%%d|T%%d" %% (case, k, threads)] = {"sha256": sha(wd), "count": int(len(wd))}
np.savez(sys.argv[2], **arrays)
json.dump({"solves": out, "dropped": dropped}, open(sys.argv[2] + ".json", "w"))
'''


def main():
    meta, dropped, arrays = {}, [], {}
    for T in THREADS:
        tmp = os.path.join(HERE, "_bjacobi_T%d.npz" % T)
        env = dict(os.environ, OMP_NUM_THREADS=str(T))
        src = WORKER % {"root": ROOT, "cases": CASES, "blocks": BLOCKS, "solves": SOLVES, "common": COMMON}
        txt = subprocess.run([sys.executable, "-c", src, str(T), tmp], capture_output=True, text=True, env=env)
        sys.stderr.write(txt.stderr[-4000:])
        txt.check_returncode()
        part = json.load(open(tmp + ".json"))
        meta.update(part["solves"])
        dropped += part["dropped"]
        os.unlink(tmp + ".json")
        with np.load(tmp) as z:
            for k in z.files:
                arrays[k] = z[k]
        os.unlink(tmp)
    for k, v in meta.items():
        assert v.get("status", 0) == 0, k
    np.savez_compressed(os.path.join(HERE, "bjacobi_bits.npz"), **arrays)
    doc = {"_source": "Lis (oracle/_ref, gcc -O3 -fopenmp, no FMA) at OMP_NUM_THREADS = 1 and 8, lis_precon_create at one thread; rhistory arrays (f64, "
                      "every bit) in bjacobi_bits.npz under the keys 'case|options|k<block>|T<threads>'; x_sha256 = sha256 of the bytes of x; "
                      "'case|WD|k<block>|T<threads>': sha256 of the nr * k * k values of precon->WD",
           "common_options": COMMON, "cases": list(CASES), "dropped": sorted(dropped), "solves": meta}
    json.dump(doc, open(os.path.join(HERE, "bjacobi_bits.json"), "w"), indent=1, sort_keys=True)
    print(len(meta), "entries written,", len(dropped), "dropped", dropped)


if __name__ == "__main__":
    main()
