"""Bit-level goldens of whole solves under -p sainv and -p is: iteration count, status, the FULL residual history and the solution from
the reference (oracle/_ref = Lis compiled from the reference sources by oracle/Makefile) at T = 1 and T = 8 OpenMP threads, and the
iteration counts alone at T = 2 and 4 (the spread the tree mode's count is held to).

The reference's scatter products (lis_matvec_ilu, lis_psolveh_is) and its dot products sum per thread chunk: liblis_amd reproduces both
under lis_amd_set_reference_reductions(T); tests/test_sainv_gpu.py and tests/test_is_gpu.py demand the same count, status, history bits
and solution bits.

Cases (tests/sainv_cases.py WHOLE): the 7-point Poisson matrix on 6 x 5 x 4 and the non-symmetric n = 120 matrix, b = A * 1, with CG,
BiCG, BiCGSTAB and GMRES(30) under -p sainv and CG, BiCG under -p is (CG only on the symmetric matrix).  Every solve must reach status 0
at every T.

    python tests/golden/make_golden_sainv.py      (needs oracle/_ref; rewrites sainv_bits.npz / .json)
"""
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
BITS_AT = (1, 8)
SPREAD_AT = (1, 2, 4, 8)

WORKER = r'''
import hashlib, json, os, sys
import numpy as np
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
import lisdrv, orc, sainv_cases as sc
threads = int(sys.argv[1])
ref = lisdrv.open_lib(orc.REF_SO, threads=threads)
out, arrays = {}, {}
for mat, opts in sc.WHOLE:
    ptr, idx, val = sc.system(mat)
    A = lisdrv.make_csr(ref, ptr, idx, val)
    res = lisdrv.solve(ref, A, sc.rhs(ptr, idx, val), opts + " " + sc.COMMON)
    key = "%%s|%%s|T%%d" %% (mat, opts, threads)
    assert res["err"] == 0 and res["status"] == 0, (key, res["err"], res["status"])
    out[key] = {"iter": int(res["iter"]), "status": int(res["status"]), "resid_hex": float(res["resid"]).hex(),
                "x_sha256": hashlib.sha256(np.ascontiguousarray(res["x"]).tobytes()).hexdigest(), "n": int(len(ptr) - 1)}
    arrays[key] = res["rhistory"]
    ref.lis_matrix_destroy(A)
np.savez(sys.argv[2], **arrays)
json.dump(out, open(sys.argv[2] + ".json", "w"))
'''


def main():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import sainv_cases as sc
    meta, arrays, counts = {}, {}, {}
    for T in SPREAD_AT:
        tmp = os.path.join(HERE, "_sainv_T%d.npz" % T)
        txt = subprocess.run([sys.executable, "-c", WORKER % {"root": ROOT}, str(T), tmp], capture_output=True, text=True,
                             env=dict(os.environ, OMP_NUM_THREADS=str(T)))
        sys.stderr.write(txt.stderr[-4000:])
        txt.check_returncode()
        got = json.load(open(tmp + ".json"))
        os.unlink(tmp + ".json")
        for k, v in got.items():
            assert v["status"] == 0, k
            counts.setdefault(k.rsplit("|", 1)[0], []).append(v["iter"])
        if T in BITS_AT:
            meta.update(got)
            with np.load(tmp) as z:
                for k in z.files:
                    arrays[k] = z[k]
        os.unlink(tmp)
    spread = {k: [min(v), max(v)] for k, v in counts.items()}
    np.savez_compressed(os.path.join(HERE, "sainv_bits.npz"), **arrays)
    doc = {"_source": "Lis (oracle/_ref, gcc -O3 -fopenmp, no FMA) at OMP_NUM_THREADS = 1 and 8; rhistory arrays (f64, every bit) in sainv_bits.npz under "
                      "the keys 'matrix|options|T<threads>'; x_sha256 = sha256 of the bytes of x; spread = [fewest, most] iterations over T = 1, 2, 4, 8",
           "common_options": sc.COMMON, "solves": meta, "spread": spread}
    json.dump(doc, open(os.path.join(HERE, "sainv_bits.json"), "w"), indent=1, sort_keys=True)
    print(len(meta), "entries written; spread", spread)


if __name__ == "__main__":
    main()
