"""Bit-level goldens of whole eigensolves: iteration count, status, eigenvalue, final residual, the FULL residual history and the eigenvector of the
reference (oracle/_ref = Lis 2.1.11 compiled by oracle/Makefile) at T = 1 and T = 8 OpenMP threads, and count, status and eigenvalue at T = 2 and 4 as well
(the reference's own spread over the order of its sums, which bounds the tree mode: tests/test_esolve_gpu.py).

The reference's dot / nrm2 depend on T (src/vector/lis_vector_ops.c:88-107, :241-259); liblis_amd's reference-order mode forms the same sums, its loops
(host/lis_esolver.c) restate lis_esolver_pi.c / _ii.c / _rqi.c / _cg.c statement for statement, and its inner BiCG / CG solves already carry the
reference's bits (tests/test_reference_order_gpu.py) -- so every case below must come back in every bit.

Cases (tests/esolve_drv.py builds the matrices; the tests rebuild them with the same code):
  sym7        7-point Poisson on 7^3 with a varied diagonal: symmetric, both extreme pairs well separated.  Every solver must end with status 0 in under
              500 outer iterations at every T (asserted below).  With -shift 0, with a non-zero -shift, with -initx_ones false, with -estorage ell.
              The start vector of -initx_ones false (esolve_drv.start_vector) lies near the lowest eigenvector, so that Rayleigh quotient iteration
              finds that pair at every T; that every symmetric case ends at ONE eigenpair over T = 1, 2, 4, 8 is asserted below as well
  mm/testmat0.mtx   the reference's own fixture (the 5-point Laplacian on 10 x 10: an even side, the all-ones start vector is orthogonal to its top
              mode -- power iteration creeps; whatever status the reference ends with is the golden)
  nonsym7     the same grid, nonsymmetric couplings: power iteration only, reference-order mode only

    python tests/golden/make_golden_esolve.py      (needs oracle/_ref; rewrites esolve_bits.npz / .json and esolve_options.json)
"""
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

ETOL = 1e-10
COMMON = " -etol 1e-10 -emaxiter 500 -eprint mem"
SOLVERS = ("pi", "ii", "rqi", "cg", "cr")
# (matrix, solvers, extra options, start vector given, must converge)
CASES = [
    ("sym7", SOLVERS, "-shift 0", False, True),
    ("sym7", SOLVERS, "-shift 0.75", False, True),
    ("sym7", SOLVERS, "-shift 0 -initx_ones false", True, True),
    ("sym7", SOLVERS, "-shift 0 -estorage ell", False, True),
    ("mm/testmat0.mtx", SOLVERS, "-shift 0", False, False),
    ("mm/testmat0.mtx", SOLVERS, "-shift 0.25", False, False),
    ("nonsym7", ("pi",), "-shift 0", False, False),
    ("nonsym7", ("pi",), "-shift 0.75", False, False),
]
THREADS_BITS = (1, 8)
THREADS_SPREAD = (2, 4)

WORKER = r'''
import json, os, sys
import numpy as np
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
import esolve_drv, orc
threads = int(sys.argv[1])
ref = esolve_drv.open_lib(orc.REF_SO, threads=threads)
out, arrays = {}, {}
for matrix, solvers, extra, given, must in %(cases)r:
    for e in solvers:
        A = esolve_drv.make_matrix(ref, matrix)           # (-estorage converts the caller's matrix for good: a fresh one per solve)
        n = A.contents.n
        opts = "-e " + e + " " + extra
        res = esolve_drv.esolve(ref, A, opts + %(common)r, esolve_drv.start_vector(n) if given else None)
        assert res["err"] == 0, (matrix, opts, res)
        if must:
            assert res["status"] == 0 and res["iter"] < 500, (matrix, opts, threads, res["iter"], res["status"])
        key = "%%s|%%s|T%%d" %% (matrix, opts, threads)
        out[key] = {"iter": int(res["iter"]), "status": int(res["status"]), "evalue_hex": float(res["evalue"]).hex(), "resid_hex": float(res["resid"]).hex(),
                    "n": int(n), "given": bool(given), "symmetric": matrix != "nonsym7"}
        arrays[key + "|rhistory"] = res["rhistory"]
        arrays[key + "|x"] = res["x"]
        print(key, res["iter"], res["status"], res["evalue"], res["resid"], file=sys.stderr, flush=True)
        ref.lis_matrix_destroy(A)
np.savez(sys.argv[2], **arrays)
json.dump(out, open(sys.argv[2] + ".json", "w"))
if threads == 1:          # the option tables (lis_esolver.c:103-122) as the reference parses them: what tests/test_esolve_cpu.py holds the parser to where oracle/_ref is absent
    parsed = {}
    for text in esolve_drv.OPTION_TEXTS:
        err, options, params = esolve_drv.parsed(ref, text)
        parsed[text] = {"err": err, "options": options, "params_hex": [float(p).hex() for p in params]}
    json.dump({"_source": "lis_esolver_set_option of Lis 2.1.11 (oracle/_ref) on a fresh esolver: return code, options[], params[]", "parsed": parsed},
              open(os.path.join(%(here)r, "esolve_options.json"), "w"), indent=1, sort_keys=True)
'''


def main():
    meta, arrays, spread = {}, {}, {}
    for T in THREADS_BITS + THREADS_SPREAD:
        tmp = os.path.join(HERE, "_es_T%d.npz" % T)
        env = dict(os.environ, OMP_NUM_THREADS=str(T))
        src = WORKER % {"root": ROOT, "here": HERE, "cases": CASES, "common": COMMON}
        txt = subprocess.run([sys.executable, "-c", src, str(T), tmp], capture_output=True, text=True, env=env)
        sys.stderr.write(txt.stderr[-6000:])
        txt.check_returncode()
        got = json.load(open(tmp + ".json"))      # (not stdout: the reference prints there too)
        os.unlink(tmp + ".json")
        for k, v in got.items():
            spread.setdefault(k.rsplit("|", 1)[0], {})["T%d" % T] = {"iter": v["iter"], "status": v["status"], "evalue_hex": v["evalue_hex"]}
        if T in THREADS_BITS:
            meta.update(got)
            with np.load(tmp) as z:
                for k in z.files:
                    arrays[k] = z[k]
        os.unlink(tmp)
    # what the tree-mode contract of tests/test_esolve_gpu.py stands on: on every symmetric case the reference itself ends with status 0 at one eigenpair
    # whatever its thread count, within the contract's own bound of its T = 1 eigenvalue
    for case, sp in sorted(spread.items()):
        if case.startswith("nonsym"):
            continue
        ref = float.fromhex(sp["T1"]["evalue_hex"])
        for t in sorted(sp):
            ev = float.fromhex(sp[t]["evalue_hex"])
            assert sp[t]["status"] == 0 and abs(ev - ref) <= 2.0 * ETOL * abs(ref), (case, t, sp[t]["status"], ev, ref)
    np.savez_compressed(os.path.join(HERE, "esolve_bits.npz"), **arrays)
    doc = {"_source": "Lis 2.1.11 (oracle/_ref, gcc -O3 -fopenmp, no FMA) at OMP_NUM_THREADS = 1 and 8; the residual history and the eigenvector (f64, every bit) "
                      "in esolve_bits.npz under 'case|options|T<threads>|rhistory' and '...|x'; spread: count, status and eigenvalue at T = 1, 2, 4, 8",
           "common_options": COMMON.strip(), "solves": meta, "spread": spread}
    json.dump(doc, open(os.path.join(HERE, "esolve_bits.json"), "w"), indent=1, sort_keys=True)
    print(len(meta), "esolves written")


if __name__ == "__main__":
    main()
