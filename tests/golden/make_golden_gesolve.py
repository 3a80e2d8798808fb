"""Bit-level goldens of the generalized eigensolvers and of lis_matrix_shift_matrix, taken from the reference (oracle/_ref = Lis 2.1.11 compiled by
oracle/Makefile) through ctypes (tests/gesolve_drv.py).

Solves (tests/gesolve_cases.py SOLVES, options COMMON): at T = 1 and T = 8 OpenMP threads the iteration count, status, eigenvalue, final residual, the FULL
residual history, the eigenvector and A's arrays after the solve; at T = 2 and 4 count, status and eigenvalue (the reference's own spread over the order of
its sums, which bounds the tree mode: tests/test_gesolve_gpu.py).  Asserted here: every solve ends with status 0 and a finite eigenvalue, at ONE eigenpair
over T = 1, 2, 4, 8.  A case the reference does not carry is replaced, not loosened.

Shifts (gesolve_cases.SHIFTS): A's arrays after every shift of each case's sequence (one thread: the dense route does not sum).  "hbm" cases are CSR
cases for the reference; the "ell" and "bsr" cases are not recorded: the reference returns LIS_SUCCESS and leaves such an A untouched (asserted below).

    python tests/golden/make_golden_gesolve.py      (needs oracle/_ref; rewrites gesolve_bits.npz / .json)
"""
import json
import math
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import gesolve_cases as gc      # noqa: E402

WORKER = r'''
import json, os, sys
import numpy as np
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
import gesolve_cases as gc, gesolve_drv as gd, lisdrv, orc
threads = int(sys.argv[1])
ref = gd.open_lib(orc.REF_SO, threads=threads)
out, arrays = {}, {}
def keep(prefix, A):
    for k, v in lisdrv.matrix_arrays(A).items():
        if isinstance(v, np.ndarray): arrays[prefix + "|" + k] = v
        else: out.setdefault(prefix, {})[k] = int(v)
for pencil, e, extra in gc.SOLVES:
    a, b = gc.PENCILS[pencil]()
    A, B = gd.make(ref, a), gd.make(ref, b)
    res = gd.gesolve(ref, A, B, ("-e %%s %%s " %% (e, extra)) + gc.COMMON)
    assert res["err"] == 0, (pencil, e, extra, res)
    key = gc.solve_key(pencil, e, extra, threads)
    out[key] = {"iter": int(res["iter"]), "status": int(res["status"]), "evalue_hex": float(res["evalue"]).hex(), "resid_hex": float(res["resid"]).hex()}
    arrays[key + "|rhistory"] = res["rhistory"]
    arrays[key + "|x"] = res["x"]
    keep(key + "|A", A)
    print(key, res["iter"], res["status"], res["evalue"], res["resid"], file=sys.stderr, flush=True)
    ref.lis_matrix_destroy(A); ref.lis_matrix_destroy(B)
if threads == 1:
    for name, (maker, sigmas, storage) in gc.SHIFTS.items():
        a, b = maker()
        A, B = gd.make(ref, a), gd.make(ref, b)
        if storage in ("ell", "bsr"):
            # the reference cannot serve these: its last step, lis_matrix_convert(dense copy, A), refuses an assembled A that is not CSR, the error is dropped,
            # and lis_matrix_shift_matrix returns LIS_SUCCESS with A as it was.  Asserted, not recorded: the tests take the model's rows in that storage
            X = lisdrv.convert(ref, A, storage); ref.lis_matrix_destroy(A); A = X
            before = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in lisdrv.matrix_arrays(A).items()}
            assert gd.shift(ref, A, B, sigmas[0]) == 0
            after = lisdrv.matrix_arrays(A)
            assert all(np.array_equal(before[k], after[k]) for k in before), name
            ref.lis_matrix_destroy(A); ref.lis_matrix_destroy(B)
            continue
        for step, s in enumerate(sigmas):
            assert gd.shift(ref, A, B, s) == 0, (name, step)
            keep("shift|%%s|%%d" %% (name, step), A)
        print("shift", name, A.contents.matrix_type, A.contents.nnz, file=sys.stderr, flush=True)
        ref.lis_matrix_destroy(A); ref.lis_matrix_destroy(B)
np.savez(sys.argv[2], **arrays)
json.dump(out, open(sys.argv[2] + ".json", "w"))
'''


def main():
    meta, arrays, spread = {}, {}, {}
    for T in gc.THREADS_BITS + gc.THREADS_SPREAD:
        tmp = os.path.join(HERE, "_ges_T%d.npz" % T)
        env = dict(os.environ, OMP_NUM_THREADS=str(T))
        txt = subprocess.run([sys.executable, "-c", WORKER % {"root": ROOT}, str(T), tmp], capture_output=True, text=True, env=env)
        sys.stderr.write(txt.stderr[-8000:])
        txt.check_returncode()
        got = json.load(open(tmp + ".json"))      # (not stdout: the reference prints there too)
        os.unlink(tmp + ".json")
        for k, v in got.items():
            if k.startswith("shift|") or k.endswith("|A"):
                continue
            spread.setdefault(k.rsplit("|", 1)[0], {})["T%d" % T] = {"iter": v["iter"], "status": v["status"], "evalue_hex": v["evalue_hex"]}
        if T in gc.THREADS_BITS:
            meta.update(got)
            with np.load(tmp) as z:
                for k in z.files:
                    arrays[k] = z[k]
        os.unlink(tmp)
    # what the tests stand on: the reference itself ends every case with status 0 at one finite eigenpair whatever its thread count
    for case, sp in sorted(spread.items()):
        ref = float.fromhex(sp["T1"]["evalue_hex"])
        assert sorted(sp) == ["T1", "T2", "T4", "T8"], case
        for t in sorted(sp):
            ev = float.fromhex(sp[t]["evalue_hex"])
            assert sp[t]["status"] == 0 and math.isfinite(ev) and abs(ev - ref) <= 2.0 * gc.ETOL * abs(ref), (case, t, sp[t]["status"], ev, ref)
    np.savez_compressed(os.path.join(HERE, "gesolve_bits.npz"), **arrays)
    doc = {"_source": "Lis 2.1.11 (oracle/_ref, gcc -O3 -fopenmp, no FMA) through ctypes: lis_gesolve at OMP_NUM_THREADS = 1 and 8 -- residual history, eigenvector and A's "
                      "arrays after the solve (f64 / i32, every bit) in gesolve_bits.npz under 'pencil|options|T<threads>|rhistory', '...|x', '...|A|<array>'; spread: count, "
                      "status and eigenvalue at T = 1, 2, 4, 8 -- and lis_matrix_shift_matrix: A's arrays after shift <step> of each case under 'shift|case|step|<array>'",
           "common_options": gc.COMMON, "solves": {k: v for k, v in meta.items() if not k.startswith("shift|")},
           "shifts": {k: v for k, v in meta.items() if k.startswith("shift|")}, "spread": spread}
    json.dump(doc, open(os.path.join(HERE, "gesolve_bits.json"), "w"), indent=1, sort_keys=True)
    print(len(spread), "gesolves,", len(doc["shifts"]), "shifted matrices written")


if __name__ == "__main__":
    main()
