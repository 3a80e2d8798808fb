"""Bit-level goldens of the eigensolvers of several pairs (-e si | li | ai): per mode the eigenvalue, the residual and the count, the status, the whole residual
history, x and every eigenvector of the reference (oracle/_ref = Lis 2.1.11 compiled by oracle/Makefile) at T = 1 and T = 8 OpenMP threads; counts and eigenvalues
at T = 2 and 4 as well.  liblis_amd's loops (host/lis_esolver.c) restate lis_esolver_si.c / _li.c / _ai.c statement for statement on sums formed in the
reference's order, so every bit case must come back in every bit (tests/test_esolve_multi_gpu.py).

Bit cases (esolve_multi_drv.BIT_CASES) run with -etol 1e-10 -emaxiter 60 -eprint mem: sixty keeps every case short, and bits are bits whether a mode converged
or not.  A -rval true case stores eigenvalues only (the reference leaves iter[] / resid[] / evector[] as the heap had them).  -e si -ie ii on nonsym7 is left
out: the reference ends modes 1 and 2 in NaN at T = 1 and not at T = 8.

Tree cases (esolve_multi_drv.TREE_CASES) run with -etol 1e-10 -emaxiter 150.  A mode is admitted to the tree-mode comparison only if the reference ends it
with resid <= etol and iter < emaxiter at ALL of T = 1, 2, 4, 8, within 2 etol |evalue| of its own T = 1 value; the list of admitted modes is written, and that
it holds the modes each case names is asserted here.

    python tests/golden/make_golden_esolve_multi.py      (needs oracle/_ref; rewrites esolve_multi_bits.npz / .json)
"""
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import esolve_multi_drv as emd      # noqa: E402

THREADS_BITS = (1, 8)
THREADS_SPREAD = (2, 4)
TREE_MAXITER = 150

WORKER = r'''
import json, os, sys
import numpy as np
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
import esolve_multi_drv as emd, orc, esolve_drv
threads = int(sys.argv[1])
ref = esolve_drv.open_lib(orc.REF_SO, threads=threads)
out, arrays = {}, {}
runs = [(m, o, emd.BIT_COMMON, "bits") for m, o in emd.BIT_CASES] + [(m, o, emd.TREE_COMMON, "tree") for m, o, _ in emd.TREE_CASES]
for matrix, opts, common, kind in runs:
    A = emd.make_matrix(ref, matrix)                  # (-estorage converts the caller's matrix for good: a fresh one per solve)
    rval = "-rval true" in opts
    res = emd.esolve(ref, A, opts + common)
    assert res["err"] == 0, (matrix, opts, res["err"])
    key = "%%s|%%s|%%s|T%%d" %% (kind, matrix, opts, threads)
    out[key] = {"status": int(res["status"]), "ss": res["ss"], "n": int(A.contents.n), "rval": rval, "evalue0_hex": float(res["evalue0"]).hex(),
                "evalue_hex": [float(v).hex() for v in res["evalue"]]}
    if not rval:
        out[key].update(iter=[int(v) for v in res["iter"]], resid_hex=[float(v).hex() for v in res["resid"]])
        if kind == "bits":
            arrays[key + "|rhistory"] = res["rhistory"]
            arrays[key + "|x"] = res["x"]
            for i, v in enumerate(res["evector"]):
                arrays[key + "|evector%%d" %% i] = v
    print(key, out[key].get("iter"), [float(v) for v in res["evalue"]], file=sys.stderr, flush=True)
    emd.release(ref, res)
    ref.lis_matrix_destroy(A)
np.savez(sys.argv[2], **arrays)
json.dump(out, open(sys.argv[2] + ".json", "w"))
'''


def main():
    meta, arrays, every = {}, {}, {}
    for T in THREADS_BITS + THREADS_SPREAD:
        tmp = os.path.join(HERE, "_esm_T%d.npz" % T)
        env = dict(os.environ, OMP_NUM_THREADS=str(T))
        txt = subprocess.run([sys.executable, "-c", WORKER % {"root": ROOT}, str(T), tmp], capture_output=True, text=True, env=env)
        sys.stderr.write(txt.stderr[-8000:])
        txt.check_returncode()
        got = json.load(open(tmp + ".json"))          # (not stdout: the reference prints there too)
        os.unlink(tmp + ".json")
        every.update(got)
        if T in THREADS_BITS:
            meta.update({k: v for k, v in got.items() if k.startswith("bits|")})
            with np.load(tmp) as z:
                for k in z.files:
                    arrays[k] = z[k]
        os.unlink(tmp)
    spread = {}
    for k, v in every.items():
        case, t = k.rsplit("|", 1)
        spread.setdefault(case, {})[t] = {"iter": v.get("iter"), "evalue_hex": v["evalue_hex"], "resid_hex": v.get("resid_hex"), "status": v["status"]}
    # the modes the tree-mode contract of tests/test_esolve_multi_gpu.py stands on
    tree = {}
    for matrix, opts, must in emd.TREE_CASES:
        case = "tree|%s|%s" % (matrix, opts)
        sp = spread[case]
        admitted = []
        for mode in range(emd.subspace(opts)):
            ref = float.fromhex(sp["T1"]["evalue_hex"][mode])
            ok = all(float.fromhex(sp[t]["resid_hex"][mode]) <= emd.ETOL and sp[t]["iter"][mode] < TREE_MAXITER
                     and abs(float.fromhex(sp[t]["evalue_hex"][mode]) - ref) <= 2.0 * emd.ETOL * abs(ref) for t in ("T1", "T2", "T4", "T8"))
            print(case, "mode", mode, "admitted" if ok else "left out", [(sp[t]["iter"][mode], float.fromhex(sp[t]["resid_hex"][mode])) for t in ("T1", "T2", "T4", "T8")], file=sys.stderr)
            if ok:
                admitted.append(mode)
        if isinstance(must, int):
            assert len(admitted) >= must, (case, admitted)
        else:
            assert set(must) <= set(admitted), (case, admitted)
        tree[case] = {"admitted": admitted,
                      "iter": {str(m): [sp[t]["iter"][m] for t in ("T1", "T2", "T4", "T8")] for m in admitted},
                      "evalue_T1_hex": {str(m): sp["T1"]["evalue_hex"][m] for m in admitted}}
    np.savez_compressed(os.path.join(HERE, "esolve_multi_bits.npz"), **arrays)
    doc = {"_source": "Lis 2.1.11 (oracle/_ref, gcc -O3 -fopenmp, no FMA) at OMP_NUM_THREADS = 1 and 8: per mode evalue / resid / iter, status; the residual history, x and "
                      "every eigenvector (f64, every bit) in esolve_multi_bits.npz under 'bits|matrix|options|T<threads>|rhistory', '...|x', '...|evector<i>'; spread: "
                      "counts and eigenvalues at T = 1, 2, 4, 8; tree: the modes the reference converges at every T, their counts over T and their T = 1 eigenvalues",
           "bit_common_options": emd.BIT_COMMON.strip(), "tree_common_options": emd.TREE_COMMON.strip(), "solves": meta,
           "spread": {k: {t: {"iter": v["iter"], "evalue_hex": v["evalue_hex"]} for t, v in sp.items()} for k, sp in spread.items()}, "tree": tree}
    json.dump(doc, open(os.path.join(HERE, "esolve_multi_bits.json"), "w"), indent=1, sort_keys=True)
    print(len(meta), "esolves written;", {k: v["admitted"] for k, v in tree.items()})


if __name__ == "__main__":
    main()
