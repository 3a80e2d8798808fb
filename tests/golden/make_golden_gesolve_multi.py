"""Bit-level goldens of several pairs of the generalized problem (-e gsi | gli | gai through lis_gesolve), taken from the reference (oracle/_ref = Lis 2.1.11
compiled by oracle/Makefile) through ctypes (tests/gesolve_multi_cases.py): per mode the eigenvalue, the residual and the count, the status, the whole residual
history, x, every eigenvector and A's arrays after the solve at T = 1 and T = 8 OpenMP threads.  liblis_amd's loops (host/lis_esolver.c) restate lis_egsi,
lis_egli and lis_egai statement for statement on sums formed in the reference's order, so every bit case must come back in every bit
(tests/test_gesolve_multi_gpu.py).  A's arrays belong to it: Lanczos and Arnoldi refine each mode through a one-pair solver that shifts A by the Ritz value
and back, and that drift -- with a rebuilt pattern where B's is not inside A's (P4) -- is part of the parity.

Bit cases (gesolve_multi_cases.BIT_CASES) run with -etol 1e-10 -emaxiter 60 -eprint mem: sixty keeps every case short, and bits are bits whether a mode
converged or not (a mode of -e gsi may end in NaN: eta = <v,w>^1/2 has no fabs there).  A -rval true case stores eigenvalues only (the reference leaves
iter[] / resid[] / evector[] as the heap had them).

Tree cases (gesolve_multi_cases.TREE_CASES) run with -etol 1e-10 -emaxiter 150 at T = 1, 2, 4, 8.  A mode is admitted to the tree-mode comparison only if the
reference ends it below -emaxiter at every T, at one finite eigenvalue: within 2 etol |evalue| of its own T = 1 value (gesolve_multi_cases.admitted).  The
admitted modes and the spread of their counts are written; that they hold the modes each case names is asserted here.  A case the reference does not carry is
replaced, not loosened.

    python tests/golden/make_golden_gesolve_multi.py      (needs oracle/_ref; rewrites gesolve_multi_bits.npz / .json)
"""
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import gesolve_multi_cases as gm      # noqa: E402

WORKER = r'''
import json, os, sys
import numpy as np
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
import gesolve_multi_cases as gm, gesolve_drv as gd, lisdrv, orc
threads = int(sys.argv[1])
ref = gd.open_lib(orc.REF_SO, threads=threads)
out, arrays = {}, {}
runs = [(p, o, gm.TREE_COMMON, "tree") for p, o, _ in gm.TREE_CASES]
if threads in gm.THREADS_BITS:
    runs = [(p, o, gm.BIT_COMMON, "bits") for p, o in gm.BIT_CASES] + runs
for pencil, opts, common, kind in runs:
    A, B = gm.make_pencil(ref, pencil)
    res = gm.gesolve(ref, A, B, opts + common)
    assert res["err"] == 0, (pencil, opts, res["err"])
    key = gm.key(kind, pencil, opts, threads)
    rval = res["rval"]
    out[key] = {"status": int(res["status"]), "ss": res["ss"], "n": int(A.contents.n), "rval": rval, "evalue0_hex": float(res["evalue0"]).hex(),
                "evalue_hex": [float(v).hex() for v in res["evalue"]]}
    if not rval:
        out[key].update(iter=[int(v) for v in res["iter"]], resid_hex=[float(v).hex() for v in res["resid"]])
        if kind == "bits":
            arrays[key + "|rhistory"] = res["rhistory"]
            arrays[key + "|x"] = res["x"]
            for i, v in enumerate(res["evector"]):
                arrays[key + "|evector%%d" %% i] = v
    if kind == "bits" and not rval:
        for k, v in lisdrv.matrix_arrays(A).items():
            if isinstance(v, np.ndarray): arrays[key + "|A|" + k] = v
            else: out[key].setdefault("A", {})[k] = int(v)
    print(key, out[key].get("iter"), [float(v) for v in res["evalue"]], file=sys.stderr, flush=True)
    gm.release(ref, res)
    ref.lis_matrix_destroy(A); ref.lis_matrix_destroy(B)
np.savez(sys.argv[2], **arrays)
json.dump(out, open(sys.argv[2] + ".json", "w"))
'''


def main():
    meta, arrays, every = {}, {}, {}
    for T in gm.THREADS_TREE:
        tmp = os.path.join(HERE, "_gesm_T%d.npz" % T)
        env = dict(os.environ, OMP_NUM_THREADS=str(T))
        txt = subprocess.run([sys.executable, "-c", WORKER % {"root": ROOT}, str(T), tmp], capture_output=True, text=True, env=env)
        sys.stderr.write(txt.stderr[-8000:])
        txt.check_returncode()
        got = json.load(open(tmp + ".json"))          # (not stdout: the reference prints there too)
        os.unlink(tmp + ".json")
        every.update(got)
        if T in gm.THREADS_BITS:
            meta.update({k: v for k, v in got.items() if k.startswith("bits|")})
            with np.load(tmp) as z:
                for k in z.files:
                    arrays[k] = z[k]
        os.unlink(tmp)
    tree = {}
    for pencil, opts, must in gm.TREE_CASES:
        case = "tree|%s|%s" % (pencil, opts)
        per_T = {"T%d" % T: {"iter": every[gm.key("tree", pencil, opts, T)]["iter"], "evalue_hex": every[gm.key("tree", pencil, opts, T)]["evalue_hex"]} for T in gm.THREADS_TREE}
        modes = [m for m in range(gm.subspace(opts)) if gm.admitted(per_T, m)]
        for m in range(gm.subspace(opts)):
            print(case, "mode", m, "admitted" if m in modes else "left out", [(per_T["T%d" % T]["iter"][m], float.fromhex(per_T["T%d" % T]["evalue_hex"][m])) for T in gm.THREADS_TREE],
                  file=sys.stderr)
        assert set(must) <= set(modes), (case, modes)
        tree[case] = {"admitted": modes, "per_T": per_T,
                      "iter": {str(m): [per_T["T%d" % T]["iter"][m] for T in gm.THREADS_TREE] for m in modes},
                      "evalue_T1_hex": {str(m): per_T["T1"]["evalue_hex"][m] for m in modes}}
    np.savez_compressed(os.path.join(HERE, "gesolve_multi_bits.npz"), **arrays)
    doc = {"_source": "Lis 2.1.11 (oracle/_ref, gcc -O3 -fopenmp, no FMA) through ctypes: lis_gesolve with -e gsi | gli | gai at OMP_NUM_THREADS = 1 and 8: per mode evalue / "
                      "resid / iter, status; the residual history, x, every eigenvector and A's arrays after the solve (f64 / i32, every bit) in gesolve_multi_bits.npz under "
                      "'bits|pencil|options|T<threads>|rhistory', '...|x', '...|evector<i>', '...|A|<array>'; tree: per case what the reference gave at T = 1, 2, 4, 8 (per_T), "
                      "the modes it carries at every T (admitted), their counts over T and their T = 1 eigenvalues",
           "bit_common_options": gm.BIT_COMMON.strip(), "tree_common_options": gm.TREE_COMMON.strip(), "solves": meta, "tree": tree}
    json.dump(doc, open(os.path.join(HERE, "gesolve_multi_bits.json"), "w"), indent=1, sort_keys=True)
    print(len(meta), "gesolves written;", {k: v["admitted"] for k, v in tree.items()})


if __name__ == "__main__":
    main()
