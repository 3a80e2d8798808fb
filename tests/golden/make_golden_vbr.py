"""Bit-level goldens of VBR storage from the reference (oracle/_ref = Lis compiled from the reference sources by oracle/Makefile), driven through the
Lis API at T = 1 and T = 8 OpenMP threads: the converted arrays in both directions with the source's arrays after its in-place sort, A x and A^T x, the
diagonal into a vector pre-filled with 7.0, scaled and shifted values, whole solves (count, status, the full residual history, x) on held VBR matrices
and with -storage vbr, and three eigensolves.

Matrices, partitions and option lines: tests/vbr_cases.py.  Everything that does not depend on the thread count is recorded at T = 1 and asserted to be
the same at T = 8; A^T x, the solves and the eigensolves are recorded at both.  Every recorded solve must converge at both, and the Jacobi solves on held
matrices use the uniform-block case.  A matrix converted with row[] / col[] given is never destroyed here: the reference frees those arrays twice.

    python tests/golden/make_golden_vbr.py      (needs oracle/_ref; rewrites vbr_bits.npz)
"""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

WORKER = r'''
import os, sys
import numpy as np
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
import vbr_cases as vc, vbr_drv as drv, esolve_drv, esolve_multi_drv, lisdrv, orc
T = int(sys.argv[1])
ref = lisdrv.open_lib(orc.REF_SO, threads=T)
out = {}
def put(key, a, dtype=None): out[key] = np.ascontiguousarray(a, dtype)
FIELDS = ("row", "col", "ptr", "bptr", "bindex", "value")
def vbr_of(m):
    csr, row, col = vc.source(m)
    A = lisdrv.make_csr(ref, *csr)
    err, B = drv.to_vbr(ref, A, row, col)
    assert err == 0, m
    return csr, A, B
for m in vc.FOUND + vc.GIVEN:
    csr, A, B = vbr_of(m)
    n = len(csr[0]) - 1
    x = vc.xvec(n)
    a = drv.arrays(B)
    put(m + "|sizes", [a["nr"], a["nc"], a["bnnz"], a["nnz"]], np.int64)
    if m in vc.ARRAYS_RECORDED:
        for f in FIELDS: put("%%s|vbr|%%s" %% (m, f), a[f])
        src = lisdrv.matrix_arrays(A)                   # (sorted in place where the conversion found the blocks: recorded where that moved something)
        if not (np.array_equal(src["index"], csr[1]) and src["value"].tobytes() == csr[2].tobytes()):
            put(m + "|source|index", src["index"]); put(m + "|source|value", src["value"])
        assert (m + "|source|index" in out) == (m in ("unsorted", "empty_rows")), m
        back = lisdrv.convert(ref, B, "csr")
        c = lisdrv.matrix_arrays(back)
        for f in ("ptr", "index", "value"): put("%%s|csr|%%s" %% (m, f), c[f])
        ref.lis_matrix_destroy(back)
    y, yt = lisdrv.matvec(ref, B, x), lisdrv.matvech(ref, B, x)
    put(m + "|y", y); put("%%s|yt|T%%d" %% (m, T), yt)
    assert drv.raw_product(ref, B, "vbr", x)[:n].tobytes() == y.tobytes() and drv.raw_product(ref, B, "vbr", x, transposed=True).tobytes() == yt.tobytes()
    err, d = drv.diagonal(ref, B, np.full(n, 7.0))
    assert err == 0
    put(m + "|diag", d)
    if m in vc.ARRAYS_RECORDED:
        assert ref.lis_matrix_shift_diagonal(B, vc.SHIFT) == 0
        put(m + "|shift|value", drv.arrays(B)["value"])
    if m in vc.SCALED:
        for action, tag in ((1, "jacobi"), (2, "symm_diag")):
            err, C2 = drv.to_vbr(ref, A, *vc.source(m)[1:])
            assert err == 0
            err, b, d = drv.scale(ref, C2, np.ones(n), action, np.full(n, vc.D_BEFORE))
            assert err == 0
            put("%%s|scale_%%s|value" %% (m, tag), drv.arrays(C2)["value"])
            put("%%s|scale_%%s|b" %% (m, tag), b); put("%%s|scale_%%s|d" %% (m, tag), d)
for m, held, opts in vc.SOLVES:
    csr, A, B = vbr_of(m)                               # (-storage converts the caller's matrix for good: a fresh one per solve)
    res = lisdrv.solve(ref, B if held else A, vc.rhs(csr), opts + " " + vc.COMMON)
    key = "%%s|T%%d" %% (vc.solve_key(m, held, opts), T)
    assert res["err"] == 0 and res["status"] == 0 and res["iter"] < 1000, (key, res["err"], res["status"], res["iter"])
    assert (B if held else A).contents.matrix_type == drv.VBR, key
    assert not (held and "jacobi" in opts) or m == vc.JACOBI_HELD, key
    put(key + "|meta", [res["iter"], res["status"]], np.int64)
    put(key + "|rhistory", res["rhistory"]); put(key + "|x", res["x"])
    print(key, res["iter"], res["status"], res["resid"], file=sys.stderr, flush=True)
for held, opts in vc.ESOLVES:
    csr, A, B = vbr_of("sym7b")
    M = B if held else A
    key = "esolve|%%s|%%s|T%%d" %% ("held" if held else "csr", opts, T)
    if "-ss" in opts:
        res = esolve_multi_drv.esolve(ref, M, opts + " " + vc.ECOMMON)
        assert res["err"] == 0 and res["status"] == 0, (key, res["err"], res["status"])
        put(key + "|meta", list(res["iter"]) + [res["status"]], np.int64)
        put(key + "|evalue", np.concatenate([res["evalue"], res["resid"]]))
        put(key + "|rhistory", res["rhistory"]); put(key + "|x", np.concatenate(res["evector"]))
        print(key, res["iter"], res["status"], res["evalue"], file=sys.stderr, flush=True)
        esolve_multi_drv.release(ref, res)
    else:
        res = esolve_drv.esolve(ref, M, opts + " " + vc.ECOMMON)
        assert res["err"] == 0 and res["status"] == 0 and res["iter"] < 500, (key, res)
        put(key + "|meta", [res["iter"], res["status"]], np.int64)
        put(key + "|evalue", [res["evalue"], res["resid"]])
        put(key + "|rhistory", res["rhistory"]); put(key + "|x", res["x"])
        print(key, res["iter"], res["status"], res["evalue"], file=sys.stderr, flush=True)
    assert M.contents.matrix_type == drv.VBR, key
np.savez(sys.argv[2], **out)
'''


def main():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import vbr_cases as vc
    got = {}
    for T in vc.THREADS:
        tmp = os.path.join(HERE, "_vbr_T%d.npz" % T)
        txt = subprocess.run([sys.executable, "-c", WORKER % {"root": ROOT}, str(T), tmp], capture_output=True, text=True,
                             env=dict(os.environ, OMP_NUM_THREADS=str(T)))
        sys.stderr.write(txt.stderr[-8000:])
        txt.check_returncode()
        with np.load(tmp) as z:
            got[T] = {k: z[k] for k in z.files}
        os.unlink(tmp)
    first, arrays = vc.THREADS[0], {}
    for T in vc.THREADS:
        for k, v in got[T].items():
            if "|T%d" % T in k:
                arrays[k] = v
            elif T == first:
                arrays[k] = v
            else:                    # thread-independent: the same bits at every T
                assert v.dtype == got[first][k].dtype and v.tobytes() == got[first][k].tobytes(), ("differs between thread counts", k)
    path = os.path.join(HERE, vc.FIXTURE)
    np.savez_compressed(path, **arrays)
    print(len(arrays), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
