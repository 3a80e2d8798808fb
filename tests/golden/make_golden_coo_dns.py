"""Bit-level goldens of COO and DNS storage from the reference (oracle/_ref = Lis compiled from the reference sources by oracle/Makefile), driven
through the Lis API at T = 1 and T = 8 OpenMP threads: converted arrays, diagonals, scaled and shifted values, A x and A^T x, the COO -> CSR
conversion with the source's arrays as its in-place sort leaves them, whole solves (count, status, the full residual history, x) and two eigensolves.

Matrices, triplet lists and option lines: tests/coo_dns_cases.py.  Everything that does not depend on the thread count is recorded at T = 1 and
asserted to be the same at T = 8; A^T x of DNS storage, the solves and the eigensolves are recorded at both.  Every recorded solve must converge.

    python tests/golden/make_golden_coo_dns.py      (needs oracle/_ref; rewrites coo_dns_bits.npz)
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
import coo_dns_cases as cc, coo_dns_drv as drv, esolve_drv, lisdrv, orc
T = int(sys.argv[1])
ref = lisdrv.open_lib(orc.REF_SO, threads=T)
out = {}
def put(key, a, dtype=None): out[key] = np.ascontiguousarray(a, dtype)
for m in cc.MATRICES:
    ptr, idx, val = cc.matrix(m)
    n = len(ptr) - 1
    x = cc.xvec(n)
    A = lisdrv.make_csr(ref, ptr, idx, val)
    for fmt in ("coo", "dns"):
        B = lisdrv.convert(ref, A, fmt)
        a = drv.arrays(B)
        put("%%s|%%s|nnz" %% (m, fmt), [a["nnz"]], np.int64)
        for f in ("row", "col", "value"):
            if f in a: put("%%s|%%s|%%s" %% (m, fmt, f), a[f])
        y, yt = lisdrv.matvec(ref, B, x), lisdrv.matvech(ref, B, x)
        put("%%s|%%s|y" %% (m, fmt), y)
        put("%%s|%%s|yt|T%%d" %% (m, fmt, T), yt)
        # the raw entry points lis_matvec_<fmt> / lis_matvech_<fmt> give the same bits: stored once
        assert drv.raw_product(ref, B, fmt, x)[:n].tobytes() == y.tobytes() and drv.raw_product(ref, B, fmt, x, transposed=True).tobytes() == yt.tobytes()
        err, d = drv.diagonal(ref, B, np.full(n, 7.0))
        assert err == 0
        put("%%s|%%s|diag" %% (m, fmt), d)
        if (m, fmt) != ("rand301", "coo"):            # (that one is the triplet list "csr2coo" below)
            back = lisdrv.convert(ref, B, "csr")      # (COO: sorts B's arrays in place)
            c = lisdrv.matrix_arrays(back)
            for f in ("ptr", "index", "value"): put("%%s|%%s|csr|%%s" %% (m, fmt, f), c[f])
            ref.lis_matrix_destroy(back)
        ref.lis_matrix_destroy(B)
        if m not in cc.UNSCALED:                     # (a zero diagonal scales by infinity; rand301 only makes the fixture large)
            for action, tag in ((1, "jacobi"), (2, "symm_diag")):
                B = lisdrv.convert(ref, A, fmt)
                err, b, d = drv.scale(ref, B, np.ones(n), action)
                assert err == 0
                put("%%s|%%s|scale_%%s|value" %% (m, fmt, tag), drv.arrays(B)["value"])
                put("%%s|%%s|scale_%%s|b" %% (m, fmt, tag), b)
                put("%%s|%%s|scale_%%s|d" %% (m, fmt, tag), d)
                ref.lis_matrix_destroy(B)
        if m != "rand301":
            B = lisdrv.convert(ref, A, fmt)
            assert ref.lis_matrix_shift_diagonal(B, cc.SHIFT) == 0
            put("%%s|%%s|shift|value" %% (m, fmt), drv.arrays(B)["value"])
            ref.lis_matrix_destroy(B)
    ref.lis_matrix_destroy(A)
for t in cc.TRIPLETS:
    n, row, col, val = cc.triplets(t)
    x = cc.xvec(n)
    A = drv.make_coo(ref, n, row, col, val)
    put("%%s|y_before" %% t, lisdrv.matvec(ref, A, x))
    B = lisdrv.convert(ref, A, "csr")
    c = lisdrv.matrix_arrays(B)
    a = drv.arrays(A)
    assert np.array_equal(c["index"], a["col"]) and c["value"].tobytes() == a["value"].tobytes()      # the CSR arrays ARE the sorted source's: stored once
    put("%%s|csr|ptr" %% t, c["ptr"])
    for f in ("row", "col", "value"): put("%%s|after|%%s" %% (t, f), a[f])
    put("%%s|y_after" %% t, lisdrv.matvec(ref, A, x))
    ref.lis_matrix_destroy(B); ref.lis_matrix_destroy(A)
ptr, idx, val = cc.matrix("stencil")
b = cc.rhs(ptr, idx, val)
for opts in cc.SOLVES:
    A = lisdrv.make_csr(ref, ptr, idx, val)         # (-storage converts the caller's matrix for good: a fresh one per solve)
    res = lisdrv.solve(ref, A, b, opts + " " + cc.COMMON)
    key = "solve|%%s|T%%d" %% (opts, T)
    assert res["err"] == 0 and res["status"] == 0 and res["iter"] < 1000, (key, res["err"], res["status"], res["iter"])
    assert A.contents.matrix_type == lisdrv.capi.FORMAT_ID[opts.split()[-1]], key
    put(key + "|meta", [res["iter"], res["status"]], np.int64)
    put(key + "|rhistory", res["rhistory"]); put(key + "|x", res["x"])
    print(key, res["iter"], res["status"], res["resid"], file=sys.stderr, flush=True)
    ref.lis_matrix_destroy(A)
for opts in cc.ESOLVES:
    A = esolve_drv.make_matrix(ref, "sym7")
    res = esolve_drv.esolve(ref, A, opts + " " + cc.ECOMMON)
    key = "esolve|%%s|T%%d" %% (opts, T)
    assert res["err"] == 0 and res["status"] == 0 and res["iter"] < 500, (key, res)
    put(key + "|meta", [res["iter"], res["status"]], np.int64)
    put(key + "|evalue", [res["evalue"], res["resid"]])
    put(key + "|rhistory", res["rhistory"]); put(key + "|x", res["x"])
    print(key, res["iter"], res["status"], res["evalue"], file=sys.stderr, flush=True)
    ref.lis_matrix_destroy(A)
np.savez(sys.argv[2], **out)
'''


def main():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import coo_dns_cases as cc
    got = {}
    for T in cc.THREADS:
        tmp = os.path.join(HERE, "_coo_dns_T%d.npz" % T)
        txt = subprocess.run([sys.executable, "-c", WORKER % {"root": ROOT}, str(T), tmp], capture_output=True, text=True,
                             env=dict(os.environ, OMP_NUM_THREADS=str(T)))
        sys.stderr.write(txt.stderr[-6000:])
        txt.check_returncode()
        with np.load(tmp) as z:
            got[T] = {k: z[k] for k in z.files}
        os.unlink(tmp)
    first, arrays = cc.THREADS[0], {}
    for T in cc.THREADS:
        for k, v in got[T].items():
            if "|T%d" % T in k:
                arrays[k] = v
            elif T == first:
                arrays[k] = v
            else:                    # thread-independent: the same bits at every T
                assert v.dtype == got[first][k].dtype and v.tobytes() == got[first][k].tobytes(), ("differs between thread counts", k)
    path = os.path.join(HERE, cc.FIXTURE)
    np.savez_compressed(path, **arrays)
    print(len(arrays), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
