"""A numpy model of lis_matrix_shift_matrix(A, B, sigma): A <- A - sigma B on two CSR matrices.

What the reference leaves in A (src/matrix/lis_matrix_ops.c:833-856: csr -> dns, lis_matrix_axpy_dns(-sigma, B, A), dns -> csr), row by row:
the union of the two rows' columns in ascending order; every entry (-sigma) * b + a with an absent term counting as 0.0, the product rounded, then the
sum rounded (Python floats: IEEE doubles, no fused multiply-add); an entry that comes out exactly 0.0 is dropped.  tests/test_gesolve_cpu.py holds this
model to the goldens (and to oracle/_ref where it exists) in every bit; tests/test_shift_matrix_gpu.py holds kernels/spgeam.hip to the model."""
import numpy as np


def shift_matrix(aptr, aidx, aval, bptr, bidx, bval, sigma):
    n = len(aptr) - 1
    assert len(bptr) - 1 == n
    ms = -float(sigma)
    ptr, idx, val = np.zeros(n + 1, np.int32), [], []
    for r in range(n):
        a, b = {}, {}
        for k in range(aptr[r], aptr[r + 1]):
            a.setdefault(int(aidx[k]), float(aval[k]))
        for k in range(bptr[r], bptr[r + 1]):
            b.setdefault(int(bidx[k]), float(bval[k]))
        for c in sorted(set(a) | set(b)):
            t = ms * b.get(c, 0.0)
            v = t + a.get(c, 0.0)
            if v != 0.0:
                idx.append(c)
                val.append(v)
        ptr[r + 1] = len(idx)
    return ptr, np.array(idx, np.int32), np.array(val, np.float64)


def in_place(aptr, aidx, result):
    """The shift keeps A's layout -- the rows already ascending, nothing added, nothing dropped -- exactly when the result's ptr and index ARE A's."""
    return bool(np.array_equal(aptr, result[0]) and np.array_equal(aidx, result[1]))


def apply(A, B, sigmas):
    """The matrix after every shift of the sequence, and whether that shift could be made in place: [(ptr, idx, val, in_place)]."""
    out, cur = [], A
    for s in sigmas:
        res = shift_matrix(*cur, *B, s)
        out.append(res + (in_place(cur[0], cur[1], res),))
        cur = res
    return out
