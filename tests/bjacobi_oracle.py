"""The block Jacobi preconditioner stated on its own, in plain Python loops with one rounded operation per step: the inverse of a
bn x bn block, the padding of the last block when bn does not divide n, and the block-diagonal product in its plain and its
transposed form.  It knows nothing of the kernels; tests/test_bjacobi_cpu.py holds it to the reference library in every bit,
tests/test_bjacobi_gpu.py holds the kernels and the library to it.

Layout: nr = ceil(n / bn) blocks, block b at d[b*bn*bn ..], entry (i, j) of a block at i + j*bn.

Every statement below is one IEEE operation, rounded once, applied to the same entry of all blocks at a time: an array here is "entry e of
every block", and numpy's elementwise + - * / on float64 round each element on its own (no fused multiply-add; a zero divisor gives the
infinity or the NaN IEEE prescribes)."""
import numpy as np


def pad_last_block(a, n, bn):
    """1.0 on the diagonal of the rows the last block has beyond n; a[e] holds entry e of every block"""
    k = n % bn
    if bn > 1 and k != 0:
        for i in range(bn - 1, k - 1, -1):
            a[i * (bn + 1)][-1] = 1.0


def invert_blocks(a, n):
    """the inverse of every n x n block (a[e]: entry e, column-major, of all blocks), in place: LU without pivoting on a copy, the reciprocal of
    each pivot kept on the diagonal, then per column a forward and a backward substitution that read and overwrite a itself"""
    lu = [v.copy() for v in a]
    for k in range(n):
        lu[k + k * n] = 1.0 / lu[k + k * n]
        for i in range(k + 1, n):
            t = lu[i + k * n] * lu[k + k * n]
            for j in range(k + 1, n):
                p = t * lu[k + j * n]
                lu[i + j * n] = lu[i + j * n] - p
            lu[i + k * n] = t
    for k in range(n):
        for i in range(n):
            t = np.full_like(a[0], 1.0 if i == k else 0.0)
            for j in range(i):
                p = lu[i + j * n] * a[j + k * n]
                t = t - p
            a[i + k * n] = t
        for i in range(n - 1, -1, -1):
            t = a[i + k * n]
            for j in range(i + 1, n):
                p = lu[i + j * n] * a[j + k * n]
                t = t - p
            a[k * n + i] = t * lu[i + i * n]


def inverse(d, n, bn):
    """WD: the blocks of d (nr*bn*bn values), the last one padded, each inverted"""
    nr = (n + bn - 1) // bn
    d = np.array(d, np.float64)
    assert d.shape == (nr * bn * bn,)
    with np.errstate(all="ignore"):
        if bn == 1:
            return 1.0 / d
        a = [d[e::bn * bn].copy() for e in range(bn * bn)]
        pad_last_block(a, n, bn)
        invert_blocks(a, bn)
    return np.stack(a, axis=1).reshape(-1)


def _apply(d, x, n, bn, transposed):
    nr = (n + bn - 1) // bn
    d = np.asarray(d, np.float64)
    xp = np.zeros(nr * bn)                           # +0.0 from n on
    xp[:n] = x
    from_zero = bn >= (4 if transposed else 5)       # the reference writes small blocks as one expression, larger ones as a loop from t = 0.0
    y = np.zeros((nr, bn))
    with np.errstate(all="ignore"):
        for i in range(bn):
            t = np.zeros(nr)
            for j in range(bn):
                p = d[(i * bn + j if transposed else i + j * bn)::bn * bn] * xp[j::bn]
                t = p if (j == 0 and not from_zero) else t + p
            y[:, i] = t
    return y.reshape(-1)[:n].copy()


def matvec(d, x, n, bn):
    """y = D x"""
    return _apply(d, x, n, bn, False)


def matvech(d, x, n, bn):
    """y = D^T x, block by block"""
    return _apply(d, x, n, bn, True)
