"""The block ILU(k) preconditioner behind -p ilu on BSR storage, stated on its own for tests: pattern, factor and M^-1 b at T row
blocks, in the reference's operation order (lis_precon_iluk.c:1289-1468, :1714-1819, :2006-2037; lis_array_matmat / _matvec / _ge).

A BSR matrix here is (bptr, bindex, value, bn, n): nr = ceil(n / bn) block rows, block k at value[k*bn*bn ..], column-major (entry
(r, c) at r + c*bn), the last block row and column zero where they reach beyond n.  Plain Python loops over Python floats: every
product and every sum is one IEEE operation rounded on its own, in the order written.  No level schedule, no search, no gather.

Pattern: ilu_oracle.symbolic on the block graph (nr, bptr, bindex) -- the reference's block routine is its point routine with block
rows for rows; T blocks of LIS_GET_ISIE over the nr BLOCK rows.
Factor of block row i: L, D, U zero, A's kept blocks copied in (of a block column stored twice the later place takes the later
block), then per pivot j of L(i) ascending  L_ij = L_ij Dinv_j  and  target -= L_ij U_jc  for the blocks of U(j) the row keeps, then
1.0 on the diagonal of the padding (last block row, bn does not divide n), then D_i inverted (bjacobi_oracle.invert_blocks, the
statement of lis_array_ge).  An entry of a product: a[r]*b[0] + a[r+bn]*b[1] (+ a[r+2bn]*b[2]), left to right from the first product.
psolve: x = b; forward x_i -= L_ij x_j term by term; backward the same with U, then x_i = Dinv_i x_i.  x reads as +0.0 from n on and
is never written there."""
import numpy as np

import bjacobi_oracle
import ilu_oracle

row_blocks = ilu_oracle.row_blocks


def symbolic(bptr, bindex, fill, T=1):
    """(Lcols, Ucols): per block row the kept block columns in term order"""
    return ilu_oracle.symbolic(bptr, bindex, fill, T)


def _matmat(a, b, bn):
    out = [0.0] * (bn * bn)
    for j in range(bn):
        for r in range(bn):
            s = a[r] * b[j * bn]
            for l in range(1, bn):
                p = a[r + l * bn] * b[l + j * bn]
                s = s + p
            out[r + j * bn] = s
    return out


def _matvec(a, x, bn):
    out = [0.0] * bn
    for r in range(bn):
        s = a[r] * x[0]
        for l in range(1, bn):
            p = a[r + l * bn] * x[l]
            s = s + p
        out[r] = s
    return out


def _invert(blk, bn):
    a = [np.array([v], np.float64) for v in blk]
    with np.errstate(all="ignore"):
        bjacobi_oracle.invert_blocks(a, bn)
    return [float(v[0]) for v in a]


def factor(bptr, bindex, value, bn, n, fill, T=1):
    """{"L": (ptr, idx, val), "U": (ptr, idx, val), "D": inverted diagonal blocks}; val holds bn*bn doubles per block"""
    nr = len(bptr) - 1
    bs = bn * bn
    assert nr == (n + bn - 1) // bn
    Lc, Uc = symbolic(bptr, bindex, fill, T)
    bptr, bindex = np.asarray(bptr).tolist(), np.asarray(bindex).tolist()
    value = np.asarray(value, np.float64).tolist()
    Lv, Uv, D = [None] * nr, [None] * nr, [None] * nr
    for lo, hi in row_blocks(nr, T):
        for i in range(lo, hi):
            lv, uv, d = [[0.0] * bs for _ in Lc[i]], [[0.0] * bs for _ in Uc[i]], [0.0] * bs
            place = {}                          # block column -> position in its part; of a column held twice, the later one
            for j, c in enumerate(Lc[i]):
                place[c] = j
            for j, c in enumerate(Uc[i]):
                place[c] = j
            for k in range(bptr[i], bptr[i + 1]):
                c = bindex[k]
                if c < lo or c >= hi:
                    continue
                blk = value[k * bs:(k + 1) * bs]
                if c < i:
                    lv[place[c]] = list(blk)
                elif c == i:
                    d = list(blk)
                else:
                    uv[place[c]] = list(blk)
            for j, piv in enumerate(Lc[i]):
                l = _matmat(lv[j], D[piv], bn)
                lv[j] = l
                for c, u in zip(Uc[piv], Uv[piv]):
                    if c != i and c not in place:
                        continue
                    t = _matmat(l, u, bn)
                    target = d if c == i else lv[place[c]] if c < i else uv[place[c]]
                    for e in range(bs):
                        target[e] = target[e] - t[e]
            if i == nr - 1 and n % bn != 0:
                for r in range(n % bn, bn):
                    d[r * (bn + 1)] = 1.0
            Lv[i], Uv[i], D[i] = lv, uv, _invert(d, bn)

    def rows(cols, vals):
        p = np.zeros(nr + 1, np.int32)
        for i in range(nr):
            p[i + 1] = p[i] + len(cols[i])
        return (p, np.array([c for r in cols for c in r], np.int32), np.array([v for r in vals for blk in r for v in blk], np.float64))
    return {"L": rows(Lc, Lv), "U": rows(Uc, Uv), "D": np.array([v for blk in D for v in blk], np.float64), "bn": bn, "n": n}


def _block_rows(part, bs):
    p, c, v = part
    p, c, v = p.tolist(), c.tolist(), v.tolist()
    return [[(c[k], v[k * bs:(k + 1) * bs]) for k in range(p[i], p[i + 1])] for i in range(len(p) - 1)]


def psolve(f, b, T=1):
    """x = M^-1 b"""
    bn, n = f["bn"], f["n"]
    bs = bn * bn
    L, U, D = _block_rows(f["L"], bs), _block_rows(f["U"], bs), f["D"].tolist()
    nr = len(L)
    x = np.asarray(b, np.float64).tolist() + [0.0] * (nr * bn - n)          # +0.0 from n on, never written

    def terms(i, rows):
        xi = x[i * bn:(i + 1) * bn]
        for c, a in rows[i]:
            s = _matvec(a, x[c * bn:(c + 1) * bn], bn)
            for r in range(bn):
                xi[r] = xi[r] - s[r]
        for r in range(bn):
            if i * bn + r >= n:
                xi[r] = 0.0
        return xi

    for lo, hi in row_blocks(nr, T):
        for i in range(lo, hi):
            x[i * bn:(i + 1) * bn] = terms(i, L)
        for i in range(hi - 1, lo - 1, -1):
            w = _matvec(D[i * bs:(i + 1) * bs], terms(i, U), bn)
            for r in range(bn):
                if i * bn + r < n:
                    x[i * bn + r] = w[r]
    return np.array(x[:n], np.float64)


def csr_to_bsr(ptr, idx, val, bn):
    """(bptr, bindex, value) of a bn x bn BSR form of a CSR matrix: the blocks of a block row ascending, zero where nothing is stored.
    A test's own way to make blocks (of an entry stored twice the later one stays); matrices with a block column stored twice are
    built block by block instead (bilu_cases.twice)"""
    n = len(ptr) - 1
    nr = (n + bn - 1) // bn
    bs = bn * bn
    bptr, bindex, value = [0], [], []
    for bi in range(nr):
        cols = sorted({int(idx[k]) // bn for i in range(bi * bn, min(n, (bi + 1) * bn)) for k in range(ptr[i], ptr[i + 1])})
        at = {c: len(bindex) + j for j, c in enumerate(cols)}
        bindex += cols
        value += [0.0] * (bs * len(cols))
        for i in range(bi * bn, min(n, (bi + 1) * bn)):
            for k in range(ptr[i], ptr[i + 1]):
                c = int(idx[k])
                value[at[c // bn] * bs + (i % bn) + (c % bn) * bn] = float(val[k])
        bptr.append(len(bindex))
    return np.array(bptr, np.int32), np.array(bindex, np.int32), np.array(value, np.float64)


def submatrix(bptr, bindex, value, bn, lo, hi):
    """the diagonal sub-matrix of block rows and columns [lo, hi), in stored order"""
    bs = bn * bn
    p, c, v = [0], [], []
    for i in range(lo, hi):
        for k in range(bptr[i], bptr[i + 1]):
            if lo <= bindex[k] < hi:
                c.append(int(bindex[k]) - lo)
                v += np.asarray(value[k * bs:(k + 1) * bs]).tolist()
        p.append(len(c))
    return np.array(p, np.int32), np.array(c, np.int32), np.array(v, np.float64)
