"""Block SSOR on BSR storage stated on its own: WD and the six triangular solves (lis_matrix_solve / lis_matrix_solveh with LOWER, UPPER,
SSOR) as plain Python loops over block rows, one ordered chain of rounded double operations per scalar row.  No schedule, no levels: the
plain solves walk the block rows in order, the transposed solves are scatters.  tests/test_bssor_cpu.py holds this file to the reference
library in every bit, tests/test_bssor_schedule_gpu.py and tests/test_bssor_gpu.py hold the kernels and the library to it.

Layout: nr = ceil(n / bn) block rows; a block is bn*bn doubles, column-major, entry (r, c) at r + c*bn.  A part (L or U) is a list with one
list per block row of (block column, block) in stored order.

Rules (every product rounded alone, every add or subtract rounded alone):
  plain       t = b_i (SSOR's backward half: +0.0); per term in stored order, c ascending: t[r] = t[r] -/+ a(r,c) * x_j[c];
              x_i = WD_i t, or x_i = x_i - WD_i t
  transposed  x = b; per source block row i in sweep order: t = WD_i^T x_i; x_i = t unless the sweep is the first of SSOR-h;
              per term of row i with target jj: x_jj[c] = x_jj[c] - (sum over r of a(r,c) * t[r])
  sums        (WD t)[r] over c, (WD^T x)[c] over r and the grouped sums over r run left to right; they start with their first product
              for bn <= 3 and at +0.0 for bn >= 4
  padding     b, x and t read as +0.0 at and beyond n (the last block when bn does not divide n); x is never written there
A numpy array below is "the bn scalar rows of one block at once": elementwise + - * on float64 round each element on its own."""
import numpy as np

import bjacobi_oracle

LOWER, UPPER, SSOR = 0, 1, 2          # LIS_MATRIX_LOWER, LIS_MATRIX_UPPER, LIS_MATRIX_SSOR
SOLVES = [(name, flag) for name in ("solve", "solveh") for flag in (LOWER, UPPER, SSOR)]


def split(bptr, bindex, value, bn):
    """(L, U, D): block columns before / after the diagonal in stored order, D the nr diagonal blocks (zero where a row stores none;
    of a diagonal block stored twice the later one, as lis_matrix_split_bsr copies them in turn)"""
    nr, bs = len(bptr) - 1, bn * bn
    value = np.asarray(value, np.float64)
    L, U, D = [[] for _ in range(nr)], [[] for _ in range(nr)], np.zeros(nr * bs)
    for i in range(nr):
        for k in range(int(bptr[i]), int(bptr[i + 1])):
            c, blk = int(bindex[k]), value[k * bs:(k + 1) * bs].copy()
            if c < i:
                L[i].append((c, blk))
            elif c > i:
                U[i].append((c, blk))
            else:
                D[i * bs:(i + 1) * bs] = blk
    return L, U, D


def make_wd(D, n, bn, omega):
    """every entry of D times omega (alpha * d), 1.0 on the diagonal of the last block's padding, every block inverted"""
    with np.errstate(all="ignore"):
        return bjacobi_oracle.inverse(np.float64(omega) * np.asarray(D, np.float64), n, bn)


def _cols(blk, bn):
    """M[r, c] = entry (r, c) of the block"""
    return blk.reshape(bn, bn).T


def _sum_over(M, v, bn):
    """out[e] = sum over q of M[e, q] * v[q], left to right; from the first product for bn <= 3, from +0.0 for bn >= 4"""
    acc = None if bn <= 3 else np.zeros(bn)
    for q in range(bn):
        p = M[:, q] * v[q]
        acc = p if acc is None else acc + p
    return acc


class _Vec:
    """n doubles seen in blocks of bn: reads give +0.0 at and beyond n, writes leave those alone"""
    def __init__(self, values, n, bn):
        nr = (n + bn - 1) // bn
        self.n, self.bn = n, bn
        self.v = np.zeros(nr * bn)
        self.v[:n] = values

    def get(self, i):
        return self.v[i * self.bn:(i + 1) * self.bn].copy()

    def put(self, i, t):
        lo = i * self.bn
        cnt = min(self.bn, self.n - lo)
        self.v[lo:lo + cnt] = t[:cnt]

    def out(self):
        return self.v[:self.n].copy()


def sweep_plain(part, order, wd, n, bn, b, x, sub):
    """one plain sweep over the block rows in `order`: x_i = WD_i (b_i - sum) or, sub, x_i = x_i - WD_i (+0.0 + sum); x: a _Vec, updated"""
    bs = bn * bn
    for i in order:
        t = np.zeros(bn) if sub else b.get(i)
        for j, blk in part[i]:
            A, xj = _cols(blk, bn), x.get(j)
            for c in range(bn):
                p = A[:, c] * xj[c]
                t = t + p if sub else t - p
        w = _sum_over(_cols(wd[i * bs:(i + 1) * bs], bn), t, bn)
        x.put(i, x.get(i) - w if sub else w)


def sweep_scatter(part, order, wd, n, bn, x, store, work=None):
    """one transposed sweep as the scatter it is: per source block row i in `order`, t = WD_i^T x_i (the padding of t +0.0), stored into
    x_i when `store`, then subtracted through every term of row i from its target.  work: a _Vec that receives every t"""
    bs = bn * bn
    for i in order:
        t = _sum_over(_cols(wd[i * bs:(i + 1) * bs], bn).T, x.get(i), bn)
        t[max(0, min(bn, n - i * bn)):] = 0.0
        if store:
            x.put(i, t)
        if work is not None:
            work.put(i, t)
        for jj, blk in part[i]:
            s = _sum_over(_cols(blk, bn).T, t, bn)
            x.put(jj, x.get(jj) - s)


def solve(L, U, wd, n, bn, b, flag):
    """lis_matrix_solve(A, B, X, flag)"""
    nr = (n + bn - 1) // bn
    up, down = range(nr), range(nr - 1, -1, -1)
    bv, x = _Vec(b, n, bn), _Vec(np.zeros(n), n, bn)
    with np.errstate(all="ignore"):
        if flag == UPPER:
            sweep_plain(U, down, wd, n, bn, bv, x, False)
        else:
            sweep_plain(L, up, wd, n, bn, bv, x, False)
            if flag == SSOR:
                sweep_plain(U, down, wd, n, bn, None, x, True)
    return x.out()


def solveh(L, U, wd, n, bn, b, flag):
    """lis_matrix_solveh(A, B, X, flag): X = B first, then the scatters in place"""
    nr = (n + bn - 1) // bn
    up, down = range(nr), range(nr - 1, -1, -1)
    x = _Vec(b, n, bn)
    with np.errstate(all="ignore"):
        if flag == LOWER:
            sweep_scatter(U, up, wd, n, bn, x, True)
        elif flag == UPPER:
            sweep_scatter(L, down, wd, n, bn, x, True)
        else:
            sweep_scatter(U, up, wd, n, bn, x, False)
            sweep_scatter(L, down, wd, n, bn, x, True)
    return x.out()


def all_solves(bptr, bindex, value, bn, n, omega, b):
    """{"wd": WD, ("solve" | "solveh", flag): x} of a BSR matrix"""
    L, U, D = split(bptr, bindex, value, bn)
    wd = make_wd(D, n, bn, omega)
    out = {"wd": wd}
    for name, flag in SOLVES:
        out[name, flag] = (solve if name == "solve" else solveh)(L, U, wd, n, bn, b, flag)
    return out


def substitution_residual(L, U, D, omega, n, bn, b, x, name, flag):
    """For LOWER / UPPER: (r, bound) per scalar row in numpy.longdouble, r = |b - M x| with M the block triangular matrix the solve
    inverts: its strict part (L or U; transposed for solveh) plus the diagonal blocks fl(omega D) (transposed for solveh).

    The bound is that of tests/ssor_oracle.substitution_residual: gamma_k (|M| |x|)_i with k = scalar terms of the row + 2, the scalar terms
    being the bn entries of every block term's row and the bn of the diagonal block's.  (The diagonal block is not divided by but multiplied
    with its computed inverse WD, which in general adds a term of the size gamma_4bn (|wD| |WD| |wD x|)_i; it is NOT part of the bound: the
    well-conditioned diagonal blocks of the cases held to this bound stay within the plain one.)"""
    ld = np.longdouble
    nr, bs = (n + bn - 1) // bn, bn * bn
    part = (L if flag == LOWER else U) if name == "solve" else (U if flag == LOWER else L)
    rows = [[] for _ in range(nr)]
    for i in range(nr):
        for c, blk in part[i]:
            if name == "solve":
                rows[i].append((c, _cols(blk, bn)))
            else:
                rows[c].append((i, _cols(blk, bn).T))
    xp, bp = np.zeros(nr * bn, ld), np.zeros(nr * bn, ld)
    xp[:n], bp[:n] = x, b
    u = ld(2.0) ** -53
    gamma = lambda k: k * u / (1 - k * u)
    r, bound = np.zeros(nr * bn, ld), np.zeros(nr * bn, ld)
    for i in range(nr):
        M = _cols(np.float64(omega) * np.asarray(D[i * bs:(i + 1) * bs], np.float64), bn).astype(ld)
        if name == "solveh":
            M = M.T
        for q in range(n % bn if (i == nr - 1 and n % bn) else bn, bn):
            M[q, q] = 1.0                                     # the padding's diagonal
        xi = xp[i * bn:(i + 1) * bn]
        s = bp[i * bn:(i + 1) * bn] - M @ xi
        a = np.abs(M) @ np.abs(xi)
        for c, A in rows[i]:
            s = s - A.astype(ld) @ xp[c * bn:(c + 1) * bn]
            a = a + np.abs(A.astype(ld)) @ np.abs(xp[c * bn:(c + 1) * bn])
        k = bn * len(rows[i]) + bn + 2
        r[i * bn:(i + 1) * bn] = np.abs(s)
        bound[i * bn:(i + 1) * bn] = gamma(k) * a
    return r[:n], bound[:n]
