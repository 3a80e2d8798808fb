"""An independent statement of the triangular solves behind -p ssor, for tests.

lis_matrix_solve / lis_matrix_solveh of a split CSR matrix with flags LOWER, UPPER and SSOR, and WD = 1 / (omega D), written from
the behaviour lis_ssor.c's header describes.  Every row is one ordered chain of individually rounded double operations: plain
Python loops over Python floats (IEEE doubles; CPython never contracts a multiply and an add), the transposed solves as the
scatter they are.  There is no level schedule here and nothing is vectorised over terms: it shares no structure with the code it
checks.  SSOR takes T row blocks cut as LIS_GET_ISIE cuts them (the first n % T blocks hold n / T + 1 rows); a block sweeps its own
rows and skips the terms that reach out of it.  LOWER / UPPER are sequential at any T.
"""
import numpy as np

LOWER, UPPER, SSOR = 0, 1, 2


def split(ptr, idx, val):
    """L (columns before the row), U (columns after it), each row's terms in stored order, and D (a row's last diagonal entry, 0.0
    when it has none)"""
    n = len(ptr) - 1
    ptr, idx, val = np.asarray(ptr).tolist(), np.asarray(idx).tolist(), np.asarray(val, np.float64).tolist()
    L, U, D = [[] for _ in range(n)], [[] for _ in range(n)], [0.0] * n
    for i in range(n):
        for k in range(ptr[i], ptr[i + 1]):
            c = idx[k]
            if c < i:
                L[i].append((c, val[k]))
            elif c > i:
                U[i].append((c, val[k]))
            else:
                D[i] = val[k]
    return L, U, D


def weights(D, omega):
    """WD: D scaled by omega, then inverted -- two roundings an entry; 1 / 0 is inf, as in C"""
    with np.errstate(all="ignore"):
        t = np.float64(omega) * np.asarray(D, np.float64)
        return 1.0 / t


def row_blocks(n, T):
    q, rem = divmod(n, T)
    out, at = [], 0
    for k in range(T):
        size = q + 1 if k < rem else q
        out.append((at, at + size))
        at += size
    return out


def solve(L, U, wd, b, flag, T=1):
    n = len(L)
    b, wd = np.asarray(b, np.float64).tolist(), np.asarray(wd, np.float64).tolist()
    x = [0.0] * n
    if flag == LOWER:
        for i in range(n):
            t = b[i]
            for c, v in L[i]:
                t -= v * x[c]
            x[i] = t * wd[i]
    elif flag == UPPER:
        for i in range(n - 1, -1, -1):
            t = b[i]
            for c, v in U[i]:
                t -= v * x[c]
            x[i] = t * wd[i]
    else:
        for lo, hi in row_blocks(n, T):
            for i in range(lo, hi):
                t = b[i]
                for c, v in L[i]:
                    if c < lo:
                        continue
                    t -= v * x[c]
                x[i] = t * wd[i]
            for i in range(hi - 1, lo - 1, -1):
                t = 0.0
                for c, v in U[i]:
                    if c < lo or c >= hi:
                        continue
                    t += v * x[c]
                x[i] -= t * wd[i]
    return np.array(x, np.float64)


def solveh(L, U, wd, b, flag, T=1):
    n = len(L)
    wd = np.asarray(wd, np.float64).tolist()
    x = np.asarray(b, np.float64).tolist()
    if flag == LOWER:
        for i in range(n):
            x[i] = x[i] * wd[i]
            xi = x[i]
            for c, v in U[i]:
                x[c] -= v * xi
    elif flag == UPPER:
        for i in range(n - 1, -1, -1):
            x[i] = x[i] * wd[i]
            xi = x[i]
            for c, v in L[i]:
                x[c] -= v * xi
    else:
        for lo, hi in row_blocks(n, T):
            for i in range(lo, hi):
                t = x[i] * wd[i]
                for c, v in U[i]:
                    if c < lo or c >= hi:
                        continue
                    x[c] -= v * t
            for i in range(hi - 1, lo - 1, -1):
                t = x[i] * wd[i]
                x[i] = t
                for c, v in L[i]:
                    if c < lo:
                        continue
                    x[c] -= v * t
    return np.array(x, np.float64)


SOLVES = [(name, flag) for name in ("solve", "solveh") for flag in (LOWER, UPPER, SSOR)]


def all_solves(ptr, idx, val, omega, b, T=1):
    """{"wd": WD, ("solve", LOWER): x, ...}: the six solves of one matrix"""
    L, U, D = split(ptr, idx, val)
    wd = weights(D, omega)
    out = {"wd": wd}
    for name, flag in SOLVES:
        out[name, flag] = (solve if name == "solve" else solveh)(L, U, wd, b, flag, T if flag == SSOR else 1)
    return out


def substitution_residual(L, U, D, omega, b, x, name, flag):
    """For LOWER / UPPER: (r, bound) with r_i = |b - M x|_i and bound_i = gamma_k (|M| |x|)_i in numpy.longdouble, M the triangular
    matrix the solve inverts -- its strict part (L or U; transposed for solveh) plus the diagonal fl(omega D) whose reciprocal WD
    holds.  k = terms of the row + 2: a term's product and at most `terms` subtractions, or for the diagonal the reciprocal, the
    final product and the subtractions before it (Higham, Accuracy and Stability, 8.1, with x = t * wd in place of t / m)."""
    n = len(D)
    ld = np.longdouble
    part = (L if flag == LOWER else U) if name == "solve" else (U if flag == LOWER else L)
    rows = [[] for _ in range(n)]
    for i in range(n):
        for c, v in part[i]:
            if name == "solve":
                rows[i].append((c, v))
            else:
                rows[c].append((i, v))
    m = np.float64(omega) * np.asarray(D, np.float64)
    u = ld(2.0) ** -53
    r, bound = np.zeros(n, ld), np.zeros(n, ld)
    for i in range(n):
        s, a = ld(b[i]) - ld(m[i]) * ld(x[i]), abs(ld(m[i]) * ld(x[i]))
        for c, v in rows[i]:
            p = ld(v) * ld(x[c])
            s -= p
            a += abs(p)
        k = len(rows[i]) + 2
        r[i], bound[i] = abs(s), k * u / (1 - k * u) * a
    return r, bound
