"""An independent statement of the ILU(k) preconditioner behind -p ilu, for tests.

Symbolic step (which entries L and U keep at fill level k), numerical factorisation, M^-1 and M^-H, written from the behaviour
lis_ilu.c's header describes.  Plain Python loops over Python floats (IEEE doubles; CPython never contracts a multiply and a
subtraction): every value is one ordered chain of individually rounded operations, row after row, pivot after pivot.  There is
no level schedule here, no search for a column's position and nothing vectorised over terms: it shares no structure with the code
it checks.  T row blocks are cut as LIS_GET_ISIE cuts them (the first n % T blocks hold n / T + 1 rows); a block factorises and
sweeps its own rows and drops every entry whose column leaves it.

Term order.  Row i of L: its kept columns before i ascending, a column stored twice twice (side by side).  Row i of U: the kept
columns after i in A's stored order, then the fill-in in the order the pivots discover it.  D apart, held as 1 / pivot.
"""
import numpy as np


def row_blocks(n, T):
    q, rem = divmod(n, T)
    out, at = [], 0
    for k in range(T):
        size = q + 1 if k < rem else q
        out.append((at, at + size))
        at += size
    return out


def symbolic(ptr, idx, fill, T=1):
    """(Lcols, Ucols): per row the list of kept columns, in term order"""
    n = len(ptr) - 1
    ptr, idx = np.asarray(ptr).tolist(), np.asarray(idx).tolist()
    Lc, Uc, Ulev = [None] * n, [None] * n, [None] * n
    for lo, hi in row_blocks(n, T):
        for i in range(lo, hi):
            low, up, seen = [], [], {}          # entries are [column, level]; seen: the entry that answers for a column
            for k in range(ptr[i], ptr[i + 1]):
                c = idx[k]
                if c < lo or c >= hi or c == i:
                    continue
                e = [c, 0]
                (low if c < i else up).append(e)
                seen[c] = e
            p = 0
            while p < len(low):                 # the smallest column not yet used as a pivot comes next (first of equals)
                rest = [e[0] for e in low[p:]]
                m = p + rest.index(min(rest))
                low[p], low[m] = low[m], low[p]
                piv, plev = low[p]
                for c, ulev in zip(Uc[piv], Ulev[piv]):
                    lev = ulev + plev + 1
                    if lev > fill:
                        continue
                    e = seen.get(c)
                    if e is None:
                        if c == i:
                            continue
                        e = [c, lev]
                        (low if c < i else up).append(e)
                        seen[c] = e
                    elif lev < e[1]:
                        e[1] = lev
                p += 1
            Lc[i] = [e[0] for e in low]
            Uc[i] = [e[0] for e in up]
            Ulev[i] = [e[1] for e in up]
    return Lc, Uc


def _recip(d):
    with np.errstate(all="ignore"):
        return float(np.float64(1.0) / np.float64(d))


def factor(ptr, idx, val, fill, T=1):
    """{"L": (ptr, idx, val), "U": (ptr, idx, val), "D": d} -- D holds 1 / pivot, 1 / 0 = inf as in C"""
    n = len(ptr) - 1
    Lc, Uc = symbolic(ptr, idx, fill, T)
    ptr, idx, val = np.asarray(ptr).tolist(), np.asarray(idx).tolist(), np.asarray(val, np.float64).tolist()
    Lv, Uv, D = [None] * n, [None] * n, [0.0] * n
    for lo, hi in row_blocks(n, T):
        for i in range(lo, hi):
            lv, uv, d = [0.0] * len(Lc[i]), [0.0] * len(Uc[i]), 0.0
            place = {}                          # column -> position in its part; of a column held twice, the later one
            for j, c in enumerate(Lc[i]):
                place[c] = j
            for j, c in enumerate(Uc[i]):
                place[c] = j
            for k in range(ptr[i], ptr[i + 1]):
                c = idx[k]
                if c < lo or c >= hi:
                    continue
                if c < i:
                    lv[place[c]] = val[k]
                elif c == i:
                    d = val[k]
                else:
                    uv[place[c]] = val[k]
            for j, piv in enumerate(Lc[i]):
                l = lv[j] * D[piv]
                lv[j] = l
                for c, u in zip(Uc[piv], Uv[piv]):
                    if c == i:
                        t = l * u
                        d = d - t
                    elif c in place:
                        t = l * u
                        if c < i:
                            lv[place[c]] = lv[place[c]] - t
                        else:
                            uv[place[c]] = uv[place[c]] - t
            Lv[i], Uv[i] = lv, uv
            D[i] = _recip(d)

    def csr(cols, vals):
        p = np.zeros(n + 1, np.int32)
        for i in range(n):
            p[i + 1] = p[i] + len(cols[i])
        return (p, np.array([c for r in cols for c in r], np.int32), np.array([v for r in vals for v in r], np.float64))
    return {"L": csr(Lc, Lv), "U": csr(Uc, Uv), "D": np.array(D, np.float64)}


def _rows(part):
    p, c, v = part
    p, c, v = p.tolist(), c.tolist(), v.tolist()
    return [list(zip(c[p[i]:p[i + 1]], v[p[i]:p[i + 1]])) for i in range(len(p) - 1)]


def psolve(f, b, T=1):
    """x = M^-1 b"""
    L, U, D = _rows(f["L"]), _rows(f["U"]), f["D"].tolist()
    x = np.asarray(b, np.float64).tolist()
    n = len(x)
    for lo, hi in row_blocks(n, T):
        for i in range(lo, hi):
            t = x[i]
            for c, v in L[i]:
                t = t - v * x[c]
            x[i] = t
        for i in range(hi - 1, lo - 1, -1):
            t = x[i]
            for c, v in U[i]:
                t = t - v * x[c]
            x[i] = D[i] * t
    return np.array(x, np.float64)


def psolveh(f, b, T=1):
    """x = M^-H b, the scatter it is"""
    L, U, D = _rows(f["L"]), _rows(f["U"]), f["D"].tolist()
    x = np.asarray(b, np.float64).tolist()
    n = len(x)
    for lo, hi in row_blocks(n, T):
        for i in range(lo, hi):
            x[i] = D[i] * x[i]
            xi = x[i]
            for c, v in U[i]:
                x[c] = x[c] - v * xi
        for i in range(hi - 1, lo - 1, -1):
            xi = x[i]
            for c, v in L[i]:
                x[c] = x[c] - v * xi
    return np.array(x, np.float64)
