"""numpy models of the two preconditioners that are applied as products, stated from the reference's text alone:

SAINV (src/precon/lis_precon_sainv.c:122-378, :735-840): factor(ptr, idx, val, tol) runs the right-looking A-biorthogonalisation with the
reference's own dense work vectors, psolve / psolveh apply M^-1 = Z D^-1 W^T and M^-H = W D^-1 Z^T as the OpenMP build does at T threads:
the gather side a row sum from +0.0 in stored order, the scatter side per thread chunk of source rows (LIS_GET_ISIE) from +0.0 and the chunk
sums folded in thread order from +0.0.

I+S (src/precon/lis_precon_is.c:417-547): is_psolve / is_psolveh on the strict upper part's rows (uptr, uidx, uval) of a split matrix.

Every product and every sum is one IEEE double operation, written out one at a time."""
import numpy as np


def chunks(n, T):
    """[(is, ie)] of LIS_GET_ISIE(k, T, n): the first n % T chunks hold n / T + 1 rows"""
    T = max(int(T), 1)
    q, rem = divmod(n, T)
    out, at = [], 0
    for k in range(T):
        size = q + 1 if k < rem else q
        out.append((at, at + size))
        at += size
    return out


def csc_of(n, ptr, idx, val):
    """columns of a CSR matrix, a column's entries by row, ties by place in the row"""
    cols = [[] for _ in range(n)]
    for i in range(n):
        for k in range(ptr[i], ptr[i + 1]):
            cols[idx[k]].append((i, val[k]))
    return cols


def factor(ptr, idx, val, tol):
    """{"W": (ptr, index, value), "Z": (...), "D": d}: rows in stored order, unit diagonal first, d[i] = 1 / pivot"""
    ptr, idx = np.asarray(ptr), np.asarray(idx)
    val = np.asarray(val, np.float64)
    n = len(ptr) - 1
    cols = csc_of(n, ptr, idx, val)
    Wi, Wv = [[i] for i in range(n)], [[np.float64(1.0)] for _ in range(n)]
    Zi, Zv = [[i] for i in range(n)], [[np.float64(1.0)] for _ in range(n)]
    d = np.zeros(n)
    tol = np.float64(tol)
    with np.errstate(all="ignore"):
        for i in range(n):
            nrm = np.float64(0.0)
            for k in range(ptr[i], ptr[i + 1]):
                a = np.abs(val[k])
                nrm = nrm if nrm >= a else a
            nrm = np.float64(1.0) / nrm
            l, il = np.zeros(n), []
            for k, ii in enumerate(Zi[i]):
                for jj, a in cols[ii]:
                    if jj > i:
                        l[jj] = l[jj] + a * Zv[i][k]
                        if jj not in il:
                            il.append(jj)
            u, iu = np.zeros(n), []
            for k, ii in enumerate(Wi[i]):
                for j in range(ptr[ii], ptr[ii + 1]):
                    jj = idx[j]
                    u[jj] = u[jj] + val[j] * Wv[i][k]
                    if jj > i and jj not in iu:
                        iu.append(jj)
            t = np.float64(0.0)
            for k, c in enumerate(Zi[i]):
                t = t + u[c] * Zv[i][k]
            d[i] = np.float64(1.0) / t
            for rows_i, rows_v, lst, vec in ((Wi, Wv, il, l), (Zi, Zv, iu, u)):
                for j in lst:
                    dd = vec[j] * d[i]
                    for ik, c in enumerate(rows_i[i]):
                        t = dd * rows_v[i][ik]
                        if not (np.abs(t) * nrm > tol):
                            continue
                        if c in rows_i[j]:
                            at = rows_i[j].index(c)
                            rows_v[j][at] = rows_v[j][at] - t
                        else:
                            rows_i[j].append(c)
                            rows_v[j].append(-t)

    def pack(ri, rv):
        p = np.zeros(n + 1, np.int32)
        for i in range(n):
            p[i + 1] = p[i] + len(ri[i])
        return p, np.array([c for r in ri for c in r], np.int32), np.array([v for r in rv for v in r], np.float64)

    return {"W": pack(Wi, Wv), "Z": pack(Zi, Zv), "D": d}


def gather(rows, x):
    """lis_matvech_ilu: y[i] = the row's sum from +0.0 in stored order"""
    p, c, v = rows
    n = len(p) - 1
    y = np.zeros(n)
    with np.errstate(all="ignore"):
        for i in range(n):
            t = np.float64(0.0)
            for k in range(p[i], p[i + 1]):
                t = t + v[k] * x[c[k]]
            y[i] = t
    return y


def scatter(rows, x, T, scale=None):
    """lis_matvec_ilu's OpenMP branch: every thread scatters its chunk of source rows into a buffer of its own from +0.0, the buffers
    are folded in thread order from +0.0.  scale: the factor formed with the stored value FIRST (lis_psolveh_is: (w u) x[i])"""
    p, c, v = rows
    n = len(p) - 1
    y = np.zeros(n)
    with np.errstate(all="ignore"):
        for lo, hi in chunks(n, T):
            w = np.zeros(n)
            for i in range(lo, hi):
                for k in range(p[i], p[i + 1]):
                    a = v[k] if scale is None else np.float64(scale) * v[k]
                    w[c[k]] = w[c[k]] + a * x[i]
            y = y + w
    return y


def psolve(f, b, T=1):
    """x = Z ((W^T-gather b) .* d)"""
    b = np.asarray(b, np.float64)
    with np.errstate(all="ignore"):
        t = gather(f["W"], b) * f["D"]
    return scatter(f["Z"], t, T)


def psolveh(f, b, T=1):
    """x = W ((Z-gather b) .* d)"""
    b = np.asarray(b, np.float64)
    with np.errstate(all="ignore"):
        t = gather(f["Z"], b) * f["D"]
    return scatter(f["W"], t, T)


def truncated(uptr, uidx, uval, m):
    """the first min(m + 1, length) entries of every row"""
    n = len(uptr) - 1
    keep = max(int(m) + 1, 0)
    p = np.zeros(n + 1, np.int32)
    ci, cv = [], []
    for i in range(n):
        hi = min(uptr[i] + keep, uptr[i + 1])
        ci += list(uidx[uptr[i]:hi])
        cv += list(uval[uptr[i]:hi])
        p[i + 1] = len(ci)
    return p, np.array(ci, np.int32), np.array(cv, np.float64)


def is_psolve(uptr, uidx, uval, alpha, m, x):
    """y[i] = x[i] - alpha * t, t the truncated row's sum from +0.0: two roundings after the sum"""
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        return x - np.float64(alpha) * gather(truncated(uptr, uidx, uval, m), x)


def is_psolveh(uptr, uidx, uval, alpha, m, x, T=1):
    """y = x - (the scatter of (alpha u) x[i], chunked as the OpenMP build's buffers are)"""
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        return x - scatter(truncated(uptr, uidx, uval, m), x, T, scale=alpha)


def strict_upper(ptr, idx, val):
    """A->U of lis_matrix_split on CSR storage: the entries right of the diagonal, in stored order"""
    n = len(ptr) - 1
    p = np.zeros(n + 1, np.int32)
    ci, cv = [], []
    for i in range(n):
        for k in range(ptr[i], ptr[i + 1]):
            if idx[k] > i:
                ci.append(idx[k])
                cv.append(val[k])
        p[i + 1] = len(ci)
    return p, np.array(ci, np.int32), np.array(cv, np.float64)
