"""Matrices, triplet lists, solve lines and numpy models shared by the COO / DNS fixture (tests/golden/make_golden_coo_dns.py), the CPU tests
(tests/test_coo_dns_cpu.py, which hold every model below to the fixture) and the GPU tests (tests/test_coo_dns_gpu.py, whose kernel-level expectations
come from these models).

Models restate the reference's loops term by term (numpy float64 scalars round every product and every sum once, as the C loops do without FMA):
  coo_matvec / coo_matvech     src/matvec/lis_matvec_coo.c:75-87, :116-128     serial walks over the triplets, y from 0.0
  dns_matvec                   src/matvec/lis_matvec_dns.c:50-85               y[i] = 0, then += value[j*n+i] * x[j], j ascending
  dns_matvech                  :87-130 (OpenMP branch)                         T row chunks LIS_GET_ISIE, each from 0.0, added in chunk order from 0.0
  group_by_key                 a stable grouping: segment c lists the entries with key == c in ascending k
"""
import numpy as np

import orc

FIXTURE = "coo_dns_bits.npz"
MATRICES = ("rand301", "stencil", "empty_rows", "dups", "one")
TRIPLETS = ("csr2coo", "shuffled", "descending")
THREADS = (1, 8)
COMMON = "-tol 1e-12 -maxiter 1000 -print mem"       # (-print mem: the reference fills rhistory only then)
SOLVES = (
    "-i cg -storage coo",
    "-i cg -p jacobi -storage dns",
    "-i bicg -storage coo",
    "-i bicg -storage dns",
    "-i bicgstab -storage dns",
    "-i gmres -storage coo",
    "-i bicgstab -scale jacobi -storage coo",
    "-i bicgstab -scale symm_diag -storage dns",
    "-i bicg -p sainv -storage coo",
)
ESOLVES = ("-e pi -estorage coo", "-e ii -estorage dns")
ECOMMON = "-etol 1e-10 -emaxiter 500 -eprint mem -shift 0"
UNSCALED = ("empty_rows", "rand301", "stencil")   # matrices whose scaled values the fixture does not hold (a zero diagonal; size -- the stencil is scaled in the solves)
SHIFT = 0.375                       # lis_matrix_shift_diagonal in the fixture


def stencil():
    """the 7-point matrix on 8 x 7 x 6 with its off-diagonal values perturbed by up to 2 %, so that A is not symmetric, and its diagonal raised by up to 25 %
    row by row (it stays diagonally dominant): Jacobi and both scalings are NOT uniform, so one that read a wrong diagonal entry changes count and history"""
    ptr, idx, val = orc.poisson3d(8, 7, 6)
    rng = np.random.default_rng(20)
    rows = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    off = val * (1.0 + 0.02 * rng.uniform(-1, 1, len(val)))
    diag = val * (1.0 + 0.25 * rng.uniform(0, 1, len(val)))
    return ptr, idx, np.where(rows == idx, diag, off)


def matrix(name):
    """(ptr, idx, val) of a CSR matrix"""
    if name == "rand301":           # 9 entries per row, the diagonal among them, columns in no order
        n, rng = 301, np.random.default_rng(301)
        ptr = (9 * np.arange(n + 1)).astype(np.int32)
        idx = np.empty(9 * n, np.int32)
        for r in range(n):
            cols = rng.choice(np.delete(np.arange(n), r), 8, replace=False)
            idx[9 * r:9 * r + 9] = rng.permutation(np.append(cols, r))
        return ptr, idx, rng.uniform(-1, 1, 9 * n)
    if name == "stencil":
        return stencil()
    if name == "empty_rows":        # rows 0, 18 and 36 of 37 hold nothing
        n, rng = 37, np.random.default_rng(37)
        lens = np.full(n, 3)
        lens[[0, 18, 36]] = 0
        ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        idx = np.concatenate([rng.permutation(np.array([r, (r + 5) % n, (r + 11) % n])) for r in range(n) if lens[r]]).astype(np.int32)
        return ptr, idx, rng.uniform(-1, 1, len(idx))
    if name == "dups":              # duplicate (i, j) entries, the diagonal twice in every third row
        n, rng = 23, np.random.default_rng(23)
        rows = []
        for r in range(n):
            c = [r, (r + 3) % n, (r + 3) % n, (r + 7) % n]
            if r % 3 == 0:
                c += [r]
            rows.append(np.array(c))
        ptr = np.concatenate([[0], np.cumsum([len(c) for c in rows])]).astype(np.int32)
        idx = np.concatenate(rows).astype(np.int32)
        return ptr, idx, rng.uniform(0.5, 1.5, len(idx))
    if name == "one":
        return np.array([0, 1], np.int32), np.array([0], np.int32), np.array([2.5])
    raise KeyError(name)


def csr2coo(ptr, idx, val):
    """ref lis_matrix_coo.c:753-763"""
    return np.repeat(np.arange(len(ptr) - 1, dtype=np.int32), np.diff(ptr)), idx.astype(np.int32).copy(), val.copy()


def triplets(kind):
    """(n, row, col, val): the triplet lists whose COO -> CSR conversion the fixture records, all of rand301"""
    ptr, idx, val = matrix("rand301")
    n = len(ptr) - 1
    row, col, v = csr2coo(ptr, idx, val)
    if kind == "shuffled":
        p = np.random.default_rng(77).permutation(len(row))
        row, col, v = row[p], col[p], v[p]
    elif kind == "descending":      # rows n-1 .. 0, a row's entries in their order
        p = np.concatenate([np.arange(ptr[r], ptr[r + 1]) for r in range(n - 1, -1, -1)])
        row, col, v = row[p], col[p], v[p]
    elif kind != "csr2coo":
        raise KeyError(kind)
    return n, row.copy(), col.copy(), v.copy()


def xvec(n, seed=5):
    return np.random.default_rng(seed).uniform(-1, 1, n)


def rhs(ptr, idx, val):
    return orc.spmv_csr(ptr, idx, val, np.ones(len(ptr) - 1))


# ---------------------------------------------------------------- conversions
def csr2dns(ptr, idx, val, np_=None):
    """ref lis_matrix_dns.c:784-797: zero-fill, then every entry in stored order (a duplicate's last value wins); column-major, flat"""
    n = len(ptr) - 1
    np_ = n if np_ is None else np_
    d = np.zeros(n * np_)
    for i in range(n):
        for k in range(ptr[i], ptr[i + 1]):
            d[idx[k] * n + i] = val[k]
    return d


def dns2csr(n, np_, d):
    """ref lis_matrix_dns.c:846-895: value != 0 kept, columns ascending"""
    m = d.reshape(np_, n).T
    keep = m != 0.0
    ptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int32)
    idx = np.concatenate([np.flatnonzero(keep[i]) for i in range(n)] + [np.zeros(0, np.int64)]).astype(np.int32)
    val = np.concatenate([m[i][keep[i]] for i in range(n)] + [np.zeros(0)])
    return ptr, idx, val


def sort_iid(key, a, b):
    """lis_sort_iid (src/system/lis_sort.c:183-213) on copies: middle pivot parked at the end, strict Hoare scans, unstable"""
    key, a, b = key.copy(), a.copy(), b.copy()

    def swap(i, j):
        key[i], key[j] = key[j], key[i]
        a[i], a[j] = a[j], a[i]
        b[i], b[j] = b[j], b[i]

    stack = [(0, len(key) - 1)]
    while stack:
        lo, hi = stack.pop()
        if hi <= lo:
            continue
        p = (lo + hi) // 2
        v = key[p]
        swap(p, hi)
        i, j = lo, hi
        while i <= j:
            while key[i] < v:
                i += 1
            while key[j] > v:
                j -= 1
            if i <= j:
                swap(i, j)
                i += 1
                j -= 1
        stack.append((lo, j))
        stack.append((i, hi))
    return key, a, b


def coo2csr(n, row, col, val):
    """ref lis_matrix_coo.c:810-833 -> (ptr, idx, val) and the source's arrays as the sort leaves them"""
    srow, scol, sval = sort_iid(row, col, val)
    ptr = np.concatenate([[0], np.cumsum(np.bincount(srow, minlength=n))]).astype(np.int32)
    return (ptr, scol.copy(), sval.copy()), (srow, scol, sval)


def group_by_key(nkeys, key, src, val):
    """segment c: the entries with key == c in ascending k (a stable sort by key)"""
    order = np.argsort(key, kind="stable")
    ptr = np.concatenate([[0], np.cumsum(np.bincount(key, minlength=nkeys))]).astype(np.int32)
    return ptr, src[order].astype(np.int32), val[order]


# ---------------------------------------------------------------- products
def coo_matvec(n, row, col, val, x):
    y = np.zeros(n)
    for k in range(len(row)):
        y[row[k]] = y[row[k]] + val[k] * x[col[k]]
    return y


def coo_matvech(np_, row, col, val, x):
    y = np.zeros(np_)
    for k in range(len(row)):
        y[col[k]] = y[col[k]] + val[k] * x[row[k]]
    return y


def dns_matvec(n, np_, d, x):
    """all rows at once, column after column: the same chain per row"""
    m = d.reshape(np_, n)
    y = np.zeros(n)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(np_):
            y = y + m[j] * x[j]
    return y


def isie(k, T, n):
    """LIS_GET_ISIE (include/lis.h of the reference, :1067-1078)"""
    q, rem = divmod(n, T)
    if k < rem:
        return k * (q + 1), k * (q + 1) + q + 1
    return k * q + rem, k * q + rem + q


def dns_matvech(n, np_, d, x, T=1):
    """all columns at once, row after row inside a chunk; the chunk sums added in chunk order from 0.0"""
    m = d.reshape(np_, n)
    y = np.zeros(np_)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(T):
            lo, hi = isie(k, T, n)
            t = np.zeros(np_)
            for i in range(lo, hi):
                t = t + m[:, i] * x[i]
            y = y + t
    return y


# ---------------------------------------------------------------- diagonal, scaling, shift (host restatements)
def coo_diagonal(n, row, col, val, before):
    """ref lis_matrix_coo.c:343-349: the last stored (i,i) wins, a row without one keeps what d held"""
    d = before.copy()
    for k in range(len(row)):
        if row[k] == col[k]:
            d[row[k]] = val[k]
    return d


def coo_scale(row, col, val, d, symm):
    """ref lis_matrix_coo.c:426-432, :456-461 (d[row]*d[row] in the symmetric form)"""
    return val * (d[row] * d[row]) if symm else val * d[row]


def dns_scale(n, np_, dns, d, symm):
    """ref lis_matrix_dns.c:453-494"""
    m = dns.reshape(np_, n).copy()
    for j in range(np_):
        m[j] = m[j] * (d[:n] * d[j]) if symm else m[j] * d[:n]
    return m.ravel()


def coo_shift(row, col, val, sigma):
    return np.where(row == col, val - sigma, val)


def dns_shift(n, dns, sigma):
    out = dns.copy()
    out[np.arange(n) * n + np.arange(n)] -= sigma
    return out
