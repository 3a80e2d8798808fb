"""The pencils (A, B), option lists and shift cases that the goldens (tests/golden/make_golden_gesolve.py), the numpy model (tests/shift_model.py) and the tests
of lis_gesolve / lis_matrix_shift_matrix share, so that all of them see the same bits.  CSR triples (ptr, idx, val), numpy only."""
import numpy as np

ROWS_PER_WORKGROUP = 256           # LISHIP_SHIFT_MATRIX_ROWS (include/liship.h): one lane per row, 256 rows per workgroup


def _csr(rows, n):
    """rows: per row a list of (column, value) in the order they are to be stored"""
    assert len(rows) == n
    ptr = np.zeros(n + 1, np.int32)
    idx, val = [], []
    for r, row in enumerate(rows):
        assert len({c for c, _ in row}) == len(row), "columns are unique within a row"
        for c, v in row:
            assert 0 <= c < n
            idx.append(c)
            val.append(v)
        ptr[r + 1] = len(idx)
    return ptr, np.array(idx, np.int32), np.array(val, np.float64)


def _rows(m):
    ptr, idx, val = m
    return [[(int(idx[k]), float(val[k])) for k in range(ptr[r], ptr[r + 1])] for r in range(len(ptr) - 1)]


def tridiag(n, lo, di, up):
    """di may be a callable of the row"""
    rows = []
    for i in range(n):
        row = []
        if i > 0:
            row.append((i - 1, lo))
        row.append((i, di(i) if callable(di) else di))
        if i < n - 1:
            row.append((i + 1, up))
        rows.append(row)
    return _csr(rows, n)


def reversed_rows(m):
    """the same matrix with every row stored in descending column order"""
    return _csr([row[::-1] for row in _rows(m)], len(m[0]) - 1)


def stencil7(l, m, n, diag, off):
    """7-point stencil on an l x m x n grid, rows in ascending column order"""
    N = l * m * n
    rows = []
    for i in range(l):
        for j in range(m):
            for k in range(n):
                r = (i * m + j) * n + k
                row = []
                if i > 0: row.append((r - m * n, off))
                if j > 0: row.append((r - n, off))
                if k > 0: row.append((r - 1, off))
                row.append((r, diag))
                if k < n - 1: row.append((r + 1, off))
                if j < m - 1: row.append((r + n, off))
                if i < l - 1: row.append((r + m * n, off))
                rows.append(row)
    return _csr(rows, N)


# ---------------------------------------------------------------------------------------------- the pencils
def mass1d(n):
    return tridiag(n, 1.0 / 6.0, 4.0 / 6.0, 1.0 / 6.0)


def P1():
    """the 1-D stiffness and mass matrices of linear elements, n = 30"""
    return tridiag(30, -1.0, 2.0, -1.0), mass1d(30)


def P2():
    """the same B; A's diagonal varied: 2 + 0.3 (i mod 5) + 0.01 i"""
    return tridiag(30, -1.0, lambda i: 2.0 + 0.3 * (i % 5) + 0.01 * i, -1.0), mass1d(30)


def P3():
    """a 3-D pencil on 6 x 5 x 4: 7-point A, B on the same pattern with diagonal 1 and off-diagonals 0.05"""
    return stencil7(6, 5, 4, 6.0, -1.0), stencil7(6, 5, 4, 1.0, 0.05)


def P4():
    """P1's A with its rows stored in descending column order, and a B whose pattern is not inside A's: the mass matrix plus 0.01 two columns away"""
    n = 30
    rows = _rows(mass1d(n))
    for i in range(n):
        if i >= 2: rows[i].insert(0, (i - 2, 0.01))
        if i < n - 2: rows[i].append((i + 2, 0.01))
    return reversed_rows(P1()[0]), _csr(rows, n)


def P3v():
    """P3 with A's diagonal varied, 6 + 0.5 (r mod 3) + 0.01 r: the grid's symmetries are gone, so the all-ones start vector has a component along the dominant
    eigenvector.  On P3 itself it has none but rounding: the reference's -e gpi then stops at 15.02 after 237 to 240 iterations at T = 1, 2, 8 and at the
    false pair 11.70 after 76 at T = 4 (make_golden_gesolve.py refuses such a case), so power iteration runs on this pencil instead"""
    A, B = P3()
    ptr, idx, val = A
    val = val.copy()
    for r in range(len(ptr) - 1):
        for k in range(ptr[r], ptr[r + 1]):
            if idx[k] == r:
                val[k] = 6.0 + 0.5 * (r % 3) + 0.01 * r
    return (ptr, idx, val), B


PENCILS = {"P1": P1, "P2": P2, "P3": P3, "P3v": P3v, "P4": P4}

COMMON = "-etol 1e-10 -emaxiter 3000 -eprint mem"
ETOL = 1e-10
# (pencil, -e, extra options)
SOLVES = [("P1", e, "") for e in ("gpi", "gii", "grqi", "gcr")] + [("P3v", "gpi", "")] + [("P3", e, "") for e in ("gii", "grqi", "gcr")] + \
         [("P2", "gcr", ""), ("P2", "gii", ""), ("P1", "gii", "-shift 0.005"), ("P1", "gcr", "-shift 0.005")]
THREADS_BITS = (1, 8)
THREADS_SPREAD = (2, 4)


def solve_key(pencil, e, extra, T):
    return "%s|-e %s%s|T%d" % (pencil, e, (" " + extra) if extra else "", T)


# ---------------------------------------------------------------------------------------------- the shift cases
def _long_rows(shuffled):
    """rows of 65 and of 300 entries in A, each merged with a row of 1 entry and with a row of 200 entries of B (n = 320; every other row: the diagonal)"""
    n = 320
    rng = np.random.default_rng(5)
    A = [[(i, 2.0 + 0.001 * i)] for i in range(n)]
    B = [[(i, 1.0)] for i in range(n)]
    for r, (la, lb) in enumerate([(65, 1), (65, 200), (300, 1), (300, 200)]):
        ca = np.sort(rng.choice(n, la, replace=False))
        cb = np.sort(rng.choice(n, lb, replace=False))
        if shuffled:
            ca, cb = rng.permutation(ca), rng.permutation(cb)
        A[r] = [(int(c), float(np.cos(1.0 + c + r))) for c in ca]
        B[r] = [(int(c), float(np.sin(2.0 + c - r))) for c in cb]
    return _csr(A, n), _csr(B, n)


def _empty_rows():
    """row 0: empty in A; row 1: empty in B; row 2: empty in both; rows 3, 4: ordinary"""
    A = _csr([[], [(0, 1.5), (1, 2.0)], [], [(2, -1.0), (3, 2.0), (4, -1.0)], [(3, -1.0), (4, 2.0)]], 5)
    B = _csr([[(0, 4.0), (1, 0.5)], [], [], [(3, 1.0)], [(3, 0.25), (4, 1.0)]], 5)
    return A, B


def _cancel():
    """row 0 cancels to empty (a = 2, b = 4, sigma = 0.5); row 1 loses its middle entry to an exact cancellation; row 2 keeps a stored zero of A only because B lifts it;
    row 3 holds a stored zero that nothing lifts (dropped)"""
    A = _csr([[(0, 2.0)], [(0, 1.0), (1, 2.0), (2, 3.0)], [(1, 0.0), (2, 5.0)], [(2, 0.0), (3, 7.0)]], 4)
    B = _csr([[(0, 4.0)], [(0, 1.0), (1, 4.0), (2, 1.0)], [(1, 3.0), (2, 1.0)], [(3, 1.0)]], 4)
    return A, B


def _n1():
    return _csr([[(0, 2.0)]], 1), _csr([[(0, 1.0)]], 1)


def _subset_unsorted():
    A, B = P3()
    return reversed_rows(A), B


def _workgroup(n):
    return lambda: (tridiag(n, -1.0, lambda i: 2.0 + 0.01 * i, -1.0), mass1d(n))


# name -> (pencil maker, the shifts applied one after another, A's storage).  "hbm" : A lives in HBM only (CSR)
SHIFTS = {
    "n1": (_n1, (0.5, -0.5), "csr"),
    "empty_rows": (_empty_rows, (0.25, -0.25), "csr"),
    "cancel": (_cancel, (0.5, -0.5), "csr"),
    "subset_sorted": (P3, (0.3, -0.3), "csr"),
    "subset_unsorted": (_subset_unsorted, (0.3, 0.2), "csr"),
    "not_subset": (P4, (0.005, -0.005), "csr"),
    "long_rows": (lambda: _long_rows(False), (0.75, -0.75), "csr"),
    "long_rows_shuffled": (lambda: _long_rows(True), (0.75, -0.75), "csr"),
    "rows_255": (_workgroup(ROWS_PER_WORKGROUP - 1), (0.1, -0.1), "csr"),
    "rows_257": (_workgroup(ROWS_PER_WORKGROUP + 1), (0.1, -0.1), "csr"),
    "sigma0": (P1, (0.0,), "csr"),
    "sigma0_not_subset": (P4, (0.0,), "csr"),
    "negative": (P1, (-0.75, 0.75), "csr"),
    "ell": (P3, (0.3, -0.3), "ell"),
    "bsr": (P1, (0.3, -0.3), "bsr"),
    "hbm_subset": (P3, (0.3, -0.3), "hbm"),
    "hbm_not_subset": (P4, (0.005, -0.005), "hbm"),
}
