"""Matrices for the conversion tests (tests/test_convert_cpu.py, tests/test_convert_gpu.py) and what they must turn into.

Generators are deterministic and return (ptr, idx, val) as int32 / int32 / float64.  Each is built to reach one place in
kernels/convert.hip or in lisd_convert_csr (host/lis_convert_hbm.c) that a column-sorted stencil never reaches; where the case rests on a
fact about the matrix (the hub block row has exactly so many distinct blocks, `unsorted` really is unsorted), a helper below states
the fact so that the tests can assert it.

The expected arrays of the native layouts come from the plain-C oracle (oracle_arrays), which test_convert_cpu.py holds to the
reference at these very shapes.  The ROW FORMS -- the CSR rows the library builds in HBM for constant-coefficient matrices -- have
no oracle routine: ell_rows / dia_rows / bsr_rows restate them from the comments in convert.hip and lis_upload.c, and
test_convert_cpu.py holds them to orc.spmv_ell / spmv_dia / spmv_bsr of the native arrays."""
import numpy as np

import orc

BLOCKS = [(1, 1), (2, 2), (2, 3), (3, 2), (4, 1), (1, 4), (5, 5), (8, 8)]
BSR_LIST = 96                                   # distinct blocks of one block row the count kernel keeps (convert.hip)
SCAN_SIZES = [1, 255, 256, 4095, 4096, 4097, 8193]
SCAN_BIG = 1025 * 4096 + 7                      # 1026 tiles of 4096: the smallest count at which scan_tile_offsets gives a lane 2 tiles


def _csr(rows, vals=None):
    """rows: list of column lists.  Values: vals, or a fixed non-repeating pattern with every seventh entry -0.0"""
    ptr = np.zeros(len(rows) + 1, np.int32)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    idx = np.array([c for r in rows for c in r], np.int32)
    if vals is None:
        k = np.arange(len(idx))
        vals = ((k * 37) % 101 - 50) / 16.0 + 0.03125
        vals[::7] = -0.0
    return ptr, idx, np.ascontiguousarray(vals, np.float64)


def _sparse_rows(n, rng, sorted_, lo=0, hi=5):
    rows = []
    for _ in range(n):
        cols = rng.choice(n, min(int(rng.integers(lo, hi + 1)), n), replace=False)
        rows.append(sorted(cols.tolist()) if sorted_ else cols.tolist())
    return rows


# ---------------------------------------------------------------- the cases
def hub(n, blocks, bnr, bnc, sorted_):
    """One block row in the middle whose bnr rows together touch exactly `blocks` distinct block columns -- block k through column
    k * bnc + (k % bnc), dealt round-robin over the rows; rows below the first also touch block 0 again, so the count is the size of a
    UNION, not a sum.  Every other row has 0 to 5 entries: no other block row comes near BSR_LIST.  Returns (ptr, idx, val), block row."""
    assert n >= blocks * bnc and n >= 3 * bnr
    rng = np.random.default_rng(1000 * blocks + 10 * bnr + bnc)
    rows = _sparse_rows(n, rng, sorted_)
    br = (n // bnr) // 2
    for ii in range(bnr):
        cols = [k * bnc + (k % bnc) for k in range(blocks) if k % bnr == ii]
        if ii > 0:
            cols.append(bnc - 1)                                   # block 0 again
        rows[br * bnr + ii] = sorted(cols) if sorted_ else cols[::-1]
    return _csr(rows), br


def distinct_blocks(ptr, idx, n, bnr, bnc, br):
    """distinct block columns of block row br"""
    lo, hi = br * bnr, min(n, (br + 1) * bnr)
    return len(set((idx[ptr[lo]:ptr[hi]] // bnc).tolist()))


def is_unsorted(ptr, idx):
    """1 when some row lists a column smaller than the one before it (equal neighbours are in order)"""
    d = np.diff(idx.astype(np.int64)) < 0
    inner = np.ones(len(idx), bool)
    inner[ptr[:-1][ptr[:-1] < len(idx)]] = False                   # the first entry of a row has no neighbour before it
    return int(np.any(d & inner[1:]))


def repeats_a_column(ptr, idx):
    """True when some row stores a column twice.  DIA keeps one value per diagonal: this library keeps the LAST stored one (so do the oracle and
    the kernels); the reference keeps whichever its unstable row sort leaves last, which no rule about the input predicts"""
    return any(len(set(idx[ptr[r]:ptr[r + 1]].tolist())) < ptr[r + 1] - ptr[r] for r in range(len(ptr) - 1))


def max_row(ptr):
    return int(np.diff(ptr).max()) if len(ptr) > 1 else 0


def edges_small():
    rng = np.random.default_rng(77)
    out = {"n1": _csr([[0]], np.array([-2.5]))}
    rows = _sparse_rows(7, rng, True, 0, 2)
    rows[3] = list(range(7))
    out["n7_full_row"] = _csr(rows)
    rows = _sparse_rows(257, rng, True, 0, 3)                       # the longest row is the last one, in the second, one-row workgroup
    rows[256] = [0, 3, 17, 64, 100, 128, 200, 255, 256]
    out["n257_longest_last"] = _csr(rows)
    rows = _sparse_rows(513, rng, True, 1, 4)                       # the only inversion is in the last row
    rows[512] = [5, 400, 399, 512]
    out["n513_inversion_last"] = _csr(rows)
    rows = _sparse_rows(40, rng, True, 1, 4)                        # equal neighbours: in order (csr_row_facts compares with <); the last one wins in DIA / BSR
    for r in range(0, 40, 3):
        rows[r] = sorted(rows[r] + [rows[r][0]])
    rows[39] = [7, 7, 7, 39]
    out["equal_neighbours"] = _csr(rows)
    return out


def empties():
    """n = 700: rows 0..255 (a whole workgroup) empty, rows 256..599 not, the last 100 empty"""
    rng = np.random.default_rng(78)
    rows = _sparse_rows(700, rng, True, 1, 6)
    for r in list(range(256)) + list(range(600, 700)):
        rows[r] = []
    return _csr(rows)


def unsorted():
    return orc.random_csr(600, 7, seed=5)


def duplicates():
    """`unsorted` with one column repeated (the first entry's, in the last slot) in every tenth row of two entries or more"""
    ptr, idx, val = unsorted()
    idx = idx.copy()
    for r in range(0, 600, 10):
        if ptr[r + 1] - ptr[r] >= 2:
            idx[ptr[r + 1] - 1] = idx[ptr[r]]
    return ptr, idx, val


BAND = [-5, -1, 0, 1, 7]
SPECIALS = [-0.0, 0.0, np.nan, np.inf, -np.inf, 5e-324, 1.5, -2.25, 1e-310, 3.0, -7.0]


def _band(n, offsets):
    return [[r + o for o in offsets if 0 <= r + o < n] for r in range(n)]


def specials():
    """300-row band; the values cycle through -0.0, +0.0, NaN, +-inf, subnormals and ordinary numbers"""
    ptr, idx, _ = _csr(_band(300, BAND))
    return ptr, idx, np.array([SPECIALS[k % len(SPECIALS)] for k in range(len(idx))])


def constant():
    """constant coefficients: the row forms are taken"""
    ptr, idx, _ = _csr(_band(300, BAND))
    rows = np.repeat(np.arange(300), np.diff(ptr))
    per_diagonal = {-5: -1.25, -1: -1.0, 0: 6.5, 1: -1.0, 7: 0.75}
    return {"constant_p3d": orc.poisson3d(9, 8, 7, sort_cols=True),
            "constant_band": (ptr, idx, np.array([per_diagonal[int(c - r)] for r, c in zip(rows, idx)]))}


def scan(m):
    """m rows, i % 3 entries in row i on the columns i-2 .. i that it needs, ascending: three diagonals, row lengths 0, 1, 2, 0, 1, 2 ..."""
    lens = np.arange(m, dtype=np.int64) % 3
    ptr = np.zeros(m + 1, np.int32)
    ptr[1:] = np.cumsum(lens)
    rows = np.repeat(np.arange(m, dtype=np.int64), lens)
    k = np.arange(len(rows), dtype=np.int64)
    idx = (rows - lens[rows] + 1 + (k - ptr[rows])).astype(np.int32)
    val = ((k * 37) % 101 - 50) / 16.0 + 0.03125
    val[::7] = -0.0
    return ptr, idx, val


def _cases():
    c = dict(edges_small())
    c["empties"] = empties()
    c["unsorted"] = unsorted()
    c["duplicates"] = duplicates()
    c["specials"] = specials()
    c.update(constant())
    for m in SCAN_SIZES:
        c["scan_%d" % m] = scan(m)
    return c


CASES = _cases()                       # name -> (ptr, idx, val); small, built once, never written to
EDGES = list(edges_small())
SORTED = [k for k, (p, i, v) in CASES.items() if not is_unsorted(p, i)]
HUB_SHAPES = [(1, 1), (1, 4), (2, 2), (2, 3), (3, 2)]          # bnr = 1, 2 and 3
HUB_N = 401                                                     # prime: every shape pads; >= 97 * 4


# ---------------------------------------------------------------- expected arrays
def oracle_arrays(fmt, ptr, idx, val, bnr=2, bnc=2):
    """the arrays of the layout, named as lisdrv.matrix_arrays names them"""
    n = len(ptr) - 1
    if fmt == "csc":
        cptr, cidx, cval = orc.csr2csc(ptr, idx, val)
        return dict(ptr=cptr, index=cidx, value=cval)
    if fmt == "ell":
        mx, eidx, ev = orc.csr2ell(ptr, idx, val)
        return dict(maxnzr=mx, index=eidx, value=ev)
    if fmt == "dia":
        sidx, sval = orc.sort_rows(ptr, idx, val)                  # csr2dia sorts its input first; of a column stored twice the LAST stored entry stays last
        nnd, off, dv = orc.csr2dia(ptr, sidx, sval)
        return dict(nnd=nnd, index=off, value=dv)
    if fmt == "jad":
        mx, perm, jptr, jidx, jval = orc.csr2jad(ptr, idx, val)
        return dict(maxnzr=mx, row=perm, ptr=jptr, index=jidx, value=jval)
    assert fmt == "bsr"
    nr, bptr, bidx, bval = orc.csr2bsr(ptr, idx, val, bnr, bnc)
    return dict(nr=nr, nc=1 + (n - 1) // bnc, bnnz=len(bidx), bptr=bptr, bindex=bidx, value=bval)


def oracle_products(fmt, ptr, idx, val, x, bnr=2, bnc=2):
    """(A x, A^T x) as the reference adds them in this storage format"""
    n = len(ptr) - 1
    a = oracle_arrays(fmt, ptr, idx, val, bnr, bnc)
    if fmt == "csc":
        return orc.spmv_csc(n, n, a["ptr"], a["index"], a["value"], x), orc.spmvh_csc(n, a["ptr"], a["index"], a["value"], x)
    if fmt == "ell":
        return orc.spmv_ell(n, a["maxnzr"], a["index"], a["value"], x), orc.spmvh_ell(n, a["maxnzr"], a["index"], a["value"], x)
    if fmt == "dia":
        return orc.spmv_dia(n, a["nnd"], a["index"], a["value"], x), orc.spmvh_dia(n, a["nnd"], a["index"], a["value"], x)
    if fmt == "jad":
        args = (n, a["maxnzr"], a["row"], a["ptr"], a["index"], a["value"], x)
        return orc.spmv_jad(*args), orc.spmvh_jad(*args)
    args = (n, a["nr"], bnr, bnc, a["bptr"], a["bindex"], a["value"], x)
    return orc.spmv_bsr(*args), orc.spmvh_bsr(*args)


def same_bits(got, want, nan_payload_free=False):
    """every bit of every double; nan_payload_free: where `want` is NaN, `got` may be any NaN"""
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    if got.shape != want.shape:
        return False
    eq = got.view(np.uint64) == want.view(np.uint64)
    if nan_payload_free:
        eq |= np.isnan(got) & np.isnan(want)
    return bool(eq.all())


def same_arrays(got, want):
    """every key of `want`: integers equal, doubles equal in every bit"""
    for k, w in want.items():
        g = got[k]
        if isinstance(w, np.ndarray) and w.dtype == np.float64:
            if not same_bits(g, w):
                return False, k
        elif not np.array_equal(np.atleast_1d(g), np.atleast_1d(w)):
            return False, k
    return True, None


# ---------------------------------------------------------------- the row forms, restated
def ell_rows(n, mx, eidx, ev):
    """convert.hip csr_to_ell_rows: CSR rows of exactly mx terms, slot after slot, padding (value 0 on the row's own column) included"""
    rptr = (np.arange(n + 1, dtype=np.int64) * mx).astype(np.int32)
    return rptr, np.ascontiguousarray(eidx.reshape(mx, n).T).ravel(), np.ascontiguousarray(ev.reshape(mx, n).T).ravel()


def dia_rows(n, ncols, off, dval):
    """convert.hip dia_to_rows: the diagonals that reach row i (0 <= i + offset < ncols), ascending, explicit zeros included"""
    nnd = len(off)
    j = np.arange(n, dtype=np.int64)[:, None] + np.asarray(off, np.int64)[None, :]            # [row, diagonal]
    reach = (j >= 0) & (j < ncols)
    rptr = np.zeros(n + 1, np.int32)
    rptr[1:] = np.cumsum(reach.sum(axis=1))
    return rptr, j[reach].astype(np.int32), np.ascontiguousarray(np.asarray(dval).reshape(nnd, n).T)[reach]


def bsr_rows(n, bnr, bnc, bptr, bidx, bval):
    """convert.hip bsr_to_rows: scalar row bi * bnr + i lists block after block of block row bi, column after column of the block,
    value[bc * bs + j * bnr + i] on column bindex[bc] * bnc + j; the padding rows of the last block row are no rows; rptr[n] = the total"""
    bs = bnr * bnc
    r = np.arange(n, dtype=np.int64)
    bi, i = r // bnr, r % bnr
    lens = np.diff(bptr).astype(np.int64)[bi] * bnc
    rptr = np.zeros(n + 1, np.int64)
    rptr[1:] = np.cumsum(lens)
    rows = np.repeat(r, lens)
    t = np.arange(int(rptr[n]), dtype=np.int64) - rptr[rows]
    blk, j = bptr[bi[rows]] + t // bnc, t % bnc
    ridx = (bidx[blk].astype(np.int64) * bnc + j).astype(np.int32) if len(rows) else np.zeros(0, np.int32)
    rval = bval[blk * bs + j * bnr + i[rows]] if len(rows) else np.zeros(0)
    return rptr.astype(np.int32), ridx, rval
