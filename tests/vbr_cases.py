"""Matrices, block partitions, solve lines and numpy models shared by the VBR fixture (tests/golden/make_golden_vbr.py), the CPU tests
(tests/test_vbr_cpu.py, which hold every model below to the fixture) and the GPU tests (tests/test_vbr_gpu.py, whose kernel-level expectations come
from these models).

A VBR matrix here is a dict: n, nr, nc, bnnz, nnz and the six arrays row, col, ptr, bptr, bindex, value (int32 / float64) of
src/matrix/lis_matrix_vbr.c.  Models restate the reference's loops term by term (numpy float64 rounds every product and every sum once, as the C
loops do without FMA):
  sort_id            src/system/lis_sort.c:90-118        the unstable quicksort of lis_matrix_sort_csr
  rowcol             lis_matrix_vbr.c:262-334            a cut at every start and end of a run of consecutive columns
  csr2vbr / vbr2csr  :501-742, :746-872                  blocks in order of first appearance, column-major, zero-filled; exact zeros dropped on the way back
  matvec             src/matvec/lis_matvec_vbr.c:117-142 one chain per row from +0.0, blocks in stored order, a block's columns ascending
  matvech            :272-313 (OpenMP branch)            T chunks of BLOCK ROWS, each a scatter from 0.0 in stored order, added in chunk order from 0.0
  diagonal / shift   lis_matrix_vbr.c:908-928, :969-989  the reference's search: right on uniform blocks only
  scale              :1055-1069, :1097-1111              value*d[i], value*d[i]*d[j]
"""
import numpy as np

import coo_dns_cases as cc
import esolve_drv

FIXTURE = "vbr_bits.npz"
THREADS = (1, 8)
TILE_ROWS, TILE_UNROLL = 256, 4          # liship_vbr_tile_info: rows of y per workgroup, columns of a block loaded ahead of their adds
# matrices whose blocks the conversion finds (a CSR source alone) ...
FOUND = ("one", "diag", "dense70", "mesh123", "mesh123s", "rand301z", "empty_rows", "unsorted")
# ... and CSR sources with row[] / col[] given through lis_matrix_set_blocksize
GIVEN = ("heights", "blockcounts", "fem3", "fem3s", "sym7b")
ARRAYS_RECORDED = ("one", "diag", "mesh123s", "empty_rows", "unsorted", "blockcounts", "fem3s")   # whose arrays the fixture holds (the others: y, A^T x, the diagonal)
COMMON = "-tol 1e-12 -maxiter 1000 -print mem"       # (-print mem: the reference fills rhistory only then)
# (matrix, held: the caller's matrix is VBR already | CSR, options)
SOLVES = (
    ("fem3", True, "-i cg"),
    ("fem3", True, "-i cg -p jacobi"),
    ("mesh123", True, "-i bicg"),
    ("mesh123", True, "-i bicgstab -p sainv"),
    ("mesh123", True, "-i gmres"),
    ("fem3", True, "-i bicgstab -scale jacobi"),
    ("fem3", False, "-i cg -storage vbr"),
    ("mesh123", False, "-i bicg -p jacobi -storage vbr"),
    ("mesh123", False, "-i bicgstab -storage vbr"),
    ("mesh123", False, "-i gmres -p sainv -storage vbr"),
)
JACOBI_HELD = "fem3"                      # uniform blocks: the reference's diagonal is the diagonal
# (held, options), all on sym7b
ESOLVES = ((False, "-e pi -estorage vbr"), (True, "-e cg"), (True, "-e si -ss 2"))
ECOMMON = "-etol 1e-10 -emaxiter 500 -eprint mem -shift 0"
SHIFT = 0.375
SCALED = ("fem3s", "mesh123s", "blockcounts")        # matrices whose scaled values the fixture holds: the diagonal found (fem3s) or missed, where d keeps D_BEFORE
D_BEFORE = 2.0                                        # what the vector D holds before lis_matrix_scale


def solve_key(m, held, opts):
    return "solve|%s|%s|%s" % (m, "held" if held else "csr", opts)


# ---------------------------------------------------------------- CSR sources
def _mesh(side, unknowns, seed, symmetric):
    """a side x side mesh of nodes, 5-point couplings, node k with unknowns[k] unknowns and a dense block for every coupling; diagonally dominant.
    symmetric: block (b, a) is the transpose of block (a, b) and the diagonal blocks are symmetric (SPD)"""
    rng = np.random.default_rng(seed)
    nodes = side * side
    start = np.concatenate([[0], np.cumsum(unknowns)])
    n = int(start[-1])
    dense = np.zeros((n, n))
    mask = np.zeros((n, n), bool)
    for a in range(nodes):
        ia, ja = divmod(a, side)
        for b in (a - side, a - 1, a, a + 1, a + side):
            ib, jb = divmod(b, side) if 0 <= b < nodes else (-9, -9)
            if b < 0 or b >= nodes or abs(ia - ib) + abs(ja - jb) > 1:
                continue
            blk = rng.uniform(-1, 1, (unknowns[a], unknowns[b]))
            if symmetric and b < a:
                blk = dense[start[b]:start[b + 1], start[a]:start[a + 1]].T
            if symmetric and b == a:
                blk = (blk + blk.T) / 2
            dense[start[a]:start[a + 1], start[b]:start[b + 1]] = blk
            mask[start[a]:start[a + 1], start[b]:start[b + 1]] = True
    off = np.abs(dense).sum(axis=1) - np.abs(np.diag(dense))
    dense[np.arange(n), np.arange(n)] = off * (1.25 + 0.5 * rng.uniform(size=n)) if not symmetric else off + 1.0 + np.arange(n) % 3
    ptr = np.concatenate([[0], np.cumsum(mask.sum(axis=1))]).astype(np.int32)
    idx = np.concatenate([np.flatnonzero(mask[i]) for i in range(n)]).astype(np.int32)
    val = np.concatenate([dense[i][mask[i]] for i in range(n)])
    return (ptr, idx, val), start.astype(np.int32)


def _csr_of_blocks(row, col, blocks, seed, fill=1.0):
    """a CSR matrix holding, for every (bi, bj) of blocks, a share `fill` of the entries of that block (at least one), rows listing their entries in the
    order of `blocks`"""
    rng = np.random.default_rng(seed)
    n = int(row[-1])
    rows = [[] for _ in range(n)]
    for bi, bj in blocks:
        h, w = row[bi + 1] - row[bi], col[bj + 1] - col[bj]
        keep = rng.uniform(size=(h, w)) < fill
        keep[rng.integers(h), rng.integers(w)] = True
        for i in range(h):
            rows[row[bi] + i] += [col[bj] + j for j in range(w) if keep[i, j]]
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    idx = np.array([c for r in rows for c in r], np.int32)
    val = rng.uniform(-1, 1, len(idx))
    val[rng.uniform(size=len(idx)) < 0.1] = 0.0        # explicit zeros: stored in the blocks, multiplied, dropped by vbr2csr
    return ptr, idx, val


HEIGHTS = [1, 2, 3, 4, 5, 6, 7, 8, 17, 63, 64, 65, 255, 256, 257, TILE_UNROLL - 1, TILE_UNROLL + 1, TILE_ROWS - 1, TILE_ROWS + 1]
BLOCKCOUNTS = [0, 1, 32, 33, 0, 2]


def given(name):
    """(ptr, idx, val), row, col of a case whose partition goes through lis_matrix_set_blocksize"""
    if name == "heights":               # block rows of every height in one matrix: they straddle wavefront and workgroup borders at every offset; row != col
        row = np.concatenate([[0], np.cumsum(HEIGHTS)]).astype(np.int32)
        n = int(row[-1])
        widths = []
        while sum(widths) < n:
            widths.append(min(1 + len(widths) % 9, n - sum(widths)))
        col = np.concatenate([[0], np.cumsum(widths)]).astype(np.int32)
        nc, rng = len(widths), np.random.default_rng(11)
        blocks = [(bi, int(bj)) for bi in range(len(HEIGHTS)) for bj in rng.choice(nc, 1 + bi % 4, replace=False)]
        return _csr_of_blocks(row, col, blocks, 12, 0.7), row, col
    if name == "blockcounts":           # block rows of 0, 1, 32 and 33 blocks (and an empty one between others)
        widths = [1 + k % 3 for k in range(36)]
        col = np.concatenate([[0], np.cumsum(widths)]).astype(np.int32)
        row = np.arange(0, int(col[-1]) + 1, int(col[-1]) // len(BLOCKCOUNTS)).astype(np.int32)
        assert row[-1] == col[-1] and len(row) == len(BLOCKCOUNTS) + 1
        rng = np.random.default_rng(13)
        blocks = [(bi, int(bj)) for bi, cnt in enumerate(BLOCKCOUNTS) for bj in rng.permutation(len(widths))[:cnt]]
        return _csr_of_blocks(row, col, blocks, 14, 0.8), row, col
    if name == "fem3":                  # 10 x 10 nodes of 3 unknowns: uniform blocks, symmetric positive definite
        csr, start = _mesh(10, [3] * 100, 15, True)
        return csr, start, start
    if name == "fem3s":                 # the same class on 4 x 4 nodes: small enough for the fixture to hold its arrays
        csr, start = _mesh(4, [3] * 16, 16, True)
        return csr, start, start
    if name == "sym7b":                 # the eigensolvers' matrix in 7 x 7 blocks
        ptr, idx, val = esolve_drv.sym_csr()
        cut = np.arange(0, len(ptr), 7).astype(np.int32)
        return (ptr, idx, val), cut, cut
    raise KeyError(name)


def found(name):
    """(ptr, idx, val) of a case whose blocks the conversion finds"""
    if name == "one":
        return np.array([0, 1], np.int32), np.array([0], np.int32), np.array([2.5])
    if name == "diag":
        n = 130
        return np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.random.default_rng(1).uniform(1, 2, n)
    if name == "dense70":               # one block: every row a chain of 70 terms
        n, rng = 70, np.random.default_rng(2)
        v = rng.uniform(-1, 1, n * n)
        v[rng.uniform(size=n * n) < 0.1] = 0.0
        v[0], v[-1] = 0.5, -0.5         # (vbr2csr drops exact zeros: the corners stay, so that the way back is one block again)
        return (n * np.arange(n + 1)).astype(np.int32), np.tile(np.arange(n, dtype=np.int32), n), v
    if name == "mesh123":               # 20 x 20 nodes with 1, 2 or 3 unknowns: variable blocks, not symmetric
        unknowns = 1 + np.random.default_rng(3).integers(0, 3, 400)
        return _mesh(20, unknowns, 4, False)[0]
    if name == "mesh123s":              # the same class on 6 x 6 nodes: small enough for the fixture to hold its arrays
        unknowns = 1 + np.random.default_rng(7).integers(0, 3, 36)
        return _mesh(6, unknowns, 8, False)[0]
    if name == "rand301z":              # scattered single entries with explicit zeros among them
        ptr, idx, val = cc.matrix("rand301")
        val = val.copy()
        val[np.random.default_rng(5).uniform(size=len(val)) < 0.15] = 0.0
        return ptr, idx, val
    if name == "empty_rows":
        return cc.matrix("empty_rows")
    if name == "unsorted":              # rows out of order, and columns stored twice: the conversion sorts the SOURCE in place, the later value stays in the block
        n, rng = 41, np.random.default_rng(6)
        rows = []
        for r in range(n):
            c = [r, (r + 1) % n, (r + 2) % n, (r + 9) % n, (r + 10) % n, (r + 20) % n]
            c += [c[r % 6], c[(r + 2) % 6]] if r % 2 == 0 else []
            rows.append(rng.permutation(np.array(c)))
        ptr = np.concatenate([[0], np.cumsum([len(c) for c in rows])]).astype(np.int32)
        return ptr, np.concatenate(rows).astype(np.int32), rng.uniform(0.5, 1.5, int(ptr[-1]))
    raise KeyError(name)


def source(name):
    """(ptr, idx, val), row or None, col or None"""
    if name in GIVEN:
        return given(name)
    return found(name), None, None


def xvec(n, seed=5):
    return cc.xvec(n, seed)


def rhs(csr):
    import orc
    return orc.spmv_csr(csr[0], csr[1], csr[2], np.ones(len(csr[0]) - 1))


# ---------------------------------------------------------------- conversions
def sort_id(key, val):
    """lis_sort_id on copies of one row: middle pivot parked at the end, strict Hoare scans, unstable"""
    key, val = key.copy(), val.copy()
    stack = [(0, len(key) - 1)]
    while stack:
        lo, hi = stack.pop()
        if hi <= lo:
            continue
        p = (lo + hi) // 2
        v = key[p]
        for a in (key, val):
            a[p], a[hi] = a[hi], a[p]
        i, j = lo, hi
        while i <= j:
            while key[i] < v:
                i += 1
            while key[j] > v:
                j -= 1
            if i <= j:
                for a in (key, val):
                    a[i], a[j] = a[j], a[i]
                i += 1
                j -= 1
        stack.append((lo, j))
        stack.append((i, hi))
    return key, val


def sort_csr(ptr, idx, val):
    """lis_matrix_sort_csr: every row by sort_id (a strictly ascending row is left as it is by any sort)"""
    idx, val = idx.copy(), val.copy()
    for i in range(len(ptr) - 1):
        idx[ptr[i]:ptr[i + 1]], val[ptr[i]:ptr[i + 1]] = sort_id(idx[ptr[i]:ptr[i + 1]], val[ptr[i]:ptr[i + 1]])
    return idx, val


def rowcol(ptr, idx):
    """lis_matrix_get_vbr_rowcol on sorted rows: the cuts, from 0 to n (a last cut below n is completed to n)"""
    n = len(ptr) - 1
    cut = np.zeros(n + 1, bool)
    for i in range(n):
        c = idx[ptr[i]:ptr[i + 1]]
        if len(c):
            cut[c[0]] = cut[c[-1] + 1] = True
            gap = np.flatnonzero(c[1:] != c[:-1] + 1)
            cut[c[gap + 1]] = True
            cut[c[gap] + 1] = True
    cut[0], cut[n] = True, True
    return np.flatnonzero(cut).astype(np.int32)


def csr2vbr(ptr, idx, val, row=None, col=None):
    """-> (vbr dict, (idx, val) of the source afterwards)"""
    n = len(ptr) - 1
    if row is None:
        idx, val = sort_csr(ptr, idx, val)
        row = col = rowcol(ptr, idx)
    nr, nc = len(row) - 1, len(col) - 1
    of_col = np.repeat(np.arange(nc), np.diff(col))
    bptr, bindex, vptr, chunks = [0], [], [0], []
    for bi in range(nr):
        h, at = row[bi + 1] - row[bi], {}
        for ii in range(h):
            for k in range(ptr[row[bi] + ii], ptr[row[bi] + ii + 1]):
                bj = of_col[idx[k]]
                if bj not in at:
                    at[bj] = len(chunks)
                    bindex.append(bj)
                    chunks.append(np.zeros((col[bj + 1] - col[bj], h)))
                    vptr.append(vptr[-1] + chunks[-1].size)
                chunks[at[bj]][idx[k] - col[bj], ii] = val[k]
        bptr.append(len(bindex))
    value = np.concatenate([c.ravel() for c in chunks] + [np.zeros(0)])
    vbr = dict(n=n, nr=nr, nc=nc, bnnz=len(bindex), nnz=len(value), row=np.asarray(row, np.int32), col=np.asarray(col, np.int32), ptr=np.array(vptr, np.int32),
               bptr=np.array(bptr, np.int32), bindex=np.array(bindex, np.int32), value=value)
    return vbr, (idx, val)


def blocks_of(v, bi):
    """(bc, first column, the block as [column][row]) of block row bi"""
    h = v["row"][bi + 1] - v["row"][bi]
    for bc in range(v["bptr"][bi], v["bptr"][bi + 1]):
        bj = v["bindex"][bc]
        w = v["col"][bj + 1] - v["col"][bj]
        yield bc, v["col"][bj], v["value"][v["ptr"][bc]:v["ptr"][bc] + w * h].reshape(w, h)


def vbr2csr(v):
    ptr, idx, val = [0], [], []
    for bi in range(v["nr"]):
        blocks = list(blocks_of(v, bi))
        for ii in range(v["row"][bi + 1] - v["row"][bi]):
            for _, c0, blk in blocks:
                keep = np.flatnonzero(blk[:, ii] != 0.0)
                idx += list(c0 + keep)
                val += list(blk[keep, ii])
            ptr.append(len(idx))
    return np.array(ptr, np.int32), np.array(idx, np.int32), np.array(val, np.float64)


# ---------------------------------------------------------------- products
def matvec(v, x):
    """all rows of a block row at once, column after column: the same chain per row"""
    y = np.zeros(v["n"])
    with np.errstate(invalid="ignore", over="ignore"):
        for bi in range(v["nr"]):
            t = np.zeros(v["row"][bi + 1] - v["row"][bi])
            for _, c0, blk in blocks_of(v, bi):
                for j in range(blk.shape[0]):
                    t = t + blk[j] * x[c0 + j]
            y[v["row"][bi]:v["row"][bi + 1]] = t
    return y


def matvech(v, x, T=1):
    """chunk t = the block rows LIS_GET_ISIE(t, T, nr); inside a chunk w[j] += value * x[i] in stored order (i inner: one w[j] at a time); y = the chunk
    sums added in chunk order from 0.0"""
    y = np.zeros(int(v["col"][-1]))
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(T):
            lo, hi = cc.isie(t, T, v["nr"])
            w = np.zeros(len(y))
            for bi in range(lo, hi):
                xi = x[v["row"][bi]:v["row"][bi + 1]]
                for _, c0, blk in blocks_of(v, bi):
                    for j in range(blk.shape[0]):
                        s = w[c0 + j]
                        for p in blk[j] * xi:
                            s = s + p
                        w[c0 + j] = s
            y = y + w
    return y


def chunk_borders(v, T):
    """the source rows where the chunks of block rows start, and n"""
    return np.array([v["row"][cc.isie(t, T, v["nr"])[0]] for t in range(T)] + [v["n"]], np.int32)


# ---------------------------------------------------------------- diagonal, shift, scaling
def _diagonal_walk(v):
    """(row, index into value[]) pairs of the reference's search"""
    n = v["n"]
    for bi in range(v["nr"]):
        k, i, h = 0, int(v["row"][bi]), int(v["row"][bi + 1] - v["row"][bi])
        for bc in range(v["bptr"][bi], v["bptr"][bi + 1]):
            bjj = int(v["bindex"][bc])
            w = int(v["col"][bjj + 1] - v["col"][bjj])
            if bjj * w <= i < (bjj + 1) * w:
                j = i % w
                while j < w and k < h and i < n:
                    yield i, int(v["ptr"][bc]) + j * h + k
                    i, k, j = i + 1, k + 1, j + 1
            if k == h:
                break


def diagonal(v, before):
    d = before.copy()
    for i, at in _diagonal_walk(v):
        d[i] = v["value"][at]
    return d


def shift(v, sigma):
    out = v["value"].copy()
    for _, at in _diagonal_walk(v):
        out[at] = out[at] - sigma
    return out


def scale(v, d, symm):
    out = v["value"].copy()
    with np.errstate(invalid="ignore", over="ignore"):       # (a stored diagonal of 0.0 scales by infinity, as in the reference)
        for bi in range(v["nr"]):
            di = d[v["row"][bi]:v["row"][bi + 1]]
            for bc, c0, blk in blocks_of(v, bi):
                new = blk * di[None, :]
                if symm:
                    new = new * d[c0:c0 + blk.shape[0], None]
                out[v["ptr"][bc]:v["ptr"][bc] + blk.size] = new.ravel()
    return out


def true_diagonal(v):
    """what a correct search would give (0.0 where no diagonal entry is stored): tells the uniform cases from the variable ones"""
    d = np.zeros(v["n"])
    for bi in range(v["nr"]):
        for _, c0, blk in blocks_of(v, bi):
            for ii in range(blk.shape[1]):
                i = v["row"][bi] + ii
                if c0 <= i < c0 + blk.shape[0]:
                    d[i] = blk[i - c0, ii]
    return d
