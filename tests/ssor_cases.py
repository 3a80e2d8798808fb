"""Matrices built to a prescribed level schedule, the schedule rules of include/liship.h restated, and the catalogue of cases that
tests/test_ssor_cpu.py (oracle against the reference library) and tests/test_ssor_schedule_gpu.py (kernels against the oracle) share.

pattern(levels): a strictly lower pattern whose forward sweep has exactly the given levels, each a list of row term counts.
system(case): A1 = D + P + mirror(P') prescribes the forward sweep on L (P) and the backward sweep on U (P' mirrored by
(i, j) -> (n-1-i, n-1-j)); A2 = D2 + (P + mirror(P'))^T prescribes the two transposed sweeps of lis_matrix_solveh.  Every row's
diagonal is 1 + the row's absolute sum and its other entries are scaled by the row length, so every solve stays finite.
Deterministic, numpy only.
"""
import numpy as np

SMALL_LEVEL = 1024      # LISHIP_SWEEP_SMALL_LEVEL: a level of more rows gets a launch of its own
LONG_ROW = 64           # LISHIP_SWEEP_LONG_ROW: a row of this many terms or more is served by a whole workgroup
OMEGA = 1.3


# ---------------------------------------------------------------- the generator
def pattern(levels, seed, sort_cols=False, duplicates=False, order="level"):
    """rows[i] = columns of row i (all < i).  Row i of level l >= 1 reads one row of level l-1 and otherwise distinct random rows
    of earlier levels.  duplicates: some rows of 3 terms or more repeat a column.  order "level": rows numbered level after level;
    "mixed": any numbering that keeps the pattern strictly lower (rows sorted by a random key larger than the keys of the rows
    they read)."""
    rng = np.random.default_rng(seed)
    start = np.concatenate(([0], np.cumsum([len(l) for l in levels]))).astype(np.int64)
    rows = []
    for l, counts in enumerate(levels):
        for c in counts:
            if l == 0:
                assert c == 0, "a row of the first level reads nothing"
                rows.append(np.zeros(0, np.int64))
                continue
            assert 1 <= c <= start[l], (l, c, int(start[l]))
            link = int(rng.integers(start[l - 1], start[l]))
            rest = rng.choice(int(start[l]) - 1, c - 1, replace=False).astype(np.int64)
            rest[rest >= link] += 1
            cols = np.concatenate(([link], rest))
            if duplicates and c >= 3 and rng.random() < 0.3:
                cols[2] = cols[1]
            rows.append(cols)
    n = len(rows)
    if order == "mixed":
        key = np.zeros(n)
        for i in range(n):
            key[i] = (key[rows[i]].max() if len(rows[i]) else 0.0) + rng.uniform(0.01, 1.0)
        new_of_old = np.empty(n, np.int64)
        old_of_new = np.argsort(key, kind="stable")
        new_of_old[old_of_new] = np.arange(n)
        rows = [new_of_old[rows[o]] for o in old_of_new]
    else:
        assert order == "level"
    out = []
    for i, cols in enumerate(rows):
        assert len(cols) == 0 or cols.max() < i
        cols = np.sort(cols, kind="stable") if sort_cols else rng.permutation(cols)
        out.append(cols)
    return out


def _assemble(offdiag, rng, sort_cols, zero_diag=()):
    """CSR of D + N: N's rows as (cols, vals); the diagonal entry anywhere in the row unless the columns are sorted"""
    n = len(offdiag)
    ptr, idx, val = [0], [], []
    for i, (cols, vals) in enumerate(offdiag):
        d = 0.0 if i in zero_diag else 1.0 + float(np.abs(vals).sum())
        cols, vals = np.concatenate((cols, [i])), np.concatenate((vals, [d]))
        perm = np.argsort(cols, kind="stable") if sort_cols else rng.permutation(len(cols))
        idx.append(cols[perm])
        val.append(vals[perm])
        ptr.append(ptr[-1] + len(cols))
    return np.array(ptr, np.int32), np.concatenate(idx).astype(np.int32), np.concatenate(val).astype(np.float64)


def matrices(pat_f, pat_b, seed, sort_cols=False, zeros=False, zero_diag=()):
    """(A1, A2), each (ptr, idx, val)"""
    n = len(pat_f)
    assert len(pat_b) == n
    rng = np.random.default_rng(seed)
    N = []
    for i in range(n):
        cols = np.concatenate((pat_f[i], n - 1 - pat_b[n - 1 - i])).astype(np.int64)
        vals = rng.uniform(-1.0, 1.0, len(cols)) / max(1, len(cols))
        if zeros and len(cols) >= 2:
            vals[rng.random(len(cols)) < 0.1] = 0.0             # explicit zeros stay terms of the row
        N.append((cols, vals))
    tc, tv = [[] for _ in range(n)], [[] for _ in range(n)]
    for i, (cols, vals) in enumerate(N):
        for c, v in zip(cols.tolist(), vals.tolist()):
            tc[c].append(i)
            tv[c].append(v)
    Nt = [(np.array(c, np.int64), np.array(v, np.float64)) for c, v in zip(tc, tv)]
    return _assemble(N, rng, sort_cols, zero_diag), _assemble(Nt, rng, sort_cols, zero_diag)


# ---------------------------------------------------------------- the schedule rules, restated
def row_block(n, T):
    """block of every row among T blocks of LIS_GET_ISIE: the first n % T blocks hold n / T + 1 rows"""
    q, rem = divmod(n, T)
    i = np.arange(n)
    head = rem * (q + 1)
    return np.where(i < head, i // (q + 1), rem + (i - head) // max(q, 1))


def sweep_terms(ptr, idx, val, T=1):
    """The four sweeps of a matrix under T row blocks: [(terms, desc)] for forward on L, backward on U, forward on U^T, backward on
    L^T; terms[i] = [(col, value)] in the order they are added.  A term is kept when its row and column lie in the same block.
    The transposed sweeps list a row's terms in the order the scatter reaches it: U^T by source row ascending, L^T descending."""
    n = len(ptr) - 1
    blk = row_block(n, T).tolist()
    ptr, idx, val = np.asarray(ptr).tolist(), np.asarray(idx).tolist(), np.asarray(val).tolist()
    L, U = [[] for _ in range(n)], [[] for _ in range(n)]
    UT, LT = [[] for _ in range(n)], [[] for _ in range(n)]
    for i in range(n):
        for k in range(ptr[i], ptr[i + 1]):
            c = idx[k]
            if c == i or blk[c] != blk[i]:
                continue
            if c < i:
                L[i].append((c, val[k]))
            else:
                U[i].append((c, val[k]))
                UT[c].append((i, val[k]))
    for i in range(n - 1, -1, -1):
        for c, v in L[i]:
            LT[c].append((i, v))
    return [(L, 0), (U, 1), (UT, 0), (LT, 1)]


def levels_of(terms, desc):
    """level of a row = 1 + the largest level of the rows its terms read (0 when it reads none)"""
    n = len(terms)
    lev = [0] * n
    for i in (range(n - 1, -1, -1) if desc else range(n)):
        best = 0
        for c, _ in terms[i]:
            assert (c > i) if desc else (c < i)
            if lev[c] + 1 > best:
                best = lev[c] + 1
        lev[i] = best
    return lev


def grouping(sizes):
    """[(l0, l1, run)]: consecutive levels of at most SMALL_LEVEL rows share one launch, every larger level has its own"""
    groups, l = [], 0
    while l < len(sizes):
        if sizes[l] <= SMALL_LEVEL:
            e = l
            while e < len(sizes) and sizes[e] <= SMALL_LEVEL:
                e += 1
            groups.append((l, e, 1))
            l = e
        else:
            groups.append((l, l + 1, 0))
            l += 1
    return groups


def sweep_stats(terms, desc):
    """what lis_amd_ssor_sweep_info reports, plus the level sizes and the longest row"""
    lev = levels_of(terms, desc)
    nlev = (max(lev) + 1) if lev else 0
    sizes, nlong = [0] * nlev, [0] * nlev
    for i, l in enumerate(lev):
        sizes[l] += 1
        nlong[l] += len(terms[i]) >= LONG_ROW
    groups = grouping(sizes)
    own = [g[0] for g in groups if not g[2]]
    return {"info": [nlev, len(groups), len(own), sum(nlong[l] for l in own), sum(nlong) - sum(nlong[l] for l in own), sum(len(t) for t in terms)],
            "sizes": sizes, "nlong": nlong, "longest": max([len(t) for t in terms], default=0), "lev": lev, "groups": groups}


# ---------------------------------------------------------------- the catalogue
EDGE_COUNTS = [1, 2, 62, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2049]     # 0 terms: every row of a first level


def level(size, counts=(), first=False):
    """`size` rows: the given term counts, the rest filled with 1, 2, 3, 1, ... (a first level: no terms anywhere)"""
    if first:
        assert not counts
        return [0] * size
    assert len(counts) <= size
    return list(counts) + [1 + k % 3 for k in range(size - len(counts))]


def _sizes(sizes, extra=None):
    """levels of the given sizes; extra[k]: term counts of the first rows of level k.  No row gets more terms than rows lie before it."""
    extra, out, before = extra or {}, [], 0
    for k, s in enumerate(sizes):
        out.append([min(c, before) for c in level(s, extra.get(k, ()), first=(k == 0))])
        before += s
    return out


ALT = [1500, 300, 1, 200, 5, 100, 1100, 50, 60, 1200, 1300, 10, 20, 1031]
CASES = {
    # level sizes across the run / own-launch switch and the 256-thread block borders; a few long rows in the large levels
    "sizes": dict(
        what="level sizes 1, 255, 256, 257, 1023, 1024, 1025, 1280, 1281, 5000 (backward: the same sizes in another order)",
        fwd=_sizes([1, 255, 256, 257, 1023, 1024, 1025, 1280, 1281, 5000], {6: (64, 300), 9: (100,)}),
        bwd=_sizes([1024, 1281, 1, 5000, 257, 1025, 255, 1280, 256, 1023], {3: (70,), 5: (257,)}),
        T=(3, 8)),
    # large level first, runs, one large level, two in a row, large level last; a level of one row and a small level of long rows only
    "alternating": dict(
        what="large first, run, large, run, two large in a row, run, large last; rows numbered in a mixed order, duplicate columns",
        fwd=_sizes(ALT, {4: (70, 64, 65, 300, 1025), 6: (64, 513), 9: (2049,)}),
        bwd=_sizes(ALT[1:] + ALT[:1], {3: (66, 64, 100, 257, 512), 8: (1023,), 13: (65,)}),
        order="mixed", duplicates=True, T=(3, 8)),
    "edges_small": dict(
        what="rows of 0 .. 2049 terms in small levels (one run; long rows by the 1024-thread workgroup); sorted columns, mixed order",
        fwd=_sizes([1000, 1000, 1000, 501, 502], {3: EDGE_COUNTS, 4: EDGE_COUNTS}),
        bwd=_sizes([1000, 1000, 1000, 502, 501], {3: EDGE_COUNTS, 4: EDGE_COUNTS}),
        order="mixed", sort_cols=True, T=(3,)),
    "edges_large": dict(
        what="rows of 0 .. 2049 terms in levels on their own launch (long rows by 256-thread workgroups, 1 .. 9 passes); explicit zeros, duplicates",
        fwd=_sizes([3000, 1500, 1102], {1: EDGE_COUNTS, 2: EDGE_COUNTS}),
        bwd=_sizes([3000, 1102, 1500], {1: EDGE_COUNTS, 2: EDGE_COUNTS}),
        zeros=True, duplicates=True, T=(3, 8)),
    "long_only": dict(
        what="own-launch levels: long rows only (no short-row block); exactly 256 and exactly 257 short rows plus long rows; one long row",
        fwd=[level(2100, first=True), [64 + k % 5 for k in range(1028)] + [257, 2049],
             level(256 + 800, [64 + k % 3 for k in range(800)]), level(257 + 790, [64 + k % 7 for k in range(790)]), level(1101, [64])],
        bwd=[level(2100, first=True), level(1101, [1024]), level(257 + 790, [65 + k % 2 for k in range(790)]),
             [64 + k % 4 for k in range(1030)], level(256 + 800, [64 + k % 9 for k in range(800)])],
        T=()),
    "n1": dict(what="n = 1", fwd=[[0]], bwd=[[0]], T=()),
    "diagonal": dict(what="a diagonal matrix: one level of 1500 rows without a term, on a launch of its own", fwd=_sizes([1500]), bwd=_sizes([1500]), T=()),
    "chain": dict(what="a bidiagonal chain: 3000 levels of one row", fwd=[[0]] + [[1]] * 2999, bwd=[[0]] + [[1]] * 2999, T=()),
    "dense": dict(what="a dense lower (and upper) triangle of 300 rows: row i has i terms", fwd=[[k] for k in range(300)], bwd=[[k] for k in range(300)], T=()),
}
# orc.heavy_tail(n, seed=3, cap=9000) at HEAVY_N rows: the first two levels of the forward sweep on L (2302 and 1270 rows) and of the
# backward sweep on U (2301 and 1250) exceed 1024 rows, asserted in tests/test_ssor_cpu.py; at the n = 3000 of tests/test_ssor_gpu.py
# no level does
HEAVY_N = 12000
SPECIAL = dict(fwd=_sizes([3000, 1100, 300, 200], {1: (64, 300)}), bwd=_sizes([3000, 1100, 300, 200], {1: (65,)}))

_cache = {}


def system(name):
    """{"A1", "A2": (ptr, idx, val), "b": rhs} of a catalogue case or "heavy"; built once"""
    if name in _cache:
        return _cache[name]
    if name == "heavy":
        import orc
        A = orc.heavy_tail(HEAVY_N, seed=3, cap=9000)
        out = {"A1": A, "b": np.random.default_rng(11).uniform(-1, 1, HEAVY_N)}
    else:
        c = CASES[name]
        seed = sorted(CASES).index(name) * 10
        opts = dict(sort_cols=c.get("sort_cols", False), duplicates=c.get("duplicates", False), order=c.get("order", "level"))
        pf, pb = pattern(c["fwd"], seed + 1, **opts), pattern(c["bwd"], seed + 2, **opts)
        A1, A2 = matrices(pf, pb, seed + 3, sort_cols=opts["sort_cols"], zeros=c.get("zeros", False))
        out = {"A1": A1, "A2": A2, "b": np.random.default_rng(seed + 4).uniform(-1, 1, len(pf))}
    _cache[name] = out
    return out


# ---------------------------------------------------------------- special values
def special_system():
    """One zero diagonal entry (WD = +inf there) and inf, NaN, -0.0 and denormals in b, on a shallow matrix of few terms a row.  The
    poisoned rows are rows that exactly one other row reads (in L and U together) and that read at most three: little depends on
    them, so most of every result stays finite (asserted in tests/test_ssor_cpu.py)."""
    if "special" in _cache:
        return _cache["special"]
    pf, pb = pattern(SPECIAL["fwd"], 71), pattern(SPECIAL["bwd"], 72)
    n = len(pf)
    (ptr, idx, val), _ = matrices(pf, pb, 73)
    readers = np.bincount(idx, minlength=n) - 1                    # minus the diagonal entry
    length = np.diff(ptr) - 1
    quiet = np.flatnonzero((readers == 1) & (length >= 1) & (length <= 3))
    assert len(quiet) >= 3
    picks = quiet[[len(quiet) // 5, len(quiet) // 2, (4 * len(quiet)) // 5]]
    A1, A2 = matrices(pf, pb, 73, zero_diag={int(picks[0])})
    b = np.random.default_rng(74).uniform(-1, 1, n)
    b[int(picks[1])] = np.inf
    b[int(picks[2])] = np.nan
    others = np.setdiff1d(np.arange(n), picks)
    b[others[10::400]] = -0.0
    b[others[20::400]] = 5e-324
    b[others[30::400]] = -2.5e-310
    out = {"A1": A1, "A2": A2, "b": b, "poisoned": picks}
    _cache["special"] = out
    return out


# ---------------------------------------------------------------- the same solves through a library with the Lis C API
def library_matrix(L, ptr, idx, val, expect_ok=True):
    """the matrix, split and with WD for OMEGA, as one iteration of a -p ssor solve leaves it"""
    import lisdrv
    A = lisdrv.make_csr(L, ptr, idx, val)
    n = A.contents.n
    out = lisdrv.solve(L, A, np.ones(n), "-i cg -p ssor -ssor_omega %r -maxiter 1" % OMEGA)
    if expect_ok:
        assert out["err"] == 0, out["err"]
    assert A.contents.is_splited and A.contents.WD
    return A


def library_wd(A):
    import ctypes as C
    from lis_amd import _capi as capi
    return np.ctypeslib.as_array(C.cast(A.contents.WD, C.POINTER(capi.MatrixDiag)).contents.value, shape=(A.contents.n,)).copy()


def library_solve(L, A, name, flag, b, alias=False):
    import lisdrv
    fn = getattr(L, "lis_matrix_" + name)
    vb = lisdrv.new_vector(L, A, b)
    vx = vb if alias else lisdrv.new_vector(L, A, np.full(len(b), 7.0))       # X's earlier content must not matter
    assert fn(A, vb, vx, flag) == 0
    out = lisdrv.get_vector(L, vx, A.contents.n)
    L.lis_vector_destroy(vb)
    if not alias:
        L.lis_vector_destroy(vx)
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def first_difference(got, want, nan_payload=True):
    """None when got is want in every bit, else (row, got, want) of the first row that differs.  nan_payload False: a NaN matches
    any NaN (sign and payload not compared), every other value must still match in every bit."""
    same = bits(got) == bits(want)
    if not nan_payload:
        same |= np.isnan(got) & np.isnan(want)
    bad = np.flatnonzero(~same)
    return None if bad.size == 0 else (int(bad[0]), float(got[bad[0]]), float(want[bad[0]]))
