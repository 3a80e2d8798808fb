"""Inputs for the edge tests of the native ELL / DIA / JAD kernels (tests/test_formats_edges_gpu.py, tests/test_format_cases_cpu.py).

Generators are deterministic and vectorised; arrays are int32 / float64 in the layouts of kernels/spmv_formats.hip (ELL and DIA column-major:
slot j of row r at j * n + r).  Each case is built to reach one branch of that file which a column-sorted stencil launched whole never reaches;
where a case rests on a fact about its arrays (a jagged diagonal really starts on an odd element, exactly half of the rows reach the band, a
launch shape does or does not meet the three conditions of fmt_plane) a helper below states the fact, and test_format_cases_cpu.py asserts it.

The expected products are orc.spmv_ell / spmv_dia / spmv_jad, which test_oracle_vs_ref.py pins to the reference.  Two things have no oracle
entry: DIA with ghost columns (ncols > n) and the plane liship_ell_scan_band reports.  dia_reference and scan_band_reference restate them;
test_format_cases_cpu.py holds the first to orc.spmv_dia bit for bit on square matrices."""
import functools

import numpy as np

import orc

# what y holds before a launch: a NaN no product can produce (0 * inf gives the default NaN, a NaN of x keeps x's payload)
SENTINEL_BITS = np.uint64(0x7FF80000DEADBEEF)
Y_PAD = 5                                      # elements of y behind the last row: a launch must leave them alone
BLOCK = 256                                    # lanes of a workgroup (spmv_formats.hip)
WG_ROWS = 2 * BLOCK                            # rows of a workgroup of the pair kernels


def sentinel(count):
    return np.full(count, SENTINEL_BITS, np.uint64).view(np.float64)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def vectors(n, seed, count=1):
    rng = np.random.default_rng(seed)
    out = [rng.uniform(-1, 1, n) for _ in range(count)]
    return out[0] if count == 1 else out


# ---------------------------------------------------------------- A. XCD strips
# name: (grid of the 7-point stencil, rows per plane handed to liship_spmv_formats_set_plane, does fmt_plane engage)
STRIP_SHAPES = {
    "four_whole_planes": ((32, 64, 64), 32768, True),        # n = 131072: grid == full
    "tail_past_full": ((37, 64, 63), 32768, True),           # n = 149184: 36 workgroups past full in natural order, the last one partial
    "plane_of_72": ((60, 50, 50), 36864, True),              # n = 150000: pb = 72, a plane that is no power of two
    "too_few_planes": ((52, 50, 50), 32768, False),          # n = 130000: 254 workgroups < 4 planes of 64
    "plane_of_65": ((37, 64, 63), 33280, False),             # pb = 65: no multiple of 8
    "plane_of_63": ((37, 64, 63), 32256, False),             # pb = 63: below 64 (and no multiple of 8)
    "odd_n": ((25, 49, 107), 32768, False),                  # n = 131075: one row per lane, a launch that is never given a plane
}


def pair_grid(n):
    """workgroups of a whole-matrix launch of the pair kernels"""
    return (n // 2 + BLOCK - 1) // BLOCK


def plane_conditions(plane_rows, n):
    """the three conditions of fmt_plane(WG_ROWS, pair_grid(n)): whole workgroups per plane, pb >= 64 and a multiple of 8, at least four planes"""
    pb = plane_rows // WG_ROWS
    return plane_rows % WG_ROWS == 0, pb >= 64 and pb % 8 == 0, 4 * pb <= pair_grid(n)


def plane_blocks(plane_rows, n):
    """what liship_spmv_formats_plane_blocks(WG_ROWS, pair_grid(n)) must return with plane_rows set"""
    return plane_rows // WG_ROWS if plane_rows > 0 and all(plane_conditions(plane_rows, n)) else 0


def launch_plane(plane_rows, n):
    """the plane the whole-matrix launch of an n-row matrix is given: an odd n takes the one-row-per-lane kernel, which is never given one --
    whatever the getter would answer for a pair launch of that size"""
    return 0 if n % 2 else plane_blocks(plane_rows, n)


def strip_unit(w, grid, plane):
    """fmt_strip_unit restated (w: array of workgroup numbers): the unit each workgroup of the launch works on"""
    w = np.asarray(w, np.int64)
    if plane <= 0:
        return w
    full = (grid // plane) * plane
    sb, xcd, slot = plane >> 3, w & 7, w >> 3
    pl = slot // sb
    return np.where(w >= full, w, pl * plane + xcd * sb + (slot - pl * sb))


@functools.lru_cache(maxsize=4)
def strip_matrix(dims):
    """the 7-point stencil of the grid with varying coefficients as ELL and DIA arrays, x, w and the oracle's products"""
    ptr, idx, val = orc.poisson3d(*dims, sort_cols=True)
    n = len(ptr) - 1
    rng = np.random.default_rng(dims[0] * 131 + dims[2])
    val = val * rng.uniform(0.5, 1.5, len(val))
    x, w = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    mx, eidx, ev = orc.csr2ell(ptr, idx, val)
    nnd, off, dv = orc.csr2dia(ptr, idx, val)
    case = dict(n=n, x=x, w=w, mx=mx, eidx=eidx, ev=ev, y_ell=orc.spmv_ell(n, mx, eidx, ev, x),
                nnd=nnd, off=off, dv=dv, y_dia=orc.spmv_dia(n, nnd, off, dv, x))
    for a in case.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return case


# ---------------------------------------------------------------- B. row ranges
RANGE_N = {"even": 1800, "odd": 1801}
RANGE_OFFSETS = {7: [0, -300, -17, -1, 1, 17, 300], 9: [0, -300, -40, -17, -1, 1, 17, 40, 300]}      # the diagonal first: stored order is not column order
GHOST = 37                                     # ghost columns of the DIA cases: ncols = n + GHOST


def ghost_offsets(n, slots):
    """offsets of a DIA matrix of n rows and n + GHOST columns that reach into the ghost columns three ways: 30 (the last 30 rows, all inside),
    50 (the last 13 rows fall past ncols: row n - 14 reads the LAST column) and n + 5 (only the first 32 rows are inside)"""
    base = [0, -300, -1, 1, 30, 50, n + 5]
    return base if slots == 7 else base + [-(n - 2), 17]


def banded(n, offsets, seed, ncols=None):
    """CSR rows with one entry on each of the given diagonals that falls inside the matrix, in the given order"""
    ncols = n if ncols is None else ncols
    rng = np.random.default_rng(seed)
    cols = np.arange(n, dtype=np.int64)[:, None] + np.asarray(offsets, np.int64)[None, :]
    inside = (cols >= 0) & (cols < ncols)
    ptr = np.zeros(n + 1, np.int32)
    ptr[1:] = np.cumsum(inside.sum(axis=1))
    idx = cols[inside].astype(np.int32)
    return ptr, idx, rng.uniform(-1, 1, len(idx))


def dia_arrays(n, offsets, seed, ncols=None):
    """DIA arrays with the diagonals in the given stored order: random values where the diagonal is inside the n x ncols matrix, 0.0 outside
    (what the reference's conversion leaves there)"""
    ncols = n if ncols is None else ncols
    rng = np.random.default_rng(seed)
    off = np.asarray(offsets, np.int32)
    cols = np.arange(n, dtype=np.int64)[None, :] + off.astype(np.int64)[:, None]
    val = np.where((cols >= 0) & (cols < ncols), rng.uniform(-1, 1, cols.shape), 0.0)
    return off, np.ascontiguousarray(val.ravel())


def dia_reference(n, ncols, off, val, x):
    """y = A x for DIA arrays of an n x ncols matrix: diagonal after diagonal in stored order, every term one rounded product and one rounded
    sum onto +0.0 (lis_matvec_dia.c:148-172 with the column bound at ncols; numpy's multiply and add are separate roundings)"""
    v = np.asarray(val).reshape(len(off), n) if len(off) else np.zeros((0, n))
    y = np.zeros(n)
    for d, o in enumerate(np.asarray(off).tolist()):
        lo, hi = max(0, -o), min(n, ncols - o)
        if lo < hi:
            y[lo:hi] += v[d, lo:hi] * x[lo + o:hi + o]
    return y


def pair_range(n, rb, re):
    """does the dispatcher of the row-range entries take the two-rows-per-lane kernel (aligned arrays given)"""
    return n % 2 == 0 and rb % 2 == 0 and (re - rb) % 2 == 0


def row_ranges(n):
    """label -> (rb, re): every parity of start and length, the cuts around one and two workgroups of one-row lanes, the ends"""
    k = 2 * (n // 5)
    r = {"empty_at_0": (0, 0), "empty_at_k": (k, k), "empty_at_n": (n, n), "whole": (0, n),
         "even_start_even_length": (k, k + 1026),               # 513 pairs: three workgroups, the last one a single lane
         "one_workgroup_of_pairs": (256, 768),
         "even_start_odd_length": (k, k + 777),
         "odd_start_even_length": (k + 1, k + 1027),
         "odd_start_odd_length": (k + 1, k + 778),
         "single_row_even": (k, k + 1), "single_row_odd": (k + 1, k + 2), "first_row": (0, 1), "last_row": (n - 1, n),
         "last_two_rows": (n - 2, n)}
    for c in (255, 256, 257, 511, 512, 513):
        r[f"head_to_{c}"] = (0, c)
        r[f"tail_from_{c}"] = (c, n)
    return r


def partitions(n):
    """three-way partitions as a multi-rank product runs them: the interior first, then the head and the tail"""
    return {"even_cuts": [(512, n - 300 - n % 2), (0, 512), (n - 300 - n % 2, n)],
            "odd_cuts": [(257, n - 301 + n % 2), (0, 257), (n - 301 + n % 2, n)]}


@functools.lru_cache(maxsize=None)
def range_ell(parity, slots):
    n = RANGE_N[parity]
    ptr, idx, val = banded(n, RANGE_OFFSETS[slots], seed=slots * 10 + n % 2)
    mx, eidx, ev = orc.csr2ell(ptr, idx, val)
    x = vectors(n, 77 + slots)
    return dict(n=n, mx=mx, eidx=eidx, ev=ev, x=x, y=orc.spmv_ell(n, mx, eidx, ev, x))


@functools.lru_cache(maxsize=None)
def range_dia(parity, slots, ghost):
    n = RANGE_N[parity]
    ncols = n + GHOST if ghost else n
    off, dv = dia_arrays(n, ghost_offsets(n, slots) if ghost else RANGE_OFFSETS[slots], seed=slots * 10 + n % 2 + 5, ncols=ncols)
    x = vectors(ncols, 78 + slots)
    y = dia_reference(n, ncols, off, dv, x) if ghost else orc.spmv_dia(n, len(off), off, dv, x)
    return dict(n=n, ncols=ncols, nnd=len(off), off=off, dv=dv, x=x, y=y)


# ---------------------------------------------------------------- C. whole-launch edges of ELL and DIA
EDGE_N = [1, 2, 3, 511, 512, 513, 514]
EDGE_SLOTS = [0, 1, 7, 8, 9, 16, 17]           # the kernels take 8 slots per batch: below, at and above one and two batches


def ell_random(n, maxnzr, seed):
    """ELL arrays with rows of 0 .. maxnzr random columns; the padding slots of a row hold (row, +0.0) as the reference's conversion writes
    them.  The last row is full; with three or more rows, row 1 is all padding."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, maxnzr + 1, n)
    lens[n - 1] = maxnzr
    if n >= 3:
        lens[1] = 0
    real = np.arange(maxnzr)[:, None] < lens[None, :]
    idx = np.where(real, rng.integers(0, n, (maxnzr, n)), np.arange(n)[None, :]).astype(np.int32)
    val = np.where(real, rng.uniform(-1, 1, (maxnzr, n)), 0.0)
    return np.ascontiguousarray(idx.ravel()), np.ascontiguousarray(val.ravel()), lens


def dia_random(n, nnd, seed):
    """DIA arrays with nnd random offsets inside the matrix, in random stored order (distinct while the matrix has that many diagonals)"""
    rng = np.random.default_rng(seed)
    inside = np.arange(-(n - 1), n)
    off = rng.choice(inside, nnd, replace=nnd > len(inside))
    return dia_arrays(n, off, seed + 1)


def ell_padding_meets_inf(n=514, maxnzr=9, seed=31):
    """x holds inf and NaN at rows that HAVE padding slots: 0.0 * inf is NaN in the reference's loop, and must be here.  Returns the arrays,
    x and the rows in question"""
    idx, val, lens = ell_random(n, maxnzr, seed)
    x = vectors(n, seed + 1)
    padded = np.flatnonzero(lens < maxnzr)
    rows = padded[[0, 1, len(padded) // 2, -1]]
    x[rows] = [np.inf, -np.inf, np.nan, np.inf]
    return idx, val, x, rows


def dia_outside(n):
    """diagonals wholly outside the matrix (|o| >= n) among real ones, and the two corner diagonals of one element each"""
    return dia_arrays(n, [n, 0, -(n - 1), -n, 3, n - 1, n + 5, -(n + 300), -2], seed=n)


def dia_masked_leak(n=514):
    """The kernel loads x[r] -- r the lane's first row -- for a slot that falls outside the matrix and must discard the product.  Rows 0, 1, n - 2
    and n - 1 have such slots (offsets -3 and 2, 5) with 0.0 stored there, x = inf in all four (so that r is one of them whether a lane owns one
    row or two) and finite in-range terms: there is no diagonal of offset 0.  The six rows that READ an inf are not the point.  Returns off,
    val, x and the four rows that must stay finite"""
    off, val = dia_arrays(n, [-3, 2, 5], seed=17)
    x = vectors(n, 18)
    rows = np.array([0, 1, n - 2, n - 1])
    x[rows] = np.inf
    return off, val, x, rows


def all_products_negative_zero(val, count):
    """values and an x that make every product of every row -0.0 (or the +0.0 of a padding slot): the sums start at +0.0 and end there"""
    return -np.abs(val) - 0.5, np.zeros(count)


# ---------------------------------------------------------------- D. JAD
JAD_N = [1, 2, 3, 511, 512, 513]
JAD_SLOTS = [0, 1, 7, 8, 9, 17]


def csr_from_lengths(lens, ncols, seed):
    lens = np.asarray(lens, np.int64)
    rng = np.random.default_rng(seed)
    ptr = np.zeros(len(lens) + 1, np.int32)
    ptr[1:] = np.cumsum(lens)
    return ptr, rng.integers(0, ncols, int(ptr[-1])).astype(np.int32), rng.uniform(-1, 1, int(ptr[-1]))


def jad_lengths(kind, n=513, maxnzr=9):
    """row lengths of the named JAD case"""
    rng = np.random.default_rng(n * 100 + maxnzr)
    if kind == "random":                          # 0 .. maxnzr entries, one full row, empty rows (they end the permutation)
        lens = rng.integers(0, maxnzr + 1, n)
        lens[n // 2] = maxnzr
        if n >= 3:
            lens[0] = 0
        return lens
    if kind == "equal":                           # every jagged diagonal has n entries
        return np.full(n, maxnzr)
    if kind == "odd_starts":                      # an odd number of rows reaches each of the later jagged diagonals
        lens = np.full(n, 1)
        lens[: 2 * (n // 4) + 1] = 3
        lens[: 2 * (n // 8) + 1] = maxnzr
        return lens
    if kind == "one_long_row":                    # every other lane leaves the batches early, one goes on for 38 of them
        lens = rng.integers(0, 6, n)
        lens[n // 3] = 300
        return lens
    if kind == "descending":                      # distinct lengths already in order: the permutation is the identity
        return np.arange(n, 0, -1)
    if kind == "ascending":                       # ... and its reverse
        return np.arange(1, n + 1)
    raise KeyError(kind)


JAD_NAMED = {"equal_512": ("equal", 512, 9), "equal_513": ("equal", 513, 8), "odd_starts_513": ("odd_starts", 513, 9),
             "odd_starts_512": ("odd_starts", 512, 17), "one_long_row": ("one_long_row", 513, 300),
             "descending_67": ("descending", 67, 67), "ascending_67": ("ascending", 67, 67)}


def jad_case(kind, n, maxnzr):
    lens = jad_lengths(kind, n, maxnzr)
    ptr, idx, val = csr_from_lengths(lens, n, seed=n * 31 + maxnzr)
    mx, perm, jptr, jidx, jval = orc.csr2jad(ptr, idx, val)
    x = vectors(n, n + maxnzr)
    return dict(n=n, mx=mx, perm=perm, jptr=jptr, jidx=jidx, jval=jval, x=x, lens=lens,
                y=orc.spmv_jad(n, mx, perm, jptr, jidx, jval, x))


# ---------------------------------------------------------------- E. liship_ell_scan_band and the diagonals
def scan_band_reference(n, maxnzr, idx):
    """the plane liship_ell_scan_band reports: the largest |c - r| over the slots with an owned column (0 <= c < n) when at least half of the
    rows have a slot at that distance, else 0"""
    if n <= 0 or maxnzr <= 0:
        return 0
    c = np.asarray(idx, np.int64).reshape(maxnzr, n)
    dist = np.where((c >= 0) & (c < n), np.abs(c - np.arange(n)[None, :]), 0)
    band = int(dist.max())
    reach = int((dist == band).any(axis=0).sum())
    return band if band > 0 and 2 * reach >= n else 0


def band_half(n, band, rows, ghosts=False):
    """ELL index array of three slots: the row itself, r + band in the first `rows` rows (padding elsewhere) and r - 1.  With ghosts, a
    fourth slot of columns n + 5 + r and a fifth of -1 - r: further away than the band, and not owned"""
    assert rows + band <= n
    r = np.arange(n)
    slots = [r, np.where(r < rows, r + band, r), np.maximum(r - 1, 0)]
    if ghosts:
        slots += [n + 5 + r, -1 - r]
    return len(slots), np.ascontiguousarray(np.concatenate(slots).astype(np.int32))


def rows_reaching(n, maxnzr, idx, band):
    c = np.asarray(idx, np.int64).reshape(maxnzr, n)
    return int((((c >= 0) & (c < n)) & (np.abs(c - np.arange(n)[None, :]) == band)).any(axis=0).sum())


def diagonal_cases():
    """name -> column-sorted CSR for the diagonal kernels"""
    n = 1000
    cases = {"stencil": orc.poisson3d(9, 8, 7, sort_cols=True)}
    ptr, idx, val = banded(n, [-5, -1, 0, 2, 7], seed=3)
    keep = ~((idx == np.repeat(np.arange(n), np.diff(ptr))) & (np.repeat(np.arange(n), np.diff(ptr)) % 3 == 0))
    lens = np.add.reduceat(keep.astype(np.int64), ptr[:-1])
    p2 = np.zeros(n + 1, np.int32)
    p2[1:] = np.cumsum(lens)
    cases["every_third_row_lacks_it"] = (p2, idx[keep], val[keep])
    cases["no_diagonal_at_all"] = banded(n, [-5, -1, 2, 7], seed=4)
    # lower-triangular rows end in their diagonal; every fourth row is longer, so the others have padding right behind the diagonal
    lower = banded(n, [-3, -1, 0], seed=5)
    rows = np.repeat(np.arange(n), np.diff(lower[0]))
    extra = np.arange(0, n - 9, 4)
    order = np.argsort(np.concatenate([rows, extra, extra]), kind="stable")
    idx3 = np.concatenate([lower[1], extra + 2, extra + 9]).astype(np.int32)[order]
    val3 = np.concatenate([lower[2], np.full(len(extra), 0.25), np.full(len(extra), -0.75)])[order]
    p3 = np.zeros(n + 1, np.int32)
    p3[1:] = np.cumsum(np.bincount(np.concatenate([rows, extra, extra]), minlength=n))
    cases["diagonal_in_the_last_real_slot"] = (p3, idx3, val3)
    return cases
