"""Inputs for the edge tests of the five native BSR kernels (tests/test_bsr_edges_gpu.py, tests/test_bsr_cases_cpu.py).

A case is built straight from a list of block-row lengths (bsr_from_lengths): which workgroup stages which blocks, where a pass of the stage ends
and which branch a group of block rows takes all follow from the lengths, and the helpers below (rows_passes, team_groups, tile_passes) recompute
them the way the kernels of kernels/spmv_formats.hip do.  test_bsr_cases_cpu.py asserts, without a GPU, that every named case reaches the edge it
is named for.  Blocks are column-major bnr x bnc, block columns distinct and unsorted within a block row, x has nc * bnc elements.

The expected product is the oracle's over ALL nr * bnr rows (product: the padding rows of the last block row are compared too);
test_bsr_cases_cpu.py holds it to an independent numpy chain (chain) and, for every block size, to the reference.  kind_model restates the choice of
kernel that liship_spmv_bsr_kind answers, dot_model the sums of liship_spmv_bsr_dot_f64 on the tree of tests/reduction_model.py."""
import functools

import numpy as np

import orc
import reduction_model as rm
from format_cases import SENTINEL_BITS, Y_PAD, bits, sentinel, vectors            # noqa: F401  (shared with the ELL / DIA / JAD edge tests)

# ---------------------------------------------------------------- the launch constants of kernels/spmv_formats.hip
GENERIC, TILE, PAIR22, ROWS, TEAM = range(5)                # LISHIP_BSR_* (include/liship.h)
KIND_NAMES = ["generic", "tile", "pair22", "rows", "team"]
WAVE = 64
ROWS_BRW = 64                                  # :449  BSR_LANES: block rows per workgroup of spmv_bsr_rows_kernel
ROWS_CAP = {2: 512, 3: 352, 4: 160}            # :1013-1015  CAP: blocks per pass of the stage (:1065-1067 with the fused sums)
ROWS_U = {2: 8, 3: 12, 4: 8}                   # :1013-1015  U: gathers per batch
ROWS_ALIGN = 4                                 # :480  ka = cb & ~3
TEAM_RPW = 8                                   # :594  RPW = WAVE / T: block rows per wavefront of spmv_bsr_team_kernel<BS, 8, 4>
TEAM_MAX = 32                                  # :610  T * SEG: the longest block row a team holds
TEAM_ALIGN = 2                                 # :638  ka = k0 & ~1
TILE_BRW = {b: 256 // b for b in (1, 2, 3, 4)}              # :271  BRW = BLOCK / BNR
TILE_CHUNK = {b: 4096 // (b * b) for b in (1, 2, 3, 4)}     # :272  CHUNK = 4096 / BS (BS = BNR * BNC there)
TILE_UP = 4                                    # :340  UP (and :417 in spmv_bsr22_kernel)
PAIR_BRW = 128                                 # :369  BRW = BLOCK / 2
PAIR_CHUNK = 1024                              # :370  CHUNK
GENERIC_ROWS = 256                             # :249  BLOCK scalar rows per workgroup of spmv_bsr_kernel
THRESHOLD = {2: 12.0, 3: 16.0, 4: 12.0}        # :974-983, :1065-1067  mean stored blocks per block row up to which the rows kernel serves
BNNZ_SHORT, BNNZ_LONG = 0, 1 << 30             # block counts that force the short-row / the long-row side of the choice


def kind_model(nr, bnnz, bnr, bnc, team=1, bidx16=True, val16=True, x16=True, y16=True):
    """the kernel a whole-matrix launch takes: the rule of liship_spmv_bsr_nnz_f64 before it had a function of its own.  *16: is the pointer
    16 B aligned; team: liship_spmv_bsr_set_team"""
    if bnr != bnc or bnr > 4 or not val16:
        return GENERIC
    if bnr == 1:
        return TILE
    known = bnnz >= 0
    mean = bnnz / nr if known and nr > 0 else 0.0
    long_rows = known and mean > THRESHOLD[bnr]
    if bnr == 2:
        if team and long_rows:
            return TEAM
        if x16 and y16 and bidx16 and not long_rows:        # (an unknown count counts as short at 2 x 2 only)
            return ROWS
        return PAIR22 if x16 else TILE
    if bnr == 3:
        if team and long_rows:
            return TEAM
        return ROWS if bidx16 and known and not long_rows else TILE
    if team == 2 and long_rows:
        return TEAM
    return ROWS if x16 and y16 and bidx16 and known and not long_rows else TILE


def kind_grid():
    """(nr, bnnz, bnr, bnc, team, bidx16, val16, x16, y16) over block sizes 1..5 and non-square ones, block counts at and one above both thresholds,
    every team switch and every pointer on and off 16 B"""
    nr = 100
    counts = [-1, 0] + [k * nr + d for k in (12, 16) for d in (0, 1)]
    sizes = [(b, b) for b in range(1, 6)] + [(1, 2), (2, 1), (2, 3), (3, 2), (3, 4), (4, 3)]
    for bnr, bnc in sizes:
        for bnnz in counts:
            for team in (0, 1, 2):
                for al in range(16):
                    yield (nr, bnnz, bnr, bnc, team) + tuple(not (al >> k) & 1 for k in range(4))


# ---------------------------------------------------------------- generators and references
def bsr_from_lengths(lens, nc, bnr, bnc, seed):
    """bptr, bidx, val of the block rows with these numbers of blocks: block columns distinct and in random order within a row, values in [-1, 1)
    and never zero.  The arrays of a matrix without a block are one element long"""
    lens = np.asarray(lens, np.int64)
    assert lens.min(initial=0) >= 0 and lens.max(initial=0) <= nc
    rng = np.random.default_rng(seed)
    bptr = np.zeros(len(lens) + 1, np.int32)
    bptr[1:] = np.cumsum(lens)
    total = int(bptr[-1])
    if total == 0:
        return bptr, np.zeros(1, np.int32), np.zeros(1)
    bidx = np.concatenate([rng.permutation(nc)[:k] for k in lens]).astype(np.int32)
    val = rng.uniform(-1, 1, total * bnr * bnc)
    val[val == 0.0] = 0.5
    return bptr, bidx, val


def product(nr, bnr, bnc, bptr, bidx, val, x):
    """the oracle's y = A x over all nr * bnr rows (orc.spmv_bsr cuts it to n)"""
    y = np.full(nr * bnr, np.nan)
    orc.lib().orc_spmv_bsr(nr * bnr, nr, bnr, bnc, np.ascontiguousarray(bptr, np.int32), np.ascontiguousarray(bidx, np.int32),
                           np.ascontiguousarray(val, np.float64), np.ascontiguousarray(x, np.float64), y)
    return y


def chain(nr, bnr, bnc, bptr, bidx, val, x):
    """the same in numpy, independent of the oracle: one rounded product and one rounded += per term, block after block in stored order, column
    after column inside a block, onto +0.0 (the bnr rows of a block row are separate chains: one array statement adds one term to each)"""
    y = np.zeros(nr * bnr)
    with np.errstate(all="ignore"):
        for br in range(nr):
            t = np.zeros(bnr)
            for b in range(int(bptr[br]), int(bptr[br + 1])):
                blk = val[b * bnr * bnc:(b + 1) * bnr * bnc]
                for j in range(bnc):
                    t = t + blk[j * bnr:(j + 1) * bnr] * x[int(bidx[b]) * bnc + j]
            y[br * bnr:(br + 1) * bnr] = t
    return y


def make(lens, bnr, bnc, seed, nc=None):
    lens = np.asarray(lens, np.int64)
    nc = max(int(lens.max(initial=0)) + 3, 40) if nc is None else nc
    bptr, bidx, val = bsr_from_lengths(lens, nc, bnr, bnc, seed)
    x = vectors(nc * bnc, seed + 1)
    return finish(dict(nr=len(lens), nc=nc, bnr=bnr, bnc=bnc, lens=lens, bptr=bptr, bidx=bidx, val=val, x=x, bnnz=int(bptr[-1])))


def finish(c):
    c["y"] = product(c["nr"], c["bnr"], c["bnc"], c["bptr"], c["bidx"], c["val"], c["x"])
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def pool_lens(nr, pool, seed):
    """nr lengths drawn from the pool; the first rows hold the pool itself, longest first, so that a matrix of one row has the longest"""
    rng = np.random.default_rng(seed)
    lens = rng.choice(pool, nr)
    k = min(nr, len(pool))
    lens[:k] = sorted(pool, reverse=True)[:k]
    return lens


def split(total, piece=37):
    q, r = divmod(total, piece)
    return [piece] * q + ([r] if r else [])


# ---------------------------------------------------------------- what the kernels do with a bptr
def rows_passes(bptr, bs):
    """spmv_bsr_rows_kernel: per workgroup the passes of its stage -- cb, the aligned start ka, the end, the staged count, whether the lone 8 B tail
    value and whether the scalar index loop is taken"""
    nr, total, bb2, cap = len(bptr) - 1, int(bptr[-1]), bs * bs, ROWS_CAP[bs]
    out = []
    for br0 in range(0, nr, ROWS_BRW):
        bb, be = int(bptr[br0]), int(bptr[min(br0 + ROWS_BRW, nr)])
        passes = []
        for cb in range(bb, be, cap):
            ka, cend = cb & ~(ROWS_ALIGN - 1), min(cb + cap, be)
            cnt = cend - ka
            pieces, quads = (cnt * bb2 + 1) >> 1, (cnt + 3) >> 2
            passes.append(dict(cb=cb, ka=ka, cend=cend, cnt=cnt, tail=ka * bb2 + 2 * pieces > total * bb2, scalar=ka + 4 * quads > total))
        out.append(passes)
    return out


def inside_a_row(bptr, pos):
    """is the block position strictly inside a block row (no row starts there)"""
    return pos not in set(np.asarray(bptr).tolist())


def team_groups(bptr, bs):
    """spmv_bsr_team_kernel: per group of eight block rows k0, k1, ka, the branch (empty / fallback / team) and whether the lone tail value is taken"""
    nr, total, bb2 = len(bptr) - 1, int(bptr[-1]), bs * bs
    out = []
    for br0 in range(0, nr, TEAM_RPW):
        br1 = min(br0 + TEAM_RPW, nr)
        k0, k1 = int(bptr[br0]), int(bptr[br1])
        longest = int(np.diff(bptr[br0:br1 + 1]).max())
        ka = k0 & ~(TEAM_ALIGN - 1)
        pieces = ((k1 - ka) * bb2 + 1) >> 1
        out.append(dict(k0=k0, k1=k1, ka=ka, longest=longest, branch="empty" if k1 == k0 else "fallback" if longest > TEAM_MAX else "team",
                        tail=ka * bb2 + 2 * pieces > total * bb2))
    return out


def tile_passes(bptr, brw, chunk):
    """the two-phase kernels: per workgroup the (first block, blocks) of its LDS passes"""
    nr = len(bptr) - 1
    out = []
    for br0 in range(0, nr, brw):
        bb, be = int(bptr[br0]), int(bptr[min(br0 + brw, nr)])
        out.append([(cb, min(chunk, be - cb)) for cb in range(bb, be, chunk)])
    return out


# ---------------------------------------------------------------- A. the rows kernel
ROWS_NR = [1, 63, 64, 65, 129]
ROWS_SLICES = ["cap-1", "cap", "cap+1", "2cap", "2cap+3"]
ROWS_TAIL_NR = 70


def rows_pool(bs):
    u = ROWS_U[bs]
    return [0, 1, u - 1, u, u + 1, 2 * u + 1]


def slice_blocks(cap, label):
    return {"cap-1": cap - 1, "cap": cap, "cap+1": cap + 1, "2cap": 2 * cap, "2cap+3": 2 * cap + 3}[label]


def slice_front(label, border):
    """bb % 4 of the workgroup under test: the first workgroup holds 64 + r blocks"""
    return (2 * ROWS_SLICES.index(label) + (border == "between")) % 4


def rows_slice_lens(bs, label, border):
    """three workgroups: 64 block rows of 64 + r blocks, 64 block rows of exactly the slice -- its first pass border, CAP blocks in, inside the
    second block row or exactly behind it -- and three more"""
    cap, total = ROWS_CAP[bs], slice_blocks(ROWS_CAP[bs], label)
    if total <= cap:                              # one pass: there is no border
        body = split(total)
    else:
        head = [100, cap - 100] if border == "between" else [100, cap - 103]
        body = head + split(total - sum(head))
    assert len(body) <= ROWS_BRW and sum(body) == total
    return [1 + slice_front(label, border)] + [1] * 63 + body + [0] * (ROWS_BRW - len(body)) + [2, 0, 1]


def rows_tail_lens(bs, m):
    """two workgroups whose last block ends the array with bnnz % 4 == m"""
    lens = pool_lens(ROWS_TAIL_NR, rows_pool(bs), 40 + bs)
    lens[-1] = 1 + (m - 1 - int(lens[:-1].sum())) % 4
    return lens


def _rows_cases(bs):
    c = {f"nr{nr}": (lambda nr=nr: pool_lens(nr, rows_pool(bs), 10 * nr + bs)) for nr in ROWS_NR}
    for label in ROWS_SLICES:
        for border in ("inside", "between"):
            c[f"slice_{label}_{border}"] = lambda label=label, border=border: rows_slice_lens(bs, label, border)
    def long_row():
        lens = pool_lens(70, rows_pool(bs), 20 + bs)
        lens[3] = 2 * ROWS_CAP[bs] + 5
        return lens
    c["long_row"] = long_row
    for m in range(4):
        c[f"tail_{m}"] = lambda m=m: rows_tail_lens(bs, m)
    def empty_end():
        lens = pool_lens(70, rows_pool(bs), 30 + bs)
        lens[59], lens[60:] = 1, 0                # the last four block rows of the first workgroup and the whole second one
        return lens
    c["empty_end"] = empty_end
    c["no_blocks"] = lambda: np.zeros(65, np.int64)
    return c


# ---------------------------------------------------------------- B. the team kernel
TEAM_NR = [1, 7, 8, 9, 17]
TEAM_POOL = [0, 1, 3, 4, 5, 31, 32]


def _team_cases(bs):
    c = {f"nr{nr}": (lambda nr=nr: pool_lens(nr, TEAM_POOL, 11 * nr + bs)) for nr in TEAM_NR}
    def empty_group():
        lens = pool_lens(24, TEAM_POOL, 50 + bs)
        lens[8:16] = 0
        return lens
    def fallback_33():
        lens = pool_lens(24, TEAM_POOL, 51 + bs)
        lens[11] = TEAM_MAX + 1
        return lens
    def k0(odd):
        lens = pool_lens(16, TEAM_POOL, 52 + bs)
        lens[:8] = [1, 3, 4, 5, 0, 31, 32, 1 if odd else 2]
        return lens
    def end(odd):
        lens = pool_lens(16, TEAM_POOL, 53 + bs)
        lens[-1] = 3 + (int(lens[:-1].sum()) + 3 + odd) % 2
        return lens
    def trailing_empty():
        lens = pool_lens(20, TEAM_POOL, 54 + bs)
        lens[13:] = 0                             # three block rows of the second group (rs == bptr[nr]) and the whole third one
        return lens
    c.update(empty_group=empty_group, fallback_33=fallback_33, k0_odd=lambda: k0(True), k0_even=lambda: k0(False),
             end_odd=lambda: end(True), end_even=lambda: end(False), trailing_empty=trailing_empty)
    return c


# ---------------------------------------------------------------- C. the two-phase kernels
# variant: (block size, block rows per workgroup, blocks per pass)
TILE_VARIANTS = {"tile1": (1, TILE_BRW[1], TILE_CHUNK[1]), "tile2": (2, TILE_BRW[2], TILE_CHUNK[2]), "tile3": (3, TILE_BRW[3], TILE_CHUNK[3]),
                 "tile4": (4, TILE_BRW[4], TILE_CHUNK[4]), "pair22": (2, PAIR_BRW, PAIR_CHUNK)}
TILE_POOL = [0, 1, 2, 3, 5]
TILE_SLICES = {"chunk-1": -1, "chunk": 0, "chunk+1": 1}


def tile_slice_lens(brw, total):
    """a workgroup of exactly `total` blocks, lengths base +- 1 and a longer last block row, and three more block rows"""
    base, rem = divmod(total, brw)
    lens = np.full(brw, base, np.int64)
    pairs = (brw - 1) // 2
    lens[0:2 * pairs:2] += 1
    lens[1:2 * pairs:2] -= 1
    lens[-1] += rem
    assert lens.min() >= 0 and lens.sum() == total
    return np.concatenate([lens, [2, 0, 1]])


def _tile_cases(variant):
    bs, brw, chunk = TILE_VARIANTS[variant]
    c = {f"nr{nr}": (lambda nr=nr: pool_lens(nr, TILE_POOL, nr + bs)) for nr in (brw - 1, brw, brw + 1)}
    for label, d in TILE_SLICES.items():
        c[f"slice_{label}"] = lambda d=d: tile_slice_lens(brw, chunk + d)
    return c


# ---------------------------------------------------------------- D. the generic kernel
GENERIC_SHAPES = [(1, 2), (2, 1), (2, 3), (3, 2), (1, 4), (4, 1), (3, 4), (4, 3), (5, 5), (6, 2)]
GENERIC_UNALIGNED = [(2, 2), (3, 3), (4, 4)]                 # square native sizes whose values are 8 B off
GENERIC_POOL = [0, 1, 2, 3, 5, 9]


def generic_nrs(bnr):
    """block rows whose scalar rows end just below, at (where bnr divides) and just above one workgroup of 256"""
    return sorted({(GENERIC_ROWS - 1) // bnr, -(-GENERIC_ROWS // bnr), -(-(GENERIC_ROWS + 1) // bnr)})


# ---------------------------------------------------------------- F / H. one configuration per kind
# name: block size, the count and team switch that force the kind, element shifts of the arrays, the kind, block rows per workgroup
KIND_CONFIGS = {
    "rows2": dict(bs=(2, 2), bnnz=BNNZ_SHORT, team=1, shift={}, kind=ROWS, wg=ROWS_BRW),
    "rows3": dict(bs=(3, 3), bnnz=BNNZ_SHORT, team=1, shift={}, kind=ROWS, wg=ROWS_BRW),
    "rows4": dict(bs=(4, 4), bnnz=BNNZ_SHORT, team=1, shift={}, kind=ROWS, wg=ROWS_BRW),
    "team2": dict(bs=(2, 2), bnnz=BNNZ_LONG, team=1, shift={}, kind=TEAM, wg=TEAM_RPW),
    "team3": dict(bs=(3, 3), bnnz=BNNZ_LONG, team=1, shift={}, kind=TEAM, wg=TEAM_RPW),
    "team4": dict(bs=(4, 4), bnnz=BNNZ_LONG, team=2, shift={}, kind=TEAM, wg=TEAM_RPW),
    "tile1": dict(bs=(1, 1), bnnz=BNNZ_LONG, team=0, shift={}, kind=TILE, wg=TILE_BRW[1]),
    "tile2": dict(bs=(2, 2), bnnz=BNNZ_LONG, team=0, shift={"x": 1}, kind=TILE, wg=TILE_BRW[2]),
    "tile3": dict(bs=(3, 3), bnnz=BNNZ_LONG, team=0, shift={}, kind=TILE, wg=TILE_BRW[3]),
    "tile4": dict(bs=(4, 4), bnnz=BNNZ_LONG, team=0, shift={}, kind=TILE, wg=TILE_BRW[4]),
    "pair22_y": dict(bs=(2, 2), bnnz=BNNZ_LONG, team=0, shift={"y": 1}, kind=PAIR22, wg=PAIR_BRW),
    "pair22_bidx": dict(bs=(2, 2), bnnz=BNNZ_SHORT, team=0, shift={"bidx": 1}, kind=PAIR22, wg=PAIR_BRW),
    "generic23": dict(bs=(2, 3), bnnz=BNNZ_SHORT, team=1, shift={}, kind=GENERIC, wg=GENERIC_ROWS // 2),
    "generic33_val": dict(bs=(3, 3), bnnz=BNNZ_SHORT, team=1, shift={"val": 1}, kind=GENERIC, wg=GENERIC_ROWS // 3),
}


def config_kind(cfg, nr):
    s = cfg["shift"]
    return kind_model(nr, cfg["bnnz"], *cfg["bs"], team=cfg["team"], bidx16=s.get("bidx", 0) % 4 == 0, val16=s.get("val", 0) % 2 == 0,
                      x16=s.get("x", 0) % 2 == 0, y16=s.get("y", 0) % 2 == 0)


def range_partitions(nr, wg):
    """label -> block-row ranges that cover [0, nr) in the order a multi-rank product runs them (the interior first)"""
    cut = wg // 2 + 3
    return {"at_a_workgroup_border": [(wg, 2 * wg), (0, wg), (2 * wg, nr)],
            "inside_a_workgroup": [(cut, wg + cut), (0, cut), (wg + cut, nr)],
            "an_empty_range_between": [(0, cut), (cut, cut), (cut, nr)],
            "single_block_rows": [(b, b + 1) for b in range(nr)]}


BORDER_NR = 100                                # the matrix of the issue: one block more than the threshold allows on average


# ---------------------------------------------------------------- G. the fused sums
DOT_NR = [1, 64, 65, 200]


def dot_lens(bs, nr, over=0):
    """block rows whose mean length is exactly the threshold of the rows kernel (+ `over` blocks in the last one)"""
    t = int(THRESHOLD[bs])
    lens = np.full(nr, t, np.int64)
    pairs = nr // 2
    lens[0:2 * pairs:2] += 3
    lens[1:2 * pairs:2] -= 3
    lens[-1] += over
    return lens


@rm._quiet
def dot_model(bs, nr, n, w, y, sumsq):
    """result[0] (sumsq: result[1]) of liship_spmv_bsr_dot_f64 as the epilogue of spmv_bsr_rows_kernel forms it: lane L of workgroup g owns block
    row 64 g + L and chains 0.0 + w[r] * y[r] over its bs rows (a row at or beyond n, and every row of a lane without a block row, adds +0.0); the
    64 lanes go through wave_sum, the workgroups' partials through fold"""
    grid = (nr + ROWS_BRW - 1) // ROWS_BRW
    rows = grid * ROWS_BRW * bs
    a, b = np.zeros(rows), np.zeros(rows)
    b[:nr * bs] = y[:nr * bs]
    if sumsq:
        a[:] = b
    else:
        a[:n] = w[:n]
    ok = (np.arange(rows) < n).reshape(grid, ROWS_BRW, bs)
    a, b = a.reshape(grid, ROWS_BRW, bs), b.reshape(grid, ROWS_BRW, bs)
    c = np.zeros((grid, ROWS_BRW))
    for i in range(bs):
        c = c + np.where(ok[:, :, i], a[:, :, i] * b[:, :, i], 0.0)
    return rm.fold(rm.wave_sum(c))


# ---------------------------------------------------------------- H. special values
SPECIAL_NR = 24
SPECIAL_VARIANTS = ["inf_nan", "negative_zero", "denormal"]


def special_case(bnr, bnc, variant):
    """24 block rows of five blocks.  inf_nan: block row 8 holds an Inf, 9 is empty, 10 holds NaN only (one team group: the clamped slots of the
    empty row read block row 8's last block); the first block of block row 3 has a zero column that meets x = Inf.  negative_zero: every product is
    -0.0.  denormal: values scaled by 2^-1025 .. 2^-1040 against x of order one"""
    lens = np.full(SPECIAL_NR, 5, np.int64)
    lens[9] = 0
    nc, bb = 40, bnr * bnc
    bptr, bidx, val = bsr_from_lengths(lens, nc, bnr, bnc, 70 + bnr * 5 + bnc)
    x = vectors(nc * bnc, 71)
    if variant == "inf_nan":
        val[int(bptr[8]) * bb + bb - 1] = np.inf
        val[int(bptr[10]) * bb:int(bptr[11]) * bb] = np.nan
        b = int(bptr[3])
        val[b * bb:b * bb + bnr] = 0.0                       # column 0 of the block: explicit zeros
        x[int(bidx[b]) * bnc] = np.inf
    elif variant == "negative_zero":
        val, x = -np.abs(val) - 0.5, np.zeros(nc * bnc)
    else:
        val = val * 2.0 ** -np.random.default_rng(72).integers(1025, 1041, len(val))
    return finish(dict(nr=SPECIAL_NR, nc=nc, bnr=bnr, bnc=bnc, lens=lens, bptr=bptr, bidx=bidx, val=val, x=x, bnnz=int(bptr[-1])))


# ---------------------------------------------------------------- the registry
FAMILIES = {f"rows{bs}": (bs, _rows_cases(bs)) for bs in (2, 3, 4)}
FAMILIES.update({f"team{bs}": (bs, _team_cases(bs)) for bs in (2, 3, 4)})
FAMILIES.update({v: (TILE_VARIANTS[v][0], _tile_cases(v)) for v in TILE_VARIANTS})


def names(family):
    return list(FAMILIES[family][1])


@functools.lru_cache(maxsize=None)
def case(family, name):
    bs, builders = FAMILIES[family]
    return make(builders[name](), bs, bs, seed=sum(map(ord, family + name)))


@functools.lru_cache(maxsize=None)
def generic_case(bnr, bnc, nr):
    return make(pool_lens(nr, GENERIC_POOL, 7 * nr + bnr), bnr, bnc, seed=100 * bnr + 10 * bnc + nr, nc=12)


@functools.lru_cache(maxsize=None)
def align_case(bs):
    return make(np.random.default_rng(bs).integers(0, 21, 130), bs, bs, seed=90 + bs)


@functools.lru_cache(maxsize=None)
def range_case(config):
    cfg = KIND_CONFIGS[config]
    nr = 2 * cfg["wg"] + 9
    return make(np.random.default_rng(nr).integers(0, 10, nr), *cfg["bs"], seed=200 + nr)


@functools.lru_cache(maxsize=None)
def border_case(bs):
    lens = np.full(BORDER_NR, int(THRESHOLD[bs]), np.int64)
    lens[57] += 1
    return make(lens, bs, bs, seed=300 + bs)


@functools.lru_cache(maxsize=None)
def dot_case(bs, nr, over=0):
    c = dict(make(dot_lens(bs, nr, over), bs, bs, seed=400 + 10 * nr + bs))
    c["w"] = vectors(nr * bs, 401 + nr)
    c["w"].setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def dot_padding_case(bs):
    """65 block rows at the threshold whose LAST scalar row holds an Inf: with n = 65 bs - 1 that row is padding, y there is infinite, and a sum
    that took its term 0.0 * Inf in would be NaN"""
    nr = 65
    c = dict(dot_case(bs, nr))
    val = c["val"].copy()
    val[(c["bnnz"] - 1) * bs * bs + bs - 1] = np.inf                          # column 0, row bs - 1 of the last block
    c["val"] = val
    return finish(c)
