"""The five native BSR kernels (kernels/spmv_formats.hip) at the edges their stages, teams, ranges and launches have, bit for bit against the oracle.

Kernel level (include/liship.h through lis_amd.load()).  What test_kernels_gpu.py leaves out: the pass borders of the LDS stages (CAP, CHUNK) and their
aligned starts, the limit of a team (32 / 33 blocks), the group of block rows without a block, the scalar fallbacks at the end of the arrays,
non-square and larger blocks, every alignment fallback of the dispatcher, block-row ranges, the fused <w,y> / <y,y> sums on the tree model, and
what a launch must NOT write.

Every comparison is on the 64 bits of each element, over all nr * bnr rows (the padding rows of the last block row included).  y is prefilled with
a NaN that no product can produce and is longer than a launch may write, in front and behind (gpu_arrays.Out): rows a launch must not touch must still
hold it.  Before every launch the test asks liship_spmv_bsr_kind which kernel the arguments get and holds the answer to bsr_cases.kind_model and to
the kind the case is written for; after it liship_spmv_bsr_last_kind must name the same one -- a case cannot drift to another kernel.  The inputs and
the facts they rest on are in tests/bsr_cases.py and asserted without a GPU in tests/test_bsr_cases_cpu.py."""
import numpy as np
import pytest

import bsr_cases as bc
import lis_amd
from gpu_arrays import Out, dev
from lis_amd import DeviceArray as DA, check

pytestmark = pytest.mark.gpu
ERR_ARG = -1                                    # LISHIP_ERR_ARG
FRONT = 2                                       # sentinel elements in front of y (16 B: the alignment stays)


@pytest.fixture(scope="module")
def lib():
    lib = lis_amd.load()
    assert lis_amd.gpu_available(), "no HIP device: the product path has no CPU fallback"
    return lib


@pytest.fixture(autouse=True)
def switches_back(lib):
    yield
    lib.liship_spmv_bsr_set_team(1)
    lib.liship_krylov_guard(None)
    lib.liship_set_reference_reductions(0)


def on16(p):
    return p % 16 == 0


class Mat:
    """the arrays of a case in HBM, each `shift[name]` elements behind an aligned address, and its y"""

    def __init__(self, c, shift=None):
        s = shift or {}
        self.c, self.nr, self.bnr, self.bnc = c, c["nr"], c["bnr"], c["bnc"]
        self.keep = [dev(c["bptr"], np.int32), dev(c["bidx"], np.int32, s.get("bidx", 0)), dev(c["val"], np.float64, s.get("val", 0)),
                     dev(c["x"], np.float64, s.get("x", 0))]
        self.bptr, self.bidx, self.val, self.x = (p for _, p in self.keep)
        self.y = Out(self.nr * self.bnr, FRONT + s.get("y", 0))

    def kind(self, lib, bnnz, team, yp):
        """the kernel these arguments get: the library's answer, held to the model"""
        model = bc.kind_model(self.nr, bnnz, self.bnr, self.bnc, team, on16(self.bidx), on16(self.val), on16(self.x), on16(yp))
        got = lib.liship_spmv_bsr_kind(self.nr, bnnz, self.bnr, self.bnc, self.bidx, self.val, self.x, yp)
        assert got == model, ("kind", bc.KIND_NAMES[model], got)
        return got

    def run(self, lib, bnnz, team, kind=None, rows=None):
        """the whole product, or block rows [rows[0], rows[1]) of it, on the kernel `kind` (None: whatever the model says); returns the kind"""
        check(lib.liship_spmv_bsr_set_team(team))
        brb, bre = rows or (0, self.nr)
        got = self.kind(lib, bnnz, team, self.y.ptr + 8 * brb * self.bnr)
        if kind is not None:
            assert got == kind, ("the case is written for", bc.KIND_NAMES[kind], "and would run", bc.KIND_NAMES[got])
        if rows is None:
            check(lib.liship_spmv_bsr_nnz_f64(self.nr, bnnz, self.bnr, self.bnc, self.bptr, self.bidx, self.val, self.x, self.y.ptr, None))
        else:
            check(lib.liship_spmv_bsr_rows_f64(self.nr, bnnz, self.bnr, self.bnc, self.bptr, self.bidx, self.val, self.x, self.y.ptr, brb, bre, None))
        if brb < bre:
            assert lib.liship_spmv_bsr_last_kind() == got, ("launched", lib.liship_spmv_bsr_last_kind(), "chosen", got)
        check(lib.liship_spmv_bsr_set_team(1))
        return got


def whole(lib, c, bnnz, team, kind, what, shift=None, special=False):
    m = Mat(c, shift)
    m.run(lib, bnnz, team, kind)
    m.y.holds(c["y"], what, special=special)


# ---------------------------------------------------------------- the choice of the kernel
def test_kind_query_is_the_model(lib):
    """liship_spmv_bsr_kind over block sizes 1..5 and non-square ones, counts at and one above both thresholds (and unknown, and 0), the team
    switch at 0 / 1 / 2 and each of the four pointers on and off 16 B: the rule the dispatcher had before the choice got a function of its own"""
    base = DA(8, np.float64)
    grid = list(bc.kind_grid())
    for nr, bnnz, bnr, bnc, team, bidx16, val16, x16, y16 in grid:
        check(lib.liship_spmv_bsr_set_team(team))
        got = lib.liship_spmv_bsr_kind(nr, bnnz, bnr, bnc, base.ptr + (0 if bidx16 else 4), base.ptr + (0 if val16 else 8),
                                       base.ptr + (0 if x16 else 8), base.ptr + (0 if y16 else 8))
        assert got == bc.kind_model(nr, bnnz, bnr, bnc, team, bidx16, val16, x16, y16), (nr, bnnz, bnr, bnc, team, bidx16, val16, x16, y16)
    check(lib.liship_spmv_bsr_set_team(1))
    for off in (8, 12):                                                        # bindex 8 B and 12 B off is off as well
        assert lib.liship_spmv_bsr_kind(100, 0, 2, 2, base.ptr + off, base.ptr, base.ptr, base.ptr) == bc.PAIR22
    assert lib.liship_spmv_bsr_kind(-1, 0, 2, 2, base.ptr, base.ptr, base.ptr, base.ptr) == ERR_ARG
    assert lib.liship_spmv_bsr_kind(5, 0, 0, 2, base.ptr, base.ptr, base.ptr, base.ptr) == ERR_ARG
    assert lib.liship_spmv_bsr_kind(5, 0, 2, 0, base.ptr, base.ptr, base.ptr, base.ptr) == ERR_ARG
    assert lib.liship_spmv_bsr_kind(0, 0, 2, 2, base.ptr, base.ptr, base.ptr, base.ptr) == bc.ROWS


# ---------------------------------------------------------------- A. the rows kernel
@pytest.mark.parametrize("bs,name", [(bs, n) for bs in (2, 3, 4) for n in bc.names(f"rows{bs}")])
def test_rows_kernel(lib, bs, name):
    """spmv_bsr_rows_kernel<bs>: block-row counts around one and two workgroups, lengths around the gather batches, slices around one and two
    passes of the stage behind every start alignment, a block row of more than two passes, the scalar index loop and the lone tail value at the
    end of the arrays, empty block rows at the end and a matrix without a block"""
    whole(lib, bc.case(f"rows{bs}", name), bc.BNNZ_SHORT, 1, bc.ROWS, (bs, name))


# ---------------------------------------------------------------- B. the team kernel
@pytest.mark.parametrize("bs,name", [(bs, n) for bs in (2, 3, 4) for n in bc.names(f"team{bs}")])
def test_team_kernel(lib, bs, name):
    """spmv_bsr_team_kernel<bs, 8, 4>: block-row counts around one and two groups, lengths up to the 32 a team holds, a group of eight block rows
    without a block (the sentinel becomes +0.0), a block row of 33 among teams (the whole-wavefront fallback), slices that start on odd and even
    blocks and end the array on either, trailing empty block rows"""
    c = bc.case(f"team{bs}", name)
    whole(lib, c, bc.BNNZ_LONG, 2 if bs == 4 else 1, bc.TEAM, (bs, name))
    if name == "empty_group":
        assert np.all(bc.bits(c["y"][8 * bs:16 * bs]) == 0)


# ---------------------------------------------------------------- C. the two-phase kernels
TILE_SHIFTS = {"tile1": [{}], "tile2": [{"x": 1}], "tile3": [{}, {"x": 1, "y": 1, "bidx": 1}], "tile4": [{}, {"y": 1}],
               "pair22": [{}, {"y": 1}, {"bidx": 1}]}


@pytest.mark.parametrize("variant,name", [(v, n) for v in bc.TILE_VARIANTS for n in bc.names(v)])
def test_tile_and_pair_kernels(lib, variant, name):
    """spmv_bsr_tile_kernel<1..4> and spmv_bsr22_kernel with the team kernel switched off: block-row counts around one workgroup, a workgroup of
    CHUNK - 1, CHUNK and CHUNK + 1 blocks (the pass border inside a block row), lengths that are no multiple of the four blocks of a read batch.
    pair22 with y or bindex off 16 B, tile<2,2> with x off it"""
    c = bc.case(variant, name)
    for shift in TILE_SHIFTS[variant]:
        whole(lib, c, bc.BNNZ_LONG, 0, bc.PAIR22 if variant == "pair22" else bc.TILE, (variant, name, shift), shift)


# ---------------------------------------------------------------- D. the generic kernel
@pytest.mark.parametrize("bnr,bnc", bc.GENERIC_SHAPES)
def test_generic_kernel_shapes(lib, bnr, bnc):
    """spmv_bsr_kernel: non-square blocks and blocks beyond 4 x 4, scalar rows just below, at and above one workgroup"""
    for nr in bc.generic_nrs(bnr):
        for bnnz in (-1, bc.BNNZ_SHORT, bc.BNNZ_LONG):
            whole(lib, bc.generic_case(bnr, bnc, nr), bnnz, 1, bc.GENERIC, (bnr, bnc, nr, bnnz))


def test_generic_kernel_serves_blocks_taller_than_a_workgroup(lib):
    """300 x 1 blocks: a block row is longer than the 256 lanes of a workgroup, and no block-rows-per-workgroup figure of the native kernels exists"""
    whole(lib, bc.generic_case(300, 1, 2), bc.BNNZ_SHORT, 1, bc.GENERIC, (300, 1, 2))


@pytest.mark.parametrize("bs", [b for b, _ in bc.GENERIC_UNALIGNED])
def test_generic_kernel_serves_values_off_16_bytes(lib, bs):
    for nr in bc.generic_nrs(bs):
        for bnnz, team in ((bc.BNNZ_SHORT, 1), (bc.BNNZ_LONG, 2)):
            whole(lib, bc.generic_case(bs, bs, nr), bnnz, team, bc.GENERIC, (bs, nr, bnnz), {"val": 1})


# ---------------------------------------------------------------- E. alignment
ALIGN_SHIFTS = [{}, {"val": 1}, {"x": 1}, {"y": 1}, {"bidx": 1}, {"bidx": 2}, {"bidx": 3}, {"val": 1, "x": 1, "y": 1, "bidx": 1}]


@pytest.mark.parametrize("bs", [2, 3, 4])
def test_every_alignment_gives_the_same_bits(lib, bs):
    """each array one element off (bindex one, two and three), alone and all together, on the short-row and the long-row side of the choice and
    with the team kernel on and off: the kernel is the one the model predicts (Mat.run), the bits are the oracle's every time"""
    c = bc.align_case(bs)
    ran = set()
    for shift in ALIGN_SHIFTS:
        m = Mat(c, shift)
        for bnnz, team in ((bc.BNNZ_SHORT, 1), (-1, 1), (bc.BNNZ_LONG, 1), (bc.BNNZ_LONG, 0), (bc.BNNZ_LONG, 2)):
            m.y.reset()
            ran.add(m.run(lib, bnnz, team))
            m.y.holds(c["y"], (bs, shift, bnnz, team))
    assert ran == ({bc.GENERIC, bc.TILE, bc.PAIR22, bc.ROWS, bc.TEAM} if bs == 2 else {bc.GENERIC, bc.TILE, bc.ROWS, bc.TEAM})


# ---------------------------------------------------------------- F. block-row ranges
@pytest.mark.parametrize("config", list(bc.KIND_CONFIGS))
def test_block_row_ranges(lib, config):
    """liship_spmv_bsr_rows_f64 on every kind of kernel: a range writes its block rows with the whole launch's bits and nothing else, an empty
    range nothing; partitions cut at a workgroup border, inside a workgroup, into single block rows and with an empty range between two others
    add up to the whole launch; ranges outside [0, nr] are refused"""
    cfg = bc.KIND_CONFIGS[config]
    c = bc.range_case(config)
    nr, bnr, bnnz, team, kind = c["nr"], c["bnr"], cfg["bnnz"], cfg["team"], cfg["kind"]
    m = Mat(c, cfg["shift"])
    m.run(lib, bnnz, team, kind)
    m.y.holds(c["y"], (config, "whole"))
    for label, parts in bc.range_partitions(nr, cfg["wg"]).items():
        for brb, bre in parts:                                                 # each part alone
            m.y.reset()
            m.run(lib, bnnz, team, kind, rows=(brb, bre))
            m.y.holds(c["y"], (config, label, brb, bre), brb * bnr, bre * bnr)
        m.y.reset()
        for brb, bre in parts:                                                 # and their union
            m.run(lib, bnnz, team, kind, rows=(brb, bre))
        m.y.holds(c["y"], (config, label, "union"))
    m.y.reset()
    check(lib.liship_spmv_bsr_set_team(team))
    for brb, bre in ((0, 0), (nr // 2, nr // 2), (nr, nr), (7, 3)):
        check(lib.liship_spmv_bsr_rows_f64(nr, bnnz, bnr, c["bnc"], m.bptr, m.bidx, m.val, m.x, m.y.ptr, brb, bre, None))
    for brb, bre in ((-1, 10), (-2, 0), (0, nr + 1), (nr, nr + 2)):
        assert lib.liship_spmv_bsr_rows_f64(nr, bnnz, bnr, c["bnc"], m.bptr, m.bidx, m.val, m.x, m.y.ptr, brb, bre, None) == ERR_ARG, (brb, bre)
    m.y.holds(c["y"], (config, "empty and refused ranges"), 0, 0)


@pytest.mark.parametrize("bs", [2, 3, 4])
def test_a_range_runs_the_kernel_of_the_whole_matrix(lib, bs):
    """100 block rows with one block more than the threshold of the rows kernel allows on average (1201 at 2 x 2 and 4 x 4, 1601 at 3 x 3): the
    matrix takes the team kernel, and so must every range of it.  Before the choice had a function of its own the range handed down its share
    bnnz * (bre - brb) / nr in integers, 600 / 50 for [0, 50): the rows kernel -- this test fails there in its kind assertion (liship_spmv_bsr_kind
    and liship_spmv_bsr_last_kind do not exist before it either)."""
    c = bc.border_case(bs)
    nr, bnnz, team = c["nr"], c["bnnz"], 2 if bs == 4 else 1
    m = Mat(c)
    m.run(lib, bnnz, team, bc.TEAM)
    m.y.holds(c["y"], (bs, "whole"))
    for brb, bre in ((0, 50), (50, 100), (0, 1), (99, 100), (57, 58), (25, 75), (0, 99), (1, 100)):
        m.y.reset()
        m.run(lib, bnnz, team, bc.TEAM, rows=(brb, bre))
        m.y.holds(c["y"], (bs, brb, bre), brb * bs, bre * bs)
    m.y.reset()
    m.run(lib, bnnz - 1, team, bc.ROWS, rows=(0, 50))                           # at the threshold the rows kernel, whole or in parts
    m.run(lib, bnnz - 1, team, bc.ROWS, rows=(50, 100))
    m.y.holds(c["y"], (bs, "at the threshold"))


# ---------------------------------------------------------------- G. the fused sums
PRE = np.array([-7.25, 3.5])                    # what result[] holds before a call


class Dot:
    def __init__(self, lib, c, shift=None):
        self.lib, self.c, self.m = lib, c, Mat(c, shift)
        self.w = dev(c["w"])
        self.work, self.res = DA(lib.liship_reduce_work_bytes() // 8, np.float64), DA(2, np.float64)

    def __call__(self, n, sumsq, bnnz=None, bs=None, nr=None):
        m = self.m
        self.res.upload(PRE)
        return self.lib.liship_spmv_bsr_dot_f64(m.nr if nr is None else nr, n, self.c["bnnz"] if bnnz is None else bnnz, m.bnr if bs is None else bs,
                                                m.bptr, m.bidx, m.val, m.x, m.y.ptr, self.w[1], sumsq, self.res.ptr, self.work.ptr, None)

    def refused(self, what, **kw):
        self.m.y.reset()
        assert self(self.m.nr * self.m.bnr, 1, **kw) == ERR_ARG, what
        self.m.y.holds(self.c["y"], what, 0, 0)
        assert np.array_equal(bc.bits(self.res.to_host()), bc.bits(PRE)), what


@pytest.mark.parametrize("nr", bc.DOT_NR)
@pytest.mark.parametrize("bs", [2, 3, 4])
def test_fused_dot_is_the_tree_model(lib, bs, nr):
    """liship_spmv_bsr_dot_f64 with the mean block-row length exactly at the threshold (served), for every n = nr * bs - k: y is the plain product
    in bits (padding rows too), result[0] = <w,y> and result[1] = <y,y> are bsr_cases.dot_model's bits -- per lane the chain over the block row's
    rows with the rows at or beyond n left out, reduction_model.wave_sum over the lanes, reduction_model.fold over the workgroups --, result[1]
    keeps what it held when it is not asked for, and two runs agree"""
    c = bc.dot_case(bs, nr)
    d = Dot(lib, c)
    assert d.m.kind(lib, c["bnnz"], 1, d.m.y.ptr) == bc.ROWS
    for k in range(bs):
        n = nr * bs - k
        for sumsq in (0, 1):
            runs = []
            for _ in range(2):
                d.m.y.reset()
                check(d(n, sumsq))
                d.m.y.holds(c["y"], (bs, nr, n, sumsq))
                runs.append(d.res.to_host().copy())
            assert np.array_equal(bc.bits(runs[0]), bc.bits(runs[1])), (n, sumsq, runs)
            want = [bc.dot_model(bs, nr, n, c["w"], c["y"], 0), bc.dot_model(bs, nr, n, c["w"], c["y"], 1) if sumsq else PRE[1]]
            print(f"bs {bs} nr {nr} n {n} sumsq {sumsq}: {runs[0].tolist()} model {[float(v) for v in want]}")
            assert np.array_equal(bc.bits(runs[0]), bc.bits(np.array(want, np.float64))), (n, sumsq, runs[0].tolist(), want)


@pytest.mark.parametrize("bs", [2, 3, 4])
def test_fused_dot_leaves_an_infinite_padding_row_out(lib, bs):
    """the last scalar row is padding (n = nr * bs - 1) and holds an Inf: y carries it, both sums stay finite and the model's -- w is not read
    beyond n, so a <w,y> that took the padding row in would add 0.0 * Inf"""
    c = bc.dot_padding_case(bs)
    d = Dot(lib, c)
    n = 65 * bs - 1
    d.m.y.reset()
    check(d(n, 1))
    d.m.y.holds(c["y"], (bs, "padding"))
    got = d.res.to_host()
    want = np.array([bc.dot_model(bs, 65, n, c["w"], c["y"], 0), bc.dot_model(bs, 65, n, c["w"], c["y"], 1)])
    assert np.isfinite(want).all() and np.array_equal(bc.bits(got), bc.bits(want)), (got, want)


@pytest.mark.parametrize("bs", [2, 3, 4])
def test_fused_dot_refuses_what_the_rows_kernel_does_not_serve(lib, bs):
    """one block above the threshold, 1 x 1 blocks, no block rows, any array off 16 B, the reference-order sums: LISHIP_ERR_ARG, y and result[]
    untouched (the caller then runs the product and one reduction)"""
    over = bc.dot_case(bs, 65, 1)
    assert over["bnnz"] == int(bc.THRESHOLD[bs]) * 65 + 1
    Dot(lib, over).refused("one block above the threshold")
    c = bc.dot_case(bs, 65)
    d = Dot(lib, c)
    d.refused("1 x 1", bs=1)
    d.refused("5 x 5", bs=5)
    d.refused("no block rows", nr=0)
    d.refused("unknown count", bnnz=-1)
    for name, step in (("val", 1), ("x", 1), ("y", 1), ("bidx", 1), ("bidx", 2)):
        Dot(lib, c, {name: step}).refused((name, step))
    try:
        check(lib.liship_set_reference_reductions(4))
        d.refused("reference-order sums")
    finally:
        check(lib.liship_set_reference_reductions(0))
    d.m.y.reset()
    check(d(65 * bs, 1))                                                       # and served again
    d.m.y.holds(c["y"], "served")


@pytest.mark.parametrize("bs", [2, 3, 4])
def test_fused_dot_behind_the_guard(lib, bs):
    """the guard of the device-driven loops (liship_krylov_guard): behind a raised flag the kernel writes nothing, behind a lowered one the call
    is the unguarded call in every bit"""
    c = bc.dot_case(bs, 65)
    d = Dot(lib, c)
    n = 65 * bs - 1
    d.m.y.reset()
    check(d(n, 1))
    plain = d.res.to_host().copy()
    d.m.y.holds(c["y"], "unguarded")
    flag = DA.from_host(np.array([1.0, 0.0]))
    try:
        check(lib.liship_krylov_guard(flag.ptr))
        d.m.y.reset()
        check(d(n, 1))
        d.m.y.holds(c["y"], "raised", 0, 0)
        check(lib.liship_krylov_guard(flag.ptr + 8))
        d.m.y.reset()
        check(d(n, 1))
        d.m.y.holds(c["y"], "lowered")
        assert np.array_equal(bc.bits(d.res.to_host()), bc.bits(plain))
    finally:
        check(lib.liship_krylov_guard(None))


# ---------------------------------------------------------------- H. special values
@pytest.mark.parametrize("variant", bc.SPECIAL_VARIANTS)
@pytest.mark.parametrize("config", list(bc.KIND_CONFIGS))
def test_special_values(lib, config, variant):
    """on every kind of kernel: an empty block row between one that holds an Inf and one of NaN stays +0.0 (the clamped slots of the team kernel
    read a neighbour's block and must drop it); an explicit zero against x = Inf gives the reference's NaN (no kernel skips zeros); products that
    are all -0.0 sum to +0.0; denormal values give the oracle's denormal sums"""
    cfg = bc.KIND_CONFIGS[config]
    c = bc.special_case(*cfg["bs"], variant)
    bnr = c["bnr"]
    m = Mat(c, cfg["shift"])
    m.run(lib, cfg["bnnz"], cfg["team"], cfg["kind"])
    m.y.holds(c["y"], (config, variant), special=True)
    got = m.y.bits()[m.y.shift:m.y.shift + c["nr"] * bnr]
    assert np.all(got[9 * bnr:10 * bnr] == 0), "the empty block row"
    if variant == "negative_zero":
        assert np.all(got == 0)
    if variant == "denormal":
        assert np.count_nonzero(got) > len(got) // 2
