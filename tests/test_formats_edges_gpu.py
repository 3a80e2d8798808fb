"""The native ELL / DIA / JAD kernels (kernels/spmv_formats.hip) at the edges their dispatchers and loops have, bit for bit against the oracle.

Kernel level (include/liship.h through lis_amd.load()).  What test_kernels_gpu.py leaves out: the XCD strips of the ELL / DIA launches at a size
an oracle can follow, the row-range entries of a multi-rank product, the one-row-per-lane and VEC = false fallbacks behind unaligned arrays, slot
counts around the batches of eight, the masks of DIA and JAD, liship_ell_scan_band and the ELL / DIA diagonal kernels.

Every comparison is on the 64 bits of each element.  y is allocated a few elements longer than a launch may write and prefilled with a NaN that no
product can produce (format_cases.SENTINEL_BITS): rows a launch must not touch, and the tail, must still hold it; rows it must write must not.
The inputs and the facts they rest on are in tests/format_cases.py and asserted without a GPU in tests/test_format_cases_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import format_cases as fc
import orc
import lis_amd
from gpu_arrays import Out, dev
from lis_amd import DeviceArray as DA, check

pytestmark = pytest.mark.gpu
ERR_ARG = -1                                    # LISHIP_ERR_ARG


@pytest.fixture(scope="module")
def lib():
    lib = lis_amd.load()
    assert lis_amd.gpu_available(), "no HIP device: the product path has no CPU fallback"
    return lib


def encode(lib, n, mx, didx_ptr):
    codes, dic, nd = C.c_void_p(), C.c_void_p(), C.c_int()
    check(lib.liship_ell_encode_indices(n, mx, didx_ptr, C.byref(codes), C.byref(dic), C.byref(nd), None))
    return codes, dic


def release(lib, codes, dic):
    for p in (codes, dic):
        if p is not None and p.value:
            check(lib.liship_free(p))


# ---------------------------------------------------------------- A. XCD strips of ELL and DIA
@pytest.mark.parametrize("name", list(fc.STRIP_SHAPES))
def test_xcd_strips_permute_workgroups_not_bits(lib, name):
    """fmt_strip_unit / fmt_plane at the smallest sizes that engage them, and at the sizes next to them that must not: with the plane set and with
    plane 0 every whole-matrix ELL / DIA entry writes the oracle's y (a unit worked on twice or never leaves sentinel rows), and the fused sums are
    the same bits either way -- the partial of a workgroup is published under the unit it worked on, so the fold order is the natural one.
    liship_spmv_formats_plane_blocks proves that the strips were on where the case says so, and off where it says that."""
    dims, plane_rows, engages = fc.STRIP_SHAPES[name]
    c = fc.strip_matrix(dims)
    n, mx, nnd, x, w = c["n"], c["mx"], c["nnd"], c["x"], c["w"]
    grid = fc.pair_grid(n)
    (_, ei), (_, ev), (_, do), (_, dv), (_, dx), (_, dw) = keep = [dev(c[k]) for k in ("eidx", "ev", "off", "dv", "x", "w")]
    work, res = DA(lib.liship_reduce_work_bytes() // 8, np.float64), DA(2, np.float64)
    y = Out(n)
    codes = dic = None
    sums = {}

    def fused(key, plane, call, yref):
        y.reset()
        res.upload(np.full(2, np.nan))
        check(call())
        y.holds(yref, (name, key, plane))
        sums.setdefault(key, {})[plane] = res.to_host().copy()

    try:
        if n % 2 == 0:
            codes, dic = encode(lib, n, mx, ei)
            assert codes.value, "the stencil must be coded"
        for plane in (plane_rows, 0):
            check(lib.liship_spmv_formats_set_plane(plane))
            got = lib.liship_spmv_formats_plane_blocks(fc.WG_ROWS, grid)
            assert got == fc.plane_blocks(plane, n), (name, plane, got)
            if n % 2 == 0:
                assert (got > 0) == (engages and plane > 0), (name, plane, got)
            y.reset()
            check(lib.liship_spmv_ell_f64(n, mx, ei, ev, dx, y.ptr, None))
            y.holds(c["y_ell"], (name, "ell", plane))
            y.reset()
            check(lib.liship_spmv_dia_f64(n, n, nnd, do, dv, dx, y.ptr, None))
            y.holds(c["y_dia"], (name, "dia", plane))
            if n % 2:                                   # the fused and coded forms do not serve an odd n: the caller runs product + dot
                y.reset()
                assert lib.liship_spmv_ell_dot_f64(n, mx, ei, ev, dx, y.ptr, dw, 1, res.ptr, work.ptr, None) == ERR_ARG
                assert lib.liship_spmv_dia_dot_f64(n, n, nnd, do, dv, dx, y.ptr, dw, 1, res.ptr, work.ptr, None) == ERR_ARG
                y.holds(c["y_ell"], (name, "refused", plane), 0, 0)
                continue
            y.reset()
            check(lib.liship_spmv_ell_coded_f64(n, mx, codes, dic, ev, dx, y.ptr, None, -1, None, None, None))
            y.holds(c["y_ell"], (name, "coded", plane))
            for sq in (0, 1):
                fused(("coded", sq), plane, lambda: lib.liship_spmv_ell_coded_f64(n, mx, codes, dic, ev, dx, y.ptr, dw, sq, res.ptr, work.ptr, None), c["y_ell"])
                fused(("ell_dot", sq), plane, lambda: lib.liship_spmv_ell_dot_f64(n, mx, ei, ev, dx, y.ptr, dw, sq, res.ptr, work.ptr, None), c["y_ell"])
                fused(("dia_dot", sq), plane, lambda: lib.liship_spmv_dia_dot_f64(n, n, nnd, do, dv, dx, y.ptr, dw, sq, res.ptr, work.ptr, None), c["y_dia"])
        for (entry, sq), by_plane in sums.items():
            on, off = by_plane[plane_rows][:1 + sq], by_plane[0][:1 + sq]
            assert np.array_equal(fc.bits(on), fc.bits(off)), (name, entry, sq, on, off)
            yref = c["y_dia"] if entry == "dia_dot" else c["y_ell"]
            assert abs(on[0] - np.dot(w, yref)) <= 1e-12 * np.abs(w * yref).sum(), (name, entry, sq)
            if sq:
                assert abs(on[1] - np.dot(yref, yref)) <= 1e-12 * np.dot(yref, yref), (name, entry, sq)
        assert len(sums) == (0 if n % 2 else 6)
    finally:
        check(lib.liship_spmv_formats_set_plane(0))
        release(lib, codes, dic)
    del keep


# ---------------------------------------------------------------- B. row ranges
@pytest.mark.parametrize("parity", ["even", "odd"])
@pytest.mark.parametrize("slots", [7, 9])
def test_ell_row_ranges(lib, parity, slots):
    """liship_spmv_ell_rows_f64 picks the pair kernel, the coded pair kernel or one row per lane from the parities of rb and re - rb: every
    range writes exactly its rows with the whole launch's bits.  With codes AND indices a range that is no pair range falls back to the indices;
    with codes alone it is refused and y stays as it was."""
    c = fc.range_ell(parity, slots)
    n, mx, yref = c["n"], c["mx"], c["y"]
    (_, ei), (_, ev), (_, dx) = keep = [dev(c[k]) for k in ("eidx", "ev", "x")]
    y = Out(n)
    codes, dic = encode(lib, n, mx, ei)
    try:
        assert bool(codes.value) == (parity == "even")
        forms = [("idx", None, None, ei)]
        if codes.value:
            forms += [("codes+idx", codes, dic, ei), ("codes", codes, dic, None)]
        for form, cd, dc, ix in forms:
            run = lambda rb, re: lib.liship_spmv_ell_rows_f64(n, mx, ix, cd, dc, ev, dx, y.ptr, rb, re, None)
            for label, (rb, re) in fc.row_ranges(n).items():
                y.reset()
                rc = run(rb, re)
                if form == "codes" and re > rb and not fc.pair_range(n, rb, re):
                    assert rc == ERR_ARG, (form, label)
                    y.holds(yref, (form, label, "refused"), 0, 0)
                    continue
                check(rc)
                y.holds(yref, (form, label), rb, re)
            for label, parts in fc.partitions(n).items():
                if form == "codes" and not all(fc.pair_range(n, rb, re) for rb, re in parts):
                    continue
                y.reset()
                for rb, re in parts:
                    check(run(rb, re))
                y.holds(yref, (form, label, "partition"))
        for bad in ((-1, 10), (-2, 0), (0, n + 1), (n, n + 2)):
            y.reset()
            assert lib.liship_spmv_ell_rows_f64(n, mx, ei, None, None, ev, dx, y.ptr, bad[0], bad[1], None) == ERR_ARG, bad
            y.holds(yref, ("refused", bad), 0, 0)
    finally:
        release(lib, codes, dic)
    del keep


@pytest.mark.parametrize("parity", ["even", "odd"])
@pytest.mark.parametrize("slots", [7, 9])
@pytest.mark.parametrize("ghost", [False, True], ids=["square", "ghost_columns"])
def test_dia_row_ranges(lib, parity, slots, ghost):
    """liship_spmv_dia_rows_f64 and the whole launch, square and with ncols = n + 37 (offsets that reach the ghost columns, x of length ncols:
    the reference there is format_cases.dia_reference, pinned to the oracle by test_format_cases_cpu.py)"""
    c = fc.range_dia(parity, slots, ghost)
    n, ncols, nnd, yref = c["n"], c["ncols"], c["nnd"], c["y"]
    (_, do), (_, dv), (_, dx) = keep = [dev(c[k]) for k in ("off", "dv", "x")]
    y = Out(n)
    check(lib.liship_spmv_dia_f64(n, ncols, nnd, do, dv, dx, y.ptr, None))
    y.holds(yref, "whole launch")
    run = lambda rb, re: lib.liship_spmv_dia_rows_f64(n, ncols, nnd, do, dv, dx, y.ptr, rb, re, None)
    for label, (rb, re) in fc.row_ranges(n).items():
        y.reset()
        check(run(rb, re))
        y.holds(yref, label, rb, re)
    for label, parts in fc.partitions(n).items():
        y.reset()
        for rb, re in parts:
            check(run(rb, re))
        y.holds(yref, (label, "partition"))
    y.reset()
    for rb, re in ((-1, 10), (0, n + 1)):
        assert run(rb, re) == ERR_ARG
    assert lib.liship_spmv_dia_rows_f64(n, n - 1, nnd, do, dv, dx, y.ptr, 0, n, None) == ERR_ARG
    assert lib.liship_spmv_dia_f64(n, n - 1, nnd, do, dv, dx, y.ptr, None) == ERR_ARG
    y.holds(yref, "refused", 0, 0)
    del keep


# ---------------------------------------------------------------- C. whole-launch edges of ELL and DIA
SHIFTS = {"aligned": (0, 0, 0), "val+8B": (1, 0, 0), "y+8B": (0, 1, 0), "idx+4B": (0, 0, 1)}


@pytest.mark.parametrize("n", fc.EDGE_N)
@pytest.mark.parametrize("maxnzr", fc.EDGE_SLOTS)
def test_ell_slot_counts_and_alignments(lib, n, maxnzr):
    """n around one workgroup of pairs, slot counts around the batches of eight (0: y[0..n) becomes +0.0 and not an element more); for even n the
    same arrays again behind 8 B / 4 B steps that rule the 16 B / 8 B loads out -- one row per lane must give the same bits"""
    idx, val, _ = fc.ell_random(n, maxnzr, seed=100 * n + maxnzr)
    x = fc.vectors(n, 7)
    yref = orc.spmv_ell(n, maxnzr, idx, val, x)
    if maxnzr == 0:
        assert np.all(fc.bits(yref) == 0)
    _, dx = kx = dev(x)
    for label, (sv, sy, si) in SHIFTS.items():
        if label != "aligned" and n % 2:
            continue
        (_, ei), (_, ev) = keep = [dev(idx, np.int32, si), dev(val, np.float64, sv)]
        y = Out(n, sy)
        check(lib.liship_spmv_ell_f64(n, maxnzr, ei, ev, dx, y.ptr, None))
        y.holds(yref, (n, maxnzr, label))
        del keep
    del kx


@pytest.mark.parametrize("n", fc.EDGE_N)
@pytest.mark.parametrize("nnd", fc.EDGE_SLOTS)
def test_dia_slot_counts_and_alignments(lib, n, nnd):
    off, val = fc.dia_random(n, nnd, seed=100 * n + nnd)
    x = fc.vectors(n, 8)
    yref = orc.spmv_dia(n, nnd, off, val, x)
    (_, do), (_, dx) = kx = [dev(off, np.int32), dev(x)]
    for label, (sv, sy, _) in list(SHIFTS.items())[:3]:
        if label != "aligned" and n % 2:
            continue
        _, dv = keep = dev(val, np.float64, sv)
        y = Out(n, sy)
        check(lib.liship_spmv_dia_f64(n, n, nnd, do, dv, dx, y.ptr, None))
        y.holds(yref, (n, nnd, label))
        del keep
    del kx


def test_ell_padding_slots_meet_inf_and_nan(lib):
    """a padding slot is (row, +0.0): with x[row] = inf the reference's loop adds 0.0 * inf = NaN, and so must every ELL kernel"""
    n, mx = 514, 9
    idx, val, x, rows = fc.ell_padding_meets_inf(n, mx)
    yref = orc.spmv_ell(n, mx, idx, val, x)
    assert np.isnan(yref[rows]).all()
    (_, ei), (_, ev), (_, dx) = keep = [dev(idx), dev(val), dev(x)]
    (_, ei4), (_, ev8) = keep2 = [dev(idx, np.int32, 1), dev(val, np.float64, 1)]
    y = Out(n)
    for what, run in (("pairs", lambda: lib.liship_spmv_ell_f64(n, mx, ei, ev, dx, y.ptr, None)),
                      ("one row per lane", lambda: lib.liship_spmv_ell_f64(n, mx, ei4, ev8, dx, y.ptr, None)),
                      ("range", lambda: lib.liship_spmv_ell_rows_f64(n, mx, ei, None, None, ev, dx, y.ptr, 0, n, None))):
        y.reset()
        check(run())
        y.holds(yref, what, special=True)
    del keep, keep2


@pytest.mark.parametrize("n", [513, 514])
def test_dia_diagonals_outside_the_matrix_and_in_its_corners(lib, n):
    """|offset| >= n: nothing of the diagonal is inside, whatever it stores; offsets -(n - 1) and n - 1: one element each"""
    off, val = fc.dia_outside(n)
    val = val.copy()
    val.reshape(len(off), n)[np.abs(off) >= n] = 3.25                  # the reference never reads a diagonal that is wholly outside
    x = fc.vectors(n, 9)
    yref = orc.spmv_dia(n, len(off), off, val, x)
    (_, do), (_, dv), (_, dx) = keep = [dev(off, np.int32), dev(val), dev(x)]
    y = Out(n)
    check(lib.liship_spmv_dia_f64(n, n, len(off), do, dv, dx, y.ptr, None))
    y.holds(yref, "whole")
    y.reset()
    check(lib.liship_spmv_dia_rows_f64(n, n, len(off), do, dv, dx, y.ptr, 1, n, None))
    y.holds(yref, "rows 1 .. n", 1, n)
    del keep


def test_dia_masked_slots_discard_what_they_load(lib):
    """a slot outside the matrix loads x[r] instead and must drop the product: 0.0 * inf would be NaN"""
    n = 514
    off, val, x, rows = fc.dia_masked_leak(n)
    yref = orc.spmv_dia(n, len(off), off, val, x)
    assert np.isfinite(yref[rows]).all()
    (_, do), (_, dv), (_, dx), (_, dv8) = keep = [dev(off, np.int32), dev(val), dev(x), dev(val, np.float64, 1)]
    y = Out(n)
    for what, v in (("pairs", dv), ("one row per lane", dv8)):
        y.reset()
        check(lib.liship_spmv_dia_f64(n, n, len(off), do, v, dx, y.ptr, None))
        assert np.isfinite(y.d.to_host(n)[rows]).all(), what
        y.holds(yref, what, special=True)
    del keep


@pytest.mark.parametrize("fmt", ["ell", "dia", "jad"])
def test_rows_of_negative_zero_products_end_as_positive_zero(lib, fmt):
    n = 514
    y = Out(n)
    if fmt == "ell":
        idx, val, _ = fc.ell_random(n, 9, seed=8)
        val, x = fc.all_products_negative_zero(val, n)
        yref = orc.spmv_ell(n, 9, idx, val, x)
        (_, a), (_, b), (_, dx) = keep = [dev(idx), dev(val), dev(x)]
        check(lib.liship_spmv_ell_f64(n, 9, a, b, dx, y.ptr, None))
    elif fmt == "dia":
        off, val = fc.dia_random(n, 9, seed=8)
        val, x = fc.all_products_negative_zero(val, n)
        yref = orc.spmv_dia(n, 9, off, val, x)
        (_, a), (_, b), (_, dx) = keep = [dev(off, np.int32), dev(val), dev(x)]
        check(lib.liship_spmv_dia_f64(n, n, 9, a, b, dx, y.ptr, None))
    else:
        c = fc.jad_case("random", n, 9)
        val, x = fc.all_products_negative_zero(c["jval"], n)
        yref = orc.spmv_jad(n, c["mx"], c["perm"], c["jptr"], c["jidx"], val, x)
        (_, a), (_, b), (_, i), (_, v), (_, dx) = keep = [dev(c["perm"]), dev(c["jptr"]), dev(c["jidx"]), dev(val), dev(x)]
        check(lib.liship_spmv_jad_f64(n, c["mx"], a, b, i, v, dx, y.ptr, None))
    assert np.all(fc.bits(yref) == 0)
    y.holds(yref, fmt)
    del keep


# ---------------------------------------------------------------- D. JAD
def run_jad(lib, c, what):
    """the case on aligned arrays (VEC), then with the values 8 B and the indices 4 B off (VEC = false): the same bits"""
    n, mx = c["n"], c["mx"]
    (_, dp), (_, dj), (_, dx) = keep = [dev(c["perm"]), dev(c["jptr"]), dev(c["x"])]
    for label, (sv, _, si) in ((k, SHIFTS[k]) for k in ("aligned", "val+8B", "idx+4B")):
        (_, di), (_, dv) = keep2 = [dev(c["jidx"], np.int32, si), dev(c["jval"], np.float64, sv)]
        y = Out(n)
        check(lib.liship_spmv_jad_f64(n, mx, dp, dj, di, dv, dx, y.ptr, None))
        y.holds(c["y"], (what, label))
        del keep2
    del keep


@pytest.mark.parametrize("n", fc.JAD_N)
@pytest.mark.parametrize("maxnzr", fc.JAD_SLOTS)
def test_jad_slot_counts_and_alignments(lib, n, maxnzr):
    """rows of 0 .. maxnzr entries around the batches of eight and around one workgroup of slot pairs; the rows without entries end the
    permutation and must become +0.0 (maxnzr = 0: all of them, and not an element more)"""
    c = fc.jad_case("random", n, maxnzr)
    assert c["mx"] == maxnzr
    run_jad(lib, c, (n, maxnzr))


@pytest.mark.parametrize("name", list(fc.JAD_NAMED))
def test_jad_named_cases(lib, name):
    """equal rows, jagged diagonals that start on odd elements (the per-slot fallback inside the VEC kernel), one row of 300 entries among
    short ones (every other lane breaks out of the batches early), identity and reversed permutations"""
    c = fc.jad_case(*fc.JAD_NAMED[name])
    run_jad(lib, c, name)


# ---------------------------------------------------------------- E. liship_ell_scan_band and the ELL / DIA diagonal kernels
def scan_band(lib, n, maxnzr, idx):
    _, di = keep = dev(idx, np.int32)
    plane = C.c_int(-7)
    check(lib.liship_ell_scan_band(n, maxnzr, di, C.byref(plane), None))
    del keep
    return plane.value


def test_scan_band_finds_the_plane_of_a_stencil(lib):
    for dims in ((9, 8, 7), (5, 4, 33)):
        ptr, idx, val = orc.poisson3d(*dims)
        n = len(ptr) - 1
        mx, eidx, _ = orc.csr2ell(ptr, idx, val)
        assert scan_band(lib, n, mx, eidx) == fc.scan_band_reference(n, mx, eidx) == dims[1] * dims[2]


@pytest.mark.parametrize("n", [63, 65, 1000])
@pytest.mark.parametrize("ghosts", [False, True], ids=["owned", "ghost_columns"])
def test_scan_band_needs_half_of_the_rows(lib, n, ghosts):
    """exactly ceil(n / 2) rows at the band: the band; one fewer: 0.  Columns that are not owned (c >= n, c < 0) are further away and ignored"""
    half, band = (n + 1) // 2, n // 3
    mx, idx = fc.band_half(n, band, half, ghosts)
    assert scan_band(lib, n, mx, idx) == fc.scan_band_reference(n, mx, idx) == band
    mx, idx = fc.band_half(n, band, half - 1, ghosts)
    assert scan_band(lib, n, mx, idx) == fc.scan_band_reference(n, mx, idx) == 0


def test_scan_band_of_matrices_without_a_plane(lib):
    for n in (1, 63, 65, 1000):
        assert scan_band(lib, n, 1, np.arange(n, dtype=np.int32)) == 0               # diagonal only
        assert scan_band(lib, n, 0, np.zeros(0, np.int32)) == 0
    assert scan_band(lib, 0, 3, np.zeros(0, np.int32)) == 0
    ptr, idx, val = orc.random_csr(1000, 6, seed=21)
    mx, eidx, _ = orc.csr2ell(ptr, idx, val)
    assert scan_band(lib, 1000, mx, eidx) == fc.scan_band_reference(1000, mx, eidx) == 0
    assert lib.liship_ell_scan_band(5, 1, None, None, None) == ERR_ARG


@pytest.mark.parametrize("name", ["stencil", "every_third_row_lacks_it", "no_diagonal_at_all", "diagonal_in_the_last_real_slot"])
def test_ell_and_dia_diagonals(lib, name):
    ptr, idx, val = fc.diagonal_cases()[name]
    n = len(ptr) - 1
    dref = orc.csr_diagonal(ptr, idx, val)
    mx, eidx, ev = orc.csr2ell(ptr, idx, val)
    nnd, off, dv = orc.csr2dia(ptr, idx, val)
    (_, a), (_, b), (_, o), (_, v) = keep = [dev(eidx), dev(ev), dev(off, np.int32), dev(dv)]
    d = Out(n)
    check(lib.liship_ell_diagonal_f64(n, mx, a, b, d.ptr, None))
    d.holds(dref, (name, "ell"))
    d.reset()
    check(lib.liship_dia_diagonal_f64(n, nnd, o, v, d.ptr, None))
    d.holds(dref, (name, "dia"))
    del keep
