"""The inputs of tests/test_formats_edges_gpu.py are what they claim to be, and the two numpy restatements agree with the oracle.

No GPU: every generator of tests/format_cases.py is held to the edge its name promises (a launch shape meets or misses the conditions of
fmt_plane as labelled, a jagged diagonal starts on an odd element, exactly half of the rows reach the band), so that a GPU test which passes
has passed at the place it was aimed at."""
import numpy as np
import pytest

import format_cases as fc
import orc


# ---------------------------------------------------------------- A. XCD strips
@pytest.mark.parametrize("name", list(fc.STRIP_SHAPES))
def test_strip_shapes_meet_or_miss_the_plane_conditions_as_labelled(name):
    dims, plane_rows, engages = fc.STRIP_SHAPES[name]
    n = dims[0] * dims[1] * dims[2]
    whole, eighths, planes = fc.plane_conditions(plane_rows, n)
    assert (fc.launch_plane(plane_rows, n) > 0) == engages
    want = {"four_whole_planes": (True, True, True), "tail_past_full": (True, True, True), "plane_of_72": (True, True, True),
            "too_few_planes": (True, True, False), "plane_of_65": (True, False, True), "plane_of_63": (True, False, True),
            "odd_n": (True, True, True)}[name]                # odd n: a pair launch of that size WOULD engage; the launch it takes has no plane
    assert (whole, eighths, planes) == want
    grid, pb = fc.pair_grid(n), plane_rows // fc.WG_ROWS
    if name == "four_whole_planes":
        assert n == 131072 and grid == 4 * pb
    if name == "tail_past_full":
        assert n == 149184 and grid - (grid // pb) * pb == 36 and n % fc.WG_ROWS != 0
    if name == "plane_of_72":
        assert n == 150000 and pb == 72
    if name == "too_few_planes":
        assert n == 130000
    if name == "odd_n":
        assert n % 2 == 1 and n >= 131072


@pytest.mark.parametrize("grid,plane", [(256, 64), (292, 64), (293, 72), (288, 72), (257, 64)])
def test_strip_unit_is_a_permutation_that_leaves_the_tail_alone(grid, plane):
    u = fc.strip_unit(np.arange(grid), grid, plane)
    assert np.array_equal(np.sort(u), np.arange(grid))
    full = (grid // plane) * plane
    assert np.array_equal(u[full:], np.arange(full, grid)) and not np.array_equal(u, np.arange(grid))
    # workgroup w runs on XCD w % 8: every XCD owns one eighth of every plane and meets the planes in order
    for xcd in range(8):
        mine = u[xcd:full:8]
        assert np.all((mine % plane) // (plane // 8) == xcd) and np.all(np.diff(mine // plane) >= 0)
    assert np.array_equal(fc.strip_unit(np.arange(grid), grid, 0), np.arange(grid))


def test_strip_matrix_is_coded_material():
    c = fc.strip_matrix((32, 64, 64))
    offsets = np.unique(c["eidx"].reshape(c["mx"], c["n"]) - np.arange(c["n"])[None, :])
    assert c["mx"] == 7 and c["nnd"] == 7 and len(offsets) <= 255 and c["n"] % 2 == 0


# ---------------------------------------------------------------- B. row ranges
@pytest.mark.parametrize("parity", ["even", "odd"])
def test_row_ranges_cover_every_dispatch(parity):
    n = fc.RANGE_N[parity]
    assert 1500 <= n <= 3000 and n % 2 == (parity == "odd")
    rr = fc.row_ranges(n)
    assert all(0 <= rb <= re <= n for rb, re in rr.values())
    pairs = {k for k, (rb, re) in rr.items() if re > rb and fc.pair_range(n, rb, re)}
    if parity == "odd":
        assert not pairs
    else:
        assert {"whole", "even_start_even_length", "one_workgroup_of_pairs", "head_to_256", "tail_from_512", "last_two_rows"} <= pairs
        assert not pairs & {"even_start_odd_length", "odd_start_even_length", "odd_start_odd_length", "single_row_even", "head_to_255",
                            "tail_from_257", "last_row"}
    rb, re = rr["even_start_even_length"]
    assert rb % 2 == 0 and (re - rb) // 2 == 2 * fc.BLOCK + 1            # three workgroups of pairs, one lane in the last
    assert rr["odd_start_even_length"][0] % 2 == 1 and rr["even_start_odd_length"][0] % 2 == 0
    for parts in fc.partitions(n).values():
        (ib, ie), (hb, he), (tb, te) = parts
        assert hb == 0 and he == ib and ie == tb and te == n and ib < ie
    assert all(fc.pair_range(n, rb, re) for rb, re in fc.partitions(n)["even_cuts"]) == (parity == "even")
    assert not any(fc.pair_range(n, rb, re) for rb, re in fc.partitions(n)["odd_cuts"][:2])


@pytest.mark.parametrize("parity", ["even", "odd"])
@pytest.mark.parametrize("slots", [7, 9])
def test_range_matrices(parity, slots):
    e = fc.range_ell(parity, slots)
    n = e["n"]
    assert e["mx"] == slots
    idx, val = e["eidx"].reshape(slots, n), e["ev"].reshape(slots, n)
    pad = (idx == np.arange(n)[None, :]) & (val == 0.0)
    assert pad[:, :300].any() and pad[:, -300:].any() and not pad[:, 300:n - 300].any()      # boundary rows are padded, interior rows full
    assert len(np.unique(idx - np.arange(n)[None, :])) <= 255                                  # liship_ell_encode_indices accepts it
    d = fc.range_dia(parity, slots, False)
    assert d["nnd"] == slots and d["ncols"] == n and not np.all(np.diff(d["off"]) > 0)          # stored order is not sorted order
    g = fc.range_dia(parity, slots, True)
    assert g["nnd"] == slots and g["ncols"] == n + fc.GHOST and len(g["x"]) == g["ncols"]
    reach = np.arange(n)[None, :] + g["off"].astype(np.int64)[:, None]
    inside = (reach >= 0) & (reach < g["ncols"])
    assert (reach[inside] >= n).any() and (reach[inside] == g["ncols"] - 1).any()               # ghost columns are read, the last one too
    assert ((reach >= g["ncols"]) & (reach < g["ncols"] + 13)).any()                             # ... and some slots fall just past it
    assert np.all(g["dv"].reshape(slots, n)[~inside] == 0.0) and np.all(g["dv"].reshape(slots, n)[inside] != 0.0)


@pytest.mark.parametrize("n,offsets", [(1800, fc.RANGE_OFFSETS[7]), (1801, fc.RANGE_OFFSETS[9]), (514, [513, 0, -513, 3, 514, -600, -2]),
                                       (1, [0]), (2, [1, -1, 0, 0]), (513, [])])
def test_dia_reference_is_the_oracle_on_square_matrices(n, offsets):
    off, val = fc.dia_arrays(n, offsets, seed=n + len(offsets))
    x = fc.vectors(n, 5)
    x[::7] = 0.0
    x[3::11] = -0.0
    val[::13] = -0.0
    assert np.array_equal(fc.bits(fc.dia_reference(n, n, off, val, x)), fc.bits(orc.spmv_dia(n, len(off), off, val, x)))


@pytest.mark.parametrize("n", fc.EDGE_N)
@pytest.mark.parametrize("nnd", fc.EDGE_SLOTS)
def test_dia_reference_is_the_oracle_on_the_edge_grid(n, nnd):
    off, val = fc.dia_random(n, nnd, seed=100 * n + nnd)
    x = fc.vectors(n, 6)
    assert len(off) == nnd and np.all(np.abs(off) < n)
    assert np.array_equal(fc.bits(fc.dia_reference(n, n, off, val, x)), fc.bits(orc.spmv_dia(n, nnd, off, val, x)))


def test_dia_reference_reads_the_ghost_columns():
    """on an n x ncols matrix the restatement is the oracle's product of the square matrix of ncols rows whose first n rows it is"""
    g = fc.range_dia("even", 9, True)
    n, ncols, nnd = g["n"], g["ncols"], g["nnd"]
    big = np.zeros((nnd, ncols))
    big[:, :n] = g["dv"].reshape(nnd, n)
    ref = orc.spmv_dia(ncols, nnd, g["off"], np.ascontiguousarray(big.ravel()), g["x"])
    assert np.array_equal(fc.bits(g["y"]), fc.bits(ref[:n]))


# ---------------------------------------------------------------- C. whole-launch edges
@pytest.mark.parametrize("n", fc.EDGE_N)
@pytest.mark.parametrize("maxnzr", fc.EDGE_SLOTS)
def test_ell_random_pads_rows_the_reference_way(n, maxnzr):
    idx, val, lens = fc.ell_random(n, maxnzr, seed=100 * n + maxnzr)
    assert idx.dtype == np.int32 and len(idx) == len(val) == n * maxnzr and lens.max(initial=0) == maxnzr
    i2, v2 = idx.reshape(maxnzr, n), val.reshape(maxnzr, n)
    pad = np.arange(maxnzr)[:, None] >= lens[None, :]
    assert np.all(i2[pad] == np.broadcast_to(np.arange(n), (maxnzr, n))[pad]) and np.all(fc.bits(v2[pad]) == 0)
    assert np.all((i2 >= 0) & (i2 < n))
    if n >= 3 and maxnzr:
        assert pad[:, 1].all() and not pad[:, n - 1].any()


def test_special_value_cases_are_what_they_say():
    idx, val, x, rows = fc.ell_padding_meets_inf()
    n, mx = 514, 9
    assert np.all((idx.reshape(mx, n)[-1, rows] == rows) & (val.reshape(mx, n)[-1, rows] == 0.0)) and not np.isfinite(x[rows]).any()
    assert np.isnan(orc.spmv_ell(n, mx, idx, val, x)[rows]).all()                      # 0.0 * inf: the oracle says NaN
    for n in (513, 514):
        off, val = fc.dia_outside(n)
        assert (np.abs(off) >= n).sum() == 4 and {n - 1, -(n - 1)} <= set(off.tolist())
        v = val.reshape(len(off), n)
        assert np.count_nonzero(v[list(off).index(n - 1)]) == 1 and np.count_nonzero(v[list(off).index(-(n - 1))]) == 1
    off, val, x, rows = fc.dia_masked_leak()
    n = 514
    reach = rows[None, :] + off.astype(np.int64)[:, None]
    masked = (reach < 0) | (reach >= n)
    assert masked.any(axis=0).all() and np.all(val.reshape(len(off), n)[:, rows][masked] == 0.0) and np.isinf(x[rows]).all()
    assert np.isfinite(x[reach[~masked]]).all() and 0 not in off.tolist()
    y = orc.spmv_dia(n, len(off), off, val, x)
    assert np.isfinite(y[rows]).all() and not np.isfinite(y[[3, 4, n - 4, n - 3, n - 7, n - 6]]).any()
    idx, val, _ = fc.ell_random(514, 9, seed=8)
    v, x = fc.all_products_negative_zero(val, 514)
    assert np.all(fc.bits(orc.spmv_ell(514, 9, idx, v, x)) == 0) and np.signbit(v * 0.0).all()


# ---------------------------------------------------------------- D. JAD
def test_jad_cases_are_what_they_say():
    seen_identity = set()
    for name, (kind, n, mx) in fc.JAD_NAMED.items():
        c = fc.jad_case(kind, n, mx)
        assert c["mx"] == mx and np.array_equal(np.sort(c["perm"]), np.arange(n)), name
        assert np.array_equal(np.diff(c["jptr"]), [(c["lens"] > j).sum() for j in range(mx)]), name
        identity = np.array_equal(c["perm"], np.arange(n))
        seen_identity.add(identity)
        if kind == "equal":
            assert np.all(np.diff(c["jptr"]) == n)
        if kind == "odd_starts":
            assert (c["jptr"][1:mx] % 2 == 1).any() and (c["jptr"][1:mx] % 2 == 0).any(), name
        if kind == "one_long_row":
            assert np.sort(c["lens"])[-2] <= 5 and c["perm"][0] == n // 3 and np.all(np.diff(c["jptr"])[6:] == 1)
        if kind == "descending":
            assert identity
        if kind == "ascending":
            assert np.array_equal(c["perm"], np.arange(n)[::-1])
    assert seen_identity == {True, False}


@pytest.mark.parametrize("n", fc.JAD_N)
@pytest.mark.parametrize("maxnzr", fc.JAD_SLOTS)
def test_jad_grid_has_empty_rows_at_the_end_of_the_permutation(n, maxnzr):
    c = fc.jad_case("random", n, maxnzr)
    assert c["mx"] == maxnzr and len(c["jptr"]) == maxnzr + 1
    empty = np.flatnonzero(c["lens"] == 0)
    if maxnzr and n >= 3:
        assert len(empty) and set(c["perm"][n - len(empty):].tolist()) == set(empty.tolist())
        assert np.all(fc.bits(c["y"][empty]) == 0)


# ---------------------------------------------------------------- E. scan band and diagonals
@pytest.mark.parametrize("n", [63, 65, 1000])
def test_band_half_has_exactly_the_rows_it_says(n):
    half, band = (n + 1) // 2, n // 3
    for ghosts in (False, True):
        mx, idx = fc.band_half(n, band, half, ghosts)
        assert fc.rows_reaching(n, mx, idx, band) == half and fc.scan_band_reference(n, mx, idx) == band
        mx, idx = fc.band_half(n, band, half - 1, ghosts)
        assert fc.rows_reaching(n, mx, idx, band) == half - 1 and fc.scan_band_reference(n, mx, idx) == 0
        if ghosts:
            c = idx.reshape(mx, n)
            far = np.abs(c - np.arange(n)[None, :]) > band
            assert far.any() and np.all((c[far] < 0) | (c[far] >= n))


def test_scan_band_reference_on_a_stencil_and_a_diagonal():
    ptr, idx, val = orc.poisson3d(9, 8, 7)
    mx, eidx, _ = orc.csr2ell(ptr, idx, val)
    assert fc.scan_band_reference(len(ptr) - 1, mx, eidx) == 56
    assert fc.scan_band_reference(100, 1, np.arange(100, dtype=np.int32)) == 0
    assert fc.scan_band_reference(1, 1, np.zeros(1, np.int32)) == 0
    assert fc.scan_band_reference(0, 3, np.zeros(0, np.int32)) == 0 and fc.scan_band_reference(5, 0, np.zeros(0, np.int32)) == 0


def test_diagonal_cases_are_what_they_say():
    cases = fc.diagonal_cases()
    for name, (ptr, idx, val) in cases.items():
        n = len(ptr) - 1
        rows = np.repeat(np.arange(n), np.diff(ptr))
        assert np.all(np.diff(idx)[np.diff(rows) == 0] > 0), name                      # column-sorted: csr2dia takes it
        has = np.zeros(n, bool)
        has[rows[idx == rows]] = True
        d = orc.csr_diagonal(ptr, idx, val)
        assert np.all(d[~has] == 0.0) and np.all(d[has] != 0.0)
        if name == "stencil":
            assert has.all()
        if name == "every_third_row_lacks_it":
            assert np.array_equal(has, np.arange(n) % 3 != 0)
        if name == "no_diagonal_at_all":
            assert not has.any()
        if name == "diagonal_in_the_last_real_slot":
            mx, eidx, ev = orc.csr2ell(ptr, idx, val)
            lens = np.diff(ptr)
            short = np.flatnonzero((lens < mx) & (np.arange(n) % 4 != 0))              # (the rows of four have entries behind their diagonal)
            assert mx == 5 and len(short) > n // 2 and has.all()
            assert np.all(eidx.reshape(mx, n)[lens[short] - 1, short] == short) and np.all(ev.reshape(mx, n)[lens[short] - 1, short] != 0.0)
