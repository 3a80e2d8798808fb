"""The facts tests/test_bsr_edges_gpu.py rests on, asserted without a GPU: every named case of tests/bsr_cases.py reaches the edge of
kernels/spmv_formats.hip it is named for (recomputed from the block-row lengths), the oracle's BSR product is an independent numpy chain and the
reference's bits at every block size, and the model of the fused sums is a sum."""
import math

import numpy as np
import pytest

import bsr_cases as bc
import orc


def every_case():
    return [(f, n) for f in bc.FAMILIES for n in bc.names(f)]


# ---------------------------------------------------------------- the generator
def test_generator_gives_distinct_unsorted_columns_and_no_zero():
    lens = [0, 5, 1, 17, 0, 40]
    bptr, bidx, val = bc.bsr_from_lengths(lens, 40, 2, 3, seed=1)
    assert bptr.dtype == bidx.dtype == np.int32 and val.dtype == np.float64
    assert np.array_equal(np.diff(bptr), lens) and len(bidx) == 63 and len(val) == 63 * 6
    rows = [bidx[bptr[r]:bptr[r + 1]] for r in range(len(lens))]
    assert all(len(set(r.tolist())) == len(r) for r in rows)
    assert any(np.any(np.diff(r) < 0) for r in rows)
    assert np.all(val != 0.0) and np.all((val >= -1) & (val < 1))
    bptr, bidx, val = bc.bsr_from_lengths([0, 0, 0], 4, 3, 3, seed=1)
    assert bptr.tolist() == [0, 0, 0, 0] and len(bidx) == 1 and len(val) == 1


@pytest.mark.parametrize("family,name", every_case())
def test_case_arrays(family, name):
    c = bc.case(family, name)
    assert len(c["x"]) == c["nc"] * c["bnc"] and len(c["y"]) == c["nr"] * c["bnr"]
    assert 1 <= c["nr"] < 1000 and c["lens"].max(initial=0) <= 2 * max(bc.ROWS_CAP.values()) + 5
    assert int(c["bidx"].max()) < c["nc"]


# ---------------------------------------------------------------- the oracle
@pytest.mark.parametrize("family,name", every_case())
def test_oracle_is_the_numpy_chain(family, name):
    c = bc.case(family, name)
    y = bc.chain(c["nr"], c["bnr"], c["bnc"], c["bptr"], c["bidx"], c["val"], c["x"])
    assert np.array_equal(bc.bits(y), bc.bits(c["y"]))


def other_cases():
    out = [bc.generic_case(bnr, bnc, nr) for bnr, bnc in bc.GENERIC_SHAPES + bc.GENERIC_UNALIGNED for nr in bc.generic_nrs(bnr)]
    out += [bc.align_case(bs) for bs in (2, 3, 4)] + [bc.border_case(bs) for bs in (2, 3, 4)] + [bc.range_case(k) for k in bc.KIND_CONFIGS]
    out += [bc.dot_case(bs, nr) for bs in (2, 3, 4) for nr in bc.DOT_NR] + [bc.dot_case(bs, 65, 1) for bs in (2, 3, 4)]
    return out


def test_oracle_is_the_numpy_chain_on_the_other_cases():
    for c in other_cases():
        y = bc.chain(c["nr"], c["bnr"], c["bnc"], c["bptr"], c["bidx"], c["val"], c["x"])
        assert np.array_equal(bc.bits(y), bc.bits(c["y"])), (c["nr"], c["bnr"], c["bnc"])


@pytest.mark.parametrize("variant", bc.SPECIAL_VARIANTS)
@pytest.mark.parametrize("shape", [(1, 1), (2, 2), (3, 3), (4, 4), (2, 3)])
def test_special_values(shape, variant):
    """the oracle against the chain where both are not NaN, NaN in the same places; and what each variant is built to show"""
    c = bc.special_case(*shape, variant)
    bnr = shape[0]
    y = bc.chain(c["nr"], c["bnr"], c["bnc"], c["bptr"], c["bidx"], c["val"], c["x"])
    nan = np.isnan(c["y"])
    assert np.array_equal(nan, np.isnan(y)) and np.array_equal(bc.bits(y[~nan]), bc.bits(c["y"][~nan]))
    assert np.all(bc.bits(c["y"][9 * bnr:10 * bnr]) == 0)                      # the empty block row: +0.0
    if variant == "inf_nan":
        assert np.isinf(c["y"][9 * bnr - 1]) and nan[10 * bnr:11 * bnr].all()
        assert nan[3 * bnr:4 * bnr].all()                                      # 0.0 * Inf in every row of the block with the zero column
        assert np.isfinite(c["y"]).sum() > c["nr"] * bnr // 2
    elif variant == "negative_zero":
        prods = c["val"][:, None] * 0.0
        assert np.all(np.signbit(prods)) and np.all(bc.bits(c["y"]) == 0)
    else:
        tiny = np.finfo(np.float64).tiny
        assert np.all(np.abs(c["val"]) < tiny) and np.all(c["val"] != 0.0)
        assert np.all(np.abs(c["y"]) < tiny) and np.count_nonzero(c["y"]) > c["nr"] * bnr // 2


RECT = [(r, c) for r in range(1, 5) for c in range(1, 5)] + [(5, 5)]


@pytest.mark.parametrize("bnr,bnc", RECT, ids=[f"{r}x{c}" for r, c in RECT])
@pytest.mark.parametrize("n", [120, 127])
def test_oracle_is_the_reference_at_every_block_size(reflib, bnr, bnc, n):
    """orc.csr2bsr and orc.spmv_bsr against lis_matrix_convert + lis_matvec (a hand-unrolled function per size in lis_matvec_bsr.c), in arrays
    and in bits; n = 127 is no multiple of 2, 3, 4 or 5"""
    import lisdrv
    ptr, idx, val = orc.random_csr(n, 7, seed=11 + n)
    x = np.random.default_rng(n).uniform(-1, 1, n)
    A = lisdrv.make_csr(reflib, ptr, idx, val)
    B = lisdrv.convert(reflib, A, "bsr", bnr, bnc)
    arrs = lisdrv.matrix_arrays(B)
    nr, bptr, bidx, bval = orc.csr2bsr(ptr, idx, val, bnr, bnc)
    assert nr == arrs["nr"]
    assert np.array_equal(bptr, arrs["bptr"]) and np.array_equal(bidx, arrs["bindex"])
    assert np.array_equal(bc.bits(bval), bc.bits(arrs["value"]))
    y = orc.spmv_bsr(n, nr, bnr, bnc, bptr, bidx, bval, x)
    assert np.array_equal(bc.bits(y), bc.bits(lisdrv.matvec(reflib, B, x)))
    reflib.lis_matrix_destroy(A)
    reflib.lis_matrix_destroy(B)


# ---------------------------------------------------------------- A. the rows kernel
@pytest.mark.parametrize("bs", [2, 3, 4])
def test_rows_cases_hit_their_edges(bs):
    fam, cap, u = f"rows{bs}", bc.ROWS_CAP[bs], bc.ROWS_U[bs]
    grid = lambda nr: -(-nr // bc.ROWS_BRW)
    for nr in bc.ROWS_NR:
        c = bc.case(fam, f"nr{nr}")
        assert c["nr"] == nr and len(bc.rows_passes(c["bptr"], bs)) == grid(nr)
        assert set(c["lens"].tolist()) <= set(bc.rows_pool(bs))
        if nr >= 6:
            assert set(c["lens"].tolist()) == {0, 1, u - 1, u, u + 1, 2 * u + 1}
        else:
            assert c["lens"][0] == 2 * u + 1                 # two full batches and a last one clamped after one block
    seen = set()
    for label in bc.ROWS_SLICES:
        total = bc.slice_blocks(cap, label)
        for border in ("inside", "between"):
            c = bc.case(fam, f"slice_{label}_{border}")
            front, mid, last = bc.rows_passes(c["bptr"], bs)
            r = bc.slice_front(label, border)
            assert len(front) == 1 and front[0]["cend"] % 4 == r == mid[0]["cb"] % 4
            assert mid[0]["cb"] - mid[0]["ka"] == r
            assert mid[-1]["cend"] - mid[0]["cb"] == total and len(mid) == -(-total // cap)
            assert [p["cb"] for p in mid] == [mid[0]["cb"] + k * cap for k in range(len(mid))]
            assert all(p["cnt"] <= cap + 3 for p in mid)         # what the stage holds: CAP + 4 blocks
            if len(mid) > 1:
                assert bc.inside_a_row(c["bptr"], mid[1]["cb"]) == (border == "inside")
                seen.add((r, border))
            assert len(last) == 1 and last[0]["cnt"] - (last[0]["cb"] - last[0]["ka"]) == 3
    assert {r for r, _ in seen} == {0, 1, 2, 3} and {b for _, b in seen} == {"inside", "between"}
    c = bc.case(fam, "long_row")
    assert c["lens"].max() == 2 * cap + 5 and len(bc.rows_passes(c["bptr"], bs)[0]) >= 3
    for m in range(4):
        c = bc.case(fam, f"tail_{m}")
        assert c["bnnz"] % 4 == m and c["nr"] > bc.ROWS_BRW
        final = bc.rows_passes(c["bptr"], bs)[-1][-1]
        assert final["cend"] == c["bnnz"] and final["scalar"] == (m != 0)
        assert final["tail"] == (bs == 3 and final["cnt"] % 2 == 1) and final["cnt"] % 2 == m % 2
        assert not any(p["scalar"] or p["tail"] for wg in bc.rows_passes(c["bptr"], bs)[:-1] for p in wg)
    c = bc.case(fam, "empty_end")
    assert not c["lens"][60:].any() and c["lens"][59] > 0 and bc.rows_passes(c["bptr"], bs)[1] == []
    c = bc.case(fam, "no_blocks")
    assert c["bnnz"] == 0 and len(c["bidx"]) == 1 and bc.rows_passes(c["bptr"], bs) == [[], []]


# ---------------------------------------------------------------- B. the team kernel
@pytest.mark.parametrize("bs", [2, 3, 4])
def test_team_cases_hit_their_edges(bs):
    fam = f"team{bs}"
    for nr in bc.TEAM_NR:
        c = bc.case(fam, f"nr{nr}")
        groups = bc.team_groups(c["bptr"], bs)
        assert c["nr"] == nr and len(groups) == -(-nr // bc.TEAM_RPW) and c["lens"].max() == bc.TEAM_MAX
        assert all(g["branch"] != "fallback" for g in groups)
        if nr >= 7:
            assert set(c["lens"].tolist()) == set(bc.TEAM_POOL)
    branches = lambda name: [g["branch"] for g in bc.team_groups(bc.case(fam, name)["bptr"], bs)]
    assert branches("empty_group") == ["team", "empty", "team"]
    assert branches("fallback_33") == ["team", "fallback", "team"] and bc.case(fam, "fallback_33")["lens"].max() == bc.TEAM_MAX + 1
    for name, odd in (("k0_odd", 1), ("k0_even", 0)):
        g = bc.team_groups(bc.case(fam, name)["bptr"], bs)[1]
        assert g["k0"] % 2 == odd and g["k0"] - g["ka"] == odd and g["branch"] == "team"
    for name, odd in (("end_odd", 1), ("end_even", 0)):
        c = bc.case(fam, name)
        g = bc.team_groups(c["bptr"], bs)[-1]
        assert g["k1"] == c["bnnz"] and (g["k1"] - g["ka"]) % 2 == odd and g["branch"] == "team"
        assert g["tail"] == (bs == 3 and odd == 1)
    c = bc.case(fam, "trailing_empty")
    assert branches("trailing_empty") == ["team", "team", "empty"]
    assert np.all(c["bptr"][13:] == c["bnnz"]) and c["lens"][12] > 0


# ---------------------------------------------------------------- C. the two-phase kernels
@pytest.mark.parametrize("variant", list(bc.TILE_VARIANTS))
def test_tile_cases_hit_their_edges(variant):
    bs, brw, chunk = bc.TILE_VARIANTS[variant]
    assert (brw, chunk) == ((128, 1024) if variant == "pair22" else {1: (256, 4096), 2: (128, 1024), 3: (85, 455), 4: (64, 256)}[bs])
    for nr in (brw - 1, brw, brw + 1):
        c = bc.case(variant, f"nr{nr}")
        assert c["nr"] == nr and len(bc.tile_passes(c["bptr"], brw, chunk)) == -(-nr // brw)
        assert set(c["lens"].tolist()) == set(bc.TILE_POOL) and all(k % bc.TILE_UP for k in bc.TILE_POOL if k)
    for label, d in bc.TILE_SLICES.items():
        c = bc.case(variant, f"slice_{label}")
        first, second = bc.tile_passes(c["bptr"], brw, chunk)
        assert sum(k for _, k in first) == chunk + d and len(second) == 1 and second[0][1] == 3
        assert [k for _, k in first] == ([chunk, 1] if d == 1 else [chunk + d])
        if d == 1:
            assert bc.inside_a_row(c["bptr"], first[1][0])
        assert np.any(c["lens"] % bc.TILE_UP != 0)


# ---------------------------------------------------------------- D / E / F. shapes, alignments, ranges
def test_generic_row_counts_surround_one_workgroup():
    for bnr, _ in bc.GENERIC_SHAPES + bc.GENERIC_UNALIGNED:
        rows = [nr * bnr for nr in bc.generic_nrs(bnr)]
        assert rows[0] <= bc.GENERIC_ROWS - 1 < rows[0] + bnr and rows[-1] >= bc.GENERIC_ROWS + 1 > rows[-1] - bnr
        assert (bc.GENERIC_ROWS in rows) == (bc.GENERIC_ROWS % bnr == 0)
    assert {nr * 1 for nr in bc.generic_nrs(1)} == {255, 256, 257}


def test_kind_model_at_the_values_the_dispatcher_documents():
    k = bc.kind_model
    assert [k(100, 1200, 2, 2), k(100, 1201, 2, 2), k(100, 1201, 2, 2, team=0)] == [bc.ROWS, bc.TEAM, bc.PAIR22]
    assert [k(100, 1600, 3, 3), k(100, 1601, 3, 3), k(100, 1601, 3, 3, team=0)] == [bc.ROWS, bc.TEAM, bc.TILE]
    assert [k(100, 1200, 4, 4), k(100, 1201, 4, 4), k(100, 1201, 4, 4, team=2)] == [bc.ROWS, bc.TILE, bc.TEAM]
    assert [k(100, -1, 2, 2), k(100, -1, 3, 3), k(100, -1, 4, 4), k(100, -1, 1, 1)] == [bc.ROWS, bc.TILE, bc.TILE, bc.TILE]
    assert [k(100, 0, 2, 2, x16=False), k(100, 0, 2, 2, y16=False), k(100, 0, 2, 2, bidx16=False)] == [bc.TILE, bc.PAIR22, bc.PAIR22]
    assert [k(100, 0, 3, 3, x16=False, y16=False), k(100, 0, 3, 3, bidx16=False)] == [bc.ROWS, bc.TILE]
    assert [k(100, 0, 4, 4, y16=False), k(100, 0, 5, 5), k(100, 0, 2, 3)] == [bc.TILE, bc.GENERIC, bc.GENERIC]
    assert all(k(100, 0, b, b, val16=False) == bc.GENERIC for b in (1, 2, 3, 4))
    assert len(list(bc.kind_grid())) == 11 * 6 * 3 * 16
    assert {bc.kind_model(*g[:4], team=g[4], bidx16=g[5], val16=g[6], x16=g[7], y16=g[8]) for g in bc.kind_grid()} == set(range(5))


def test_kind_configs_force_their_kind():
    for name, cfg in bc.KIND_CONFIGS.items():
        c = bc.range_case(name)
        assert bc.config_kind(cfg, c["nr"]) == cfg["kind"], name
        assert c["nr"] == 2 * cfg["wg"] + 9 < 1000 and c["lens"].max() <= bc.TEAM_MAX
        parts = bc.range_partitions(c["nr"], cfg["wg"])
        for label, p in parts.items():
            covered = np.zeros(c["nr"], int)
            for rb, re in p:
                covered[rb:re] += 1
            assert np.all(covered == 1), (name, label)
        assert any(rb == re for rb, re in parts["an_empty_range_between"])
    assert {cfg["kind"] for cfg in bc.KIND_CONFIGS.values()} == set(range(5))


@pytest.mark.parametrize("bs", [2, 3, 4])
def test_border_case_truncates_to_the_other_side(bs):
    """the whole matrix is one block over the threshold; the share bnnz * (bre - brb) / nr of half of it, in integers, is not"""
    c = bc.border_case(bs)
    t, nr = int(bc.THRESHOLD[bs]), bc.BORDER_NR
    team = 2 if bs == 4 else 1
    assert c["bnnz"] == t * nr + 1 and bc.kind_model(nr, c["bnnz"], bs, bs, team=team) == bc.TEAM
    assert bc.kind_model(50, c["bnnz"] * 50 // nr, bs, bs, team=team) == bc.ROWS


# ---------------------------------------------------------------- G. the fused sums
@pytest.mark.parametrize("bs", [2, 3, 4])
@pytest.mark.parametrize("nr", bc.DOT_NR)
def test_dot_cases_and_model(bs, nr):
    c = bc.dot_case(bs, nr)
    assert c["bnnz"] == int(bc.THRESHOLD[bs]) * nr and bc.kind_model(nr, c["bnnz"], bs, bs) == bc.ROWS
    assert bc.dot_case(bs, 65, 1)["bnnz"] == int(bc.THRESHOLD[bs]) * 65 + 1
    for k in range(bs):
        n = nr * bs - k
        for sumsq in (0, 1):
            a = c["y"][:n] if sumsq else c["w"][:n]
            terms = (a * c["y"][:n]).tolist()
            exact = math.fsum(terms)
            bound = (n - 1) * 2.0 ** -53 * math.fsum(map(abs, terms)) + np.spacing(abs(exact))
            assert abs(float(bc.dot_model(bs, nr, n, c["w"], c["y"], sumsq)) - exact) <= bound, (n, sumsq)
    if bs > 1 and nr * bs > 2:                               # the padding rows are not in the sums: they would change them
        n = nr * bs - (bs - 1)
        assert bc.dot_model(bs, nr, n, c["w"], c["y"], 1) != bc.dot_model(bs, nr, nr * bs, c["w"], c["y"], 1)


@pytest.mark.parametrize("bs", [2, 3, 4])
def test_dot_padding_case_has_an_infinite_padding_row(bs):
    c = bc.dot_padding_case(bs)
    n = 65 * bs - 1
    assert np.isinf(c["y"][n]) and np.isfinite(c["y"][:n]).all() and np.isfinite(c["w"]).all()
    assert np.array_equal(bc.bits(c["y"]), bc.bits(bc.chain(c["nr"], bs, bs, c["bptr"], c["bidx"], c["val"], c["x"])))
    for sumsq in (0, 1):
        assert np.isfinite(bc.dot_model(bs, 65, n, c["w"], c["y"], sumsq))
        assert bc.dot_model(bs, 65, n, c["w"], c["y"], sumsq) == bc.dot_model(bs, 65, n, c["w"], np.where(np.isinf(c["y"]), 1.0, c["y"]), sumsq)
