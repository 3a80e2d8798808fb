"""What kernels/convert.hip is held to (tests/test_convert_gpu.py) is held to the reference here, without a GPU.

For every matrix of tests/convert_cases.py and every storage format, the oracle's arrays equal the reference's (oracle/_ref) and the
library's own host routine's (lis_convert.c), every index and every bit of every value -- -0.0, NaN, infinities and subnormals
included.  Three DIA cases have no reference to be held to and are tested by name (test_dia_where_the_reference_defines_nothing).
The row-form restatements (ell_rows / dia_rows / bsr_rows) multiply, as plain CSR rows, to the bits orc.spmv_ell / spmv_dia /
spmv_bsr give on the native arrays.  The facts the generators promise are asserted."""
import numpy as np
import pytest

import convert_cases as cc
import lis_amd
import lisdrv
import orc

FORMATS = [("csc", 0, 0), ("ell", 0, 0), ("dia", 0, 0), ("jad", 0, 0)] + [("bsr", r, c) for r, c in cc.BLOCKS]
FMT_IDS = [f if f != "bsr" else "bsr%dx%d" % (r, c) for f, r, c in FORMATS]
HUBS = [(blocks, r, c, s) for blocks in (cc.BSR_LIST, cc.BSR_LIST + 1) for r, c in cc.HUB_SHAPES for s in (True, False)]
HUB_IDS = ["hub%d_%dx%d_%s" % (b, r, c, "sorted" if s else "unsorted") for b, r, c, s in HUBS]


@pytest.fixture(scope="module")
def lib():
    lib = lis_amd.load()
    assert lib.initialize([]) == 0
    lib.dll.lis_amd_set_device_convert(0)          # the host routine is what this file checks, with or without a GPU in the machine
    yield lib
    lib.dll.lis_amd_set_device_convert(1)


def _converted(L, csr, fmt, bnr, bnc):
    A = lisdrv.make_csr(L, *csr)
    B = lisdrv.convert(L, A, fmt, bnr or 2, bnc or 2)
    got = lisdrv.matrix_arrays(B)
    L.lis_matrix_destroy(A); L.lis_matrix_destroy(B)
    return got


def _check(lib, reflib, csr, fmt, bnr, bnc):
    """reflib = None: the oracle and the host routine only"""
    want = cc.oracle_arrays(fmt, *csr, bnr, bnc)
    for who, L in (("reference", reflib), ("host routine", lib)):
        if L is None:
            continue
        ok, key = cc.same_arrays(_converted(L, csr, fmt, bnr, bnc), want)
        assert ok, (who, fmt, bnr, bnc, key)
    return want


# DIA where the reference defines nothing to hold the oracle to; tested by name below, against the host routine alone
DIA_NO_REFERENCE = {"equal_neighbours": "a column twice in a row", "duplicates": "a column twice in a row", "scan_1": "no entry at all"}
PAIRS = [(c, f) for c in cc.CASES for f in FORMATS if not (f[0] == "dia" and c in DIA_NO_REFERENCE)]


def _row_forms(case, fmt, bnr, bnc, want):
    csr = cc.CASES[case]
    n = len(csr[0]) - 1
    # the row forms, held to the native products (x finite; with NaN / inf values the sums are NaN in the same places, any payload)
    x = np.random.default_rng(4).uniform(-1, 1, n)
    loose = case == "specials"
    if fmt == "ell":
        rows = cc.ell_rows(n, want["maxnzr"], want["index"], want["value"])
        assert cc.same_bits(orc.spmv_csr(*rows, x), orc.spmv_ell(n, want["maxnzr"], want["index"], want["value"], x), loose)
    elif fmt == "dia":
        rows = cc.dia_rows(n, n, want["index"], want["value"])
        assert cc.same_bits(orc.spmv_csr(*rows, x), orc.spmv_dia(n, want["nnd"], want["index"], want["value"], x), loose)
    elif fmt == "bsr":
        rows = cc.bsr_rows(n, bnr, bnc, want["bptr"], want["bindex"], want["value"])
        xp = np.concatenate([x, np.zeros(bnc)])                   # the padding columns of the last block column multiply zeros
        assert cc.same_bits(orc.spmv_csr(*rows, xp), orc.spmv_bsr(n, want["nr"], bnr, bnc, want["bptr"], want["bindex"], want["value"], x), loose)
        assert rows[0][n] == len(rows[1]) == len(rows[2])


@pytest.mark.parametrize("case,fmt", PAIRS, ids=["%s-%s" % (c, FMT_IDS[FORMATS.index(f)]) for c, f in PAIRS])
def test_oracle_reference_and_host_routine_agree(lib, reflib, case, fmt):
    fmt, bnr, bnc = fmt
    _row_forms(case, fmt, bnr, bnc, _check(lib, reflib, cc.CASES[case], fmt, bnr, bnc))


@pytest.mark.parametrize("case", list(DIA_NO_REFERENCE))
def test_dia_where_the_reference_defines_nothing(lib, reflib, case):
    """NOT held to the reference.  A row that stores a column twice: lis_matrix_convert_csr2dia sorts every row with an unstable sort, and which of the two
    values the diagonal keeps follows from that sort's internals; this library, its oracle and its kernels keep the LAST stored one, and the divergence is
    asserted here so that it stays a known one.  A matrix without entries: the reference reads the first element of an array of none."""
    csr = cc.CASES[case]
    want = _check(lib, None, csr, "dia", 0, 0)
    _row_forms(case, "dia", 0, 0, want)
    if len(csr[1]) == 0:
        assert want["nnd"] == 0
        return
    assert cc.repeats_a_column(*csr[:2])
    ptr, idx, val = csr
    n = len(ptr) - 1
    off = want["index"].tolist()
    for r in range(n):                                           # last stored entry wins, row by row
        last = {int(c): v for c, v in zip(idx[ptr[r]:ptr[r + 1]], val[ptr[r]:ptr[r + 1]])}
        for c, v in last.items():
            assert cc.same_bits(want["value"][off.index(c - r) * n + r:off.index(c - r) * n + r + 1], np.array([v]))
    ok, _ = cc.same_arrays(_converted(reflib, csr, "dia", 0, 0), want)
    assert not ok                                                # the known divergence: were it gone, these cases would belong in the test above


@pytest.mark.parametrize("blocks,bnr,bnc,sorted_", HUBS, ids=HUB_IDS)
def test_hub_block_row_sits_on_the_border(lib, reflib, blocks, bnr, bnc, sorted_):
    (ptr, idx, val), br = cc.hub(cc.HUB_N, blocks, bnr, bnc, sorted_)
    n = cc.HUB_N
    assert cc.distinct_blocks(ptr, idx, n, bnr, bnc, br) == blocks
    assert max(cc.distinct_blocks(ptr, idx, n, bnr, bnc, b) for b in range(1 + (n - 1) // bnr) if b != br) <= 5 * bnr < cc.BSR_LIST
    assert cc.is_unsorted(ptr, idx) == (not sorted_)
    want = _check(lib, reflib, (ptr, idx, val), "bsr", bnr, bnc)
    assert want["bptr"][br + 1] - want["bptr"][br] == blocks


def test_the_cases_are_what_they_say():
    C = cc.CASES
    assert cc.is_unsorted(*C["unsorted"][:2]) and cc.is_unsorted(*C["duplicates"][:2]) and cc.is_unsorted(*C["n513_inversion_last"][:2])
    ptr, idx, _ = C["n513_inversion_last"]
    assert not cc.is_unsorted(ptr[:-1], idx[:ptr[-2]])                                      # ... and only its last row is
    ptr, idx, _ = C["duplicates"]
    dup = [r for r in range(600) if len(set(idx[ptr[r]:ptr[r + 1]].tolist())) < ptr[r + 1] - ptr[r]]
    assert len(dup) >= 50 and all(r % 10 == 0 for r in dup)
    ptr, idx, _ = C["equal_neighbours"]
    assert not cc.is_unsorted(ptr, idx) and np.any((np.diff(idx) == 0) & (np.isin(np.arange(1, len(idx)), ptr, invert=True)))
    ptr = C["n257_longest_last"][0]
    assert np.argmax(np.diff(ptr)) == 256 and np.sum(np.diff(ptr) == cc.max_row(ptr)) == 1
    assert len(C["n1"][0]) == 2 and cc.max_row(C["n7_full_row"][0]) == 7
    lens = np.diff(C["empties"][0])
    assert not lens[:256].any() and lens[256:600].all() and not lens[600:].any() and len(lens) == 700
    v = C["specials"][2]
    assert np.isnan(v).any() and np.isinf(v).any() and np.signbit(v[v == 0]).any() and (~np.signbit(v[v == 0])).any() and (v == 5e-324).any()
    assert [c for c in cc.CASES if cc.repeats_a_column(*cc.CASES[c][:2])] == ["equal_neighbours", "duplicates"]
    for name in cc.SORTED:
        assert not cc.is_unsorted(*C[name][:2])
    assert {"specials", "empties", "constant_p3d", "constant_band", "scan_4097"} <= set(cc.SORTED)
    for m in cc.SCAN_SIZES:
        ptr, idx, val = cc.scan(m)
        assert np.array_equal(np.diff(ptr), np.arange(m) % 3) and (len(idx) == 0 or (0 <= idx.min() and idx.max() < m))
        assert len(idx) == 0 or set(np.unique(idx - np.repeat(np.arange(m), np.diff(ptr))).tolist()) <= {-2, -1, 0}
    assert (cc.SCAN_BIG + 4095) // 4096 == 1026
