"""X -> CSR without a GPU: the numpy models of tests/tocsr_cases.py, which tests/test_tocsr_gpu.py holds the kernels and the HBM path to, are held here to the
reference (oracle/_ref, one thread) and to the library's own host routine (lisi_convert_to_csr, lis_amd_set_device_convert(0)) on every source of that module --
every integer, and every bit of every value: zeros of both signs, NaN with a payload, infinities and subnormals included.  The facts the hand-written sources
promise are asserted."""
import numpy as np
import pytest

import convert_cases as cc
import lis_amd
import tocsr_cases as tc
import tocsr_drv as drv


@pytest.fixture(scope="module")
def lib():
    lib = lis_amd.load()
    assert lib.initialize([]) == 0
    lib.dll.lis_amd_set_device_convert(0)          # the host routine is what this file checks, with or without a GPU in the machine
    yield lib
    lib.dll.lis_amd_set_device_convert(1)


def _converted(L, s):
    A = drv.make(L, s)
    err, B = drv.to_csr(L, A)
    assert err == 0
    got = drv.csr_arrays(B)
    L.lis_matrix_destroy(B); L.lis_matrix_destroy(A)
    return got


@pytest.mark.parametrize("key", [k for k in tc.ALL if k not in tc.NO_REFERENCE])
def test_model_reference_and_host_routine_agree(lib, reflib, key):
    s = tc.source(key)
    want = tc.model(s)
    for who, L in (("reference", reflib), ("host routine", lib)):
        ok, which = tc.same_csr(_converted(L, s), want)
        assert ok, (who, key, which)


@pytest.mark.parametrize("key", list(tc.NO_REFERENCE))
def test_bsr_where_the_reference_defines_nothing(lib, key):
    """NOT held to the reference: a block that reaches beyond the n rows or columns holds non-zeros there.  lis_matrix_convert_bsr2csr counts such a value of
    a padding row past the end of its ptr[] and gives one of a padding column a column >= n (tocsr_cases.NO_REFERENCE); the host routine, the model and the
    kernels leave them out, and with the padding zeroed -- the same source as csr2bsr would have stored it -- the reference agrees (the test above)."""
    s = tc.source(key)
    assert key in tc.HAND and s["fmt"] == "bsr" and (s["n"] % s["bnr"] or s["n"] % s["bnc"])
    clean = dict(s, value=tc._bsr_padding_zeroed(s))
    assert not cc.same_bits(clean["value"], s["value"])
    want = tc.model(s)
    assert tc.same_csr(tc.model(clean), want)[0]
    ok, which = tc.same_csr(_converted(lib, s), want)
    assert ok, (key, which)


@pytest.mark.parametrize("key", [k for k in tc.ALL if tc.source(k)["fmt"] in ("csc", "jad")])
def test_csc_and_jad_rows_of_the_upload_are_the_conversion(key):
    """CSC and JAD have no kernel: lis_convert_tocsr.c copies the three arrays of the source's HBM copy.  That copy is laid out by upload_csc_as_csr /
    upload_jad_as_csr (lis_upload.c; restated in tocsr_cases), or by build_csc / build_jad as a clone of the CSR source's rows; both must be the rows of
    csc2csr / jad2csr -- which the test above holds to the reference -- on every case, rows out of order and columns stored twice included"""
    s = tc.source(key)
    rows = tc.csc_upload_rows(s) if s["fmt"] == "csc" else tc.jad_upload_rows(s)
    ok, which = tc.same_csr(rows, tc.model(s))
    assert ok, (key, which)
    name = tc.FROM_CSR[key][0]
    if not cc.is_unsorted(*cc.CASES[name][:2]) or s["fmt"] == "jad":      # (CSC is built in HBM from rows in ascending column order only: lisd_convert_csr)
        ok, which = tc.same_csr(cc.CASES[name], tc.model(s))              # build_csc / build_jad: the copy is a clone of the CSR source
        assert ok, (key, "clone", which)


def test_the_host_path_is_counted_and_leaves_nothing_in_hbm(lib):
    s = tc.source("ell_specials")
    before = drv.stats(lib)
    A = drv.make(lib, s)
    err, B = drv.to_csr(lib, A)
    assert err == 0 and lib.dll.lis_amd_matrix_lazy_arrays(B) == 0
    after = drv.stats(lib)
    assert (after[0] - before[0], after[1] - before[1]) == (0, 1)
    lib.lis_matrix_destroy(B); lib.lis_matrix_destroy(A)


def _dropped(s):
    """per row: (stored entries the model could keep, kept)"""
    return np.diff(tc.model(s)[0])


def test_the_cases_are_what_they_say():
    H = tc.HAND
    bits = lambda v: np.ascontiguousarray(v, np.float64).view(np.uint64)
    # one row stores +0.0, -0.0, NaN (one with a payload), both infinities and a subnormal; the zeros go, the others stay with their bits
    row = np.array(tc.SPECIAL_ROW)
    assert (row == 0).sum() == 3 and np.signbit(row[row == 0]).sum() == 2 and np.isnan(row).sum() == 2 and np.isinf(row).sum() == 2 and (row == 5e-324).sum() == 1
    assert bits(row[6:7])[0] == 0x7FF8000000ABCDEF
    for key in ("ell_specials", "dns_specials"):
        s = H[key]
        ptr, idx, val = tc.model(s)
        r1 = val[ptr[1]:ptr[2]]
        stored = tc.SPECIAL_ROW if key == "ell_specials" else tc.SPECIAL_ROW[:s["n"]]
        kept = [v for v in stored if v != 0.0]
        assert bits(r1).tolist() == bits(np.array(kept)).tolist(), key
        assert ptr[3] == ptr[2], key                                    # row 2: all dropped
        assert ptr[4] - ptr[3] == (s["maxnzr"] if key == "ell_specials" else s["n"]), key      # row 3: none dropped
    s = H["dia_corners"]
    assert set([-(s["n"] - 1), s["n"] - 1]) <= set(s["index"].tolist()) and list(s["index"]) != sorted(s["index"])
    d = _dropped(s)
    reach = [(sum(0 <= i + int(o) < s["n"] for o in s["index"])) for i in range(s["n"])]
    assert d[2] == 0 and reach[2] > 0 and d[3] == reach[3] > 0
    ptr, idx, val = tc.model(s)
    assert (0 in idx[ptr[s["n"] - 1]:ptr[s["n"]]]) and (s["n"] - 1 in idx[ptr[0]:ptr[1]])       # the corners are reached and kept
    assert H["ell_maxnzr1"]["maxnzr"] == 1 and H["dia_nnd1"]["nnd"] == 1 and H["dia_nnd1_top"]["nnd"] == 1
    assert H["dia_nnd1"]["index"][0] == -5 and np.diff(tc.model(H["dia_nnd1"])[0]).tolist() == [0, 0, 0, 0, 0, 1]
    assert H["dia_nnd1_top"]["index"][0] == 5 and np.diff(tc.model(H["dia_nnd1_top"])[0]).tolist() == [1, 0, 0, 0, 0, 0]
    for key in ("ell_n1", "dia_n1", "dns_n1", "bsr_2x2_n1", "vbr_n1"):
        assert H[key]["n"] == 1 and len(tc.model(H[key])[0]) == 2, key
    assert tc.model(H["bsr_2x2_n1"])[2].tolist() == [3.5]               # the padding row and column hold values that are no entries
    for bnr, bnc in tc.BSR_SHAPES:
        s = H["bsr_%dx%d_n7" % (bnr, bnc)]
        assert (s["bnr"], s["bnc"]) == (bnr, bnc) and (bnr == 1 or s["n"] % bnr != 0)
        out_of_order = any(np.any(np.diff(s["bindex"][s["bptr"][b]:s["bptr"][b + 1]]) < 0) for b in range(s["nr"]))
        assert out_of_order and (s["value"] == 0).any() and np.isnan(s["value"]).any()
        assert cc.is_unsorted(*tc.model(s)[:2])                         # ... and the rows keep the blocks' stored order
    s = H["vbr_1to3"]
    assert set(np.diff(s["row"]).tolist()) == {1, 2, 3} and (s["value"] == 0).any() and np.signbit(s["value"][s["value"] == 0]).any()
    assert len(tc.model(s)[1]) < s["nnz"]
    # the sources made from CSR: what the conversion dropped are exactly the format's padding zeros and the stored zeros of the CSR matrix
    for name in ("specials", "empties", "unsorted"):
        csr = cc.CASES[name]
        nz = int(np.count_nonzero(csr[2] != 0.0))
        for fmt in ("ell", "dns", "csc", "jad"):
            got = len(tc.model(tc.source("%s-%s" % (name, fmt)))[1])
            assert got == (len(csr[1]) if fmt in ("csc", "jad") else nz), (name, fmt)
    assert set(tc.KERNEL_FORMATS) | {"csc", "jad"} == set(tc.FORMATS)


@pytest.mark.parametrize("fmt", tc.KERNEL_FORMATS)
def test_random_sources_are_valid_and_hit_every_kind_of_value(fmt):
    for n, width in ((1, 1), (7, 2), (65, 7), (257, 33)):
        s = tc.random_source(fmt, n, width)
        ptr, idx, val = tc.model(s)
        assert ptr[-1] == len(idx) == len(val) and (len(idx) == 0 or (idx.min() >= 0 and idx.max() < s.get("np", n)))
        assert not (val == 0.0).any()
        if n * width >= 64 and fmt in ("ell", "dns"):                # (every stored value is an entry there)
            assert np.isnan(val).any() and np.isinf(val).any() and (s["value"] == 0).any() and np.signbit(s["value"][s["value"] == 0]).any()
