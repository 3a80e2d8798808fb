"""lis_gesolve and lis_matrix_shift_matrix, the parts that need no GPU: the numpy model of the shift (tests/shift_model.py) against the goldens taken from the
reference (tests/golden/gesolve_bits.*) and, where oracle/_ref exists, against the reference itself, in every bit; every refusal of lis_gesolve -- its code, its
words, A, B and x untouched --; the prototypes in the headers and the exported symbols.  The GPU side is tests/test_shift_matrix_gpu.py and test_gesolve_gpu.py."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import gesolve_cases as gc
import gesolve_drv as gd
import lis_amd
import lisdrv
import shift_model as sm
from lis_amd import _capi as capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
META = json.load(open(os.path.join(GOLDEN, "gesolve_bits.json")))
BITS = np.load(os.path.join(GOLDEN, "gesolve_bits.npz"))
CSR_SHIFTS = sorted(k for k, v in gc.SHIFTS.items() if v[2] in ("csr", "hbm"))


@pytest.fixture(scope="module")
def lib():
    lib = lis_amd.load()
    assert lib.initialize([]) == 0
    return lib


def _same_csr(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, "ptr")
    assert np.array_equal(got[1], want[1]), (what, "index")
    assert np.array_equal(np.asarray(got[2]).view(np.int64), np.asarray(want[2]).view(np.int64)), (what, "value")


# ---------------------------------------------------------------------------------------------- the model
@pytest.mark.parametrize("name", CSR_SHIFTS)
def test_model_equals_the_goldens_in_every_bit(name):
    maker, sigmas, _ = gc.SHIFTS[name]
    A, B = maker()
    for step, (ptr, idx, val, _) in enumerate(sm.apply(A, B, sigmas)):
        key = "shift|%s|%d" % (name, step)
        assert META["shifts"][key]["nnz"] == len(idx)
        _same_csr((ptr, idx, val), (BITS[key + "|ptr"], BITS[key + "|index"], BITS[key + "|value"]), key)


def test_every_shift_case_of_the_issue_is_among_the_goldens():
    assert len(CSR_SHIFTS) == len(gc.SHIFTS) - 2 and {gc.SHIFTS[k][2] for k in gc.SHIFTS} == {"csr", "hbm", "ell", "bsr"}
    want = sum(len(gc.SHIFTS[k][1]) for k in CSR_SHIFTS)
    assert len(META["shifts"]) == want


@pytest.mark.parametrize("name", CSR_SHIFTS)
def test_model_equals_the_reference(reflib, name):
    maker, sigmas, _ = gc.SHIFTS[name]
    a, b = maker()
    A, B = gd.make(reflib, a), gd.make(reflib, b)
    for step, (ptr, idx, val, _) in enumerate(sm.apply(a, b, sigmas)):
        assert gd.shift(reflib, A, B, sigmas[step]) == 0
        assert A.contents.nnz == len(idx)
        _same_csr(gd.csr_arrays(A), (ptr, idx, val), (name, step))
    reflib.lis_matrix_destroy(A)
    reflib.lis_matrix_destroy(B)


def test_the_paths_of_the_cases_are_the_ones_they_are_named_for():
    """which shifts keep A's layout (one launch on the GPU) and which rebuild it, by the model's own rule"""
    paths = {k: [p[3] for p in sm.apply(*gc.SHIFTS[k][0](), gc.SHIFTS[k][1])] for k in gc.SHIFTS}
    assert paths["subset_sorted"] == [True, True] and paths["subset_unsorted"] == [False, True] and paths["not_subset"] == [False, False]
    assert paths["cancel"] == [False, False] and paths["empty_rows"] == [False, False] and paths["n1"] == [True, True]
    assert paths["sigma0"] == [True] and paths["sigma0_not_subset"] == [False] and paths["negative"] == [True, True]
    assert paths["long_rows"] == [False, False] and paths["long_rows_shuffled"] == [False, False]
    assert paths["rows_255"] == [True, True] and paths["rows_257"] == [True, True]
    A, B = gc.SHIFTS["cancel"][0]()
    ptr, idx, val, _ = sm.apply(A, B, (0.5,))[0]
    assert ptr.tolist() == [0, 0, 2, 4, 5] and idx.tolist() == [0, 2, 1, 2, 3]          # row 0 empty, row 1 lost its middle entry, row 3 its stored zero
    lens = np.diff(gc.SHIFTS["long_rows"][0]()[0][0])[:4].tolist(), np.diff(gc.SHIFTS["long_rows"][0]()[1][0])[:4].tolist()
    assert lens == ([65, 65, 300, 300], [1, 200, 1, 200])


def test_the_round_trip_does_not_give_the_bits_back():
    """+sigma then -sigma: the pattern comes back, the values in general do not (the reference has that drift, and so has the library)"""
    A, B = gc.P3()
    back = sm.apply(A, B, (0.3, -0.3))[1]
    assert np.array_equal(back[0], A[0]) and np.array_equal(back[1], A[1])
    assert not np.array_equal(back[2].view(np.int64), A[2].view(np.int64)) and np.allclose(back[2], A[2], rtol=1e-15, atol=0)


# ---------------------------------------------------------------------------------------------- refusals
def _snapshot(lib, A, B, vx):
    def arrays(M):
        return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in lisdrv.matrix_arrays(M).items()}
    return arrays(A), (arrays(B) if B else None), lisdrv.get_vector(lib, vx).copy()


def _same(s1, s2):
    for m1, m2 in zip(s1[:2], s2[:2]):
        assert (m1 is None) == (m2 is None)
        for k in (m1 or {}):
            assert np.array_equal(m1[k], m2[k]), k
    assert np.array_equal(s1[2].view(np.int64), s2[2].view(np.int64))


# (options, B given, through lis_esolve, code, words the message must hold)
REFUSED = [
    ("-e cr", True, False, 5, ["generalized", "-e cr", "standard"]), ("-e pi", True, False, 5, ["generalized"]), ("-e si -ss 2", True, False, 5, ["generalized"]),
    ("-e gpi", False, True, 5, ["not served", "without a matrix B"]), ("-e gii", False, True, 5, ["not served"]), ("-e grqi", False, True, 5, ["not served"]),
    ("-e gcr", False, True, 5, ["not served"]), ("-e gcr", False, False, 5, ["not served", "without a matrix B"]),
    ("-e gcg", True, False, 5, ["not served", "never updates x", "NaN", "-e gcr"]),
    ("-e gsi", True, False, 5, ["not served", "several pairs"]), ("-e gli", True, False, 5, ["not served", "several pairs"]), ("-e gai", True, False, 5, ["not served", "several pairs"]),
    ("-e gii -ef quad", True, False, 1, ["Quad precision is not enabled"]), ("-e gii -ef switch", True, False, 1, ["Quad precision is not enabled"]),
    ("-e gii -estorage msr", True, False, 5, ["not served"]), ("-e gii -emaxiter -3", True, False, 1, []),
]


@pytest.mark.parametrize("text,with_b,through_esolve,code,words", REFUSED)
def test_refusals_fire_before_A_B_or_x_is_touched(lib, text, with_b, through_esolve, code, words, capfd):
    a, b = gc.P4()                                     # unsorted rows: any touch of A would show
    A, B = gd.make(lib, a), (gd.make(lib, b) if with_b else None)
    vx = lisdrv.new_vector(lib, A, np.cos(np.arange(len(a[0]) - 1.0)))
    before = _snapshot(lib, A, B, vx)
    E = capi.PE()
    assert lib.lis_esolver_create(C.byref(E)) == 0 and lib.lis_esolver_set_option(text.encode(), E) == 0
    ev = C.c_double(-7.0)
    err = lib.lis_esolve(A, vx, C.byref(ev), E) if through_esolve else lib.lis_gesolve(A, B, vx, C.byref(ev), E)
    assert err == code and ev.value == -7.0 and E.contents.retcode == code
    message = capfd.readouterr().out
    for w in words:
        assert w in message, (w, message)
    _same(before, _snapshot(lib, A, B, vx))
    assert not E.contents.evalue                       # nothing was allocated for a refused solve
    lib.lis_esolver_destroy(E)
    lib.lis_vector_destroy(vx)
    lib.lis_matrix_destroy(A)
    if B:
        lib.lis_matrix_destroy(B)


def test_A_and_B_of_different_size_are_an_illegal_argument(lib, capfd):
    a, _ = gc.P1()
    _, b = gc.SHIFTS["rows_255"][0]()
    A, B = gd.make(lib, a), gd.make(lib, b)
    vx = lisdrv.new_vector(lib, A, np.ones(30))
    before = _snapshot(lib, A, B, vx)
    E = capi.PE()
    assert lib.lis_esolver_create(C.byref(E)) == 0 and lib.lis_esolver_set_option(b"-e gii", E) == 0
    ev = C.c_double(-7.0)
    assert lib.lis_gesolve(A, B, vx, C.byref(ev), E) == capi.LIS_ERR_ILL_ARG and ev.value == -7.0
    assert "matrix B" in capfd.readouterr().out
    assert gd.shift(lib, A, B, 0.5) == capi.LIS_ERR_ILL_ARG
    assert "differ in size" in capfd.readouterr().out
    _same(before, _snapshot(lib, A, B, vx))
    lib.lis_esolver_destroy(E)
    lib.lis_vector_destroy(vx)
    lib.lis_matrix_destroy(A)
    lib.lis_matrix_destroy(B)


def test_a_split_matrix_is_not_shifted_by_a_matrix(lib, capfd):
    a, b = gc.P1()
    A, B = gd.make(lib, a), gd.make(lib, b)
    assert lib.lis_matrix_split(A) == 0
    assert gd.shift(lib, A, B, 0.5) == capi.LIS_ERR_NOT_IMPLEMENTED
    assert "split" in capfd.readouterr().out
    lib.lis_matrix_destroy(A)
    lib.lis_matrix_destroy(B)


# ---------------------------------------------------------------------------------------------- headers and symbols
def test_the_headers_declare_the_new_prototypes():
    def text(name):
        return re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", name)).read())
    assert "LIS_INT lis_matrix_shift_matrix(LIS_MATRIX A, LIS_MATRIX B, LIS_SCALAR sigma);" in text("lis.h")
    assert "LIS_INT lis_amd_last_shift_matrix(LIS_INT info[3]);" in text("lis_amd.h")
    assert "LIS_INT lis_amd_matrix_device_csr(LIS_MATRIX A, LIS_INT **dptr, LIS_INT **dindex, LIS_SCALAR **dvalue);" in text("lis_amd.h")
    h = text("liship.h")
    for name in ("liship_csr_shift_matrix_try_f64", "liship_csr_shift_matrix_scan", "liship_csr_shift_matrix_fill_f64"):
        assert "int " + name + "(" in h, name
    assert "#define LISHIP_SHIFT_MATRIX_ROWS %d" % gc.ROWS_PER_WORKGROUP in h


def test_the_symbols_are_exported_and_bound():
    dll = C.CDLL(lis_amd.LIB_PATH)
    for name in ("lis_matrix_shift_matrix", "lis_amd_last_shift_matrix", "lis_amd_matrix_device_csr", "liship_csr_shift_matrix_try_f64",
                 "liship_csr_shift_matrix_scan", "liship_csr_shift_matrix_fill_f64"):
        assert hasattr(dll, name), name
    assert "lis_matrix_shift_matrix" in capi._PROTOS and "lis_amd_last_shift_matrix" in capi._AMD_PROTOS
    for name in ("liship_csr_shift_matrix_try_f64", "liship_csr_shift_matrix_scan", "liship_csr_shift_matrix_fill_f64"):
        assert name in lis_amd._LISHIP


def test_the_golden_solves_are_the_cases_of_the_issue():
    keys = {gc.solve_key(p, e, x, T) for p, e, x in gc.SOLVES for T in gc.THREADS_BITS}
    assert keys == {k for k in META["solves"] if not k.endswith("|A")}
    for p, e, x in gc.SOLVES:
        case = gc.solve_key(p, e, x, 1).rsplit("|", 1)[0]
        assert sorted(META["spread"][case]) == ["T1", "T2", "T4", "T8"]
        assert all(v["status"] == 0 for v in META["spread"][case].values())
    # the counts measured for the issue on P1 and P2
    count = lambda p, e, T: META["spread"]["%s|-e %s" % (p, e)]["T%d" % T]["iter"]
    assert [count("P1", e, T) for e in ("gpi", "gii", "grqi", "gcr") for T in (1, 8)] == [233, 233, 11, 11, 5, 5, 63, 63]
    assert [count("P2", e, T) for e in ("gcr", "gii") for T in (1, 2, 4, 8)] == [102] * 4 + [165] * 4
