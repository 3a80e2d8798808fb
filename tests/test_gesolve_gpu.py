"""Whole generalized eigensolves on the GPU (host/lis_esolver_single.c: -e gpi | gii | grqi | gcr through lis_gesolve with a matrix B) against the reference's bits.

Reference-order mode: with lis_amd_set_reference_reductions(T) a gesolve must reproduce oracle/_ref at T threads IN EVERY BIT -- iteration count, status, the
eigenvalue, the final residual, every entry of the residual history, the eigenvector, and A's arrays after the solve (the shifts of -e grqi and of -shift
leave the reference's drift in them).  Fixtures: tests/golden/gesolve_bits.{json,npz}, written by tests/golden/make_golden_gesolve.py at T = 1 and 8.  The cases
are gesolve_cases.SOLVES: the four solvers on P1 and P3 (power iteration on P3v: the reference does not carry it on P3, see there), gcr and gii on P2, gii and gcr
with -shift 0.005 on P1.

Default (tree) mode: the iteration count lies inside the reference's own spread over T = 1, 2, 4, 8 widened by 1 at each end, and
|evalue - evalue_ref(T = 1)| <= 2 etol |evalue_ref| -- the bar of tests/test_esolve_gpu.py, for the same reason: both runs stop with a relative residual of at
most etol.  That the reference itself ends every case with status 0 at ONE eigenpair over T = 1, 2, 4, 8 is asserted where the fixtures are made.

Fused and unfused: the dot groups taken in one pass (liship_multidot_f64) or as separate dots (lis_amd_set_loop_mode(UNFUSED), LIS_AMD_NO_FUSION=1) give equal
bits, in both modes."""
import json
import os

import numpy as np
import pytest

import gesolve_cases as gc
import gesolve_drv as gd
import lis_amd
import lisdrv

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
META = json.load(open(os.path.join(HERE, "golden", "gesolve_bits.json")))
BITS = np.load(os.path.join(HERE, "golden", "gesolve_bits.npz"))
LOOP_UNFUSED = 2
CASES = [gc.solve_key(p, e, x, 0).rsplit("|", 1)[0] for p, e, x in gc.SOLVES]
BY_CASE = {gc.solve_key(p, e, x, 0).rsplit("|", 1)[0]: (p, e, x) for p, e, x in gc.SOLVES}


@pytest.fixture(scope="module")
def lib():
    lib = lis_amd.load()
    assert lis_amd.gpu_available(), "no HIP device: the product path has no CPU fallback"
    assert lib.initialize([]) == 0
    lib.dll.lis_amd_set_residency(0)
    yield lib
    lib.dll.lis_amd_set_reference_reductions(0)
    lib.dll.lis_amd_set_loop_mode(0)


def _run(lib, case, T, loop_mode=0):
    pencil, e, extra = BY_CASE[case]
    a, b = gc.PENCILS[pencil]()
    A, B = gd.make(lib, a), gd.make(lib, b)
    assert lib.dll.lis_amd_set_reference_reductions(T) == 0
    lib.dll.lis_amd_set_loop_mode(loop_mode)
    try:
        res = gd.gesolve(lib, A, B, "-e %s %s %s" % (e, extra, gc.COMMON))
    finally:
        lib.dll.lis_amd_set_reference_reductions(0)
        lib.dll.lis_amd_set_loop_mode(0)
    assert res["err"] == 0, (case, res)
    res["A"] = lisdrv.matrix_arrays(A)
    res["B"] = gd.csr_arrays(B)
    assert all(np.array_equal(u, v) for u, v in zip(res["B"], b)), "B is read, never written"
    lib.lis_matrix_destroy(A)
    lib.lis_matrix_destroy(B)
    return res


def _same_bits(a, b, what):
    assert len(a) == len(b), what
    diff = np.flatnonzero(np.asarray(a).view(np.int64) != np.asarray(b).view(np.int64))
    assert diff.size == 0, (what, "first differing entry", int(diff[0]), float(a[diff[0]]).hex(), float(b[diff[0]]).hex())


@pytest.mark.parametrize("T", gc.THREADS_BITS)
@pytest.mark.parametrize("case", CASES)
def test_gesolve_carries_the_reference_bits_at_its_thread_count(lib, case, T):
    key = "%s|T%d" % (case, T)
    want = META["solves"][key]
    res = _run(lib, case, T)
    print(key, res["iter"], res["status"], float(res["evalue"]).hex(), float(res["resid"]).hex())
    assert (res["iter"], res["status"]) == (want["iter"], want["status"]), (key, res["iter"], res["status"])
    assert float(res["evalue"]).hex() == want["evalue_hex"] and float(res["resid"]).hex() == want["resid_hex"], key
    _same_bits(res["rhistory"], BITS[key + "|rhistory"], key + " rhistory")
    _same_bits(res["x"], BITS[key + "|x"], key + " x")
    assert res["A"]["nnz"] == META["solves"][key + "|A"]["nnz"]
    assert np.array_equal(res["A"]["ptr"], BITS[key + "|A|ptr"]) and np.array_equal(res["A"]["index"], BITS[key + "|A|index"])
    _same_bits(res["A"]["value"], BITS[key + "|A|value"], key + " A's values afterwards")


@pytest.mark.parametrize("case", CASES)
def test_tree_mode_stays_inside_the_reference_spread(lib, case):
    sp = META["spread"][case]
    counts = [sp[t]["iter"] for t in sp]
    ref = float.fromhex(sp["T1"]["evalue_hex"])
    res = _run(lib, case, 0)
    print(case, "iter", res["iter"], "reference", counts, "evalue", res["evalue"], "reference", ref, "distance / bound", abs(res["evalue"] - ref) / (2.0 * gc.ETOL * abs(ref)))
    assert res["status"] == 0
    assert min(counts) - 1 <= res["iter"] <= max(counts) + 1, (case, res["iter"], counts)
    assert abs(res["evalue"] - ref) <= 2.0 * gc.ETOL * abs(ref), (case, res["evalue"], ref)


FUSED_CASES = [c for c in CASES if "-e grqi" in c or "-e gcr" in c]      # (-e gpi and -e gii have no two sums that share a vector: nothing to fuse)


@pytest.mark.parametrize("T", [0, 8])
@pytest.mark.parametrize("case", FUSED_CASES)
def test_fused_and_unfused_dot_groups_give_equal_bits(lib, case, T):
    a, b = _run(lib, case, T, 0), _run(lib, case, T, LOOP_UNFUSED)
    assert (a["iter"], a["status"]) == (b["iter"], b["status"])
    assert float(a["evalue"]).hex() == float(b["evalue"]).hex() and float(a["resid"]).hex() == float(b["resid"]).hex()
    _same_bits(a["rhistory"], b["rhistory"], case + " rhistory")
    _same_bits(a["x"], b["x"], case + " x")
    _same_bits(a["A"]["value"], b["A"]["value"], case + " A")


def test_estorage_converts_A_and_the_solve_finds_the_same_pair(lib):
    """-estorage ell: A is converted for good, as for lis_esolve; B stays as it is.  (No golden: the reference's shift leaves an ELL matrix untouched.)"""
    from lis_amd import _capi as capi
    a, b = gc.P3()
    A, B = gd.make(lib, a), gd.make(lib, b)
    res = gd.gesolve(lib, A, B, "-e grqi -estorage ell " + gc.COMMON)
    ref = float.fromhex(META["spread"]["P3|-e grqi"]["T1"]["evalue_hex"])
    assert res["err"] == 0 and res["status"] == 0 and abs(res["evalue"] - ref) <= 2.0 * gc.ETOL * abs(ref)
    assert A.contents.matrix_type == capi.LIS_MATRIX_ELL and B.contents.matrix_type == capi.LIS_MATRIX_CSR
    lib.lis_matrix_destroy(A)
    lib.lis_matrix_destroy(B)
