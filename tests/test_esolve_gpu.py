"""Whole eigensolves on the GPU (host/lis_esolver.c, host/lis_esolver_single.c) against the reference's bits.

Reference-order mode: with lis_amd_set_reference_reductions(T) an esolve must reproduce oracle/_ref at T threads IN EVERY BIT -- iteration count, status,
every entry of the residual history, the eigenvalue, the final residual, the eigenvector.  Fixtures: tests/golden/esolve_bits.{json,npz}, written by
tests/golden/make_golden_esolve.py at T = 1 and 8.

Default (tree) mode, the symmetric matrices: the iteration count lies inside the reference's own spread over T = 1, 2, 4, 8 widened by 1 at each end (the
project's rule for tree-mode counts), and |evalue - evalue_ref(T = 1)| <= 2 etol |evalue_ref|: both runs stop with a residual of at most etol |theta|, and for
a symmetric matrix an eigenvalue lies within the residual of a unit vector's Rayleigh quotient.  At -etol 1e-10 that bound stands well clear of n 2^-53.
Every symmetric golden case enters.  That the reference itself ends each of them with status 0 at ONE eigenpair over T = 1, 2, 4, 8 is asserted where the
fixtures are made (make_golden_esolve.py); the start vector of -initx_ones false lies close to an eigenvector for that reason (esolve_drv.start_vector).

Fused and unfused: the Gram blocks of -e cg and -e cr taken in one pass (liship_multidot_f64) or as separate dots (lis_amd_set_loop_mode(UNFUSED)) give
equal bits, in both modes."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import esolve_drv
import lis_amd
from lis_amd import _capi as capi

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
META = json.load(open(os.path.join(HERE, "golden", "esolve_bits.json")))
BITS = np.load(os.path.join(HERE, "golden", "esolve_bits.npz"))
COMMON = " " + META["common_options"]
ETOL = 1e-10
KEYS = sorted(META["solves"])
LOOP_UNFUSED = 2


def _bound_kept(ev, ref):
    return abs(ev - ref) <= 2.0 * ETOL * abs(ref)


TREE_CASES = [c for c in sorted(META["spread"]) if not c.startswith("nonsym")]


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
    matrix, opts = case.split("|")
    given = "-initx_ones false" in opts
    A = esolve_drv.make_matrix(lib, matrix)                 # (-estorage converts the caller's matrix for good: a fresh one per solve)
    n = A.contents.n
    assert lib.dll.lis_amd_set_reference_reductions(T) == 0
    lib.dll.lis_amd_set_loop_mode(loop_mode)
    try:
        res = esolve_drv.esolve(lib, A, opts + COMMON, esolve_drv.start_vector(n) if given else None)
    finally:
        lib.dll.lis_amd_set_reference_reductions(0)
        lib.dll.lis_amd_set_loop_mode(0)
    assert res["err"] == 0, (case, res)
    if "-estorage ell" in opts:
        assert A.contents.matrix_type == capi.LIS_MATRIX_ELL                      # converted for good, as -storage in lis_solve
    lib.lis_matrix_destroy(A)
    return res


def _same_bits(a, b, what):
    assert len(a) == len(b), what
    diff = np.flatnonzero(np.asarray(a).view(np.int64) != np.asarray(b).view(np.int64))
    assert diff.size == 0, (what, "first differing entry", int(diff[0]), float(a[diff[0]]).hex(), float(b[diff[0]]).hex())


@pytest.mark.parametrize("key", KEYS)
def test_esolve_carries_the_reference_bits_at_its_thread_count(lib, key):
    case, tag = key.rsplit("|", 1)
    want = META["solves"][key]
    res = _run(lib, case, int(tag[1:]))
    print(key, res["iter"], res["status"], float(res["evalue"]).hex(), float(res["resid"]).hex())
    assert (res["iter"], res["status"]) == (want["iter"], want["status"]), (key, res["iter"], res["status"])
    _same_bits(res["rhistory"], BITS[key + "|rhistory"], key + " rhistory")
    assert float(res["evalue"]).hex() == want["evalue_hex"] and float(res["resid"]).hex() == want["resid_hex"], key
    _same_bits(res["x"], BITS[key + "|x"], key + " x")


@pytest.mark.parametrize("case", TREE_CASES)
def test_tree_mode_stays_inside_the_reference_spread(lib, case):
    sp = META["spread"][case]
    counts = [sp[t]["iter"] for t in sp]
    ref = float.fromhex(sp["T1"]["evalue_hex"])
    res = _run(lib, case, 0)
    print(case, "iter", res["iter"], "reference", counts, "evalue", res["evalue"], "reference", ref, "distance / bound", abs(res["evalue"] - ref) / (2.0 * ETOL * abs(ref)))
    assert res["status"] == 0
    assert min(counts) - 1 <= res["iter"] <= max(counts) + 1, (case, res["iter"], counts)
    assert _bound_kept(res["evalue"], ref), (case, res["evalue"], ref)


FUSED_CASES = [c for c in sorted(META["spread"]) if "-e cg" in c or "-e cr" in c]


@pytest.mark.parametrize("T", [0, 8])
@pytest.mark.parametrize("case", FUSED_CASES)
def test_fused_and_unfused_gram_blocks_give_equal_bits(lib, case, T):
    a, b = _run(lib, case, T, 0), _run(lib, case, T, LOOP_UNFUSED)
    assert (a["iter"], a["status"]) == (b["iter"], b["status"])
    assert float(a["evalue"]).hex() == float(b["evalue"]).hex() and float(a["resid"]).hex() == float(b["resid"]).hex()
    _same_bits(a["rhistory"], b["rhistory"], case + " rhistory")
    _same_bits(a["x"], b["x"], case + " x")


def _ell_walk_transposed(n, maxnzr, index, value):
    """the transposed rows of an ELL matrix in the order lis_matvech_ell's scatter meets their entries: slot after slot, within a slot row after row"""
    cols = [[] for _ in range(n)]
    for j in range(maxnzr):
        for i in range(n):
            cols[int(index[j * n + i])].append((i, value[j * n + i]))
    tptr = np.zeros(n + 1, np.int32)
    tptr[1:] = np.cumsum([len(c) for c in cols])
    return tptr, np.array([i for c in cols for i, _ in c], np.int32), np.array([v for c in cols for _, v in c], np.float64)


@pytest.mark.parametrize("T", [2, 3, 8])
def test_ell_transposed_product_takes_the_thread_chunks_of_the_reference(lib, T):
    """What the BiCG inside -e ii / -e rqi -estorage ell multiplies by at T > 1: lis_matvech on ELL storage groups a column's terms by the row chunk of the
    thread that owns them, each chunk's terms in the ELL walk's order (lis_matvec_ell.c:182-222); the kernel alone on rows in no particular order, too."""
    import lisdrv
    import reduction_cases as rc
    import reduction_model as rm
    from lis_amd import DeviceArray as DA, check
    ptr, idx, val = esolve_drv.nonsym_csr()
    n = len(ptr) - 1
    x = rc.wide(np.random.default_rng(T), n)
    A0 = lisdrv.make_csr(lib, ptr, idx, val * rc.wide(np.random.default_rng(5), len(val)))
    A = lisdrv.convert(lib, A0, "ell")
    a = lisdrv.matrix_arrays(A)
    tptr, tidx, tval = _ell_walk_transposed(n, a["maxnzr"], a["index"], a["value"])
    want = rm.spmv_transposed_chunked(n, n, T, tptr, tidx, tval, x)
    assert lib.dll.lis_amd_set_reference_reductions(T) == 0
    try:
        got = lisdrv.matvech(lib, A, x)
    finally:
        lib.dll.lis_amd_set_reference_reductions(0)
    assert np.array_equal(got.view(np.int64), want.view(np.int64))
    assert not np.array_equal(want.view(np.int64), rm.spmv_transposed_chunked(n, n, 1, tptr, tidx, tval, x).view(np.int64))      # (the grouping moves bits on this data)
    for nsrc in (1, 5, 13, 100):
        rows, cptr, cidx, cval, cx = rc.chunked_case(nsrc, T)
        rng = np.random.default_rng(nsrc)
        for c in range(rows):                                                  # every row's entries shuffled
            o = rng.permutation(cptr[c + 1] - cptr[c]) + cptr[c]
            cidx[cptr[c]:cptr[c + 1]], cval[cptr[c]:cptr[c + 1]] = cidx[o], cval[o]
        d = [DA.from_host(cptr, np.int32), DA.from_host(cidx if len(cidx) else np.zeros(1, np.int32), np.int32), DA.from_host(cval if len(cval) else np.zeros(1), np.float64),
             DA.from_host(cx, np.float64), DA.from_host(np.full(rows + 1, 7.25), np.float64)]
        check(lib.liship_spmv_csr_transposed_chunked_unordered_f64(rows, nsrc, T, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, d[4].ptr, None))
        check(lib.liship_device_synchronize())
        y = d[4].to_host()
        assert np.array_equal(y[:rows].view(np.int64), rm.spmv_transposed_chunked(rows, nsrc, T, cptr, cidx, cval, cx).view(np.int64)) and y[rows] == 7.25
    assert lib.liship_spmv_csr_transposed_chunked_unordered_f64(3, 3, 0, None, None, None, None, None, None) == -1
    lib.lis_matrix_destroy(A)
    lib.lis_matrix_destroy(A0)


def test_getters_history_file_and_the_unshift(lib, tmp_path):
    """The getters of test/etest1.c after a solve with -shift: A comes back with the reference's drift (shift(s) then shift(-s), tests/esolve_model.py), x is a
    unit vector, the history file holds iter + 1 lines."""
    import esolve_model as em
    import lisdrv
    ptr, idx, val = esolve_drv.sym_csr()
    A = lisdrv.make_csr(lib, ptr, idx, val)
    vx = lisdrv.new_vector(lib, A)
    E = capi.PE()
    assert lib.lis_esolver_create(C.byref(E)) == 0
    assert lib.lis_esolver_set_option(b"-e cr -shift 0.3 -etol 1e-10 -emaxiter 500 -eprint mem", E) == 0
    ev = C.c_double()
    assert lib.lis_esolve(A, vx, C.byref(ev), E) == 0
    it, it1, it2, itq, nesol, st = (C.c_int() for _ in range(6))
    res, t, ti, tp, tpc, tpi = (C.c_double() for _ in range(6))
    assert lib.lis_esolver_get_iter(E, C.byref(it)) == 0 and lib.lis_esolver_get_iterex(E, C.byref(it1), C.byref(it2), C.byref(itq)) == 0
    assert (it1.value, it2.value, itq.value) == (it.value, it.value, 0)
    assert lib.lis_esolver_get_status(E, C.byref(st)) == 0 and st.value == 0
    assert lib.lis_esolver_get_residualnorm(E, C.byref(res)) == 0 and 0.0 < res.value < 1e-10
    assert lib.lis_esolver_get_esolver(E, C.byref(nesol)) == 0 and nesol.value == capi.LIS_ESOLVER_CR
    assert lib.lis_esolver_get_time(E, C.byref(t)) == 0 and t.value > 0.0
    assert lib.lis_esolver_get_timeex(E, C.byref(t), C.byref(ti), C.byref(tp), C.byref(tpc), C.byref(tpi)) == 0
    x = lisdrv.get_vector(lib, vx)
    assert abs(np.linalg.norm(x) - 1.0) < 1e-14
    assert abs(float(x @ lisdrv.matvec(lib, A, x)) - ev.value) < 1e-9 * abs(ev.value)
    vh = lisdrv.new_vector(lib, A)
    assert lib.lis_esolver_get_rhistory(E, vh) == 0
    rh = lisdrv.get_vector(lib, vh)[:it.value + 1]
    assert rh[0] == 1.0 and rh[-1] == res.value
    path = tmp_path / "rhistory.txt"
    assert lib.lis_esolver_output_rhistory(E, str(path).encode()) == 0
    lines = open(path).read().split()
    assert len(lines) == it.value + 1 and lines[-1] == "%e" % res.value
    want = em.shift_csr_values(ptr, idx, em.shift_csr_values(ptr, idx, val, 0.3), -0.3)
    got = lisdrv.matrix_arrays(A)["value"]
    assert np.array_equal(got.view(np.int64), want.view(np.int64))
    lib.lis_esolver_destroy(E)
    lib.lis_vector_destroy(vx)
    lib.lis_vector_destroy(vh)
    lib.lis_matrix_destroy(A)
