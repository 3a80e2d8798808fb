"""Eigensolves of several pairs on the GPU (-e si | li | ai, host/lis_esolver_multi.c) against the reference's bits.

Reference-order mode: with lis_amd_set_reference_reductions(T) a solve must reproduce oracle/_ref at T threads IN EVERY BIT of every mode -- eigenvalue,
residual and count per mode, the status, every entry of the residual history, x and every eigenvector -- read from the struct and through the getters.
Fixtures: tests/golden/esolve_multi_bits.{json,npz}, written by tests/golden/make_golden_esolve_multi.py at T = 1 and 8.  Where the reference ends a mode in
NaN (a start vector that the orthogonalisation wipes out: 0 * inf) the same entries must be NaN here; WHICH NaN is not compared, as in
tests/test_reduction_tree_gpu.py: IEEE 754 leaves the sign and payload of a generated NaN to the processor, and x86 and gfx950 choose differently.

Default (tree) mode, for the modes the reference itself converges at T = 1, 2, 4 and 8 (the fixture lists them): the count lies inside the reference's
spread over T widened by 1 at each end, and |evalue - evalue_ref(T = 1)| <= 2 etol |evalue_ref| -- the rule of tests/test_esolve_gpu.py.

Fused and unfused (the device chains and liship_ritz_tail_f64 against the plain lis_vector_* calls): equal bits at T = 0 and 8."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import esolve_drv
import esolve_model as em
import esolve_multi_drv as emd
import lis_amd
import lisdrv
from lis_amd import _capi as capi

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
META = json.load(open(os.path.join(HERE, "golden", "esolve_multi_bits.json")))
BITS = np.load(os.path.join(HERE, "golden", "esolve_multi_bits.npz"))
KEYS = sorted(META["solves"])
LOOP_UNFUSED = 2
NAN_BITS = np.float64(np.nan).view(np.uint64)


@pytest.fixture(scope="module")
def lib():
    lib = lis_amd.load()
    assert lis_amd.gpu_available(), "no HIP device: the product path has no CPU fallback"
    assert lib.initialize([]) == 0
    lib.dll.lis_amd_set_residency(0)
    yield lib
    lib.dll.lis_amd_set_reference_reductions(0)
    lib.dll.lis_amd_set_loop_mode(0)


def _solve(lib, matrix, opts, T, loop_mode=0):
    """-> (A, result): E and vx of the result stay alive for the getters (emd.release)"""
    A = emd.make_matrix(lib, matrix)                        # (-estorage converts the caller's matrix for good: a fresh one per solve)
    assert lib.dll.lis_amd_set_reference_reductions(T) == 0
    lib.dll.lis_amd_set_loop_mode(loop_mode)
    try:
        res = emd.esolve(lib, A, opts)
    finally:
        lib.dll.lis_amd_set_reference_reductions(0)
        lib.dll.lis_amd_set_loop_mode(0)
    assert res["err"] == 0, (matrix, opts, res["err"])
    return A, res


def _canon(a):
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    b = a.view(np.uint64).copy()
    b[np.isnan(a)] = NAN_BITS
    return b


def _same_bits(a, b, what):
    a, b = _canon(a), _canon(b)
    assert len(a) == len(b), what
    diff = np.flatnonzero(a != b)
    assert diff.size == 0, (what, "first differing entry", int(diff[0]), hex(a[diff[0]]), hex(b[diff[0]]))


def _hex_array(hexes):
    return np.array([float.fromhex(h) for h in hexes])


def _vector_of(lib, call):
    v = capi.PV()
    assert lib.lis_vector_create(capi.LIS_COMM_WORLD, C.byref(v)) == 0
    assert call(v) == 0
    out = lisdrv.get_vector(lib, v)
    lib.lis_vector_destroy(v)
    return out


@pytest.mark.parametrize("key", KEYS)
def test_every_mode_carries_the_reference_bits_at_its_thread_count(lib, key):
    _, matrix, opts, tag = key.split("|")
    want = META["solves"][key]
    A, res = _solve(lib, matrix, opts + " " + META["bit_common_options"], int(tag[1:]))
    E, n, ss = res["E"], A.contents.n, want["ss"]
    print(key, res.get("iter"), [float(v).hex() for v in res["evalue"]])
    assert res["status"] == want["status"] and float(res["evalue0"]).hex() == want["evalue0_hex"]
    _same_bits(res["evalue"], _hex_array(want["evalue_hex"]), key + " evalue")
    _same_bits(_vector_of(lib, lambda v: lib.lis_esolver_get_evalues(E, v)), res["evalue"], key + " get_evalues")
    ev, rn, it = C.c_double(), C.c_double(), C.c_int()
    for mode in range(ss):
        assert lib.lis_esolver_get_specific_evalue(E, mode, C.byref(ev)) == 0
        _same_bits([ev.value], res["evalue"][mode:mode + 1], key + " specific evalue")
    if want["rval"]:                                           # Ritz values only: nothing else is compared (heap contents in the reference); here iter / resid are 0
        assert not _vector_of(lib, lambda v: lib.lis_esolver_get_iters(E, v)).any() and not _vector_of(lib, lambda v: lib.lis_esolver_get_residualnorms(E, v)).any()
        M = capi.PM()
        assert lib.lis_matrix_create(capi.LIS_COMM_WORLD, C.byref(M)) == 0
        assert lib.lis_esolver_get_evectors(E, M) == capi.LIS_ERR_ILL_ARG       # -rval true leaves no eigenvectors
        lib.lis_matrix_destroy(M)
    else:
        assert [int(v) for v in res["iter"]] == want["iter"], (key, res["iter"], want["iter"])
        _same_bits(res["resid"], _hex_array(want["resid_hex"]), key + " resid")
        _same_bits(res["rhistory"], BITS[key + "|rhistory"], key + " rhistory")
        _same_bits(res["x"], BITS[key + "|x"], key + " x")
        for mode in range(ss):
            _same_bits(res["evector"][mode], BITS[key + "|evector%d" % mode], key + " evector %d" % mode)
        # the getters
        assert [int(v) for v in _vector_of(lib, lambda v: lib.lis_esolver_get_iters(E, v))] == want["iter"]
        _same_bits(_vector_of(lib, lambda v: lib.lis_esolver_get_residualnorms(E, v)), res["resid"], key + " get_residualnorms")
        assert lib.lis_esolver_get_iter(E, C.byref(it)) == 0 and it.value == want["iter"][0]
        vy = lisdrv.new_vector(lib, A)
        for mode in range(ss):
            assert lib.lis_esolver_get_specific_residualnorm(E, mode, C.byref(rn)) == 0 and lib.lis_esolver_get_specific_iter(E, mode, C.byref(it)) == 0
            _same_bits([rn.value], res["resid"][mode:mode + 1], key + " specific resid")
            assert it.value == want["iter"][mode]
            assert lib.lis_esolver_get_specific_evector(E, mode, vy) == 0
            _same_bits(lisdrv.get_vector(lib, vy), res["evector"][mode], key + " specific evector")
        for bad in (-1, ss):
            assert lib.lis_esolver_get_specific_evalue(E, bad, C.byref(ev)) == capi.LIS_ERR_ILL_ARG
            assert lib.lis_esolver_get_specific_evector(E, bad, vy) == capi.LIS_ERR_ILL_ARG
        lib.lis_vector_destroy(vy)
        # lis_esolver_get_evectors: an n x n CSR matrix whose columns 0 .. ss - 1 are the vectors (every entry stored, zeros included), and nothing else
        M = capi.PM()
        assert lib.lis_matrix_create(capi.LIS_COMM_WORLD, C.byref(M)) == 0
        assert lib.lis_esolver_get_evectors(E, M) == 0
        m = lisdrv.matrix_arrays(M)
        assert (m["type"], m["n"], M.contents.gn, m["nnz"]) == (capi.LIS_MATRIX_CSR, n, n, n * ss)
        assert np.array_equal(m["ptr"], np.arange(n + 1) * ss) and np.array_equal(m["index"], np.tile(np.arange(ss), n))
        _same_bits(m["value"], np.stack(res["evector"], axis=1).reshape(-1), key + " get_evectors")
        lib.lis_matrix_destroy(M)
    if "-estorage ell" in opts:
        assert A.contents.matrix_type == capi.LIS_MATRIX_ELL                      # converted for good, as -storage in lis_solve
    emd.release(lib, res)
    lib.lis_matrix_destroy(A)


@pytest.mark.parametrize("case", sorted(META["tree"]))
def test_tree_mode_stays_inside_the_reference_spread_mode_by_mode(lib, case):
    _, matrix, opts = case.split("|")
    tree = META["tree"][case]
    A, res = _solve(lib, matrix, opts + " " + META["tree_common_options"], 0)
    for mode in tree["admitted"]:
        counts = tree["iter"][str(mode)]
        ref = float.fromhex(tree["evalue_T1_hex"][str(mode)])
        got_iter, got_ev = int(res["iter"][mode]), float(res["evalue"][mode])
        print(case, "mode", mode, "iter", got_iter, "reference", counts, "evalue", got_ev, "reference", ref, "distance / bound", abs(got_ev - ref) / (2.0 * emd.ETOL * abs(ref)))
        assert min(counts) - 1 <= got_iter <= max(counts) + 1, (case, mode, got_iter, counts)
        assert abs(got_ev - ref) <= 2.0 * emd.ETOL * abs(ref), (case, mode, got_ev, ref)
    emd.release(lib, res)
    lib.lis_matrix_destroy(A)


FUSED_CASES = [(m, o) for m, o in emd.BIT_CASES if "-e si" in o or "-e ai" in o]


@pytest.mark.parametrize("T", [0, 8])
@pytest.mark.parametrize("matrix,opts", FUSED_CASES, ids=[m + " " + o for m, o in FUSED_CASES])
def test_fused_and_unfused_loops_give_equal_bits(lib, matrix, opts, T):
    full = opts + " " + META["bit_common_options"]
    (A1, a), (A2, b) = _solve(lib, matrix, full, T, 0), _solve(lib, matrix, full, T, LOOP_UNFUSED)
    assert a["status"] == b["status"] and [int(v) for v in a["iter"]] == [int(v) for v in b["iter"]]
    for k in ("evalue", "resid", "rhistory", "x"):
        _same_bits(a[k], b[k], (matrix, opts, k))
    for mode in range(a["ss"]):
        _same_bits(a["evector"][mode], b["evector"][mode], (matrix, opts, "evector", mode))
    for A, r in ((A1, a), (A2, b)):
        emd.release(lib, r)
        lib.lis_matrix_destroy(A)


def test_a_shifted_subspace_solve_leaves_the_shift_unshift_drift_in_A(lib):
    ptr, idx, val = esolve_drv.sym_csr()
    A, res = _solve(lib, "sym7", "-e si -ss 3 -ie ii -shift 0.75 " + META["bit_common_options"], 0)
    want = em.shift_csr_values(ptr, idx, em.shift_csr_values(ptr, idx, val, 0.75), -0.75)
    got = lisdrv.matrix_arrays(A)["value"]
    assert np.array_equal(got.view(np.int64), want.view(np.int64))
    emd.release(lib, res)
    lib.lis_matrix_destroy(A)


def test_a_second_solve_with_a_smaller_subspace_answers_for_the_new_one(lib):
    """-ss 4, then -ss 2 on the same esolver: the four eigenvectors and the six work vectors of the first solve are destroyed -- none of them is a live object
    of the library any more, unless the second solve's own vectors took its address -- and every getter answers for two modes"""
    is_live = lib.dll.lis_is_malloc
    is_live.restype, is_live.argtypes = C.c_int, [C.c_void_p]
    A = emd.make_matrix(lib, "sym7")
    n = A.contents.n
    vx = lisdrv.new_vector(lib, A)
    ev = C.c_double()
    E = capi.PE()
    assert lib.lis_esolver_create(C.byref(E)) == 0

    def owned():
        e = E.contents
        vecs, work = C.cast(e.evector, C.POINTER(C.c_void_p)), C.cast(e.work, C.POINTER(C.c_void_p))
        ss = e.options[2]
        assert all(vecs[i] for i in range(ss)) and not vecs[ss]
        return [vecs[i] for i in range(ss)] + [work[i] for i in range(e.worklen)]

    assert lib.lis_esolver_set_option(b"-e li -ss 4 -etol 1e-10 -emaxiter 60", E) == 0
    assert lib.lis_esolve(A, vx, C.byref(ev), E) == 0
    first = owned()
    assert len(first) == 4 + 6 and all(is_live(p) for p in first)
    assert lib.lis_esolver_set_option(b"-ss 2", E) == 0
    assert lib.lis_esolve(A, vx, C.byref(ev), E) == 0
    second = owned()
    assert len(second) == 2 + 4
    assert [p for p in first if is_live(p) and p not in second] == []
    evs = _vector_of(lib, lambda v: lib.lis_esolver_get_evalues(E, v))
    assert len(evs) == 2 and evs[0] == ev.value
    assert lib.lis_esolver_get_specific_evalue(E, 2, C.byref(C.c_double())) == capi.LIS_ERR_ILL_ARG
    M = capi.PM()
    assert lib.lis_matrix_create(capi.LIS_COMM_WORLD, C.byref(M)) == 0
    assert lib.lis_esolver_get_evectors(E, M) == 0 and M.contents.nnz == 2 * n
    lib.lis_matrix_destroy(M)
    its = _vector_of(lib, lambda v: lib.lis_esolver_get_iters(E, v))
    assert len(its) == 2 and int(its[0]) == E.contents.iter[0] and 0 < int(its[1]) <= 60
    lib.lis_esolver_destroy(E)
    assert [p for p in second if is_live(p)] == []                                   # lis_esolver_destroy takes the eigenvectors with it
    lib.lis_vector_destroy(vx)
    lib.lis_matrix_destroy(A)


@pytest.mark.parametrize("text", ["-e si", "-e li", "-e ai", "-e si -ss 1", "-e ai -ss 1 -ie pi"])
def test_a_subspace_of_one_vector_is_still_refused(lib, text, capfd):
    A = emd.make_matrix(lib, "sym7")
    vx = lisdrv.new_vector(lib, A, np.full(A.contents.n, 0.5))
    E = capi.PE()
    assert lib.lis_esolver_create(C.byref(E)) == 0
    assert lib.lis_esolver_set_option(text.encode(), E) == 0
    ev = C.c_double(-7.0)
    assert lib.lis_esolve(A, vx, C.byref(ev), E) == capi.LIS_ERR_NOT_IMPLEMENTED
    assert "not served" in capfd.readouterr().out and ev.value == -7.0
    assert np.array_equal(lisdrv.get_vector(lib, vx), np.full(A.contents.n, 0.5))
    lib.lis_esolver_destroy(E)
    lib.lis_vector_destroy(vx)
    lib.lis_matrix_destroy(A)
