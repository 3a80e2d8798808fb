"""Several pairs of the generalized problem on the GPU (-e gsi | gli | gai through lis_gesolve, host/lis_esolver_multi.c) against the reference's bits.

Reference-order mode: with lis_amd_set_reference_reductions(T) a solve must reproduce oracle/_ref at T threads IN EVERY BIT of every mode -- eigenvalue,
residual and count per mode, the status, every entry of the residual history, x, every eigenvector and A's arrays after the solve (the shift of -shift and the
shifts of the refinements leave their drift there; where B's pattern is not inside A's the arrays are rebuilt) -- read from the struct and through the getters.
Fixtures: tests/golden/gesolve_multi_bits.{json,npz}, written by tests/golden/make_golden_gesolve_multi.py from the reference at T = 1 and 8.  Where the
reference has NaN (a mode of -e gsi whose <v,w> went negative) the same entries must be NaN; which NaN is not compared.  A -rval true case compares Ritz values.

Default (tree) mode, for the modes the reference itself carries at T = 1, 2, 4 and 8 (the fixture lists them): the count lies inside the reference's spread
over T widened by 1 at each end, and |evalue - evalue_ref(T = 1)| <= 2 etol |evalue_ref|.

Fused and unfused (the device chains and the pair passes against the plain lis_vector_* calls): equal bits at T = 0 and 8, for every bit case."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import gesolve_drv as gd
import gesolve_multi_cases as gm
import lis_amd
import lisdrv
from lis_amd import _capi as capi

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
META = json.load(open(os.path.join(HERE, "golden", "gesolve_multi_bits.json")))
BITS = np.load(os.path.join(HERE, "golden", "gesolve_multi_bits.npz"))
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


def _solve(lib, pencil, opts, T, loop_mode=0):
    """-> (A, B, result): E and vx of the result stay alive for the getters (gm.release)"""
    A, B = gm.make_pencil(lib, pencil)
    assert lib.dll.lis_amd_set_reference_reductions(T) == 0
    lib.dll.lis_amd_set_loop_mode(loop_mode)
    try:
        res = gm.gesolve(lib, A, B, opts)
    finally:
        lib.dll.lis_amd_set_reference_reductions(0)
        lib.dll.lis_amd_set_loop_mode(0)
    assert res["err"] == 0, (pencil, opts, res["err"])
    return A, B, res


def _done(lib, A, B, res):
    gm.release(lib, res)
    lib.lis_matrix_destroy(A)
    lib.lis_matrix_destroy(B)


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


def _evectors_as_csr(lib, E, n, ss, evectors, what):
    """lis_esolver_get_evectors: an n x n CSR matrix whose columns 0 .. ss - 1 are the vectors (every entry stored, zeros included), and nothing else"""
    M = capi.PM()
    assert lib.lis_matrix_create(capi.LIS_COMM_WORLD, C.byref(M)) == 0
    assert lib.lis_esolver_get_evectors(E, M) == 0
    m = lisdrv.matrix_arrays(M)
    assert (m["type"], m["n"], M.contents.gn, m["nnz"]) == (capi.LIS_MATRIX_CSR, n, n, n * ss)
    assert np.array_equal(m["ptr"], np.arange(n + 1) * ss) and np.array_equal(m["index"], np.tile(np.arange(ss), n))
    _same_bits(m["value"], np.stack(evectors, axis=1).reshape(-1), what)
    lib.lis_matrix_destroy(M)


@pytest.mark.parametrize("key", KEYS)
def test_every_mode_carries_the_reference_bits_at_its_thread_count(lib, key):
    _, pencil, opts, tag = key.split("|")
    want = META["solves"][key]
    A, B, res = _solve(lib, pencil, opts + " " + META["bit_common_options"], int(tag[1:]))
    E, n, ss = res["E"], A.contents.n, want["ss"]
    print(key, res.get("iter"), [float(v).hex() for v in res["evalue"]])
    assert res["status"] == want["status"]
    _same_bits([res["evalue0"]], [float.fromhex(want["evalue0_hex"])], key + " evalue0")
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
        # A's arrays after the solve
        a = lisdrv.matrix_arrays(A)
        for k, v in a.items():
            if isinstance(v, np.ndarray):
                w = BITS[key + "|A|" + k]
                assert v.dtype == w.dtype and np.array_equal(v.view(np.uint8), w.view(np.uint8)), (key, "A", k)
            else:
                assert int(v) == want["A"][k], (key, "A", k, v)
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
        _evectors_as_csr(lib, E, n, ss, res["evector"], key + " get_evectors")
    _done(lib, A, B, res)


@pytest.mark.parametrize("case", sorted(META["tree"]))
def test_tree_mode_stays_inside_the_reference_spread_mode_by_mode(lib, case):
    _, pencil, opts = case.split("|")
    tree = META["tree"][case]
    A, B, res = _solve(lib, pencil, opts + " " + META["tree_common_options"], 0)
    assert tree["admitted"]
    for mode in tree["admitted"]:
        counts = tree["iter"][str(mode)]
        ref = float.fromhex(tree["evalue_T1_hex"][str(mode)])
        got_iter, got_ev = int(res["iter"][mode]), float(res["evalue"][mode])
        print(case, "mode", mode, "iter", got_iter, "reference", counts, "evalue", got_ev, "reference", ref, "distance / bound", abs(got_ev - ref) / (2.0 * gm.ETOL * abs(ref)))
        assert min(counts) - 1 <= got_iter <= max(counts) + 1, (case, mode, got_iter, counts)
        assert abs(got_ev - ref) <= 2.0 * gm.ETOL * abs(ref), (case, mode, got_ev, ref)
    _done(lib, A, B, res)


@pytest.mark.parametrize("T", [0, 8])
@pytest.mark.parametrize("pencil,opts", gm.BIT_CASES, ids=[p + " " + o for p, o in gm.BIT_CASES])
def test_fused_and_unfused_loops_give_equal_bits(lib, pencil, opts, T):
    full = opts + " " + META["bit_common_options"]
    (A1, B1, a), (A2, B2, b) = _solve(lib, pencil, full, T, 0), _solve(lib, pencil, full, T, LOOP_UNFUSED)
    assert a["status"] == b["status"]
    _same_bits(a["evalue"], b["evalue"], (pencil, opts, "evalue"))
    _same_bits(a["x"], b["x"], (pencil, opts, "x"))
    if not a["rval"]:
        assert [int(v) for v in a["iter"]] == [int(v) for v in b["iter"]]
        for k in ("resid", "rhistory"):
            _same_bits(a[k], b[k], (pencil, opts, k))
        for mode in range(a["ss"]):
            _same_bits(a["evector"][mode], b["evector"][mode], (pencil, opts, "evector", mode))
    _same_bits(lisdrv.matrix_arrays(A1)["value"], lisdrv.matrix_arrays(A2)["value"], (pencil, opts, "A"))
    _done(lib, A1, B1, a)
    _done(lib, A2, B2, b)


def test_a_second_solve_with_a_smaller_subspace_answers_for_the_new_one(lib):
    """-e gli -ss 4, then -ss 2 on the same esolver: the work vectors are 4 + ss, as lis_egli_malloc_work counts them, and every getter answers for two modes"""
    A, B = gm.make_pencil(lib, "P3")
    n = A.contents.n
    vx = lisdrv.new_vector(lib, A)
    ev = C.c_double()
    E = capi.PE()
    assert lib.lis_esolver_create(C.byref(E)) == 0
    assert lib.lis_esolver_set_option(b"-e gli -ss 4 -etol 1e-10 -emaxiter 60", E) == 0
    assert lib.lis_gesolve(A, B, vx, C.byref(ev), E) == 0
    assert E.contents.worklen == 4 + 4
    assert len(_vector_of(lib, lambda v: lib.lis_esolver_get_evalues(E, v))) == 4
    assert lib.lis_esolver_set_option(b"-ss 2", E) == 0
    assert lib.lis_gesolve(A, B, vx, C.byref(ev), E) == 0
    assert E.contents.worklen == 4 + 2
    vecs = C.cast(E.contents.evector, C.POINTER(C.c_void_p))
    assert vecs[0] and vecs[1] and not vecs[2]
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
    lib.lis_vector_destroy(vx)
    lib.lis_matrix_destroy(A)
    lib.lis_matrix_destroy(B)


@pytest.mark.parametrize("opts,worklen", [("-e gsi -ss 3 -ige gii", 5 + 3), ("-e gai -ss 3", 3 + 3)])
def test_the_eigenvectors_come_back_as_csr_columns(lib, opts, worklen):
    A, B, res = _solve(lib, "P3", opts + " -etol 1e-10 -emaxiter 30", 0)
    assert res["E"].contents.worklen == worklen
    _evectors_as_csr(lib, res["E"], A.contents.n, 3, res["evector"], opts)
    _same_bits(res["x"], res["evector"][0], opts + " x is mode 0's vector")
    _done(lib, A, B, res)


def test_after_a_lanczos_solve_on_p4_the_hbm_copy_of_A_and_its_host_arrays_agree(lib):
    """B's pattern is not inside A's: every refinement's shift rebuilds A's arrays, in HBM and at home"""
    A, B, res = _solve(lib, "P4", "-e gli -ss 4 " + META["bit_common_options"], 0)
    host = gd.csr_arrays(A)
    dev = gd.hbm_csr_arrays(lib, A)
    for h, d, what in zip(host, dev, ("ptr", "index", "value")):
        assert h.dtype == d.dtype and np.array_equal(h.view(np.uint8), d.view(np.uint8)), what
    _done(lib, A, B, res)
