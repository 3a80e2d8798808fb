"""Several pairs of the generalized problem (-e gsi | gli | gai through lis_gesolve), the parts that need no GPU: the refusals of lis_gesolve -- code, words,
A, B and x untouched, nothing allocated --, the getters of several pairs on an esolver that never solved, the admission rule of the fixture
(tests/golden/gesolve_multi_bits.json) and the numpy model of the two pair passes (tests/pair_pass_model.py).  The GPU side is
tests/test_gesolve_multi_gpu.py and tests/test_pair_pass_gpu.py."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import gesolve_multi_cases as gm
import lis_amd
import lisdrv
import pair_pass_model as ppm
from lis_amd import _capi as capi

HERE = os.path.dirname(os.path.abspath(__file__))
META = json.load(open(os.path.join(HERE, "golden", "gesolve_multi_bits.json")))
NI, ILL = capi.LIS_ERR_NOT_IMPLEMENTED, capi.LIS_ERR_ILL_ARG


@pytest.fixture(scope="module")
def lib():
    lib = lis_amd.load()
    assert lib.initialize([]) == 0
    return lib


def _snapshot(lib, A, B, vx):
    out = []
    for M in (A, B):
        out.append({k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in lisdrv.matrix_arrays(M).items()})
    return out, lisdrv.get_vector(lib, vx).copy()


def _same(s1, s2):
    for m1, m2 in zip(s1[0], s2[0]):
        for k in m1:
            assert np.array_equal(m1[k], m2[k]), k
    assert np.array_equal(s1[1].view(np.int64), s2[1].view(np.int64))


# (options, with a B, code, words of the message)
REFUSALS = [
    ("-e gsi", True, NI, ["not served", "several pairs", "-ss 1", "-e gpi"]),
    ("-e gli -ss 1", True, NI, ["not served", "several pairs"]),
    ("-e gai -ss 1 -ige gpi", True, NI, ["not served", "several pairs"]),
    ("-e gsi -ss 2 -ige grqi", True, NI, ["not served", "-ige", "gpi, gii"]),
    ("-e gsi -ss 2 -ige gcr", True, NI, ["not served", "-ige"]),
    ("-e gsi -ss 2 -ige ii", True, NI, ["not served", "-ige"]),
    ("-e gli -ss 2 -ige gcg", True, NI, ["not served", "-ige", "gpi, gii, grqi, gcr"]),
    ("-e gai -ss 2 -ige gcg", True, NI, ["not served", "-ige"]),
    ("-e gai -ss 2 -ige cr", True, NI, ["not served", "-ige"]),
    ("-e gsi -ss 31", True, ILL, ["LIS_EOPTIONS_SUBSPACE"]),
    ("-e gli -ss 31", True, ILL, ["LIS_EOPTIONS_SUBSPACE"]),
    ("-e gai -ss 400", True, ILL, ["LIS_EOPTIONS_SUBSPACE"]),
    ("-e gsi -ss 3 -m 3", True, ILL, ["LIS_EOPTIONS_MODE"]),
    ("-e gli -ss 3 -m 3", True, ILL, ["LIS_EOPTIONS_MODE"]),
    ("-e gai -ss 3 -m 4", True, ILL, ["LIS_EOPTIONS_MODE"]),
    ("-e gsi -ss 3", False, NI, ["not served", "without a matrix B"]),
    ("-e gli -ss 3", False, NI, ["not served", "without a matrix B"]),
    ("-e gai -ss 3", False, NI, ["not served", "without a matrix B"]),
    ("-e gli -ss 3 -ef quad", True, ILL, ["Quad precision is not enabled"]),
]


@pytest.mark.parametrize("text,with_b,code,words", REFUSALS, ids=[r[0] + ("" if r[1] else " no B") for r in REFUSALS])
def test_refusals_fire_before_A_B_or_x_is_touched(lib, text, with_b, code, words, capfd):
    A, B = gm.make_pencil(lib, "P1")
    n = A.contents.n
    assert n == 30
    vx = lisdrv.new_vector(lib, A, np.linspace(0.5, 1.5, n))
    before = _snapshot(lib, A, B, vx)
    E = capi.PE()
    assert lib.lis_esolver_create(C.byref(E)) == 0
    assert lib.lis_esolver_set_option(text.encode(), E) == 0
    ev = C.c_double(-7.0)
    capfd.readouterr()
    assert lib.lis_gesolve(A, B if with_b else None, vx, C.byref(ev), E) == code
    assert ev.value == -7.0 and E.contents.retcode == code
    message = capfd.readouterr().out
    for word in words:
        assert word in message, (word, message)
    _same(before, _snapshot(lib, A, B, vx))
    assert not E.contents.evalue and not E.contents.evector and not E.contents.work      # nothing was allocated for a refused solve
    lib.lis_esolver_destroy(E)
    lib.lis_vector_destroy(vx)
    lib.lis_matrix_destroy(A)
    lib.lis_matrix_destroy(B)


@pytest.mark.parametrize("e", ["gsi", "gli", "gai"])
def test_a_generalized_solver_of_several_pairs_is_refused_through_lis_esolve(lib, e, capfd):
    A, B = gm.make_pencil(lib, "P1")
    vx = lisdrv.new_vector(lib, A, np.ones(30))
    E = capi.PE()
    assert lib.lis_esolver_create(C.byref(E)) == 0
    assert lib.lis_esolver_set_option(("-e %s -ss 3" % e).encode(), E) == 0
    ev = C.c_double(-7.0)
    assert lib.lis_esolve(A, vx, C.byref(ev), E) == NI and ev.value == -7.0
    assert "without a matrix B" in capfd.readouterr().out
    lib.lis_esolver_destroy(E)
    lib.lis_vector_destroy(vx)
    lib.lis_matrix_destroy(A)
    lib.lis_matrix_destroy(B)


@pytest.mark.parametrize("e", ["gsi", "gli", "gai"])
def test_getters_of_several_pairs_on_an_esolver_that_never_solved(lib, e, capfd):
    A, B = gm.make_pencil(lib, "P1")
    M = capi.PM()
    assert lib.lis_matrix_create(capi.LIS_COMM_WORLD, C.byref(M)) == 0
    vx = lisdrv.new_vector(lib, A, np.ones(30))
    E = capi.PE()
    assert lib.lis_esolver_create(C.byref(E)) == 0
    assert lib.lis_esolver_set_option(("-e %s -ss 3" % e).encode(), E) == 0
    ev, iv = C.c_double(-7.0), C.c_int(-7)
    calls = (lambda: lib.lis_esolver_get_evalues(E, vx), lambda: lib.lis_esolver_get_residualnorms(E, vx), lambda: lib.lis_esolver_get_iters(E, vx),
             lambda: lib.lis_esolver_get_evectors(E, M), lambda: lib.lis_esolver_get_specific_evalue(E, 0, C.byref(ev)),
             lambda: lib.lis_esolver_get_specific_evector(E, 0, vx), lambda: lib.lis_esolver_get_specific_residualnorm(E, 0, C.byref(ev)),
             lambda: lib.lis_esolver_get_specific_iter(E, 0, C.byref(iv)))
    for call in calls:
        assert call() == ILL
        assert "no eigensolve has filled" in capfd.readouterr().out
    # a refused solve fills nothing either
    assert lib.lis_esolver_set_option(b"-ige gcg", E) == 0
    assert lib.lis_gesolve(A, B, vx, C.byref(ev), E) == NI
    capfd.readouterr()
    for call in calls:
        assert call() == ILL
        assert "no eigensolve has filled" in capfd.readouterr().out
    assert (ev.value, iv.value) == (-7.0, -7)
    assert np.array_equal(lisdrv.get_vector(lib, vx), np.ones(30)) and M.contents.n == 0
    lib.lis_esolver_destroy(E)
    lib.lis_vector_destroy(vx)
    lib.lis_matrix_destroy(A)
    lib.lis_matrix_destroy(B)
    lib.lis_matrix_destroy(M)


# ---------------------------------------------------------------------------------------------- the fixture
def test_the_fixture_holds_every_case_of_the_shared_list():
    want = sorted(gm.key("bits", p, o, T) for p, o in gm.BIT_CASES for T in gm.THREADS_BITS)
    assert sorted(META["solves"]) == want
    assert sorted(META["tree"]) == sorted("tree|%s|%s" % (p, o) for p, o, _ in gm.TREE_CASES)
    assert META["bit_common_options"] == gm.BIT_COMMON.strip() and META["tree_common_options"] == gm.TREE_COMMON.strip()
    with np.load(os.path.join(HERE, "golden", "gesolve_multi_bits.npz")) as z:
        names = set(z.files)
    for key, v in META["solves"].items():
        assert len(v["evalue_hex"]) == v["ss"]
        if v["rval"]:
            assert not any(name.startswith(key + "|") for name in names) and "iter" not in v       # Ritz values only
        else:
            assert {key + "|rhistory", key + "|x", key + "|A|ptr", key + "|A|index", key + "|A|value"} <= names
            assert all(key + "|evector%d" % m in names for m in range(v["ss"])) and len(v["iter"]) == v["ss"] == len(v["resid_hex"])


def test_the_fixture_admits_by_its_own_rule_and_holds_the_modes_each_case_names():
    for pencil, opts, must in gm.TREE_CASES:
        tree = META["tree"]["tree|%s|%s" % (pencil, opts)]
        assert sorted(tree["per_T"]) == ["T1", "T2", "T4", "T8"]
        modes = [m for m in range(gm.subspace(opts)) if gm.admitted(tree["per_T"], m)]
        assert modes == tree["admitted"] and set(must) <= set(modes)
        for m in modes:
            assert tree["iter"][str(m)] == [tree["per_T"]["T%d" % T]["iter"][m] for T in gm.THREADS_TREE]
            assert tree["evalue_T1_hex"][str(m)] == tree["per_T"]["T1"]["evalue_hex"][m]


def test_the_admission_rule_leaves_out_what_it_should():
    hexes = lambda *v: [float(x).hex() for x in v]
    good = {"T%d" % T: {"iter": [20, 149], "evalue_hex": hexes(2.0, 3.0)} for T in gm.THREADS_TREE}
    assert gm.admitted(good, 0) and gm.admitted(good, 1)
    at_maxiter = dict(good, T4={"iter": [20, gm.TREE_MAXITER], "evalue_hex": hexes(2.0, 3.0)})
    assert gm.admitted(at_maxiter, 0) and not gm.admitted(at_maxiter, 1)
    nan = dict(good, T1={"iter": [20, 30], "evalue_hex": hexes(2.0, float("nan"))})
    assert gm.admitted(nan, 0) and not gm.admitted(nan, 1)
    nan8 = dict(good, T8={"iter": [20, 30], "evalue_hex": hexes(float("nan"), 3.0)})
    assert not gm.admitted(nan8, 0) and gm.admitted(nan8, 1)
    other_pair = dict(good, T2={"iter": [20, 30], "evalue_hex": hexes(2.0 * (1 + 3e-10), 3.0 * (1 + 1e-10))})
    assert not gm.admitted(other_pair, 0) and gm.admitted(other_pair, 1)


# ---------------------------------------------------------------------------------------------- the model of the pair passes
SIZES = [1, 2, 3, 255, 256, 257, 2047, 2048, 2049, 4097]


@pytest.mark.parametrize("vec", [True, False])
@pytest.mark.parametrize("n", SIZES)
def test_the_model_gives_every_element_to_one_lane_in_the_order_of_the_walk(n, vec):
    lanes = ppm.lane_elements(n, vec)
    met = np.concatenate([np.array(mine) for _, _, mine in lanes])
    assert sorted(met.tolist()) == list(range(n))
    assert ppm.grid(n) - 1 == (n - 1) // 2048
    # the last workgroup has work, but for the 16 B walk of n = 2048 k + 1: block 0's lane 0 takes the odd tail, and the workgroup launched for it meets nothing
    assert max(b for b, _, _ in lanes) == (ppm.grid(n) - 2 if vec and n % 2048 == 1 and n > 1 else ppm.grid(n) - 1)
    first = dict(((b, t), mine) for b, t, mine in lanes)
    if vec:
        assert first[(0, 0)][:2] == ([0, 1] if n >= 2 else [0])
        if n % 2:
            assert first[(0, 0)][-1] == n - 1                    # the odd tail: lane 0 of block 0, after its own pairs
        if n >= 2 * 256 + 2:
            assert first[(0, 0)][2:4] == [512, 513] and first[(0, 1)][:2] == [2, 3]
        if n > 2048 + 1:
            assert first[(1, 0)][:2] == [2048, 2049]
    else:
        assert first[(0, 0)][0] == 0
        if n > 256:
            assert first[(0, 0)][1] == 256 and first[(0, 1)][0] == 1
        if n > 2048:
            assert first[(1, 0)][0] == 2048


@pytest.mark.parametrize("vec", [True, False])
@pytest.mark.parametrize("n", SIZES)
def test_the_model_is_one_rounded_product_with_the_reciprocal_formed_once(n, vec):
    rng = np.random.default_rng(n)
    v, w = rng.uniform(-2.0, 2.0, n), rng.uniform(-2.0, 2.0, n)
    o0, o1 = ppm.scale2_to(0.3, v, w, vec)
    assert np.array_equal(o0, np.float64(0.3) * v) and np.array_equal(o1, np.float64(0.3) * w)
    s = 7.3
    a = np.float64(1.0) / np.sqrt(np.float64(s))
    o0, o1 = ppm.scale2_inv_sqrt(s, v, w, vec)
    assert np.array_equal(o0, a * v) and np.array_equal(o1, a * w)
    assert not np.array_equal(o0, v / np.sqrt(np.float64(s))) or n < 8           # (a quotient per element is another rounding: the factor is formed once)


def test_the_model_at_the_special_values_of_s():
    v, w = np.array([1.0, 0.0, -2.0]), np.array([0.0, 3.0, np.inf])
    o0, o1 = ppm.scale2_inv_sqrt(0.0, v, w)                       # inf; 0 * inf = NaN
    assert np.isposinf(o0[0]) and np.isnan(o0[1]) and np.isneginf(o0[2]) and np.isnan(o1[0]) and np.isposinf(o1[1]) and np.isposinf(o1[2])
    o0, o1 = ppm.scale2_inv_sqrt(-1.0, v, w)                      # NaN everywhere
    assert np.isnan(o0).all() and np.isnan(o1).all()
    o0, o1 = ppm.scale2_inv_sqrt(np.inf, v, w)                    # 0; 0 * inf = NaN
    assert np.array_equal(o0, [0.0, 0.0, -0.0]) and np.signbit(o0[2]) and np.array_equal(o1[:2], [0.0, 0.0]) and np.isnan(o1[2])


def test_the_headers_declare_the_pair_passes_and_the_library_exports_them(lib):
    root = os.path.dirname(HERE)
    text = open(os.path.join(root, "include", "liship.h")).read()
    assert "int  liship_scale2_inv_sqrt_f64(int n, const double *s, double *v, double *w, void *stream);" in text
    assert "int  liship_scale2_to_f64(int n, double alpha, const double *in0, const double *in1, double *out0, double *out1, void *stream);" in text
    for name in ("liship_scale2_inv_sqrt_f64", "liship_scale2_to_f64"):
        assert hasattr(lib.dll, name) and name not in lib.liship_missing
