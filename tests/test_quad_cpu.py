"""-f quad without a GPU: the numpy model of the double-double arithmetic and of the quad kernels' sums (tests/quad_model.py) equals the reference's
quad build in every bit (tests/golden/quad_bits.npz, made by tests/golden/make_golden_quad.py); the host's scalar steps (kernels/dd.hpp compiled as C and
by the host pass of hipcc) equal them too; and the switch: off, -f quad answers as the reference built without --enable-quad does; on, what is not served
is refused with LIS_ERR_NOT_IMPLEMENTED and a message that names it, A, b and x untouched."""
import ctypes as C
import os

import numpy as np
import pytest

import lis_amd
import lisdrv
import quad_cases as qc
import quad_model as qm
from lis_amd import _capi as capi

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(HERE, "golden", "quad_bits.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def lib():
    lib = lis_amd.load()
    assert lib.initialize([]) == 0
    return lib


def bits(a):
    return np.atleast_1d(np.asarray(a, np.float64)).view(np.uint64)


def same(gold, key, pair):
    for part, v in zip(("hi", "lo"), pair):
        want, got = gold[f"{key}/{part}"], bits(v)
        bad = np.flatnonzero(want != got)
        assert not len(bad), (key, part, bad[:8].tolist(), [hex(x) for x in got[bad[:4]]], [hex(x) for x in want[bad[:4]]])


# ------------------------------------------------------------------ the model against the reference
@pytest.mark.parametrize("op", ["add", "mul", "muld", "div"])
def test_model_scalar_ops(gold, op):
    a, b = qc.scalar_pairs()
    got = {"add": lambda: qm.add(a, b), "mul": lambda: qm.mul(a, b), "muld": lambda: qm.muld(a, b[0]), "div": lambda: qm.div(a, b)}[op]()
    same(gold, "scalar/" + op, got)


def test_model_packed_product_is_the_scalar_one_swapped():
    a, b = qc.scalar_pairs()
    for got, want in zip(qm.mul2(a, b), qm.mul(b, a)):
        assert np.array_equal(bits(got), bits(want))
    # and the two forms do differ: the place of an element in its chunk decides its bits
    assert np.any(bits(qm.mul2(a, b)[1]) != bits(qm.mul(a, b)[1]))


@pytest.mark.parametrize("T", qc.THREADS)
def test_model_vector_ops(gold, T):
    n = qc.VEC_N
    x, y = qc.dd_vector(n, 21), qc.dd_vector(n, 22)
    al = qc.dd_vector(1, 23, -2, 2)
    alpha = (al[0][0], al[1][0])
    same(gold, f"vec/axpyz/T{T}", qm.axpyz(alpha, x, y, T))
    same(gold, f"vec/axpy/T{T}", qm.axpy(alpha, x, y, T))
    same(gold, f"vec/xpay/T{T}", qm.xpay(x, alpha, y, T))


def test_model_muld_vector(gold):
    same(gold, "vec/muld", qm.muld(qc.dd_vector(qc.VEC_N, 31), qc.dd_vector(qc.VEC_N, 32)[0]))


@pytest.mark.parametrize("T", qc.THREADS)
@pytest.mark.parametrize("n", qc.DOT_SIZES)
def test_model_dot(gold, n, T):
    x, y = qc.dot_vectors(n)
    same(gold, f"dot/{n}/T{T}", qm.dot_ref(x, y, T))


def test_dot_inputs_cancel():
    x, y = qc.dot_vectors(1024)
    t = qm.mul2(y, x)
    got = qm.dot_ref(x, y, 1)
    assert abs(got[0]) < 1e-18 * np.sum(np.abs(t[0]))


def test_model_rows(gold):
    ptr, idx, val, x, _ = qc.rows_matrix()
    y = qm.spmv_csr(ptr, idx, val, x)
    same(gold, "rows/T1", y)
    t = abs(val[ptr[10]] * x[0][idx[ptr[10]]])
    assert 0.0 < abs(y[0][10]) < 1e-18 * t               # the cancelling row


def test_model_rows_transposed(gold):
    ptr, idx, val, _, ncols = qc.rows_matrix()
    xt = qc.transposed_input()
    same(gold, "rows_t/T1", qm.spmv_csr_t(ptr, idx, val, xt, ncols))


def test_tree_model_agrees_with_reference_to_quad_accuracy():
    """the tree is another order of the same adds: not the reference's bits, but its value to ~1e-30 of the terms"""
    x, y = qc.dd_vector(5000, 3, -2, 2), qc.dd_vector(5000, 4, -2, 2)
    a, b = qm.dot_tree(x, y), qm.dot_ref(x, y, 1)
    scale = float(np.sum(np.abs(x[0] * y[0])))
    assert abs((a[0] - b[0]) + (a[1] - b[1])) < 1e-28 * scale


# ------------------------------------------------------------------ dd.hpp as the host compilers built it
def test_host_scalar_steps(lib, gold):
    a, b = qc.scalar_pairs()
    f = lib.dll.lis_amd_quad_scalar
    for op, key in ((0, "add"), (1, "mul"), (2, "div")):
        hi, lo = np.zeros(len(a[0])), np.zeros(len(a[0]))
        for i in range(len(a[0])):
            out = (C.c_double * 2)()
            assert f(op, (C.c_double * 2)(a[0][i], a[1][i]), (C.c_double * 2)(b[0][i], b[1][i]), out) == 0
            hi[i], lo[i] = out[0], out[1]
        same(gold, "scalar/" + key, (hi, lo))
    out = (C.c_double * 2)()
    assert f(3, (C.c_double * 2)(1.5, -2.0 ** -60), None, out) == 0 and (out[0], out[1]) == (-1.5, 2.0 ** -60)
    assert f(9, (C.c_double * 2)(1.0, 0.0), (C.c_double * 2)(1.0, 0.0), out) == capi.LIS_ERR_ILL_ARG


def test_kernel_side_scalar_ops_and_fma_two_prod(lib, gold):
    a, b = qc.scalar_pairs()
    res = {k: (np.zeros(len(a[0])), np.zeros(len(a[0]))) for k in range(7)}
    for i in range(len(a[0])):
        for op in range(7):
            out = (C.c_double * 2)()
            assert lib.liship_dd_scalar(op, a[0][i], a[1][i], b[0][i], b[1][i], out) == 0
            res[op][0][i], res[op][1][i] = out[0], out[1]
    same(gold, "scalar/add", res[0])
    same(gold, "scalar/mul", res[1])
    same(gold, "scalar/muld", res[3])
    same(gold, "scalar/div", res[4])
    for got, want in zip(res[2], qm.mul2(a, b)):
        assert np.array_equal(bits(got), bits(want))
    for got, want in zip(res[5], res[6]):                  # the fma's error term is Dekker's
        assert np.array_equal(bits(got), bits(want))


# ------------------------------------------------------------------ the switch and the refusals
def _system(lib, fmt=None):
    ptr, idx, val = qc.solve_matrices()["poisson1d"]
    A = lisdrv.make_csr(lib, ptr, idx, val)
    if fmt:
        B = lisdrv.convert(lib, A, fmt)
        lib.lis_matrix_destroy(A)
        A = B
    n = len(ptr) - 1
    b = np.linspace(1.0, 2.0, n)
    x = np.linspace(-1.0, 1.0, n)
    return A, lisdrv.new_vector(lib, A, b), lisdrv.new_vector(lib, A, x), b, x


def _text(capfd):
    o = capfd.readouterr()
    return o.out + o.err


def _solve(lib, A, vb, vx, options):
    S = capi.PS()
    assert lib.lis_solver_create(C.byref(S)) == 0
    assert lib.lis_solver_set_option(options.encode(), S) == 0
    err = lib.lis_solve(A, vb, vx, S)
    st = S.contents.retcode
    lib.lis_solver_destroy(S)
    return err, st


def test_switch_round_trips_and_is_off_by_default(lib):
    d = lib.dll
    assert d.lis_amd_get_quad_precision() == 0
    assert d.lis_amd_set_quad_precision(1) == 0 and d.lis_amd_get_quad_precision() == 1
    assert d.lis_amd_set_quad_precision(0) == 0 and d.lis_amd_get_quad_precision() == 0


def test_switch_off_answers_as_today(lib, capfd):
    A, vb, vx, b, x = _system(lib)
    assert lib.dll.lis_amd_get_quad_precision() == 0
    for f in ("quad", "switch"):
        err, st = _solve(lib, A, vb, vx, f"-i cg -f {f}")
        assert err == capi.LIS_ERR_ILL_ARG and st == capi.LIS_ERR_ILL_ARG
        assert "Quad precision is not enabled" in _text(capfd)
    assert lib.dll.lis_amd_last_solve_quad() == 0
    assert np.array_equal(lisdrv.get_vector(lib, vb), b) and np.array_equal(lisdrv.get_vector(lib, vx), x)


REFUSALS = [
    ("-i gmres -f quad", None, "GMRES"),
    ("-i cr -f quad", None, "CR"),
    ("-i bicgstabl -f quad", None, "BiCGSTAB(l)"),
    ("-i cg -f switch", None, "-f switch"),
    ("-i cg -p ilu -f quad", None, "ILU"),
    ("-i cg -p ssor -f quad", None, "SSOR"),
    ("-i bicg -p sainv -f quad", None, "SAINV"),
    ("-i cg -f quad -storage ell", None, "-storage"),
    ("-i cg -f quad", "ell", "storage type"),
    ("-i cg -f quad", "csc", "storage type"),
    ("-i cg -f quad -scale jacobi", None, "-scale"),
]


@pytest.mark.parametrize("options,fmt,names", REFUSALS)
def test_switch_on_refuses_by_name_and_touches_nothing(lib, capfd, options, fmt, names):
    A, vb, vx, b, x = _system(lib, fmt)
    before = lisdrv.matrix_arrays(A)
    lib.dll.lis_amd_set_quad_precision(1)
    try:
        err, st = _solve(lib, A, vb, vx, options)
    finally:
        lib.dll.lis_amd_set_quad_precision(0)
    msg = _text(capfd)
    assert err == capi.LIS_ERR_NOT_IMPLEMENTED and st == capi.LIS_ERR_NOT_IMPLEMENTED, (err, st, msg)
    assert names in msg, msg
    assert lib.dll.lis_amd_last_solve_quad() == 0
    after = lisdrv.matrix_arrays(A)
    assert A.contents.is_splited == 0 and A.contents.is_scaled == 0
    assert before.keys() == after.keys()
    for k, v in before.items():
        assert np.array_equal(v, after[k]), k
    assert np.array_equal(lisdrv.get_vector(lib, vb), b) and np.array_equal(lisdrv.get_vector(lib, vx), x)


def test_switch_on_refuses_a_split_matrix(lib, capfd):
    A, vb, vx, b, x = _system(lib)
    assert lib.lis_matrix_split(A) == 0
    lib.dll.lis_amd_set_quad_precision(1)
    try:
        err, st = _solve(lib, A, vb, vx, "-i cg -f quad")
    finally:
        lib.dll.lis_amd_set_quad_precision(0)
    assert err == capi.LIS_ERR_NOT_IMPLEMENTED and "split" in _text(capfd)
    assert A.contents.is_splited == 1


def test_eigensolvers_keep_todays_answer_off_and_refuse_on(lib, capfd):
    A, _, vx, _, _ = _system(lib)
    ev = C.c_double()
    for on, want, text in ((0, capi.LIS_ERR_ILL_ARG, "Quad precision is not enabled"), (1, capi.LIS_ERR_NOT_IMPLEMENTED, "eigensolvers")):
        for f in ("quad", "switch"):
            E = capi.PE()
            assert lib.lis_esolver_create(C.byref(E)) == 0
            assert lib.lis_esolver_set_option(f"-e pi -ef {f}".encode(), E) == 0
            lib.dll.lis_amd_set_quad_precision(on)
            try:
                err = lib.lis_esolve(A, vx, C.byref(ev), E)
            finally:
                lib.dll.lis_amd_set_quad_precision(0)
            assert err == want and text in _text(capfd)
            lib.lis_esolver_destroy(E)


def test_environment_variable_sets_the_switch():
    import subprocess
    import sys
    code = ("import lis_amd; lib = lis_amd.load(); assert lib.initialize([]) == 0; print(lib.dll.lis_amd_get_quad_precision())")
    for env, want in (({}, "0"), ({"LIS_AMD_QUAD_PRECISION": "1"}, "1")):
        e = dict(os.environ, **env)
        e.pop("LIS_AMD_QUAD_PRECISION", None) if not env else None
        out = subprocess.run([sys.executable, "-c", code], env=e, cwd=os.path.dirname(HERE), capture_output=True, text=True)
        assert out.returncode == 0 and out.stdout.strip() == want, (out.stdout, out.stderr)
