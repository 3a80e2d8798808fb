"""-p is on the GPU (lis_is.c, kernels/sainv.hip) against tests/sainv_oracle.py in every bit, and whole solves against
tests/golden/sainv_bits.{json,npz} (make_golden_sainv.py).

M^-1 = I - alpha S with S the first m + 1 stored entries of every row of the strict upper part: psolve and psolveh are the model's bits
in the default mode (T = 0) and in the reference-order mode at T = 1, 3, 8 and T = 300 > n chunks, for m = 0, 3 and 1000 (longer than
any row), alpha = 1 and 0.7, on matrices with rows that have nothing right of the diagonal and rows that store a column twice."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import lis_amd
import lisdrv
import sainv_cases as sc
import sainv_oracle as so
from lis_amd import _capi as capi

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
G = json.load(open(os.path.join(HERE, "golden", "sainv_bits.json")))
GH = np.load(os.path.join(HERE, "golden", "sainv_bits.npz"))
MODES = (0, 1, 3, 8, 300)


@pytest.fixture(scope="module")
def lib():
    lib = lis_amd.load()
    assert lis_amd.gpu_available(), "no HIP device: the product path has no CPU fallback"
    assert lib.initialize([]) == 0
    lib.dll.lis_amd_set_residency(0)
    return lib


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def library_psolve(lib, A, alpha, m, x, transposed):
    vx, vy = lisdrv.new_vector(lib, A, x), lisdrv.new_vector(lib, A, np.full(len(x), 7.0))
    assert lib.dll.lis_amd_is_psolve(A, alpha, m, vx, vy, transposed) == 0
    out = lisdrv.get_vector(lib, vy, A.contents.n)
    lib.lis_vector_destroy(vx)
    lib.lis_vector_destroy(vy)
    return out


def last_is(lib):
    m = C.c_int()
    return lib.dll.lis_amd_last_solve_is(C.byref(m)), m.value


@pytest.mark.parametrize("T", MODES)
@pytest.mark.parametrize("mat", sc.IS_MATRICES)
def test_psolves_are_the_model(lib, mat, T):
    ptr, idx, val = sc.system(mat)
    n = len(ptr) - 1
    U = so.strict_upper(ptr, idx, val)
    A = lisdrv.make_csr(lib, ptr, idx, val)
    assert lib.lis_matrix_split(A) == 0
    assert lib.dll.lis_amd_set_reference_reductions(T) == 0
    try:
        for alpha, m in sc.IS_PARAMS:
            for vname, x in sc.inputs(n).items():
                for transposed, want in ((0, so.is_psolve(*U, alpha, m, x)), (1, so.is_psolveh(*U, alpha, m, x, max(T, 1)))):
                    y = library_psolve(lib, A, alpha, m, x, transposed)
                    bad = np.flatnonzero(bits(y) != bits(want))
                    assert bad.size == 0, (mat, T, alpha, m, vname, transposed, int(bad[0]), float(y[bad[0]]), float(want[bad[0]]))
    finally:
        lib.dll.lis_amd_set_reference_reductions(0)
    assert A.contents.is_splited
    lib.lis_matrix_destroy(A)


def test_the_cases_are_what_they_say():
    up = so.strict_upper(*sc.system("empty_upper"))[0]
    lens = np.diff(up).tolist()
    assert [i for i, k in enumerate(lens) if k == 0] == [0, 3, 4, 7, 9, 11] and lens[1] == 6 and max(lens) < 1000
    p0, p3 = (so.truncated(*so.strict_upper(*sc.system("empty_upper")), m)[0] for m in (0, 3))
    assert np.diff(p0).max() == 1 and np.diff(p3)[1] == 4
    u = so.strict_upper(*sc.system("twice"))
    assert u[1][u[0][2]:u[0][3]].tolist().count(5) == 2


def test_psolve_refuses_an_unsplit_matrix_and_y_equal_to_x(lib):
    ptr, idx, val = sc.system("p654")
    A = lisdrv.make_csr(lib, ptr, idx, val)
    vx, vy = lisdrv.new_vector(lib, A, np.ones(len(ptr) - 1)), lisdrv.new_vector(lib, A)
    assert lib.dll.lis_amd_is_psolve(A, 1.0, 3, vx, vy, 0) == capi.LIS_ERR_ILL_ARG
    assert lib.lis_matrix_split(A) == 0
    assert lib.dll.lis_amd_is_psolve(A, 1.0, 3, vx, vx, 0) == capi.LIS_ERR_ILL_ARG
    assert lib.dll.lis_amd_is_psolve(A, 1.0, 3, vx, vy, 0) == 0
    lib.lis_vector_destroy(vx)
    lib.lis_vector_destroy(vy)
    lib.lis_matrix_destroy(A)


WHOLE = [w for w in sc.WHOLE if "-p is" in w[1]]


@pytest.mark.parametrize("T", [1, 8])
@pytest.mark.parametrize("mat,opts", WHOLE)
def test_reference_order_mode_is_the_reference_at_T_threads(lib, mat, opts, T):
    key = f"{mat}|{opts}|T{T}"
    want = G["solves"][key]
    ptr, idx, val = sc.system(mat)
    assert lib.dll.lis_amd_set_reference_reductions(T) == 0
    try:
        A = lisdrv.make_csr(lib, ptr, idx, val)
        out = lisdrv.solve(lib, A, sc.rhs(ptr, idx, val), opts + " " + G["common_options"])
        said = last_is(lib)
        split = bool(A.contents.is_splited)
        lib.lis_matrix_destroy(A)
    finally:
        lib.dll.lis_amd_set_reference_reductions(0)
    assert out["err"] == 0 and said == (1, 3) and split
    assert lib.dll.lis_amd_last_solve_sainv(None, None, None) == 0 and lib.dll.lis_amd_last_solve_ssor(None, None, None, None) == 0
    assert lib.dll.lis_amd_last_solve_ilu(None, None, None, None) == 0 and lib.dll.lis_amd_last_solve_renumbered() == 0
    assert (out["iter"], out["status"]) == (want["iter"], want["status"]), (key, out["iter"], want["iter"])
    diff = np.flatnonzero(bits(out["rhistory"]) != bits(GH[key]))
    assert diff.size == 0, (key, int(diff[0]))
    assert hashlib.sha256(np.ascontiguousarray(out["x"]).tobytes()).hexdigest() == want["x_sha256"], key


@pytest.mark.parametrize("mat,opts", WHOLE)
def test_tree_mode_stays_inside_the_reference_spread(lib, mat, opts):
    lo, hi = G["spread"][f"{mat}|{opts}"]
    ptr, idx, val = sc.system(mat)
    A = lisdrv.make_csr(lib, ptr, idx, val)
    out = lisdrv.solve(lib, A, sc.rhs(ptr, idx, val), opts + " " + G["common_options"])
    lib.lis_matrix_destroy(A)
    print("I+S TREE %s %s iter=%d spread=[%d, %d]" % (mat, opts, out["iter"], lo, hi))
    assert out["err"] == 0 and out["status"] == 0 and last_is(lib) == (1, 3)
    assert lo - 1 <= out["iter"] <= hi + 1, (mat, opts, out["iter"], lo, hi)


def test_options_reach_the_preconditioner_and_the_system_is_left_row_scaled(lib):
    """-p is solves the system scaled by 1 / diag (ref lis_solver.c:613-636): A is left split AND scaled, as the reference leaves it; x is the
    solution of the caller's system"""
    ptr, idx, val = sc.system("nonsym")
    b = sc.rhs(ptr, idx, val)
    for opts, m in (("-is_m 1 -is_alpha 0.7", 1), ("", 3)):
        A = lisdrv.make_csr(lib, ptr, idx, val)
        out = lisdrv.solve(lib, A, b, "-i bicgstab -p is -tol 1e-10 " + opts)
        assert out["err"] == 0 and out["status"] == 0 and last_is(lib) == (1, m)
        assert A.contents.is_splited and A.contents.is_scaled and np.all(lisdrv.split_arrays(A)["D"] == 1.0)
        assert np.abs(out["x"] - 1.0).max() < 1e-6
        lib.lis_matrix_destroy(A)
    A = lisdrv.make_csr(lib, ptr, idx, val)
    out = lisdrv.solve(lib, A, b, "-i bicgstab -p jacobi -tol 1e-10")
    assert out["err"] == 0 and last_is(lib) == (0, 0) and not A.contents.is_scaled
    lib.lis_matrix_destroy(A)


@pytest.mark.parametrize("opts,says", [("-i bicg -p is -is_level 0", "-is_level 0"), ("-i bicg -p is -scale jacobi", "-scale"),
                                       ("-i bicg -p is -adds true", "-adds true"), ("-i jacobi -p is", "Jacobi solver"),
                                       ("-i bicg -p is -storage ell", "CSR storage only")])
def test_refusals_say_which_and_leave_A_untouched(lib, opts, says, capfd):
    ptr, idx, val = sc.system("p654")
    A = lisdrv.make_csr(lib, ptr, idx, val)
    before = lisdrv.matrix_arrays(A)
    capfd.readouterr()
    out = lisdrv.solve(lib, A, sc.rhs(ptr, idx, val), opts)
    assert out["err"] == capi.LIS_ERR_NOT_IMPLEMENTED
    text = "".join(capfd.readouterr())
    assert says in text and "(A is untouched)" in text, (opts, text[-400:])
    after = lisdrv.matrix_arrays(A)
    assert not A.contents.is_splited and after["type"] == capi.LIS_MATRIX_CSR
    assert np.array_equal(before["index"], after["index"]) and np.array_equal(bits(before["value"]), bits(after["value"]))
    lib.lis_matrix_destroy(A)


def test_other_storage_is_refused(lib, capfd):
    ptr, idx, val = sc.system("p654")
    A0 = lisdrv.make_csr(lib, ptr, idx, val)
    E = lisdrv.convert(lib, A0, "ell")
    before = lisdrv.matrix_arrays(E)
    capfd.readouterr()
    out = lisdrv.solve(lib, E, sc.rhs(ptr, idx, val), "-i bicg -p is")
    assert out["err"] == capi.LIS_ERR_NOT_IMPLEMENTED and "CSR storage only" in "".join(capfd.readouterr())
    after = lisdrv.matrix_arrays(E)
    assert after["type"] == capi.LIS_MATRIX_ELL and not E.contents.is_splited and np.array_equal(bits(before["value"]), bits(after["value"]))
    lib.lis_matrix_destroy(E)
    lib.lis_matrix_destroy(A0)
