"""-p sainv on the GPU (lis_sainv.c, kernels/sainv.hip) against tests/sainv_oracle.py in every bit, and whole solves against
tests/golden/sainv_bits.{json,npz} (make_golden_sainv.py: the reference at T = 1 and T = 8, its iteration spread over T = 1, 2, 4, 8).

The factor (pattern, stored order, every value of W, Z and d) is built on the host and does not depend on T; the two psolves are the
model's bits in the default mode (T = 0: one chain per output) and in the reference-order mode at T = 1, 3, 8 and T = 300 > n chunks.
Whole solves are the reference's in every bit in the reference-order mode; in the default mode only the dot / nrm2 folds of the Krylov
loops differ and the count stays inside the reference's spread widened by 1.
Not asserted: sign and payload of a NaN (none of these cases produces one)."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import lis_amd
import lisdrv
import orc
import sainv_cases as sc
import sainv_oracle as so
from lis_amd import _capi as capi

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
G = json.load(open(os.path.join(HERE, "golden", "sainv_bits.json")))
GH = np.load(os.path.join(HERE, "golden", "sainv_bits.npz"))
P_INT, P_DBL = capi.P_INT, capi.P_DBL
MODES = (0, 1, 3, 8, 300)
CASES = sc.SAINV_CASES + (("p654_fill", "p654", 0.01),)        # beyond the table: the stencil with a drop small enough to keep fill-in


@pytest.fixture(scope="module")
def lib():
    lib = lis_amd.load()
    assert lis_amd.gpu_available(), "no HIP device: the product path has no CPU fallback"
    assert lib.initialize([]) == 0
    lib.dll.lis_amd_set_residency(0)
    lib.dll.lis_amd_matrix_host_modified.argtypes = [capi.PM]
    return lib


class mode:
    """the library with lis_amd_set_reference_reductions(T) for the duration of a with block (T = 0: the default mode)"""
    def __init__(self, lib, T):
        self.lib, self.T = lib, T

    def __enter__(self):
        assert self.lib.dll.lis_amd_set_reference_reductions(self.T) == 0

    def __exit__(self, *a):
        self.lib.dll.lis_amd_set_reference_reductions(0)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


_models = {}


def model(case):
    """the model's factor of a case, computed once"""
    if case not in _models:
        _, mat, tol = next(c for c in CASES if c[0] == case)
        _models[case] = so.factor(*sc.system(mat), tol)
    return _models[case]


def library_factor(lib, A, tol):
    sizes = (C.c_int * 3)()
    assert lib.dll.lis_amd_sainv_factor(A, tol, sizes) == 0
    n, wn, zn = sizes[0], sizes[1], sizes[2]
    assert n == A.contents.n
    wp, zp = np.zeros(n + 1, np.int32), np.zeros(n + 1, np.int32)
    wi, zi = np.zeros(max(wn, 1), np.int32), np.zeros(max(zn, 1), np.int32)
    wv, zv, d = np.full(max(wn, 1), 7.0), np.full(max(zn, 1), 7.0), np.full(max(n, 1), 7.0)
    as_i, as_d = (lambda a: a.ctypes.data_as(P_INT)), (lambda a: a.ctypes.data_as(P_DBL))
    assert lib.dll.lis_amd_sainv_copy(A, tol, as_i(wp), as_i(wi), as_d(wv), as_i(zp), as_i(zi), as_d(zv), as_d(d)) == 0
    assert wp[-1] == wn and zp[-1] == zn
    return {"W": (wp, wi[:wn], wv[:wn]), "Z": (zp, zi[:zn], zv[:zn]), "D": d[:n]}


def library_psolve(lib, A, tol, b, transposed, alias=False):
    vb = lisdrv.new_vector(lib, A, b)
    vx = vb if alias else lisdrv.new_vector(lib, A, np.full(len(b), 7.0))
    assert lib.dll.lis_amd_sainv_psolve(A, tol, vb, vx, transposed) == 0
    out = lisdrv.get_vector(lib, vx, A.contents.n)
    lib.lis_vector_destroy(vb)
    if not alias:
        lib.lis_vector_destroy(vx)
    return out


def check_psolves(lib, A, tol, want, T, tag):
    n = A.contents.n
    for vname, b in sc.inputs(n).items():
        for transposed, fn in ((0, so.psolve), (1, so.psolveh)):
            x = fn(want, b, max(T, 1))
            for alias in (False, True):
                y = library_psolve(lib, A, tol, b, transposed, alias)
                bad = np.flatnonzero(bits(y) != bits(x))
                assert bad.size == 0, tag + (vname, transposed, alias, int(bad[0]), float(y[bad[0]]), float(x[bad[0]]))


@pytest.mark.parametrize("T", MODES)
@pytest.mark.parametrize("case", [c[0] for c in CASES])
def test_factor_and_psolves_are_the_model(lib, case, T):
    _, mat, tol = next(c for c in CASES if c[0] == case)
    ptr, idx, val = sc.system(mat)
    want = model(case)
    with mode(lib, T):
        A = lisdrv.make_csr(lib, ptr, idx, val)
        got = library_factor(lib, A, tol)
        assert sc.factor_differences(got, want) == [], (case, T)
        check_psolves(lib, A, tol, want, T, (case, T))
        after = lisdrv.matrix_arrays(A)
        assert not A.contents.is_splited and after["type"] == capi.LIS_MATRIX_CSR
        assert np.array_equal(after["ptr"], ptr) and np.array_equal(after["index"], idx) and np.array_equal(bits(after["value"]), bits(val))
        lib.lis_matrix_destroy(A)


def test_the_cases_are_what_the_table_says():
    full, ident = model("tri65_full"), model("tri65_identity")
    assert np.diff(full["W"][0]).tolist() == list(range(1, 66)) and np.diff(full["Z"][0]).tolist() == list(range(1, 66))      # rows of 1 .. 65 entries: past a wavefront
    ptr, idx, val = sc.system("tri65")
    assert ident["W"][0][-1] == ident["Z"][0][-1] == 65 and np.array_equal(ident["D"], 1.0 / val[idx == np.repeat(np.arange(65), np.diff(ptr))])
    assert model("one")["D"][0] == 1.0 / -2.5
    rows = [sc.system("twice")[1][a:b].tolist() for a, b in zip(sc.system("twice")[0][:-1], sc.system("twice")[0][1:])]
    assert rows[2].count(5) == 2 and rows[6].count(1) == 2 and rows[4].count(4) == 2
    assert model("p654_fill")["W"][0][-1] > 120 and model("nonsym")["W"][0][-1] != model("nonsym")["Z"][0][-1]
    assert (len(sc.system("dom257")[0]) - 1) % 64 != 0


@pytest.mark.parametrize("fmt", ["ell", "bsr"])
@pytest.mark.parametrize("T", [0, 3])
def test_other_storage_is_built_through_the_csr_copy(lib, fmt, T):
    ptr, idx, val = sc.system("p654")
    want = model("p654_fill")
    with mode(lib, T):
        A0 = lisdrv.make_csr(lib, ptr, idx, val)
        A = lisdrv.convert(lib, A0, fmt)
        before = lisdrv.matrix_arrays(A)
        got = library_factor(lib, A, 0.01)
        assert sc.factor_differences(got, want) == [], (fmt, T)
        check_psolves(lib, A, 0.01, want, T, (fmt, T))
        after = lisdrv.matrix_arrays(A)
        assert after["type"] == before["type"] == capi.FORMAT_ID[fmt] and not A.contents.is_splited
        assert np.array_equal(before["index" if fmt == "ell" else "bindex"], after["index" if fmt == "ell" else "bindex"])
        assert np.array_equal(bits(before["value"]), bits(after["value"]))
        # and a whole solve on that storage
        out = lisdrv.solve(lib, A, sc.rhs(ptr, idx, val), "-i bicgstab -p sainv -sainv_drop 0.01 -tol 1e-10")
        assert out["err"] == 0 and out["status"] == 0 and last_sainv(lib)[0] == 1
        assert A.contents.matrix_type == capi.FORMAT_ID[fmt]
        lib.lis_matrix_destroy(A)
        lib.lis_matrix_destroy(A0)


def last_sainv(lib):
    w, z, b = C.c_int(), C.c_int(), C.c_int()
    r = lib.dll.lis_amd_last_solve_sainv(C.byref(w), C.byref(z), C.byref(b))
    return r, w.value, z.value, b.value


def others_say_no(lib):
    return (lib.dll.lis_amd_last_solve_ilu(None, None, None, None) == 0 and lib.dll.lis_amd_last_solve_ssor(None, None, None, None) == 0 and
            lib.dll.lis_amd_last_solve_bjacobi(None, None, None) == 0 and lib.dll.lis_amd_last_solve_is(None) == 0 and
            lib.dll.lis_amd_last_solve_renumbered() == 0)


WHOLE = [w for w in sc.WHOLE if "-p sainv" in w[1]]


@pytest.mark.parametrize("T", [1, 8])
@pytest.mark.parametrize("mat,opts", WHOLE)
def test_reference_order_mode_is_the_reference_at_T_threads(lib, mat, opts, T):
    key = f"{mat}|{opts}|T{T}"
    want = G["solves"][key]
    ptr, idx, val = sc.system(mat)
    f = model(mat)
    with mode(lib, T):
        A = lisdrv.make_csr(lib, ptr, idx, val)
        out = lisdrv.solve(lib, A, sc.rhs(ptr, idx, val), opts + " " + G["common_options"])
        said = last_sainv(lib)
        lib.lis_matrix_destroy(A)
    assert out["err"] == 0
    assert said == (1, int(f["W"][0][-1]), int(f["Z"][0][-1]), T) and others_say_no(lib)
    assert (out["iter"], out["status"]) == (want["iter"], want["status"]), (key, out["iter"], want["iter"])
    diff = np.flatnonzero(bits(out["rhistory"]) != bits(GH[key]))
    assert diff.size == 0, (key, int(diff[0]))
    assert sha(out["x"]) == want["x_sha256"], key


@pytest.mark.parametrize("mat,opts", WHOLE)
def test_tree_mode_stays_inside_the_reference_spread(lib, mat, opts):
    lo, hi = G["spread"][f"{mat}|{opts}"]
    ptr, idx, val = sc.system(mat)
    A = lisdrv.make_csr(lib, ptr, idx, val)
    out = lisdrv.solve(lib, A, sc.rhs(ptr, idx, val), opts + " " + G["common_options"])
    assert last_sainv(lib)[0] == 1 and last_sainv(lib)[3] == 1
    lib.lis_matrix_destroy(A)
    print("SAINV TREE %s %s iter=%d spread=[%d, %d]" % (mat, opts, out["iter"], lo, hi))
    assert out["err"] == 0 and out["status"] == 0
    assert lo - 1 <= out["iter"] <= hi + 1, (mat, opts, out["iter"], lo, hi)


@pytest.mark.parametrize("solver", ["bicr", "crs", "bicrstab", "gpbicr", "bicrsafe"])
def test_the_other_solvers_that_apply_the_transposed_preconditioner(lib, solver):
    """M^-H through W and Z swapped: the solvers beside BiCG that call psolveh reach the solution of the non-symmetric system"""
    ptr, idx, val = sc.system("nonsym")
    A = lisdrv.make_csr(lib, ptr, idx, val)
    out = lisdrv.solve(lib, A, sc.rhs(ptr, idx, val), f"-i {solver} -p sainv -tol 1e-10 -maxiter 400")
    lib.lis_matrix_destroy(A)
    assert out["err"] == 0 and out["status"] == 0 and last_sainv(lib)[0] == 1
    assert np.abs(out["x"] - 1.0).max() < 1e-6


def info_of(lib, A, tol):
    info = (C.c_double * 6)()
    assert lib.dll.lis_amd_sainv_info(A, tol, info) == 0
    return list(info)


def test_a_second_solve_reuses_the_factor_and_an_edit_rebuilds_it(lib):
    ptr, idx, val = sc.system("nonsym")
    b = sc.rhs(ptr, idx, val)
    opts = "-i bicgstab -p sainv -tol 1e-10 -maxiter 400"
    A = lisdrv.make_csr(lib, ptr, idx, val)
    first = lisdrv.solve(lib, A, b, opts)
    info = info_of(lib, A, sc.DROP)
    f = model("nonsym")
    assert info[1:3] == [float(f["W"][0][-1]), float(f["Z"][0][-1])] and info[4] == 2.0 and info[0] > 0.0
    n = len(ptr) - 1
    assert info[3] == 12.0 * (info[1] + info[2]) + 8.0 * (n + 1) + 40.0 * n
    second = lisdrv.solve(lib, A, b, opts)
    assert info_of(lib, A, sc.DROP)[5] == info[5], "the second solve built the factor again"
    assert first["err"] == second["err"] == 0 and first["iter"] == second["iter"] and np.array_equal(bits(first["x"]), bits(second["x"]))
    # another tolerance is another factor
    assert info_of(lib, A, 0.2)[5] == info[5] + 1
    # an edit of the values, announced: the next use builds from the new values
    live = np.ctypeslib.as_array(A.contents.value, shape=(len(val),))
    live *= 1.0 + 0.25 * np.cos(np.arange(len(val)))
    edited = live.copy()
    assert lib.dll.lis_amd_matrix_host_modified(A) == 0
    third = lisdrv.solve(lib, A, b, opts)
    assert third["err"] == 0 and third["status"] == 0 and not np.array_equal(third["x"], first["x"])
    assert info_of(lib, A, sc.DROP)[5] == info[5] + 2
    assert sc.factor_differences(library_factor(lib, A, sc.DROP), so.factor(ptr, idx, edited, sc.DROP)) == []
    lib.lis_matrix_destroy(A)


def test_sainv_then_ilu_then_sainv_each_report_their_own(lib):
    ptr, idx, val = sc.system("p654")
    b = sc.rhs(ptr, idx, val)
    A = lisdrv.make_csr(lib, ptr, idx, val)
    for k, p in enumerate(("sainv", "ilu", "sainv", "jacobi")):
        out = lisdrv.solve(lib, A, b, f"-i cg -p {p} -tol 1e-10")
        assert out["err"] == 0 and out["status"] == 0
        assert last_sainv(lib)[0] == (p == "sainv") and lib.dll.lis_amd_last_solve_ilu(None, None, None, None) == (p == "ilu")
        if p != "sainv":
            assert last_sainv(lib) == (0, 0, 0, 0)
    assert not A.contents.is_splited
    lib.lis_matrix_destroy(A)


@pytest.mark.parametrize("opts,says", [("-i cg -p sainv -scale jacobi", "-scale"), ("-i cg -p sainv -adds true", "-adds true"),
                                       ("-i jacobi -p sainv", "Jacobi solver"), ("-i cg -p hybrid", "preconditioner 4 is not served"),
                                       ("-i cg -p saamg", "preconditioner 7 is not served")])
def test_refusals_say_which_and_leave_A_untouched(lib, opts, says, capfd):
    ptr, idx, val = sc.system("p654")
    A = lisdrv.make_csr(lib, ptr, idx, val)
    before = lisdrv.matrix_arrays(A)
    capfd.readouterr()
    out = lisdrv.solve(lib, A, sc.rhs(ptr, idx, val), opts)
    assert out["err"] == capi.LIS_ERR_NOT_IMPLEMENTED
    text = "".join(capfd.readouterr())
    assert says in text, (opts, text[-400:])
    after = lisdrv.matrix_arrays(A)
    assert not A.contents.is_splited and np.array_equal(before["index"], after["index"]) and np.array_equal(bits(before["value"]), bits(after["value"]))
    lib.lis_matrix_destroy(A)


def test_split_matrix_is_refused_until_merged(lib, capfd):
    ptr, idx, val = sc.system("p654")
    b = sc.rhs(ptr, idx, val)
    A = lisdrv.make_csr(lib, ptr, idx, val)
    assert lisdrv.solve(lib, A, b, "-i cg -p ssor -tol 1e-10")["err"] == 0 and A.contents.is_splited
    capfd.readouterr()
    out = lisdrv.solve(lib, A, b, "-i cg -p sainv -tol 1e-10")
    assert out["err"] == capi.LIS_ERR_NOT_IMPLEMENTED and A.contents.is_splited and "split matrix" in "".join(capfd.readouterr())
    assert lib.lis_matrix_merge(A) == 0
    out = lisdrv.solve(lib, A, b, "-i cg -p sainv -tol 1e-10")
    assert out["err"] == 0 and out["status"] == 0 and last_sainv(lib)[0] == 1
    lib.lis_matrix_destroy(A)


@pytest.mark.parametrize("p", ["sainv", "is"])
def test_a_matrix_in_hbm_only_is_refused(lib, capfd, p):
    from lis_amd import DeviceArray as DA
    ptr, idx, val = sc.system("p654")
    n = len(ptr) - 1
    dptr, didx, dval = DA.from_host(ptr, np.int32), DA.from_host(idx, np.int32), DA.from_host(val, np.float64)
    A = capi.PM()
    assert lib.lis_matrix_create(0, C.byref(A)) == 0 and lib.lis_matrix_set_size(A, n, 0) == 0
    fn = lib.dll.lis_amd_matrix_set_csr_device
    fn.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, capi.PM]
    assert fn(len(idx), n, dptr.ptr, didx.ptr, dval.ptr, A) == 0
    dptr.ptr = didx.ptr = dval.ptr = None                                  # owned by A now
    x = np.linspace(-1.0, 1.0, n)
    y = lisdrv.matvec(lib, A, x)
    capfd.readouterr()
    out = lisdrv.solve(lib, A, sc.rhs(ptr, idx, val), "-i bicg -p " + p)
    assert out["err"] == capi.LIS_ERR_NOT_IMPLEMENTED
    text = "".join(capfd.readouterr())
    assert "HBM only" in text and "(A is untouched)" in text
    assert A.contents.matrix_type == capi.LIS_MATRIX_CSR and not A.contents.is_splited and sc.same_bits(lisdrv.matvec(lib, A, x), y)
    lib.lis_matrix_destroy(A)
