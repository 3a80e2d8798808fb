"""-p ilu on the GPU (lis_ilu.c on lis_sweep.c, kernels/ilu.hip, the sweeps of kernels/sptrsv.hip) against tests/ilu_oracle.py in every bit, against
tests/golden/ilu_bits.{json,npz} (make_golden_ilu.py: the reference at T = 1 and T = 8) and against the reference library itself.

The factor and the two psolves are the reference's bits at any block count: pattern, term order, every value.  Whole solves are the
reference's in every bit in the reference-order mode (lis_amd_set_reference_reductions(T)); in the default mode only the dot / nrm2
folds of the Krylov loops differ, so CG and BiCG counts are equal and the others within 2.

The built-to-order matrices (tests/ssor_cases.py) put levels of 1 .. 5000 rows and rows of 0 .. 2049 terms in front of the
factorisation: each case first proves through lis_amd_ilu_factor_info / lis_amd_ilu_info that it got the launches it is for.
Not asserted: sign and payload of a NaN (none of these cases produces one)."""
import ctypes as C
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import ilu_cases
import ilu_oracle
import lis_amd
import lisdrv
import orc
import ssor_cases
from lis_amd import _capi as capi

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
MM = os.path.join(HERE, "golden", "mm")
G = json.load(open(os.path.join(HERE, "golden", "ilu_bits.json")))
GH = np.load(os.path.join(HERE, "golden", "ilu_bits.npz"))
P_INT, P_DBL = capi.P_INT, capi.P_DBL


@pytest.fixture(scope="module")
def lib():
    lib = lis_amd.load()
    assert lis_amd.gpu_available(), "no HIP device: the product path has no CPU fallback"
    assert lib.initialize([]) == 0
    lib.dll.lis_amd_set_residency(0)
    lib.dll.lis_amd_matrix_host_modified.argtypes = [capi.PM]         # (the lis_amd_ilu_* prototypes come from lis_amd/_capi.py)
    return lib


class blocks:
    """the library at T row blocks (the reference-order mode) for the duration of a with block"""
    def __init__(self, lib, T):
        self.lib, self.T = lib, T

    def __enter__(self):
        assert self.lib.dll.lis_amd_set_reference_reductions(self.T if self.T > 1 else 0) == 0

    def __exit__(self, *a):
        self.lib.dll.lis_amd_set_reference_reductions(0)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def library_factor(lib, A, fill):
    sizes = (C.c_int * 3)()
    assert lib.dll.lis_amd_ilu_factor(A, fill, sizes) == 0
    n, ln, un = sizes[0], sizes[1], sizes[2]
    assert n == A.contents.n
    lp, up = np.zeros(n + 1, np.int32), np.zeros(n + 1, np.int32)
    li, ui = np.zeros(max(ln, 1), np.int32), np.zeros(max(un, 1), np.int32)
    lv, uv, d = np.full(max(ln, 1), 7.0), np.full(max(un, 1), 7.0), np.full(max(n, 1), 7.0)
    as_i, as_d = (lambda a: a.ctypes.data_as(P_INT)), (lambda a: a.ctypes.data_as(P_DBL))
    assert lib.dll.lis_amd_ilu_copy(A, fill, as_i(lp), as_i(li), as_d(lv), as_i(up), as_i(ui), as_d(uv), as_d(d)) == 0
    assert lp[-1] == ln and up[-1] == un
    return {"L": (lp, li[:ln], lv[:ln]), "U": (up, ui[:un], uv[:un]), "D": d[:n]}


def library_psolve(lib, A, fill, b, transposed, alias=False):
    vb = lisdrv.new_vector(lib, A, b)
    vx = vb if alias else lisdrv.new_vector(lib, A, np.full(len(b), 7.0))
    assert lib.dll.lis_amd_ilu_psolve(A, fill, vb, vx, transposed) == 0
    out = lisdrv.get_vector(lib, vx, A.contents.n)
    lib.lis_vector_destroy(vb)
    if not alias:
        lib.lis_vector_destroy(vx)
    return out


def check_against_oracle(lib, ptr, idx, val, fill, T, b, tag):
    want = ilu_oracle.factor(ptr, idx, val, fill, T)
    with blocks(lib, T):
        A = lisdrv.make_csr(lib, ptr, idx, val)
        got = library_factor(lib, A, fill)
        assert ilu_cases.factor_differences(got, want) == [], tag
        for transposed, fn in ((0, ilu_oracle.psolve), (1, ilu_oracle.psolveh)):
            x = fn(want, b, T)
            for alias in (False, True):
                y = library_psolve(lib, A, fill, b, transposed, alias)
                bad = np.flatnonzero(bits(y) != bits(x))
                assert bad.size == 0, tag + (transposed, alias, int(bad[0]), float(y[bad[0]]), float(x[bad[0]]))
        after = lisdrv.matrix_arrays(A)
        assert not A.contents.is_splited and after["type"] == capi.LIS_MATRIX_CSR
        assert np.array_equal(after["ptr"], ptr) and np.array_equal(after["index"], idx) and np.array_equal(bits(after["value"]), bits(val))
        lib.lis_matrix_destroy(A)
    return want


@pytest.mark.parametrize("T", ilu_cases.THREADS)
@pytest.mark.parametrize("fill", ilu_cases.FILLS)
@pytest.mark.parametrize("name", ilu_cases.NAMED)
def test_factor_and_psolves_are_the_oracle(lib, name, fill, T):
    ptr, idx, val = ilu_cases.system(name)
    check_against_oracle(lib, ptr, idx, val, fill, T, ilu_cases.rhs(len(ptr) - 1), (name, fill, T))


def expected_schedule(f, serial):
    """what lis_amd_ilu_factor_info and lis_amd_ilu_info must report, from the oracle's pattern and the restated rules of
    tests/ssor_cases.py: the forward levels of L; a row is given to a workgroup when it holds LONG_ROW terms or more in L and U"""
    (lp, lc, _), (up, uc, _) = f["L"], f["U"]
    n = len(lp) - 1
    L = [[(int(c), 0.0) for c in lc[lp[i]:lp[i + 1]]] for i in range(n)]
    U = [[(int(c), 0.0) for c in uc[up[i]:up[i + 1]]] for i in range(n)]
    lev = ssor_cases.levels_of(L, 0)
    nlev = max(lev) + 1 if n else 0
    sizes, nlong = [0] * nlev, [0] * nlev
    for i, l in enumerate(lev):
        sizes[l] += 1
        nlong[l] += (len(L[i]) + len(U[i])) >= ssor_cases.LONG_ROW
    groups = ssor_cases.grouping(sizes)
    own = [g[0] for g in groups if not g[2]]
    factor_info = [nlev, len(groups), len(own), sum(nlong[l] for l in own), sum(nlong) - sum(nlong[l] for l in own), int(serial)]
    psolve_launches = ssor_cases.sweep_stats(L, 0)["info"][1] + ssor_cases.sweep_stats(U, 1)["info"][1]
    return factor_info, psolve_launches


BUILT = [(name, key, T) for name, c in ssor_cases.CASES.items() for key in ("A1", "A2") for T in (1,) + tuple(c["T"])
         if not (key == "A2" and T > 1)]


@pytest.mark.parametrize("name,key,T", BUILT)
def test_built_to_order_matrices(lib, name, key, T):
    s = ssor_cases.system(name)
    ptr, idx, val = s[key]
    n = len(ptr) - 1
    want = check_against_oracle(lib, ptr, idx, val, 0, T, s["b"], (name, key, T))
    assert np.isfinite(want["D"]).all() and np.isfinite(want["L"][2]).all() and np.isfinite(want["U"][2]).all()
    dup = any(len(set(r)) != len(r) for r in (idx[ptr[i]:ptr[i + 1]].tolist() for i in range(n)))
    finfo, launches = expected_schedule(want, dup)
    with blocks(lib, T):
        A = lisdrv.make_csr(lib, ptr, idx, val)
        fi, info = (C.c_int * 6)(), (C.c_double * 6)()
        assert lib.dll.lis_amd_ilu_factor_info(A, 0, fi) == 0 and lib.dll.lis_amd_ilu_info(A, 0, info) == 0
        lib.lis_matrix_destroy(A)
    print("ILU SCHEDULE %s %s T=%d factor=%s psolve launches=%d nnz=%d" % (name, key, T, list(fi), int(info[4]), int(info[1])))
    if T == 1:            # (under T blocks a duplicate may lie across a block border: the library may or may not see it; the bits above hold either way)
        assert list(fi) == finfo, (name, key, T, list(fi), finfo)
    else:
        assert list(fi)[:5] == finfo[:5], (name, key, T, list(fi), finfo)
    assert int(info[1]) == int(want["L"][0][-1] + want["U"][0][-1]) and int(info[2]) == finfo[0] and int(info[4]) == launches


@pytest.mark.parametrize("name,T", [("sizes", 1), ("edges_small", 1), ("edges_large", 1), ("edges_large", 3), ("alternating", 1)])
def test_built_to_order_matrices_with_fill(lib, name, T):
    """fill level 1 on the level-size and row-length cases: discovered fill-in (U rows that are not ascending: the search through the
    ascending copy and its places) through rows given to a workgroup, in runs and in levels on their own launch"""
    s = ssor_cases.system(name)
    ptr, idx, val = s["A1"]
    want = check_against_oracle(lib, ptr, idx, val, 1, T, s["b"], (name, "fill1", T))
    up, uc = want["U"][0], want["U"][1]
    assert any(uc[k] < uc[k - 1] for i in range(len(up) - 1) for k in range(up[i] + 1, up[i + 1])), "no row of U out of order: the case misses its point"
    kept0 = sum(len(r) for part in ilu_oracle.symbolic(ptr, idx, 0, T) for r in part)            # (under T blocks fewer than A holds)
    assert int(want["L"][0][-1] + want["U"][0][-1]) > kept0, "fill level 1 added nothing"
    finfo, launches = expected_schedule(want, False)
    with blocks(lib, T):
        A = lisdrv.make_csr(lib, ptr, idx, val)
        fi, info = (C.c_int * 6)(), (C.c_double * 6)()
        assert lib.dll.lis_amd_ilu_factor_info(A, 1, fi) == 0 and lib.dll.lis_amd_ilu_info(A, 1, info) == 0
        lib.lis_matrix_destroy(A)
    print("ILU SCHEDULE %s fill 1 T=%d factor=%s psolve launches=%d nnz=%d" % (name, T, list(fi), int(info[4]), int(info[1])))
    assert list(fi)[:5] == finfo[:5] and fi[3] + fi[4] > 0, (name, T, list(fi), finfo)
    assert int(info[4]) == launches and int(info[3]) == fi[1] + 2


def test_catalogue_reaches_both_factorisation_paths(lib):
    """levels on their own launch and runs, rows by a thread and rows by a workgroup in both, the parallel and the one-thread form"""
    seen = {"own": 0, "run_groups": 0, "long_own": 0, "long_run": 0, "serial_long": 0, "parallel_long": 0}
    for name in ("sizes", "alternating", "edges_small", "edges_large", "long_only"):
        ptr, idx, val = ssor_cases.system(name)["A1"]
        A = lisdrv.make_csr(lib, ptr, idx, val)
        fi = (C.c_int * 6)()
        assert lib.dll.lis_amd_ilu_factor_info(A, 0, fi) == 0
        lib.lis_matrix_destroy(A)
        seen["own"] += fi[2]
        seen["run_groups"] += fi[1] - fi[2]
        seen["long_own"] += fi[3]
        seen["long_run"] += fi[4]
        seen["serial_long" if fi[5] else "parallel_long"] += fi[3] + fi[4]
    assert all(v > 0 for v in seen.values()), seen


def test_n0_and_n1(lib):
    one = (np.array([0, 1], np.int32), np.array([0], np.int32), np.array([4.0]))
    want = check_against_oracle(lib, *one, 0, 1, np.array([3.0]), ("n1",))
    assert want["D"][0] == 0.25
    # n = 0: the Lis API makes no matrix without rows (lis_matrix_set_size refuses 0, 0); the kernel entry takes one and launches nothing
    A = capi.PM()
    assert lib.lis_matrix_create(capi.LIS_COMM_WORLD, C.byref(A)) == 0
    assert lib.lis_matrix_set_size(A, 0, 0) == capi.LIS_ERR_ILL_ARG
    lib.lis_matrix_destroy(A)

    class IluT(C.Structure):
        _fields_ = [("n", C.c_int), ("serial", C.c_int)] + [(k, C.c_void_p) for k in ("aptr", "aindex", "avalue", "lptr", "lcol", "uptr", "ucol", "uskey", "uspos", "lval", "uval", "d")]

    class SweepT(C.Structure):
        _fields_ = [(k, C.c_int) for k in ("nlev", "nrows", "nnz", "ngroups")] + [(k, C.c_void_p) for k in ("lptr", "llong", "rows", "rptr", "col", "val", "groups", "h_nrows", "h_nshort")]
    fn = lib.dll.liship_ilu_factor_f64
    fn.argtypes = [C.POINTER(IluT), C.POINTER(SweepT), C.c_void_p]
    assert fn(C.byref(IluT()), C.byref(SweepT()), None) == 0
    assert fn(None, C.byref(SweepT()), None) == -1
    one_row = IluT()
    one_row.n = 1
    assert fn(C.byref(one_row), C.byref(SweepT()), None) == -1           # a schedule of another size, NULL arrays: an argument error, no launch


def from_file(L, path):
    A, b, x = capi.PM(), capi.PV(), capi.PV()
    assert L.lis_matrix_create(capi.LIS_COMM_WORLD, C.byref(A)) == 0
    assert L.lis_vector_create(capi.LIS_COMM_WORLD, C.byref(b)) == 0 and L.lis_vector_create(capi.LIS_COMM_WORLD, C.byref(x)) == 0
    assert L.lis_input(A, b, x, path.encode()) == 0
    return A


def matrix(L, case):
    if case == "poisson32":
        return lisdrv.make_csr(L, *orc.poisson3d(32, 32, 32))
    return from_file(L, os.path.join(MM, "testmat0.mtx"))


def last_ilu(lib):
    f, b, l, p = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    r = lib.dll.lis_amd_last_solve_ilu(C.byref(f), C.byref(b), C.byref(l), C.byref(p))
    return r, f.value, b.value, l.value, p.value


GOLDEN_SOLVES = ("-i cg", "-i bicgstab", "-i gmres -restart 30", "-i bicg", "-i cg -ilu_fill 1", "-i cg -ilu_fill 2")


@pytest.mark.parametrize("T", [1, 8])
@pytest.mark.parametrize("case", ["poisson32", "mm/testmat0.mtx"])
def test_reference_order_mode_is_the_reference_at_T_threads(lib, case, T):
    common = G["common_options"]
    for solver in GOLDEN_SOLVES:
        key = f"{case}|{solver}|T{T}"
        want = G["solves"][key]
        A = matrix(lib, case)
        n = A.contents.n
        b = lisdrv.matvec(lib, A, np.ones(n))
        assert lib.dll.lis_amd_set_reference_reductions(T) == 0
        try:
            out = lisdrv.solve(lib, A, b, solver + " " + common)
            r, fill, blk, lev, la = last_ilu(lib)
        finally:
            lib.dll.lis_amd_set_reference_reductions(0)
        assert out["err"] == 0
        assert r == 1 and blk == T and lev > 0 and 0 < la <= 2 * lev and fill == (int(solver[-1]) if "fill" in solver else 0)
        assert lib.dll.lis_amd_last_solve_ssor(None, None, None, None) == 0 and lib.dll.lis_amd_last_solve_renumbered() == 0
        assert (out["iter"], out["status"]) == (want["iter"], want["status"]), (key, out["iter"], want["iter"])
        diff = np.flatnonzero(bits(out["rhistory"]) != bits(GH[key]))
        assert diff.size == 0, (key, int(diff[0]))
        assert sha(out["x"]) == want["x_sha256"], key
        lib.lis_matrix_destroy(A)


@pytest.mark.parametrize("T", [1, 8])
@pytest.mark.parametrize("case", ["poisson32", "mm/testmat0.mtx"])
def test_factor_and_psolves_match_the_golden_at_T(lib, case, T):
    with blocks(lib, T):
        A = matrix(lib, case)
        n = A.contents.n
        b = ilu_cases.rhs(n)
        for fill in ilu_cases.FILLS:
            f = library_factor(lib, A, fill)
            got = {"L": f["L"][2], "U": f["U"][2], "D": f["D"], "psolve": library_psolve(lib, A, fill, b, 0), "psolveh": library_psolve(lib, A, fill, b, 1)}
            for tag, a in got.items():
                want = G["solves"][f"{case}|{tag}|fill{fill}|T{T}"]
                assert len(a) == want["count"] and sha(a) == want["sha256"], (case, tag, fill, T)
        lib.lis_matrix_destroy(A)


def test_levels_of_the_poisson_factorisation(lib):
    A = matrix(lib, "poisson32")
    info = (C.c_double * 6)()
    assert lib.dll.lis_amd_ilu_info(A, 0, info) == 0
    assert int(info[1]) == A.contents.nnz - A.contents.n and int(info[2]) == 94           # nx + ny + nz - 2 levels
    lib.lis_matrix_destroy(A)


SOLVERS = ["-i cg", "-i bicgstab", "-i gmres -restart 30", "-i bicg"]


@pytest.mark.parametrize("case", ["poisson32", "mm/testmat0.mtx"])
@pytest.mark.parametrize("fill", [0, 1])
def test_solves_default_mode(lib, reflib, case, fill):
    for solver in SOLVERS:
        outs = {}
        for tag, L in (("amd", lib), ("ref", reflib)):
            A = matrix(L, case)
            b = lisdrv.matvec(L, A, np.ones(A.contents.n))
            outs[tag] = lisdrv.solve(L, A, b, f"{solver} -p ilu -ilu_fill {fill} -tol 1e-12 -maxiter 3000")
            if tag == "amd":
                assert last_ilu(lib)[:3] == (1, fill, 1)
                assert lib.dll.lis_amd_last_solve_ssor(None, None, None, None) == 0 and lib.dll.lis_amd_last_solve_renumbered() == 0
            L.lis_matrix_destroy(A)
        a, r = outs["amd"], outs["ref"]
        assert a["err"] == 0 and a["status"] == r["status"] == 0, (case, solver, a["status"], r["status"])
        if solver in ("-i cg", "-i bicg"):
            assert a["iter"] == r["iter"], (case, solver, a["iter"], r["iter"])
        else:
            assert abs(a["iter"] - r["iter"]) <= 2, (case, solver, a["iter"], r["iter"])
        assert a["resid"] <= 1e-12


def test_every_served_solver_with_ilu(lib, reflib):
    """the systems of test_more_solvers_gpu.py, with the bars tests/test_ssor_gpu.py holds -p ssor to"""
    systems = {"p3d": ilu_cases.system("p3d"), "nonsym": ilu_cases.system("nonsym")}
    solvers = ["cgs", "cr", "gpbicg", "tfqmr", "bicgsafe", "orthomin", "bicr", "crs", "bicrstab", "gpbicr", "bicrsafe", "fgmres",
               "minres", "cocg", "cocr", "idrs", "idr1", "bicgstabl"]
    for mat, (ptr, idx, val) in systems.items():
        solvers_here = solvers if mat == "p3d" else [s for s in solvers if s not in ("minres", "cocg", "cocr", "cr")]   # symmetric-only methods
        b = orc.spmv_csr(ptr, idx, val, np.ones(len(ptr) - 1))
        for s in solvers_here:
            opts = f"-i {s} -p ilu -tol 1e-12 -maxiter 400"
            res = {}
            for tag, L in (("amd", lib), ("ref", reflib)):
                A = lisdrv.make_csr(L, ptr, idx, val)
                res[tag] = lisdrv.solve(L, A, b, opts)
                L.lis_matrix_destroy(A)
            a, r = res["amd"], res["ref"]
            assert a["err"] == 0 and a["status"] == r["status"], (mat, s, a["status"], r["status"])
            if r["status"] == 0:
                if mat == "p3d" and s != "fgmres":
                    assert a["iter"] == r["iter"], (mat, s, a["iter"], r["iter"])
                else:
                    assert abs(a["iter"] - r["iter"]) <= max(3, r["iter"] // 10), (mat, s, a["iter"], r["iter"])


def test_jacobi_solver_with_ilu_stays_refused(lib):
    ptr, idx, val = ilu_cases.system("p3d")
    A = lisdrv.make_csr(lib, ptr, idx, val)
    out = lisdrv.solve(lib, A, orc.spmv_csr(ptr, idx, val, np.ones(len(ptr) - 1)), "-i jacobi -p ilu -maxiter 5")
    assert out["err"] == capi.LIS_ERR_NOT_IMPLEMENTED
    lib.lis_matrix_destroy(A)


def unchanged(A, before):
    after = lisdrv.matrix_arrays(A)
    return (not A.contents.is_splited and after["type"] == before["type"] and
            all(np.array_equal(before[k], after[k]) for k in ("ptr", "index")) and np.array_equal(bits(before["value"]), bits(after["value"])))


def test_A_is_untouched_by_an_ilu_solve(lib):
    ptr, idx, val = ilu_cases.system("nonsym")
    A = lisdrv.make_csr(lib, ptr, idx, val)
    before = lisdrv.matrix_arrays(A)
    out = lisdrv.solve(lib, A, orc.spmv_csr(ptr, idx, val, np.ones(len(ptr) - 1)), "-i bicgstab -p ilu -ilu_fill 1 -tol 1e-12")
    assert out["err"] == 0 and out["status"] == 0
    assert unchanged(A, before)
    assert last_ilu(lib)[0] == 1
    # and a solve without it says so
    out = lisdrv.solve(lib, A, orc.spmv_csr(ptr, idx, val, np.ones(len(ptr) - 1)), "-i bicgstab -p jacobi -tol 1e-12")
    assert out["err"] == 0 and last_ilu(lib) == (0, 0, 0, 0, 0)
    lib.lis_matrix_destroy(A)


@pytest.mark.parametrize("opts,says", [("-p ilu -storage ell", "-storage"), ("-p ilu -storage bsr", "-storage"), ("-p ilu -scale jacobi", "-scale"),
                                       ("-p ilu -adds true", "-adds true"), ("-p ilu -ilu_fill -1", "-ilu_fill -1"),
                                       ("-p iluc", "preconditioner 8 is not served"), ("-p ilut", "preconditioner 9 is not served")])
def test_refusals_say_which_and_leave_A_untouched(lib, opts, says, capfd):
    ptr, idx, val = orc.poisson3d(6, 5, 4)
    A = lisdrv.make_csr(lib, ptr, idx, val)
    before = lisdrv.matrix_arrays(A)
    b = orc.spmv_csr(ptr, idx, val, np.ones(len(ptr) - 1))
    capfd.readouterr()
    out = lisdrv.solve(lib, A, b, "-i cg " + opts)
    assert out["err"] == capi.LIS_ERR_NOT_IMPLEMENTED
    text = "".join(capfd.readouterr())
    assert says in text, (opts, text[-400:])
    assert unchanged(A, before)
    lib.lis_matrix_destroy(A)


def test_other_storage_is_refused(lib):
    ptr, idx, val = orc.poisson3d(6, 5, 4)
    A = lisdrv.make_csr(lib, ptr, idx, val)
    E = lisdrv.convert(lib, A, "ell")
    before = lisdrv.matrix_arrays(E)
    out = lisdrv.solve(lib, E, orc.spmv_csr(ptr, idx, val, np.ones(len(ptr) - 1)), "-i cg -p ilu")
    assert out["err"] == capi.LIS_ERR_NOT_IMPLEMENTED
    after = lisdrv.matrix_arrays(E)
    assert after["type"] == capi.LIS_MATRIX_ELL and np.array_equal(before["index"], after["index"]) and np.array_equal(before["value"], after["value"])
    lib.lis_matrix_destroy(E)
    lib.lis_matrix_destroy(A)


def test_split_matrix_is_refused_loudly(lib, capfd):
    """an earlier -p ssor solve leaves A split: -p ilu on it is refused, A stays split and keeps solving with -p ssor;
    after lis_matrix_merge the same A is served"""
    ptr, idx, val = orc.poisson3d(6, 5, 4)
    b = orc.spmv_csr(ptr, idx, val, np.ones(len(ptr) - 1))
    A = lisdrv.make_csr(lib, ptr, idx, val)
    first = lisdrv.solve(lib, A, b, "-i cg -p ssor -tol 1e-12")
    assert first["err"] == 0 and A.contents.is_splited
    capfd.readouterr()
    out = lisdrv.solve(lib, A, b, "-i cg -p ilu -tol 1e-12")
    assert out["err"] == capi.LIS_ERR_NOT_IMPLEMENTED and A.contents.is_splited
    assert "split matrix" in "".join(capfd.readouterr())
    again = lisdrv.solve(lib, A, b, "-i cg -p ssor -tol 1e-12")
    assert again["err"] == 0 and again["iter"] == first["iter"]
    assert lib.dll.lis_amd_last_solve_ssor(None, None, None, None) == 1 and last_ilu(lib)[0] == 0
    assert lib.lis_matrix_merge(A) == 0
    out = lisdrv.solve(lib, A, b, "-i cg -p ilu -tol 1e-12")
    assert out["err"] == 0 and out["status"] == 0 and last_ilu(lib)[0] == 1
    lib.lis_matrix_destroy(A)


def test_value_edit_between_two_solves(lib, reflib):
    ptr, idx, val = ilu_cases.system("nonsym")
    n = len(ptr) - 1
    b = orc.spmv_csr(ptr, idx, val, np.ones(n))
    opts = "-i bicgstab -p ilu -tol 1e-12 -maxiter 500 -print mem"
    res = {}
    for tag, L in (("amd", lib), ("ref", reflib)):
        A = lisdrv.make_csr(L, ptr, idx, val)
        first = lisdrv.solve(L, A, b, opts)
        live = np.ctypeslib.as_array(A.contents.value, shape=(len(val),))
        live *= 1.0 + 0.25 * np.cos(np.arange(len(val)))
        if tag == "amd":
            assert lib.dll.lis_amd_matrix_host_modified(A) == 0
        second = lisdrv.solve(L, A, b, opts)
        res[tag] = (first, second)
        if tag == "amd":
            edited = live.copy()
            f = library_factor(lib, A, 0)
            assert ilu_cases.factor_differences(f, ilu_oracle.factor(ptr, idx, edited, 0)) == []
        L.lis_matrix_destroy(A)
    for k in (0, 1):
        a, r = res["amd"][k], res["ref"][k]
        assert a["err"] == 0 and a["status"] == r["status"] == 0 and abs(a["iter"] - r["iter"]) <= 2, (k, a["iter"], r["iter"])
    assert not np.array_equal(res["amd"][0]["x"], res["amd"][1]["x"])


def test_value_edit_in_the_reference_order_mode_is_the_reference(lib, reflib):
    """the second answer after an edit, in every bit of its history (one block, the reference at one thread)"""
    ptr, idx, val = ilu_cases.system("p3d")
    n = len(ptr) - 1
    b = orc.spmv_csr(ptr, idx, val, np.ones(n))
    opts = "-i cg -p ilu -tol 1e-12 -maxiter 500 -print mem"
    res = {}
    for tag, L in (("amd", lib), ("ref", reflib)):
        if tag == "amd":
            assert lib.dll.lis_amd_set_reference_reductions(1) == 0
        try:
            A = lisdrv.make_csr(L, ptr, idx, val)
            lisdrv.solve(L, A, b, opts)
            live = np.ctypeslib.as_array(A.contents.value, shape=(len(val),))
            live[np.asarray(idx) == np.repeat(np.arange(n), np.diff(ptr))] *= 1.5            # a heavier diagonal: still symmetric positive definite
            if tag == "amd":
                assert lib.dll.lis_amd_matrix_host_modified(A) == 0
            res[tag] = lisdrv.solve(L, A, b, opts)
            L.lis_matrix_destroy(A)
        finally:
            if tag == "amd":
                lib.dll.lis_amd_set_reference_reductions(0)
    a, r = res["amd"], res["ref"]
    assert (a["iter"], a["status"]) == (r["iter"], r["status"]) and a["status"] == 0
    assert np.array_equal(bits(a["rhistory"]), bits(r["rhistory"])) and np.array_equal(bits(a["x"]), bits(r["x"]))


@pytest.mark.parametrize("extra", [[], ["-ilu_fill", "1"]])
def test_test3b_driver_with_ilu(tmp_path, extra):
    drv = os.path.join(os.path.dirname(HERE), "oracle", "_ref", "drivers")
    rep = {}
    for tag in ("amd", "ref"):
        exe = os.path.join(drv, f"test3b_{tag}")
        if not os.path.exists(exe):
            pytest.skip(f"{exe} not built")
        out = subprocess.run([exe, "10", "9", "8", "1", str(tmp_path / f"s_{tag}"), str(tmp_path / f"r_{tag}"), "-i", "cg", "-p", "ilu", "-adds", "false"] + extra,
                             capture_output=True, text=True, timeout=600, env=dict(os.environ, OMP_NUM_THREADS="1"), check=True).stdout
        rep[tag] = (int(re.search(r"number of iterations = (\d+)", out).group(1)), re.search(r"linear solver status\s*:\s*(.*)", out).group(1).strip())
    assert rep["amd"] == rep["ref"], rep
