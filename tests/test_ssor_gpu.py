"""-p ssor on the GPU (lis_ssor.c on lis_sweep.c, kernels/sptrsv.hip) against the reference library itself (oracle/_ref, one OpenMP thread) and
against tests/golden/ssor_bits.{json,npz} (make_golden_ssor.py: the reference at T = 1 and T = 8).

The preconditioner's bits are the reference's: the sweeps add every row's terms in the reference's order with its roundings.  Only the
dot / nrm2 folds of the Krylov loops differ in the default mode, so CG and BiCG counts are equal, the others within 2; in the
reference-order mode (lis_amd_set_reference_reductions(T)) whole solves are the reference's at T threads in every bit."""
import ctypes as C
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import lis_amd
import lisdrv
import orc
import queen_class
from lis_amd import _capi as capi

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
MM = os.path.join(HERE, "golden", "mm")
G = json.load(open(os.path.join(HERE, "golden", "ssor_bits.json")))
GH = np.load(os.path.join(HERE, "golden", "ssor_bits.npz"))


@pytest.fixture(scope="module")
def lib():
    lib = lis_amd.load()
    assert lis_amd.gpu_available(), "no HIP device: the product path has no CPU fallback"
    assert lib.initialize([]) == 0
    lib.dll.lis_amd_set_residency(0)
    return lib


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def from_file(L, path):
    A, b, x = capi.PM(), capi.PV(), capi.PV()
    assert L.lis_matrix_create(capi.LIS_COMM_WORLD, C.byref(A)) == 0
    assert L.lis_vector_create(capi.LIS_COMM_WORLD, C.byref(b)) == 0 and L.lis_vector_create(capi.LIS_COMM_WORLD, C.byref(x)) == 0
    assert L.lis_input(A, b, x, path.encode()) == 0
    return A


def matrix(L, case):
    if case.startswith("poisson"):
        N = int(case[7:])
        return lisdrv.make_csr(L, *orc.poisson3d(N, N, N))
    if case == "random":
        return lisdrv.make_csr(L, *random_with_diagonal())
    if case == "heavy":
        return lisdrv.make_csr(L, *orc.heavy_tail(3000, seed=3, cap=9000))
    if case == "queen_mini":
        path, _, _ = queen_class.generate("mini")
        try:
            return from_file(L, path)
        finally:
            os.unlink(path)
    return from_file(L, os.path.join(MM, case))


def random_with_diagonal():
    """orc.random_csr (unsorted columns, some rows empty but for the diagonal: empty L / U rows) with a diagonal entry in every row,
    placed after the row's other entries, so that WD is finite"""
    ptr, idx, val = orc.random_csr(700, 9, seed=4)
    rows, cols, vals = [], [], []
    p2 = [0]
    for r in range(len(ptr) - 1):
        c, v = list(idx[ptr[r]:ptr[r + 1]]), list(val[ptr[r]:ptr[r + 1]])
        if r not in c:
            c.append(r)
            v.append(4.0 + r % 3)
        cols += c
        vals += v
        p2.append(len(cols))
    return np.array(p2, np.int32), np.array(cols, np.int32), np.array(vals)


def wd_of(A):
    return np.ctypeslib.as_array(C.cast(A.contents.WD, C.POINTER(capi.MatrixDiag)).contents.value, shape=(A.contents.n,)).copy()


def triangular(L, A, fn, flag, b, alias=False):
    vb = lisdrv.new_vector(L, A, b)
    vx = vb if alias else lisdrv.new_vector(L, A)
    assert fn(A, vb, vx, flag) == 0
    out = lisdrv.get_vector(L, vx, A.contents.n)
    L.lis_vector_destroy(vb)
    if not alias:
        L.lis_vector_destroy(vx)
    return out


SWEEP_CASES = ["poisson32", "testmat0.mtx", "testmat.mtx", "testmat2.mtx", "random", "heavy", "queen_mini"]


@pytest.mark.parametrize("case", SWEEP_CASES)
def test_sweeps_are_the_reference_bit_for_bit(lib, reflib, case):
    mats = {}
    for tag, L in (("amd", lib), ("ref", reflib)):
        A = matrix(L, case)
        n = A.contents.n
        out = lisdrv.solve(L, A, lisdrv.matvec(L, A, np.ones(n)), "-i cg -p ssor -ssor_omega 1.3 -maxiter 1")
        assert out["err"] == 0
        assert A.contents.is_splited
        mats[tag] = (L, A)
    n = mats["ref"][1].contents.n
    assert np.array_equal(bits(wd_of(mats["amd"][1])), bits(wd_of(mats["ref"][1])))
    b = np.random.default_rng(11).uniform(-1, 1, n)
    for name in ("lis_matrix_solve", "lis_matrix_solveh"):
        for flag in (capi.LIS_MATRIX_LOWER, capi.LIS_MATRIX_UPPER, capi.LIS_MATRIX_SSOR):
            got = triangular(lib, mats["amd"][1], getattr(lib, name), flag, b)
            want = triangular(reflib, mats["ref"][1], getattr(reflib, name), flag, b)
            diff = np.flatnonzero(bits(got) != bits(want))
            assert diff.size == 0, (case, name, flag, int(diff[0]), got[diff[0]], want[diff[0]])
            alias = triangular(lib, mats["amd"][1], getattr(lib, name), flag, b, alias=True)
            assert np.array_equal(bits(alias), bits(got)), (case, name, flag, "aliased")
    for L, A in mats.values():
        L.lis_matrix_destroy(A)


def test_state_after_the_solve(lib, reflib):
    """A stays split (the product adds D, L, U); a second solve with another omega keeps the first omega's WD"""
    mats = {}
    for tag, L in (("amd", lib), ("ref", reflib)):
        A = matrix(L, "testmat0.mtx")
        n = A.contents.n
        b = lisdrv.matvec(L, A, np.ones(n))
        first = lisdrv.solve(L, A, b, "-i cg -p ssor -ssor_omega 1.3 -tol 1e-12")
        wd1 = wd_of(A)
        second = lisdrv.solve(L, A, b, "-i cg -p ssor -ssor_omega 0.7 -tol 1e-12")
        assert np.array_equal(bits(wd_of(A)), bits(wd1))                   # stale WD, as in the reference
        y = lisdrv.matvec(L, A, np.random.default_rng(2).uniform(-1, 1, n))
        mats[tag] = (first, second, y, wd1)
    assert np.array_equal(bits(mats["amd"][2]), bits(mats["ref"][2]))
    assert np.array_equal(bits(mats["amd"][3]), bits(mats["ref"][3]))
    for k in (0, 1):
        assert mats["amd"][k]["iter"] == mats["ref"][k]["iter"] and mats["amd"][k]["status"] == 0


SOLVERS = ["-i cg", "-i bicgstab", "-i gmres -restart 30", "-i bicg", "-i bicr"]


@pytest.mark.parametrize("case", ["poisson32", "poisson64", "testmat0.mtx", "queen_mini"])
@pytest.mark.parametrize("omega", ["1.0", "1.2"])
def test_solves_default_mode(lib, reflib, case, omega):
    for solver in SOLVERS:
        outs = {}
        for tag, L in (("amd", lib), ("ref", reflib)):
            A = matrix(L, case)
            b = lisdrv.matvec(L, A, np.ones(A.contents.n))
            outs[tag] = lisdrv.solve(L, A, b, f"{solver} -p ssor -ssor_omega {omega} -tol 1e-12 -maxiter 3000")
            if tag == "amd":
                assert lib.dll.lis_amd_last_solve_ssor(None, None, None, None) == 1
                assert lib.dll.lis_amd_last_solve_renumbered() == 0
            L.lis_matrix_destroy(A)
        a, r = outs["amd"], outs["ref"]
        assert a["err"] == 0 and a["status"] == r["status"] == 0, (case, solver, a["status"], r["status"])
        if solver in ("-i cg", "-i bicg"):
            assert a["iter"] == r["iter"], (case, solver, a["iter"], r["iter"])
        else:
            assert abs(a["iter"] - r["iter"]) <= 2, (case, solver, a["iter"], r["iter"])
        assert a["resid"] <= 1e-12


def test_every_served_solver_with_ssor(lib, reflib):
    """the systems of test_more_solvers_gpu.py, with that file's bars"""
    import sys
    sys.path.insert(0, os.path.join(HERE, "golden"))
    from make_golden_scale import test_matrix as nonsym_matrix
    systems = {"p3d": orc.poisson3d(8, 7, 6), "nonsym": nonsym_matrix(n=120, seed=9)}
    solvers = ["cgs", "cr", "gpbicg", "tfqmr", "bicgsafe", "orthomin", "bicr", "crs", "bicrstab", "gpbicr", "bicrsafe", "fgmres",
               "minres", "cocg", "cocr", "idrs", "idr1", "bicgstabl"]
    for mat, (ptr, idx, val) in systems.items():
        if mat == "p3d":
            solvers_here = solvers
        else:
            solvers_here = [s for s in solvers if s not in ("minres", "cocg", "cocr", "cr")]   # symmetric-only methods
        b = orc.spmv_csr(ptr, idx, val, np.ones(len(ptr) - 1))
        for s in solvers_here:
            opts = f"-i {s} -p ssor -tol 1e-12 -maxiter 400"
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


@pytest.mark.parametrize("T", [1, 8])
@pytest.mark.parametrize("case", ["poisson32", "mm/testmat0.mtx"])
def test_reference_order_mode_is_the_reference_at_T_threads(lib, case, T):
    common = G["common_options"]
    for solver in ("-i cg", "-i bicgstab", "-i gmres -restart 30", "-i bicg"):
        key = f"{case}|{solver}|T{T}"
        want = G["solves"][key]
        A = matrix(lib, "poisson32" if case == "poisson32" else "testmat0.mtx")
        n = A.contents.n
        b = lisdrv.matvec(lib, A, np.ones(n))
        assert lib.dll.lis_amd_set_reference_reductions(T) == 0
        try:
            out = lisdrv.solve(lib, A, b, solver + " " + common)
            blk, lf, lb, la = C.c_int(), C.c_int(), C.c_int(), C.c_int()
            assert lib.dll.lis_amd_last_solve_ssor(C.byref(blk), C.byref(lf), C.byref(lb), C.byref(la)) == 1
        finally:
            lib.dll.lis_amd_set_reference_reductions(0)
        assert blk.value == T and lf.value > 0
        assert (out["iter"], out["status"]) == (want["iter"], want["status"]), (key, out["iter"], want["iter"])
        diff = np.flatnonzero(bits(out["rhistory"]) != bits(GH[key]))
        assert diff.size == 0, (key, int(diff[0]))
        assert sha(out["x"]) == want["x_sha256"], key
        lib.lis_matrix_destroy(A)


@pytest.mark.parametrize("T", [1, 8])
@pytest.mark.parametrize("case", ["poisson32", "mm/testmat0.mtx"])
def test_wd_and_ssor_solves_match_the_golden_at_T(lib, case, T):
    A = matrix(lib, "poisson32" if case == "poisson32" else "testmat0.mtx")
    n = A.contents.n
    assert lib.dll.lis_amd_set_reference_reductions(T) == 0
    try:
        lisdrv.solve(lib, A, lisdrv.matvec(lib, A, np.ones(n)), "-i cg -p ssor -ssor_omega 1.3 -maxiter 1")
        assert sha(wd_of(A)) == G["solves"][f"{case}|wd|T{T}"]["sha256"]
        b = np.arange(1, n + 1, dtype=np.float64) / n
        for tag, fn in (("solve", lib.lis_matrix_solve), ("solveh", lib.lis_matrix_solveh)):
            assert sha(triangular(lib, A, fn, capi.LIS_MATRIX_SSOR, b)) == G["solves"][f"{case}|{tag}|T{T}"]["sha256"], (case, tag, T)
    finally:
        lib.dll.lis_amd_set_reference_reductions(0)
    lib.lis_matrix_destroy(A)


def test_levels_of_the_poisson_schedule(lib):
    """nx+ny+nz-2 levels at T = 1; at T = 8 the deepest of the 8 LIS_GET_ISIE row blocks"""
    for T in (1, 8):
        A = matrix(lib, "poisson32")
        b = lisdrv.matvec(lib, A, np.ones(A.contents.n))
        assert lib.dll.lis_amd_set_reference_reductions(T) == 0
        try:
            lisdrv.solve(lib, A, b, "-i cg -p ssor -maxiter 2")
            blk, lf, lb, la = C.c_int(), C.c_int(), C.c_int(), C.c_int()
            assert lib.dll.lis_amd_last_solve_ssor(C.byref(blk), C.byref(lf), C.byref(lb), C.byref(la)) == 1
        finally:
            lib.dll.lis_amd_set_reference_reductions(0)
        lib.lis_matrix_destroy(A)
        want = 94 if T == 1 else block_depth(32, T)
        assert (blk.value, lf.value, lb.value) == (T, want, want), (T, blk.value, lf.value, lb.value)
        assert 0 < la.value <= 2 * want


def block_depth(N, T):
    """levels of the forward sweep of 7-point Poisson N^3 cut into T LIS_GET_ISIE row blocks (Python restatement of the level rule)"""
    n = N ** 3
    q, rem = divmod(n, T)
    blk = np.array([i // (q + 1) if i < rem * (q + 1) else rem + (i - rem * (q + 1)) // q for i in range(n)])
    lev = np.zeros(n, np.int64)
    for i in range(n):
        z, r = divmod(i, N * N)
        y, x = divmod(r, N)
        best = 0
        for j in ((i - 1) if x > 0 else -1, (i - N) if y > 0 else -1, (i - N * N) if z > 0 else -1):
            if j >= 0 and blk[j] == blk[i]:
                best = max(best, lev[j] + 1)
        lev[i] = best
    return int(lev.max()) + 1


def test_ssor_solve_never_runs_renumbered(lib, reflib):
    """the 7-point matrix with its nodes numbered at random, renumbered at plan time: CG + Jacobi iterates on P A P^T, CG + SSOR after it
    neither builds nor uses that form (its sweeps follow the caller's row order) and counts as the reference does"""
    from test_kernels_gpu import _scrambled_poisson
    ptr, idx, val = _scrambled_poisson(True, vary=False)
    n = len(ptr) - 1
    b = orc.spmv_csr(ptr, idx, val, np.ones(n))
    dll = lib.dll
    dll.lis_amd_set_reorder_after.argtypes = [C.c_longlong]
    dll.lis_amd_set_reorder_after(0)                # the renumbered form at plan time
    try:
        A = lisdrv.make_csr(lib, ptr, idx, val)
        jac = lisdrv.solve(lib, A, b, "-i cg -p jacobi -tol 1e-10 -maxiter 500")
        assert jac["err"] == 0 and dll.lis_amd_last_solve_renumbered() == 1
        got = lisdrv.solve(lib, A, b, "-i cg -p ssor -tol 1e-10 -maxiter 500")
        assert dll.lis_amd_last_solve_renumbered() == 0 and dll.lis_amd_last_solve_ssor(None, None, None, None) == 1
    finally:
        dll.lis_amd_set_reorder_after(4096)
    R = lisdrv.make_csr(reflib, ptr, idx, val)
    want = lisdrv.solve(reflib, R, b, "-i cg -p ssor -tol 1e-10 -maxiter 500")
    assert got["status"] == want["status"] == 0 and got["iter"] == want["iter"], (got["iter"], want["iter"])
    lib.lis_matrix_destroy(A)
    reflib.lis_matrix_destroy(R)


def test_test3b_driver_with_ssor(tmp_path):
    drv = os.path.join(os.path.dirname(HERE), "oracle", "_ref", "drivers")
    rep = {}
    for tag in ("amd", "ref"):
        exe = os.path.join(drv, f"test3b_{tag}")
        if not os.path.exists(exe):
            pytest.skip(f"{exe} not built")
        out = subprocess.run([exe, "10", "9", "8", "1", str(tmp_path / f"s_{tag}"), str(tmp_path / f"r_{tag}"), "-i", "cg", "-p", "ssor", "-adds", "false"],
                             capture_output=True, text=True, timeout=600, env=dict(os.environ, OMP_NUM_THREADS="1"), check=True).stdout
        rep[tag] = (int(re.search(r"number of iterations = (\d+)", out).group(1)), re.search(r"linear solver status\s*:\s*(.*)", out).group(1).strip())
    assert rep["amd"] == rep["ref"], rep


@pytest.mark.parametrize("opts", ["-p ssor -storage ell", "-p ssor -scale jacobi", "-p ssor -adds true"])
def test_refusals_leave_A_untouched(lib, opts):
    ptr, idx, val = orc.poisson3d(6, 5, 4)
    A = lisdrv.make_csr(lib, ptr, idx, val)
    before = lisdrv.matrix_arrays(A)
    b = orc.spmv_csr(ptr, idx, val, np.ones(len(ptr) - 1))
    out = lisdrv.solve(lib, A, b, "-i cg " + opts)
    assert out["err"] == capi.LIS_ERR_NOT_IMPLEMENTED
    after = lisdrv.matrix_arrays(A)
    assert not A.contents.is_splited and after["type"] == capi.LIS_MATRIX_CSR
    for k in ("ptr", "index", "value"):
        assert np.array_equal(before[k], after[k])
    lib.lis_matrix_destroy(A)
