"""-p ssor on BSR storage on the GPU (lis_ssor.c on lis_sweep.c, kernels/bsptrsv.hip) through the Lis C API, against
tests/golden/bssor_bits.npz (make_golden_bssor.py: the reference at T = 1 and T = 8) and tests/bssor_oracle.py.

A->WD->value, lis_matrix_solve and lis_matrix_solveh with LOWER, UPPER and SSOR are the reference's in every bit, whichever way the BSR
matrix came to be (lis_matrix_set_bsr, lis_matrix_convert, -storage bsr -storage_block k).  Whole solves are the reference's at T threads
in every bit in the reference-order mode (lis_amd_set_reference_reductions(T)); in the default mode only the dot / nrm2 folds differ and
the bar is that of tests/test_bjacobi_gpu.py: the CG and BiCG counts are the reference's at one thread.
Not reachable in a one-rank test: the refusal of several ranks."""
import ctypes as C

import numpy as np
import pytest

import bilu_cases
import bssor_cases as cases
import bssor_oracle as oracle
import lis_amd
import lisdrv
import orc
import ssor_cases
from lis_amd import DeviceArray as DA, _capi as capi

pytestmark = pytest.mark.gpu
G = np.load(cases.GOLDEN)
same_bits = cases.same_bits


@pytest.fixture(scope="module")
def lib():
    lib = lis_amd.load()
    assert lis_amd.gpu_available(), "no HIP device: the product path has no CPU fallback"
    assert lib.initialize([]) == 0
    lib.dll.lis_amd_set_residency(0)
    lib.dll.lis_amd_matrix_host_modified.argtypes = [capi.PM]
    return lib


def bsr_matrix(lib, name, bn, route):
    """the named matrix as a BSR matrix of bn x bn blocks: "set" lis_matrix_set_bsr, "convert" lis_matrix_convert, "storage" still CSR
    (the solve's -storage bsr -storage_block bn converts it)"""
    ptr, idx, val = cases.system(name)
    if route == "set":
        return bilu_cases.make_bsr(lib, cases.to_bsr(ptr, idx, val, bn) + (bn, len(ptr) - 1))
    A = lisdrv.make_csr(lib, ptr, idx, val)
    if route == "storage":
        return A
    B = lisdrv.convert(lib, A, "bsr", bn, bn)
    lib.lis_matrix_destroy(A)
    return B


def last_ssor(lib):
    blk, lf, lb, la = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    r = lib.dll.lis_amd_last_solve_ssor(C.byref(blk), C.byref(lf), C.byref(lb), C.byref(la))
    return r, blk.value, lf.value, lb.value, la.value


def check_against_golden(lib, A, name, bn, omega, tag):
    n = A.contents.n
    got = cases.all_library_solves(lib, A, cases.rhs(n))
    bad = [what for what, v in got.items() if not same_bits(v, G[cases.tri_key(name, bn, omega, what)])]
    assert bad == [], (tag, bad)


# ---------------------------------------------------------------- WD and the triangular solves
@pytest.mark.parametrize("bn", cases.TRI_BNS)
@pytest.mark.parametrize("route", ["set", "convert", "storage"])
def test_wd_and_the_six_solves_are_the_golden(lib, route, bn):
    """n = 105: bn = 2, 4, 8 leave a partial last block.  A is BSR and split afterwards, and products on it still equal the oracle"""
    name, omega = "p105", 1.3
    A = cases.prepared(lib, bsr_matrix(lib, name, bn, route), omega, bn if route == "storage" else 0)
    a = A.contents
    n = a.n
    assert (a.bnr, a.bnc, a.nr) == (bn, bn, (n + bn - 1) // bn)
    check_against_golden(lib, A, name, bn, omega, (route, bn))
    ptr, idx, val = cases.system(name)
    bptr, bidx, bval = cases.to_bsr(ptr, idx, val, bn)
    x = np.linspace(-1.0, 1.0, n)
    assert same_bits(lisdrv.matvec(lib, A, x), orc.spmv_split_bsr(n, a.nr, bn, bn, bptr, bidx, bval, x)), (route, bn)
    lib.lis_matrix_destroy(A)


@pytest.mark.parametrize("omega", cases.OMEGAS)
@pytest.mark.parametrize("name", cases.TRI_NAMES)
def test_every_triangular_case_of_the_golden(lib, name, omega):
    for bn in cases.TRI_BNS:
        A = cases.prepared(lib, bsr_matrix(lib, name, bn, "storage"), omega, bn)
        check_against_golden(lib, A, name, bn, omega, (name, bn, omega))
        lib.lis_matrix_destroy(A)


def test_special_values_through_the_api(lib):
    """a zero diagonal block entry row (a zero pivot: inf and NaN in WD), inf and -0.0 in b: the library is the model, a NaN matching any NaN"""
    ptr, idx, val = cases.system("p120")
    n, bn = len(ptr) - 1, 3
    bptr, bidx, bval = cases.to_bsr(ptr, idx, val, bn)
    bval = bval.copy()
    k = int(np.flatnonzero(bidx[bptr[5]:bptr[6]] == 5)[0]) + int(bptr[5])
    bval[k * 9] = 0.0                                                          # the first pivot of block row 5
    b = cases.rhs(n)
    b[40], b[41], b[77] = np.inf, -0.0, -np.inf
    A = cases.prepared(lib, bilu_cases.make_bsr(lib, (bptr, bidx, bval, bn, n)), 1.3)
    want = cases.model_solves((bptr, bidx, bval), bn, n, 1.3, b)
    assert not np.isfinite(want["wd"]).all()
    got = cases.all_library_solves(lib, A, b)
    bad = [what for what, v in got.items() if not same_bits(v, want[what], False)]
    assert bad == []
    lib.lis_matrix_destroy(A)


# ---------------------------------------------------------------- whole solves
@pytest.mark.parametrize("T", cases.THREADS)
@pytest.mark.parametrize("case,bn", cases.RUNS)
def test_reference_order_mode_is_the_reference_at_T_threads(lib, case, bn, T):
    ptr, idx, val = cases.system(case)
    n = len(ptr) - 1
    for solver in cases.SOLVERS:
        A = lisdrv.make_csr(lib, ptr, idx, val)
        b = lisdrv.matvec(lib, A, np.ones(n))
        assert lib.dll.lis_amd_set_reference_reductions(T) == 0
        try:
            out = lisdrv.solve(lib, A, b, "%s -storage_block %d %s" % (solver, bn, cases.COMMON))
        finally:
            lib.dll.lis_amd_set_reference_reductions(0)
        key = (case, solver, bn, T)
        assert out["err"] == 0 and A.contents.matrix_type == capi.LIS_MATRIX_BSR and A.contents.is_splited
        r = last_ssor(lib)
        assert r[:2] == (1, 1) and lib.dll.lis_amd_last_solve_ssor_block() == bn and lib.dll.lis_amd_last_solve_renumbered() == 0, (key, r)
        it, status = G[cases.run_key(case, solver, bn, T, "meta")]
        assert (out["iter"], out["status"]) == (it, status), (key, out["iter"], it)
        diff = np.flatnonzero(cases.bits(out["rhistory"]) != cases.bits(G[cases.run_key(case, solver, bn, T, "rhistory")]))
        assert diff.size == 0, (key, int(diff[0]))
        assert same_bits(out["x"], G[cases.run_key(case, solver, bn, T, "x")]), key
        lib.lis_matrix_destroy(A)


@pytest.mark.parametrize("case,bn", cases.RUNS)
def test_default_mode_counts_are_the_reference_at_one_thread(lib, case, bn):
    """the rule of tests/test_bjacobi_gpu.py: CG and BiCG, whose counts do not move with the order of the folds"""
    ptr, idx, val = cases.system(case)
    n = len(ptr) - 1
    for solver in ("-i cg", "-i bicg"):
        it, status = G[cases.run_key(case, solver, bn, 1, "meta")]
        if status != 0:
            continue                                                             # (CG on the nonsymmetric matrix: no count to hold)
        A = lisdrv.make_csr(lib, ptr, idx, val)
        out = lisdrv.solve(lib, A, lisdrv.matvec(lib, A, np.ones(n)), "%s -storage_block %d %s" % (solver, bn, cases.COMMON))
        assert out["err"] == 0 and (out["iter"], out["status"]) == (it, 0), (case, solver, bn, out["iter"], it)
        assert lib.dll.lis_amd_last_solve_ssor_block() == bn
        lib.lis_matrix_destroy(A)


def test_every_served_solver_with_block_ssor(lib):
    """every solver that takes -p ssor on CSR storage, those that call psolveh (BiCG, BiCR, CRS, BiCRSTAB, GPBiCR, BiCRSafe) among them, takes it on BSR storage: the
    status of the same solve on CSR storage, and where that is 0 the same answer"""
    ptr, idx, val = cases.system("p105")
    n = len(ptr) - 1
    b = orc.spmv_csr(ptr, idx, val, np.ones(n))
    for s in ("cg", "bicg", "bicgstab", "gmres",                                  # ... and the list of tests/test_ssor_gpu.py's test of the same name
              "cgs", "cr", "gpbicg", "tfqmr", "bicgsafe", "orthomin", "bicr", "crs", "bicrstab", "gpbicr", "bicrsafe", "fgmres", "minres", "cocg",
              "cocr", "idrs", "idr1", "bicgstabl"):
        outs = {}
        for storage in ("", " -storage bsr -storage_block 3"):
            A = lisdrv.make_csr(lib, ptr, idx, val)
            outs[storage] = lisdrv.solve(lib, A, b, "-i %s -p ssor%s -tol 1e-12 -maxiter 400" % (s, storage))
            assert lib.dll.lis_amd_last_solve_ssor_block() == (3 if storage else 1) or outs[storage]["err"] != 0, s
            lib.lis_matrix_destroy(A)
        point, block = outs[""], outs[" -storage bsr -storage_block 3"]
        assert (block["err"], block["status"]) == (point["err"], point["status"]), (s, block["err"], block["status"], point["err"], point["status"])
        if point["err"] == 0 and point["status"] == 0:
            assert np.abs(block["x"] - 1.0).max() < 1e-9, s


# ---------------------------------------------------------------- state
def test_last_solve_reports_point_and_block_forms(lib):
    ptr, idx, val = cases.system("p105")
    n = len(ptr) - 1
    b = orc.spmv_csr(ptr, idx, val, np.ones(n))
    A = lisdrv.make_csr(lib, ptr, idx, val)
    assert lisdrv.solve(lib, A, b, "-i cg -p jacobi")["err"] == 0 and lib.dll.lis_amd_last_solve_ssor_block() == 0
    assert lisdrv.solve(lib, A, b, "-i cg -p ssor")["err"] == 0 and lib.dll.lis_amd_last_solve_ssor_block() == 1
    lib.lis_matrix_destroy(A)
    for bn in (1, 4):
        A = lisdrv.make_csr(lib, ptr, idx, val)
        assert lisdrv.solve(lib, A, b, "-i cg -p ssor -storage bsr -storage_block %d" % bn)["err"] == 0
        assert lib.dll.lis_amd_last_solve_ssor_block() == bn and last_ssor(lib)[:2] == (1, 1)
        lib.lis_matrix_destroy(A)


def test_a_second_omega_keeps_the_first_wd(lib):
    """A->WD is built only while A->use_wd is not SOR, here as in the reference"""
    name, bn = "p120", 4
    A = cases.prepared(lib, bsr_matrix(lib, name, bn, "storage"), 1.3, bn)
    first = cases.wd_of(A)
    assert same_bits(first, G[cases.tri_key(name, bn, 1.3, "wd")])
    n = A.contents.n
    out = lisdrv.solve(lib, A, cases.rhs(n), "-i cg -p ssor -ssor_omega 1.0 -tol 1e-12")
    assert out["err"] == 0 and out["status"] == 0 and same_bits(cases.wd_of(A), first)
    lib.lis_matrix_destroy(A)


def test_a_host_edit_of_the_values_is_seen(lib):
    """a split matrix sweeps over its parts: the program edits A->L->value and A->U->value, says so through lis_amd_matrix_host_modified,
    and the next solves run on the edited blocks (WD stays: it is not rebuilt while use_wd says SOR)"""
    name, bn, omega = "p105", 2, 1.3
    ptr, idx, val = cases.system(name)
    n = len(ptr) - 1
    A = cases.prepared(lib, bsr_matrix(lib, name, bn, "storage"), omega, bn)
    b = cases.rhs(n)
    before = cases.library_solve(lib, A, "solve", oracle.SSOR, b)
    assert same_bits(before, G[cases.tri_key(name, bn, omega, "solve2")])
    a = A.contents
    for core in (a.L.contents, a.U.contents):
        live = np.ctypeslib.as_array(core.value, shape=(core.bnnz * bn * bn,))
        live *= 0.75
    assert lib.dll.lis_amd_matrix_host_modified(A) == 0
    bptr, bidx, bval = cases.to_bsr(ptr, idx, val, bn)
    L, U, D = oracle.split(bptr, bidx, bval, bn)
    scaled = lambda part: [[(c, blk * 0.75) for c, blk in row] for row in part]
    wd = oracle.make_wd(D, n, bn, omega)
    for solve, flag in oracle.SOLVES:
        want = (oracle.solve if solve == "solve" else oracle.solveh)(scaled(L), scaled(U), wd, n, bn, b, flag)
        assert same_bits(cases.library_solve(lib, A, solve, flag, b), want), (solve, flag)
    assert not np.array_equal(cases.library_solve(lib, A, "solve", oracle.SSOR, b), before)
    lib.lis_matrix_destroy(A)


def test_bjacobi_then_ssor_on_the_same_matrix(lib):
    name, bn = "p120", 3
    ptr, idx, val = cases.system(name)
    n = len(ptr) - 1
    b = orc.spmv_csr(ptr, idx, val, np.ones(n))
    A = lisdrv.make_csr(lib, ptr, idx, val)
    first = lisdrv.solve(lib, A, b, "-i cg -p bjacobi -storage bsr -storage_block %d -tol 1e-12" % bn)
    assert first["err"] == 0 and first["status"] == 0 and A.contents.is_splited and lib.dll.lis_amd_last_solve_ssor_block() == 0
    second = lisdrv.solve(lib, A, b, "-i cg -p ssor -ssor_omega 1.3 -tol 1e-12")
    assert second["err"] == 0 and second["status"] == 0 and lib.dll.lis_amd_last_solve_ssor_block() == bn
    assert np.abs(second["x"] - 1.0).max() < 1e-9
    check_against_golden(lib, A, name, bn, 1.3, "after bjacobi")
    lib.lis_matrix_destroy(A)


def test_schedule_introspection_counts_block_rows_and_block_terms(lib):
    name, bn = "poisson8x7x6", 2
    ptr, idx, val = cases.system(name)
    n = len(ptr) - 1
    A = cases.prepared(lib, bsr_matrix(lib, name, bn, "storage"), 1.3, bn)
    bptr, bidx, bval = cases.to_bsr(ptr, idx, val, bn)
    sweeps = ssor_cases.sweep_terms(bptr, bidx, np.zeros(len(bidx)))                # the block graph as a point pattern
    assert lib.dll.lis_amd_set_reference_reductions(8) == 0                         # one block at every T
    try:
        for w, (terms, desc) in enumerate(sweeps):
            info = (C.c_int * 6)()
            assert lib.dll.lis_amd_ssor_sweep_info(A, w, info) == 0
            assert list(info) == ssor_cases.sweep_stats(terms, desc)["info"], (w, list(info))
        sched = (C.c_double * 4)()
        assert lib.dll.lis_amd_ssor_schedule_info(A, sched) == 0
    finally:
        lib.dll.lis_amd_set_reference_reductions(0)
    fwd, bwd = ssor_cases.sweep_stats(*sweeps[0]), ssor_cases.sweep_stats(*sweeps[1])
    assert int(sched[2]) == fwd["info"][1] + bwd["info"][1] and int(sched[3]) == fwd["info"][0]
    nr, bs = len(bptr) - 1, bn * bn
    per_sweep = lambda nnz: 4.0 * nr + 4.0 * (nr + 1) + (4.0 + 8.0 * bs) * nnz + (16.0 * bn + 8.0 * bs) * nr
    assert sched[1] == per_sweep(fwd["info"][5]) + per_sweep(bwd["info"][5])
    vb, vx = lisdrv.new_vector(lib, A, cases.rhs(n)), lisdrv.new_vector(lib, A)
    ms = (C.c_double * 2)()
    assert lib.dll.lis_amd_ssor_psolve_times(A, vb, vx, 2, ms) == 0 and ms[0] > 0 and ms[1] > 0
    assert same_bits(lisdrv.get_vector(lib, vx, n), cases.library_solve(lib, A, "solve", oracle.SSOR, cases.rhs(n)))
    lib.lis_vector_destroy(vb)
    lib.lis_vector_destroy(vx)
    lib.lis_matrix_destroy(A)


# ---------------------------------------------------------------- refusals
def snapshot(A):
    return lisdrv.matrix_arrays(A), bool(A.contents.is_splited)


def unchanged(A, before):
    a, split = snapshot(A)
    b, was_split = before
    return split == was_split and a["type"] == b["type"] and all(
        np.array_equal(cases.bits(a[k]) if a[k].dtype == np.float64 else a[k], cases.bits(b[k]) if b[k].dtype == np.float64 else b[k])
        for k in a if isinstance(a[k], np.ndarray))


def refused(lib, A, b, opts, says, capfd):
    before = snapshot(A)
    capfd.readouterr()
    out = lisdrv.solve(lib, A, b, opts + " -maxiter 5")
    assert out["err"] == capi.LIS_ERR_NOT_IMPLEMENTED
    text = "".join(capfd.readouterr())
    assert says in text and "(A is untouched)" in text, (opts, text[-400:])
    assert unchanged(A, before)


@pytest.mark.parametrize("opts,says", [("-i cg -p ssor -storage bsr -storage_block 2 -scale jacobi", "-scale"), ("-i cg -p ssor -storage bsr -storage_block 2 -adds true", "-adds true"),
                                       ("-i cg -p ssor -storage bsr -storage_block 9", "larger blocks are a follow-up")])
def test_refusals_say_which_and_leave_A_untouched(lib, opts, says, capfd):
    ptr, idx, val = orc.poisson3d(6, 5, 4)
    A = lisdrv.make_csr(lib, ptr, idx, val)
    refused(lib, A, orc.spmv_csr(ptr, idx, val, np.ones(len(ptr) - 1)), opts, says, capfd)
    assert A.contents.matrix_type == capi.LIS_MATRIX_CSR
    lib.lis_matrix_destroy(A)


def test_blocks_the_sweeps_do_not_hold_are_refused(lib, capfd):
    ptr, idx, val = orc.poisson3d(6, 5, 4)
    b = orc.spmv_csr(ptr, idx, val, np.ones(len(ptr) - 1))
    A = lisdrv.make_csr(lib, ptr, idx, val)
    for bnr, bnc, says in ((2, 3, "2 x 3 blocks"), (9, 9, "9 x 9 blocks")):
        B = lisdrv.convert(lib, A, "bsr", bnr, bnc)
        refused(lib, B, b, "-i cg -p ssor", says, capfd)
        lib.lis_matrix_destroy(B)
    assert lib.lis_matrix_set_blocksize(A, 2, 3, None, None) == 0
    refused(lib, A, b, "-i cg -p ssor -storage bsr -storage_block 0", "2 x 3 blocks", capfd)      # the conversion's own sizes
    lib.lis_matrix_destroy(A)


def test_a_matrix_in_hbm_only_is_refused(lib, capfd):
    ptr, idx, val = orc.poisson3d(6, 5, 4)
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
    out = lisdrv.solve(lib, A, orc.spmv_csr(ptr, idx, val, np.ones(n)), "-i cg -p ssor -storage bsr -storage_block 2")
    assert out["err"] == capi.LIS_ERR_NOT_IMPLEMENTED
    text = "".join(capfd.readouterr())
    assert "HBM only" in text and "(A is untouched)" in text
    assert A.contents.matrix_type == capi.LIS_MATRIX_CSR and not A.contents.is_splited and same_bits(lisdrv.matvec(lib, A, x), y)
    lib.lis_matrix_destroy(A)
