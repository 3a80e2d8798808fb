"""-p bjacobi on the GPU (lis_bjacobi.c, kernels/bdiag.hip) against tests/bjacobi_oracle.py in every bit and against
tests/golden/bjacobi_bits.{json,npz} (make_golden_bjacobi.py: the reference at T = 1 and T = 8).

The kernels are driven through liship_bdiag_inverse_f64 / liship_bdiag_matvec_f64 with hand-built blocks: block sizes 1 .. 5, 7, 8 (the
compile-time sizes, both sides of each start rule), 9 and 16 (the generic form); 1 .. 1025 blocks (inside a wavefront, across one, across
a workgroup, several workgroups); every residue n % bn.  The library's WD and psolves are the oracle's bits on the CPU test's matrices;
whole solves are the reference's in every bit in the reference-order mode (lis_amd_set_reference_reductions(T)); in the default mode only the
dot / nrm2 folds differ, and the CG and BiCG counts are the reference's at one thread.
Not asserted: sign and payload of a NaN.  Not reachable in a one-rank test: the refusal of several ranks."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import bjacobi_cases as cases
import bjacobi_oracle as oracle
import lis_amd
import lisdrv
import orc
from lis_amd import DeviceArray as DA, _capi as capi, check

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
G = json.load(open(os.path.join(HERE, "golden", "bjacobi_bits.json")))
GH = np.load(os.path.join(HERE, "golden", "bjacobi_bits.npz"))
P_DBL = capi.P_DBL
bits, same_bits = cases.bits, cases.same_bits

KERNEL_BNS = (1, 2, 3, 4, 5, 7, 8, 9, 16)
KERNEL_NRS = (1, 2, 63, 64, 65, 255, 256, 257, 1025)


@pytest.fixture(scope="module")
def lib():
    lib = lis_amd.load()
    assert lis_amd.gpu_available(), "no HIP device: the product path has no CPU fallback"
    assert lib.initialize([]) == 0
    lib.dll.lis_amd_set_residency(0)
    lib.dll.lis_amd_matrix_host_modified.argtypes = [capi.PM]
    return lib


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ---------------------------------------------------------------- the kernels
def kernel_inverse(lib, d, n, bn):
    nr = (n + bn - 1) // bn
    dd = DA.from_host(d, np.float64)
    work = DA.zeros(nr * bn * bn, np.float64) if bn > 8 else None
    check(lib.liship_bdiag_inverse_f64(n, nr, bn, dd.ptr, work.ptr if work else None, None))
    return dd.to_host()


def kernel_matvec(lib, d, x, n, bn, transposed):
    nr = (n + bn - 1) // bn
    dd, dx, dy = DA.from_host(d, np.float64), DA.from_host(x, np.float64), DA.from_host(np.full(n + 3, 7.0))
    check(lib.liship_bdiag_matvec_f64(n, nr, bn, transposed, dd.ptr, dx.ptr, dy.ptr, None))
    y = dy.to_host()
    assert np.array_equal(y[n:], [7.0, 7.0, 7.0]), "rows at or beyond n were written"
    return y[:n]


_wd = {}


def hand_built(bn, nr, residue):
    """(n, d, WD by the oracle) for nr blocks whose last one holds `residue` rows (0: a whole block), computed once per shape"""
    key = (bn, nr, residue)
    if key not in _wd:
        n = nr * bn - ((bn - residue) % bn)
        d = cases.random_blocks(nr, bn, 1000 * bn + nr)
        _wd[key] = (n, d, oracle.inverse(d, n, bn))
    return _wd[key]


def check_kernels(lib, bn, nr, residue):
    n, d, wd = hand_built(bn, nr, residue)
    got = kernel_inverse(lib, d, n, bn)
    bad = np.flatnonzero(bits(got) != bits(wd))
    assert bad.size == 0, ("inverse", bn, nr, residue, int(bad[0]), float(got[bad[0]]), float(wd[bad[0]]))
    x = cases.random_vector(n, 7 * bn + nr)
    for transposed, fn in ((0, oracle.matvec), (1, oracle.matvech)):
        for blocks in (wd, d):                       # the inverse, and the raw blocks with their subnormal and -0.0 entries
            y, want = kernel_matvec(lib, blocks, x, n, bn, transposed), fn(blocks, x, n, bn)
            bad = np.flatnonzero(bits(y) != bits(want))
            assert bad.size == 0, ("matvec", bn, nr, residue, transposed, int(bad[0]), float(y[bad[0]]), float(want[bad[0]]))


@pytest.mark.parametrize("nr", KERNEL_NRS)
@pytest.mark.parametrize("bn", KERNEL_BNS)
def test_kernels_are_the_oracle(lib, bn, nr):
    check_kernels(lib, bn, nr, (nr * 5 + 1) % bn)      # the residues take turns over the block counts ...


@pytest.mark.parametrize("bn", [b for b in KERNEL_BNS if b > 1])
def test_every_residue_of_the_last_block(lib, bn):
    for residue in range(bn):                          # ... and each one is met here, on 3 blocks and on 66
        check_kernels(lib, bn, 3, residue)
        check_kernels(lib, bn, 66, residue)


@pytest.mark.parametrize("bn", (2, 3, 4, 5, 9))
def test_negative_zero_first_products(lib, bn):
    d, x, n = cases.negative_zero_case(bn)
    for transposed, fn, first in ((0, oracle.matvec, bn <= 4), (1, oracle.matvech, bn <= 3)):
        y = kernel_matvec(lib, d, x, n, bn, transposed)
        assert same_bits(y, fn(d, x, n, bn)), (bn, transposed)
        assert np.signbit(y[:bn]).all() == first and not np.signbit(y[bn:]).any(), (bn, transposed)


@pytest.mark.parametrize("bn", (2, 3, 8, 9))
def test_a_zero_pivot_goes_on_as_in_the_reference(lib, bn):
    """a given matrix whose block 1 starts with a zero pivot, run once: the other blocks in every bit, that block in the places of its
    infinities and NaNs"""
    nr = 5
    d = cases.random_blocks(nr, bn, 99 + bn)
    d[bn * bn] = 0.0
    want = oracle.inverse(d, nr * bn, bn)
    got = kernel_inverse(lib, d, nr * bn, bn)
    blk = slice(bn * bn, 2 * bn * bn)
    assert not np.isfinite(want[blk]).all()
    assert np.array_equal(np.isnan(got[blk]), np.isnan(want[blk])) and np.array_equal(np.isinf(got[blk]), np.isinf(want[blk]))
    keep = np.ones(len(d), bool)
    keep[blk] = False
    assert same_bits(got[keep], want[keep])


def test_kernel_arguments(lib):
    d = DA.zeros(16, np.float64)
    assert lib.liship_bdiag_inverse_f64(0, 0, 3, None, None, None) == 0
    assert lib.liship_bdiag_inverse_f64(7, 2, 3, d.ptr, None, None) == -1             # 7 rows in blocks of 3 are 3 blocks
    assert lib.liship_bdiag_inverse_f64(9, 1, 9, d.ptr, None, None) == -1             # the generic form needs its work array
    assert lib.liship_bdiag_matvec_f64(4, 2, 2, 0, d.ptr, d.ptr, d.ptr, None) == -1   # y must not be x


# ---------------------------------------------------------------- the library
def library_wd(lib, A):
    out = np.full(A.contents.nr * A.contents.bnr * A.contents.bnc, 7.0)
    assert lib.dll.lis_amd_bjacobi_copy(A, out.ctypes.data_as(P_DBL)) == 0
    return out


def library_psolve(lib, A, b, transposed):
    vb, vx = lisdrv.new_vector(lib, A, b), lisdrv.new_vector(lib, A, np.full(len(b), 7.0))
    assert lib.dll.lis_amd_bjacobi_psolve(A, transposed, vb, vx) == 0
    out = lisdrv.get_vector(lib, vx, A.contents.n)
    lib.lis_vector_destroy(vb)
    lib.lis_vector_destroy(vx)
    return out


def last_bjacobi(lib):
    bn, nr, fb = C.c_int(), C.c_int(), C.c_int()
    r = lib.dll.lis_amd_last_solve_bjacobi(C.byref(bn), C.byref(nr), C.byref(fb))
    return r, bn.value, nr.value, fb.value


def precon_create(lib, A, options):
    """(err, solver, precon as a pointer to the public struct) of lis_precon_create on A"""
    S = capi.PS()
    assert lib.lis_solver_create(C.byref(S)) == 0
    assert lib.lis_solver_set_option(options.encode(), S) == 0
    S.contents.A = A
    create = lib.dll.lis_precon_create
    create.restype, create.argtypes = C.c_int, [capi.PS, C.POINTER(C.c_void_p)]
    pp = C.c_void_p()
    err = create(S, C.byref(pp))
    return err, S, pp


def precon_destroy(lib, S, pp):
    destroy = lib.dll.lis_precon_destroy
    destroy.restype, destroy.argtypes = C.c_int, [C.c_void_p]
    destroy(pp)
    lib.lis_solver_destroy(S)


@pytest.mark.parametrize("bn", cases.BNS)
@pytest.mark.parametrize("name", cases.NAMED)
def test_wd_and_psolves_are_the_oracle(lib, name, bn):
    ptr, idx, val = cases.system(name)
    n = len(ptr) - 1
    A = lisdrv.make_csr(lib, ptr, idx, val)
    err, S, pp = precon_create(lib, A, "-p bjacobi -storage bsr -storage_block %d" % bn)
    assert err == 0
    a = A.contents
    assert a.matrix_type == capi.LIS_MATRIX_BSR and a.is_splited and (a.bnr, a.bnc, a.nr) == (bn, bn, (n + bn - 1) // bn)
    want = oracle.inverse(cases.diagonal_blocks(ptr, idx, val, bn), n, bn)
    P = C.cast(pp, C.POINTER(cases.Precon)).contents
    WD = P.WD.contents
    assert (P.precon_type, WD.bn, WD.nr, WD.n) == (10, bn, a.nr, n)
    assert same_bits(np.ctypeslib.as_array(WD.value, shape=(len(want),)), want), "precon->WD"
    assert same_bits(library_wd(lib, A), want), "lis_amd_bjacobi_copy"
    for b in (cases.rhs(n), np.full(n, -0.0)):
        assert same_bits(library_psolve(lib, A, b, 0), oracle.matvec(want, b, n, bn)), "psolve"
        assert same_bits(library_psolve(lib, A, b, 1), oracle.matvech(want, b, n, bn)), "psolveh"
    precon_destroy(lib, S, pp)
    lib.lis_matrix_destroy(A)


@pytest.mark.parametrize("T", [1, 8])
@pytest.mark.parametrize("case", G["cases"])
def test_reference_order_mode_is_the_reference_at_T_threads(lib, case, T):
    ptr, idx, val = cases.golden_system(case)
    n = len(ptr) - 1
    for k in (2, 3, 4, 5):
        for solver in ("-i cg", "-i bicgstab", "-i gmres -restart 30", "-i bicg"):
            key = f"{case}|{solver}|k{k}|T{T}"
            if key in G["dropped"]:
                continue
            want = G["solves"][key]
            A = lisdrv.make_csr(lib, ptr, idx, val)
            b = lisdrv.matvec(lib, A, np.ones(n))
            assert lib.dll.lis_amd_set_reference_reductions(T) == 0
            try:
                out = lisdrv.solve(lib, A, b, f"{solver} -storage_block {k} " + G["common_options"])
            finally:
                lib.dll.lis_amd_set_reference_reductions(0)
            assert out["err"] == 0
            assert last_bjacobi(lib) == (1, k, (n + k - 1) // k, 0) and lib.dll.lis_amd_last_solve_renumbered() == 0
            assert (out["iter"], out["status"]) == (want["iter"], want["status"]), (key, out["iter"], want["iter"])
            diff = np.flatnonzero(bits(out["rhistory"]) != bits(GH[key]))
            assert diff.size == 0, (key, int(diff[0]))
            assert sha(out["x"]) == want["x_sha256"], key
            if solver == "-i cg":
                assert sha(library_wd(lib, A)) == G["solves"][f"{case}|WD|k{k}|T{T}"]["sha256"], key
            lib.lis_matrix_destroy(A)


@pytest.mark.parametrize("case", G["cases"])
def test_default_mode_counts_are_the_reference_at_one_thread(lib, case):
    ptr, idx, val = cases.golden_system(case)
    n = len(ptr) - 1
    for k in (2, 3, 4, 5):
        for solver in ("-i cg", "-i bicg"):
            key = f"{case}|{solver}|k{k}|T1"
            if key in G["dropped"]:
                continue
            A = lisdrv.make_csr(lib, ptr, idx, val)
            out = lisdrv.solve(lib, A, lisdrv.matvec(lib, A, np.ones(n)), f"{solver} -storage_block {k} " + G["common_options"])
            assert out["err"] == 0 and (out["iter"], out["status"]) == (G["solves"][key]["iter"], 0), (key, out["iter"])
            assert last_bjacobi(lib)[:2] == (1, k)
            lib.lis_matrix_destroy(A)


def test_every_served_solver_with_bjacobi(lib, reflib):
    ptr, idx, val = cases.system("p105")
    n = len(ptr) - 1
    b = orc.spmv_csr(ptr, idx, val, np.ones(n))
    for s in ("cgs", "cr", "gpbicg", "tfqmr", "bicgsafe", "orthomin", "bicr", "crs", "bicrstab", "gpbicr", "bicrsafe", "fgmres", "minres", "cocg",
              "cocr", "idrs", "idr1", "bicgstabl"):
        opts = f"-i {s} -p bjacobi -storage bsr -storage_block 3 -tol 1e-12 -maxiter 400"
        A = lisdrv.make_csr(lib, ptr, idx, val)
        a = lisdrv.solve(lib, A, b, opts)
        lib.lis_matrix_destroy(A)
        A = lisdrv.make_csr(reflib, ptr, idx, val)
        r = cases.reference_solve(reflib, A, b, opts)
        reflib.lis_matrix_destroy(A)
        assert a["err"] == 0 and a["status"] == r["status"], (s, a["status"], r["status"])
        if r["status"] == 0:
            assert abs(a["iter"] - r["iter"]) <= max(3, r["iter"] // 10), (s, a["iter"], r["iter"])
            assert last_bjacobi(lib)[:2] == (1, 3)


# ---------------------------------------------------------------- fallback, state, refusals
def test_a_matrix_without_blocks_falls_back_to_jacobi(lib):
    ptr, idx, val = cases.system("testmat0")
    n = len(ptr) - 1
    b = orc.spmv_csr(ptr, idx, val, np.ones(n))
    outs = {}
    for p in ("bjacobi", "jacobi"):
        A = lisdrv.make_csr(lib, ptr, idx, val)
        outs[p] = lisdrv.solve(lib, A, b, f"-i bicgstab -p {p} -tol 1e-12 -maxiter 500 -print mem")
        assert outs[p]["err"] == 0 and outs[p]["status"] == 0
        assert A.contents.matrix_type == capi.LIS_MATRIX_CSR and not A.contents.is_splited
        assert last_bjacobi(lib) == (0, 0, 0, 1 if p == "bjacobi" else 0)
        lib.lis_matrix_destroy(A)
    a, j = outs["bjacobi"], outs["jacobi"]
    assert a["iter"] == j["iter"] and same_bits(a["rhistory"], j["rhistory"]) and same_bits(a["x"], j["x"])
    # the solver's option reads back Jacobi, and the preconditioner is one
    A = lisdrv.make_csr(lib, ptr, idx, val)
    err, S, pp = precon_create(lib, A, "-p bjacobi")
    got = C.c_int()
    assert err == 0 and lib.lis_solver_get_precon(S, C.byref(got)) == 0 and got.value == 1
    P = C.cast(pp, C.POINTER(cases.Precon)).contents
    assert P.precon_type == 1 and not P.WD and bool(P.D)
    precon_destroy(lib, S, pp)
    lib.lis_matrix_destroy(A)


def test_state_after_a_served_solve(lib):
    ptr, idx, val = cases.system("p105")
    n = len(ptr) - 1
    b = orc.spmv_csr(ptr, idx, val, np.ones(n))
    A = lisdrv.make_csr(lib, ptr, idx, val)
    opts = "-i cg -p bjacobi -storage bsr -storage_block %d -tol 1e-12 -print mem"
    first = lisdrv.solve(lib, A, b, opts % 4)
    a = A.contents
    assert first["err"] == 0 and first["status"] == 0 and a.matrix_type == capi.LIS_MATRIX_BSR and a.is_splited and a.bnr == 4
    wd = library_wd(lib, A)
    second = lisdrv.solve(lib, A, b, opts % 4)
    assert second["err"] == 0 and second["iter"] == first["iter"] and same_bits(second["rhistory"], first["rhistory"]) and same_bits(second["x"], first["x"])
    # another -storage_block: A is BSR already, so the first blocks stay (lis_matrix_convert_self converts on another TYPE only)
    third = lisdrv.solve(lib, A, b, opts % 2)
    assert third["err"] == 0 and A.contents.bnr == 4 and last_bjacobi(lib) == (1, 4, (n + 3) // 4, 0)
    assert same_bits(third["rhistory"], first["rhistory"]) and same_bits(library_wd(lib, A), wd)
    lib.lis_matrix_destroy(A)


def test_a_host_edit_changes_wd(lib):
    """a split matrix multiplies by its parts and lis_precon_create inverts A->D, here as in the reference (A->value is not read again once A is
    split): the program edits the values of the diagonal blocks it solves with, says so through lis_amd_matrix_host_modified, and the next solve
    inverts the edited blocks"""
    ptr, idx, val = cases.system("p105")
    n, bn = len(ptr) - 1, 3
    b = orc.spmv_csr(ptr, idx, val, np.ones(n))
    A = lisdrv.make_csr(lib, ptr, idx, val)
    opts = "-i cg -p bjacobi -storage bsr -storage_block 3 -tol 1e-12"
    first = lisdrv.solve(lib, A, b, opts)
    assert first["err"] == 0
    before = library_wd(lib, A)
    a = A.contents
    count = a.nr * bn * bn
    live = np.ctypeslib.as_array(a.D.contents.value, shape=(count,))
    live *= 1.5                                                    # heavier diagonal blocks: still symmetric positive definite
    edited = live.copy()
    assert lib.dll.lis_amd_matrix_host_modified(A) == 0
    second = lisdrv.solve(lib, A, b, opts)
    assert second["err"] == 0 and second["status"] == 0
    after = library_wd(lib, A)
    assert same_bits(after, oracle.inverse(edited, n, bn)) and not np.array_equal(after, before)
    assert not np.array_equal(second["x"], first["x"])
    lib.lis_matrix_destroy(A)


def snapshot(A):
    a = lisdrv.matrix_arrays(A)
    return a, bool(A.contents.is_splited)


def unchanged(A, before):
    a, split = snapshot(A)
    b, was_split = before
    return split == was_split and a["type"] == b["type"] and all(
        np.array_equal(bits(a[k]) if a[k].dtype == np.float64 else a[k], bits(b[k]) if b[k].dtype == np.float64 else b[k])
        for k in a if isinstance(a[k], np.ndarray))


@pytest.mark.parametrize("opts,says", [("-i cg -p bjacobi -storage bsr -scale jacobi", "-scale"), ("-i cg -p bjacobi -storage bsr -adds true", "-adds true"),
                                       ("-i cg -p bjacobi -storage vbr", "VBR"), ("-i jacobi -p bjacobi -storage bsr", "Jacobi solver")])
def test_refusals_say_which_and_leave_A_untouched(lib, opts, says, capfd):
    ptr, idx, val = orc.poisson3d(6, 5, 4)
    A = lisdrv.make_csr(lib, ptr, idx, val)
    before = snapshot(A)
    b = orc.spmv_csr(ptr, idx, val, np.ones(len(ptr) - 1))
    capfd.readouterr()
    out = lisdrv.solve(lib, A, b, opts + " -maxiter 5")
    assert out["err"] == capi.LIS_ERR_NOT_IMPLEMENTED
    text = "".join(capfd.readouterr())
    assert says in text and "(A is untouched)" in text, (opts, text[-400:])
    assert unchanged(A, before)
    lib.lis_matrix_destroy(A)


def test_non_square_blocks_are_refused(lib, capfd):
    ptr, idx, val = orc.poisson3d(6, 5, 4)
    A = lisdrv.make_csr(lib, ptr, idx, val)
    B = lisdrv.convert(lib, A, "bsr", 2, 3)
    before = snapshot(B)
    capfd.readouterr()
    out = lisdrv.solve(lib, B, orc.spmv_csr(ptr, idx, val, np.ones(len(ptr) - 1)), "-i cg -p bjacobi")
    assert out["err"] == capi.LIS_ERR_NOT_IMPLEMENTED
    text = "".join(capfd.readouterr())
    assert "2 x 3 blocks" in text and "(A is untouched)" in text
    assert unchanged(B, before)
    lib.lis_matrix_destroy(B)
    lib.lis_matrix_destroy(A)


def test_non_square_blocks_of_the_conversion_are_refused(lib, capfd):
    """a CSR matrix whose lis_matrix_set_blocksize says 2 x 3 and -storage_block 0 (the matrix's own sizes): the conversion would make blocks
    that cannot be split, so the refusal comes before it; with -storage_block 3 the same matrix gets 3 x 3 blocks and is served"""
    ptr, idx, val = orc.poisson3d(6, 5, 4)
    b = orc.spmv_csr(ptr, idx, val, np.ones(len(ptr) - 1))
    A = lisdrv.make_csr(lib, ptr, idx, val)
    assert lib.lis_matrix_set_blocksize(A, 2, 3, None, None) == 0
    before = snapshot(A)
    capfd.readouterr()
    out = lisdrv.solve(lib, A, b, "-i cg -p bjacobi -storage bsr -storage_block 0 -maxiter 5")
    assert out["err"] == capi.LIS_ERR_NOT_IMPLEMENTED
    text = "".join(capfd.readouterr())
    assert "2 x 3 blocks" in text and "(A is untouched)" in text
    assert A.contents.matrix_type == capi.LIS_MATRIX_CSR and unchanged(A, before)
    out = lisdrv.solve(lib, A, b, "-i cg -p bjacobi -storage bsr -storage_block 3 -tol 1e-12")
    assert out["err"] == 0 and out["status"] == 0 and last_bjacobi(lib)[:2] == (1, 3) and A.contents.is_splited
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
    out = lisdrv.solve(lib, A, orc.spmv_csr(ptr, idx, val, np.ones(n)), "-i cg -p bjacobi -storage bsr -storage_block 2")
    assert out["err"] == capi.LIS_ERR_NOT_IMPLEMENTED
    text = "".join(capfd.readouterr())
    assert "HBM only" in text and "(A is untouched)" in text
    assert A.contents.matrix_type == capi.LIS_MATRIX_CSR and not A.contents.is_splited and same_bits(lisdrv.matvec(lib, A, x), y)
    lib.lis_matrix_destroy(A)
