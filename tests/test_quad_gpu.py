"""-f quad on the GPU.  The kernel entries of lis_amd/csrc/kernels/quad.hip against the numpy model (tests/quad_model.py, itself held to the reference's
bits by tests/test_quad_cpu.py) and against the reference's goldens (tests/golden/quad_bits.npz), every element of hi and lo, with outputs that are longer
than a launch may write and a sentinel around them; then whole solves: in the reference-order mode every recorded solve of the reference's quad build in
count, status and every bit of rhistory, x and resid; in the default mode inside the reference's own spread over its thread counts; and the refusals.

Dots in the reference-order mode: the goldens hold T = 1, 2, 4, 8 (the generator's thread counts); T = 3, a count that splits no size evenly, goes
against the model, which the CPU tests hold to those goldens."""
import ctypes as C
import os

import numpy as np
import pytest

import format_cases as fc
import lis_amd
import lisdrv
import quad_cases as qc
import quad_model as qm
from gpu_arrays import Out, dev
from lis_amd import DeviceArray as DA, _capi as capi, check

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
EW_TILE = 8192 * 256            # lanes of the widest element-wise launch: one element more and lane 0 takes a second one
DOT_TILE = 1024 * 256           # the same for the tree's first level


@pytest.fixture(scope="module")
def lib():
    lib = lis_amd.load()
    assert lis_amd.gpu_available()
    assert lib.initialize([]) == 0
    yield lib
    lib.liship_set_reference_reductions(0)
    lib.dll.lis_amd_set_reference_reductions(0)
    lib.dll.lis_amd_set_quad_precision(0)


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(HERE, "golden", "quad_bits.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def work(lib):
    return DA(max(lib.liship_dot_dd_work_bytes() // 8, 2048), np.float64)


def bits(a):
    return np.atleast_1d(np.asarray(a, np.float64)).view(np.uint64)


class PairOut:
    """a (hi, lo) output in HBM, each part n elements behind `shift` with the sentinel around; `init`: the part's contents before the launch (in-place operations)"""

    def __init__(self, n, shift=0, init=None):
        self.hi, self.lo = Out(n, shift), Out(n, shift)
        if init is not None and n:
            for o, v in zip((self.hi, self.lo), init):
                full = fc.sentinel(o.d.count)
                full[shift:shift + n] = v
                o.d.upload(full)

    def holds(self, pair, what):
        self.hi.holds(np.asarray(pair[0], np.float64), (what, "hi"))
        self.lo.holds(np.asarray(pair[1], np.float64), (what, "lo"))


def dpair(pair, shift):
    a, b = dev(pair[0], np.float64, shift), dev(pair[1], np.float64, shift)
    return (a[0], b[0]), a[1], b[1]


VEC_SIZES = [0, 1, 63, 64, 65, 255, 256, 257, EW_TILE + 1]
# every small size at both shifts in both modes; the size past the tile once per mode, at either shift (its model takes seconds)
VEC_CASES = [(n, T, shift) for n in VEC_SIZES[:-1] for T in (0, 3) for shift in (0, 1)] + [(EW_TILE + 1, 0, 1), (EW_TILE + 1, 3, 0)]


# ------------------------------------------------------------------ vector operations
@pytest.mark.parametrize("n,T,shift", VEC_CASES)
def test_vector_ops_against_model(lib, n, T, shift):
    x, y = qc.dd_vector(n, 300 + n % 1000), qc.dd_vector(n, 400 + n % 1000)
    al = qc.dd_vector(1, 23, -2, 2)
    alpha = (float(al[0][0]), float(al[1][0]))
    d = qc.dd_vector(n, 500 + n % 1000)[0]
    kx, xh, xl = dpair(x, shift)
    ky, yh, yl = dpair(y, shift)
    kd, dptr = dev(d, np.float64, shift)
    check(lib.liship_set_reference_reductions(T))
    try:
        z = PairOut(n, shift)
        check(lib.liship_axpyz_dd_f64(n, alpha[0], alpha[1], xh, xl, yh, yl, z.hi.ptr, z.lo.ptr, None))
        z.holds(qm.axpyz(alpha, x, y, T), "axpyz")
        o = PairOut(n, shift, y)
        check(lib.liship_axpy_dd_f64(n, alpha[0], alpha[1], xh, xl, o.hi.ptr, o.lo.ptr, None))
        o.holds(qm.axpy(alpha, x, y, T), "axpy")
        o = PairOut(n, shift, y)
        check(lib.liship_xpay_dd_f64(n, xh, xl, alpha[0], alpha[1], o.hi.ptr, o.lo.ptr, None))
        o.holds(qm.xpay(x, alpha, y, T), "xpay")
        o = PairOut(n, shift)
        check(lib.liship_muld_dd_f64(n, xh, xl, dptr, o.hi.ptr, o.lo.ptr, None))
        o.holds(qm.muld(x, d), "muld")
        o = PairOut(n, shift, x)                         # in place: x = x * d
        check(lib.liship_muld_dd_f64(n, o.hi.ptr, o.lo.ptr, dptr, o.hi.ptr, o.lo.ptr, None))
        o.holds(qm.muld(x, d), "muld in place")
        o = PairOut(n, shift)
        check(lib.liship_widen_dd_f64(n, dptr, o.hi.ptr, o.lo.ptr, None))
        o.holds((d, np.zeros(n)), "widen")
    finally:
        check(lib.liship_set_reference_reductions(0))
    del kx, ky, kd


@pytest.mark.parametrize("T", qc.THREADS)
def test_vector_ops_against_goldens(lib, gold, T):
    n = qc.VEC_N
    x, y = qc.dd_vector(n, 21), qc.dd_vector(n, 22)
    al = qc.dd_vector(1, 23, -2, 2)
    alpha = (float(al[0][0]), float(al[1][0]))
    kx, xh, xl = dpair(x, 0)
    ky, yh, yl = dpair(y, 0)
    want = lambda k: (gold[k + "/hi"].view(np.float64), gold[k + "/lo"].view(np.float64))      # noqa: E731
    check(lib.liship_set_reference_reductions(T))
    try:
        z = PairOut(n)
        check(lib.liship_axpyz_dd_f64(n, alpha[0], alpha[1], xh, xl, yh, yl, z.hi.ptr, z.lo.ptr, None))
        z.holds(want(f"vec/axpyz/T{T}"), "axpyz")
        o = PairOut(n, 0, y)
        check(lib.liship_axpy_dd_f64(n, alpha[0], alpha[1], xh, xl, o.hi.ptr, o.lo.ptr, None))
        o.holds(want(f"vec/axpy/T{T}"), "axpy")
        o = PairOut(n, 0, y)
        check(lib.liship_xpay_dd_f64(n, xh, xl, alpha[0], alpha[1], o.hi.ptr, o.lo.ptr, None))
        o.holds(want(f"vec/xpay/T{T}"), "xpay")
    finally:
        check(lib.liship_set_reference_reductions(0))
    b, dd = qc.dd_vector(n, 31), qc.dd_vector(n, 32)[0]
    kb, bh, bl = dpair(b, 0)
    kd, dptr = dev(dd, np.float64, 0)
    o = PairOut(n)
    check(lib.liship_muld_dd_f64(n, bh, bl, dptr, o.hi.ptr, o.lo.ptr, None))
    o.holds(want("vec/muld"), "muld")
    del kx, ky, kb, kd


# ------------------------------------------------------------------ dots
def run_dot(lib, work, x, y, shift, T):
    n = len(x[0])
    kx, xh, xl = dpair(x, shift)
    ky, yh, yl = dpair(y, shift)
    res = Out(2)
    check(lib.liship_set_reference_reductions(T))
    try:
        check(lib.liship_dot_dd_f64(n, xh, xl, yh, yl, res.ptr, work.ptr, None))
    finally:
        check(lib.liship_set_reference_reductions(0))
    del kx, ky
    return res


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("n", sorted(set(VEC_SIZES[:-1] + [2048, 2049, DOT_TILE + 1])))
def test_dot_tree_against_model(lib, work, n, shift):
    x, y = qc.dd_vector(n, 600 + n % 1000, -3, 3), qc.dd_vector(n, 700 + n % 1000, -3, 3)
    res = run_dot(lib, work, x, y, shift, 0)
    res.holds(np.array(qm.dot_tree(x, y)), ("dot tree", n))


@pytest.mark.parametrize("T", [1, 2, 4, 8])
@pytest.mark.parametrize("n", qc.DOT_SIZES)
def test_dot_reference_order_against_goldens(lib, work, gold, n, T):
    x, y = qc.dot_vectors(n)
    for shift in (0, 1):
        res = run_dot(lib, work, x, y, shift, T)
        want = np.array([gold[f"dot/{n}/T{T}/hi"].view(np.float64)[0], gold[f"dot/{n}/T{T}/lo"].view(np.float64)[0]])
        res.holds(want, ("dot", n, T, shift))


@pytest.mark.parametrize("n", qc.DOT_SIZES + [2049])          # 2049: a chunk longer than the kernel's tile of terms at T = 1 .. 2
@pytest.mark.parametrize("T", [1, 3])
def test_dot_reference_order_against_model(lib, work, n, T):
    x, y = qc.dot_vectors(n)
    res = run_dot(lib, work, x, y, 1, T)
    res.holds(np.array(qm.dot_ref(x, y, T)), ("dot", n, T))


# ------------------------------------------------------------------ products
def run_spmv(lib, ptr, idx, val, x, transposed=False, shift=0):
    rows = len(ptr) - 1
    dp, di, dv = DA.from_host(ptr, np.int32), DA.from_host(idx if len(idx) else np.zeros(1, np.int32), np.int32), \
        DA.from_host(val if len(val) else np.zeros(1), np.float64)
    kx, xh, xl = dpair(x, shift)
    y = PairOut(rows, shift)
    f = lib.liship_spmv_csr_t_dd_f64 if transposed else lib.liship_spmv_csr_dd_f64
    check(f(rows, dp.ptr, di.ptr, dv.ptr, xh, xl, y.hi.ptr, y.lo.ptr, None))
    check(lib.liship_device_synchronize())
    del kx
    return y


def transpose_csr(ptr, idx, val, ncols):
    """the transposed CSR copy in scatter order: row j lists the entries of column j in ascending row of A"""
    rows = np.repeat(np.arange(len(ptr) - 1, dtype=np.int32), np.diff(ptr))
    order = np.argsort(idx, kind="stable")
    tptr = np.zeros(ncols + 1, np.int32)
    tptr[1:] = np.cumsum(np.bincount(idx, minlength=ncols))
    return tptr, rows[order].astype(np.int32), np.asarray(val)[order]


def big_matrix(lib, long_row):
    """one row more than a workgroup's block of rows, ~9 entries a row (a block's entries span more than one LDS stage); long_row: a row of one stage + 1 entries"""
    rows = lib.liship_spmv_csr_dd_rows_per_block() + 1
    stage = lib.liship_spmv_csr_dd_stage()
    ncols = stage + 200
    ptr, idx, val = qc_random(rows, ncols, 9, stage + 1 if long_row else None)
    return ptr, idx, val, ncols


def qc_random(rows, ncols, avg, long_row):
    import orc
    ptr, idx, val = orc.random_csr(rows, avg, seed=rows + (1 if long_row else 0), ncols=ncols, long_row=long_row)
    rng = np.random.default_rng(rows)
    val = rng.choice([-1.0, 1.0], len(idx)) * 10.0 ** rng.uniform(-8, 8, len(idx))
    return ptr, idx, val


def test_spmv_golden_rows(lib, gold):
    ptr, idx, val, x, _ = qc.rows_matrix()
    for shift in (0, 1):
        y = run_spmv(lib, ptr, idx, val, x, shift=shift)
        y.holds((gold["rows/T1/hi"].view(np.float64), gold["rows/T1/lo"].view(np.float64)), "golden rows")


@pytest.mark.parametrize("long_row", [False, True])
def test_spmv_past_one_block_and_past_one_stage(lib, long_row):
    ptr, idx, val, ncols = big_matrix(lib, long_row)
    if long_row:
        assert np.max(np.diff(ptr)) > lib.liship_spmv_csr_dd_stage()
    x = qc.dd_vector(ncols, 88)
    y = run_spmv(lib, ptr, idx, val, x)
    y.holds(qm.spmv_csr(ptr, idx, val, x), ("spmv", long_row))


def test_spmv_empty(lib):
    x = qc.dd_vector(4, 1)
    y = run_spmv(lib, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0), x)            # no rows: nothing written
    y.holds((np.zeros(0), np.zeros(0)), "no rows")
    y = run_spmv(lib, np.zeros(6, np.int32), np.zeros(0, np.int32), np.zeros(0), x)            # rows without entries: (0, 0)
    y.holds((np.zeros(5), np.zeros(5)), "empty rows")
    y = run_spmv(lib, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0), x, transposed=True)
    y.holds((np.zeros(0), np.zeros(0)), "no rows, transposed")


def test_spmv_transposed_golden(lib, gold):
    ptr, idx, val, _, ncols = qc.rows_matrix()
    xt = qc.transposed_input()
    tptr, tidx, tval = transpose_csr(ptr, idx, val, ncols)
    assert tptr[ncols] == tptr[ncols - 1]                     # the empty column
    for shift in (0, 1):
        y = run_spmv(lib, tptr, tidx, tval, xt, transposed=True, shift=shift)
        y.holds((gold["rows_t/T1/hi"].view(np.float64), gold["rows_t/T1/lo"].view(np.float64)), "golden transposed")


def test_spmv_transposed_past_one_block(lib):
    ptr, idx, val, ncols = big_matrix(lib, True)
    x = qc.dd_vector(len(ptr) - 1, 89)
    tptr, tidx, tval = transpose_csr(ptr, idx, val, ncols)
    y = run_spmv(lib, tptr, tidx, tval, x, transposed=True)
    y.holds(qm.spmv_csr_t(ptr, idx, val, x, ncols), "transposed")


# ------------------------------------------------------------------ whole solves
class Quad:
    def __init__(self, lib, T):
        self.lib, self.T = lib, T

    def __enter__(self):
        assert self.lib.dll.lis_amd_set_quad_precision(1) == 0
        assert self.lib.dll.lis_amd_set_reference_reductions(self.T) == 0

    def __exit__(self, *a):
        self.lib.dll.lis_amd_set_reference_reductions(0)
        self.lib.dll.lis_amd_set_quad_precision(0)


@pytest.fixture(scope="module")
def systems(lib):
    out = {}
    for mat, (ptr, idx, val) in qc.solve_matrices().items():
        out[mat] = (lisdrv.make_csr(lib, ptr, idx, val), qc.solve_rhs(mat, ptr, idx, val), len(ptr) - 1)
    return out


SOLVES = [(m, s, p) for m in ("poisson1d", "convdiff") for s in qc.SOLVERS for p in qc.PRECONS]


@pytest.mark.parametrize("mat,solver,precon", SOLVES)
def test_solves_carry_the_reference_bits(lib, gold, systems, mat, solver, precon):
    A, b, n = systems[mat]
    for T in qc.solve_threads(solver):
        for zeros in (True, False):
            key = qc.solve_key(mat, solver, precon, zeros, T)
            with Quad(lib, T):
                r = lisdrv.solve(lib, A, b, qc.solve_options(solver, precon, zeros), x0=None if zeros else qc.solve_x0(n))
            assert lib.dll.lis_amd_last_solve_quad() == 1
            print(key, "iter", r["iter"], "golden", int(gold[key + "/iter"][0]), "resid", r["resid"])
            assert r["err"] == 0 and r["status"] == int(gold[key + "/status"][0]), key
            assert r["iter"] == int(gold[key + "/iter"][0]), key
            assert np.array_equal(bits(r["rhistory"]), gold[key + "/rhistory"]), key
            assert np.array_equal(bits(r["x"]), gold[key + "/x"]), key
            assert np.array_equal(bits(r["resid"]), gold[key + "/resid"]), key


@pytest.mark.parametrize("mat,solver,precon", SOLVES)
def test_default_mode_stays_inside_the_reference_spread(lib, gold, systems, mat, solver, precon):
    A, b, n = systems[mat]
    for zeros in (True, False):
        with Quad(lib, 0):
            r = lisdrv.solve(lib, A, b, qc.solve_options(solver, precon, zeros), x0=None if zeros else qc.solve_x0(n))
        assert lib.dll.lis_amd_last_solve_quad() == 1
        counts = [int(gold[qc.solve_key(mat, solver, precon, zeros, T) + "/iter"][0]) for T in qc.solve_threads(solver)]
        x1 = gold[qc.solve_key(mat, solver, precon, zeros, 1) + "/x"].view(np.float64)
        spread = float(gold[f"spread/{mat}/{solver}/{precon}/{'zeros' if zeros else 'x0'}"][0])
        dist = float(np.max(np.abs(r["x"] - x1)))
        print(mat, solver, precon, zeros, "iter", r["iter"], "reference", counts, "max|x - x_ref|", dist, "4 x spread", 4 * spread)
        assert r["err"] == 0 and r["status"] == 0
        assert min(counts) - 1 <= r["iter"] <= max(counts) + 1          # (BiCG: the one golden count +- 1)
        if solver != "bicg":
            assert dist <= 4.0 * spread


def test_what_a_quad_solve_leaves_behind(lib, systems, capfd):
    A, b, n = systems["convdiff"]
    vb, vx = lisdrv.new_vector(lib, A, b), lisdrv.new_vector(lib, A)
    S = capi.PS()
    assert lib.lis_solver_create(C.byref(S)) == 0
    assert lib.lis_solver_set_option((qc.solve_options("bicgstab", "jacobi", False) + " -conv_cond nrm2_b").encode(), S) == 0
    lisdrv.set_vector(lib, vx, np.ones(n))
    ptr, idx, val = qc.solve_matrices()["convdiff"]
    import orc
    first = np.linalg.norm(b - orc.spmv_csr(ptr, idx, val, np.ones(n))) / np.linalg.norm(b)
    capfd.readouterr()
    with Quad(lib, 0):
        assert lib.lis_solve(A, vb, vx, S) == 0
    o = capfd.readouterr()
    assert "precision             : quad" in o.out + o.err
    it, itd, itq = C.c_int(), C.c_int(), C.c_int()
    assert lib.lis_solver_get_iterex(S, C.byref(it), C.byref(itd), C.byref(itq)) == 0
    assert it.value > 0 and itd.value == 0 and itq.value == it.value
    assert S.contents.precision == 1
    assert S.contents.rhistory[0] != 1.0 and abs(S.contents.rhistory[0] - first) < 1e-12 * first      # ||b - A x0|| / ||b||, written by the quad initial residual
    assert lib.dll.lis_amd_last_solve_quad() == 1
    # a double solve afterwards: the flag drops, the banner says double
    assert lib.lis_solver_set_option(b"-f double -tol 1e-10", S) == 0
    assert lib.lis_solve(A, vb, vx, S) == 0
    o = capfd.readouterr()
    assert "precision             : double" in o.out + o.err
    assert lib.dll.lis_amd_last_solve_quad() == 0
    assert lib.lis_solver_get_iterex(S, C.byref(it), C.byref(itd), C.byref(itq)) == 0
    assert itd.value == it.value and itq.value == 0
    lib.lis_solver_destroy(S)


@pytest.mark.parametrize("conv", ["nrm2_b", "nrm1_b -tol_w 1e-20"])       # nrm1_b: tol = ||b||_1 * tol_w + tol, and tol_w is 1 by default
def test_other_convergence_conditions_converge(lib, systems, conv):
    A, b, n = systems["convdiff"]
    with Quad(lib, 0):
        r = lisdrv.solve(lib, A, b, qc.solve_options("cg", "jacobi", True) + f" -conv_cond {conv}")
    assert r["iter"] > 10
    assert r["err"] == 0 and r["status"] == 0 and lib.dll.lis_amd_last_solve_quad() == 1
    ptr, idx, val = qc.solve_matrices()["convdiff"]
    import orc
    res = b - orc.spmv_csr(ptr, idx, val, r["x"])
    assert np.linalg.norm(res) <= 1e-14 * np.linalg.norm(b)


REFUSALS = ["-i gmres -f quad", "-i cg -f switch", "-i cg -p ilu -f quad", "-i bicg -p ssor -f quad", "-i cg -f quad -storage ell", "-i cg -f quad -scale jacobi"]


@pytest.mark.parametrize("options", REFUSALS)
def test_refusals_on_the_device(lib, systems, options):
    A, b, n = systems["convdiff"]
    vb, vx = lisdrv.new_vector(lib, A, b), lisdrv.new_vector(lib, A, np.ones(n))
    before = lisdrv.matrix_arrays(A)
    dbl = lisdrv.solve(lib, A, b, "-i bicgstab -p jacobi -tol 1e-12")            # A and b are in HBM by now
    S = capi.PS()
    assert lib.lis_solver_create(C.byref(S)) == 0
    assert lib.lis_solver_set_option(options.encode(), S) == 0
    with Quad(lib, 0):
        err = lib.lis_solve(A, vb, vx, S)
    assert err == capi.LIS_ERR_NOT_IMPLEMENTED and S.contents.retcode == capi.LIS_ERR_NOT_IMPLEMENTED
    assert lib.dll.lis_amd_last_solve_quad() == 0
    lib.lis_solver_destroy(S)
    after = lisdrv.matrix_arrays(A)
    for k, v in before.items():
        assert np.array_equal(v, after[k]), k
    assert A.contents.is_splited == 0 and A.contents.is_scaled == 0 and A.contents.matrix_type == capi.LIS_MATRIX_CSR
    assert np.array_equal(bits(lisdrv.get_vector(lib, vb)), bits(b)) and np.array_equal(lisdrv.get_vector(lib, vx), np.ones(n))
    again = lisdrv.solve(lib, A, b, "-i bicgstab -p jacobi -tol 1e-12")          # the HBM copy serves the same bits as before
    assert again["iter"] == dbl["iter"] and np.array_equal(bits(again["x"]), bits(dbl["x"]))
