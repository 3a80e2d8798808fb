"""-p ilu on BSR storage on the GPU (lis_ilu.c on lis_sweep.c, kernels/ilu.hip) against tests/bilu_oracle.py in every bit, against
tests/golden/bilu_bits.npz, and against the reference library at one thread in a child process (bilu_cases: the reference's block ILU
is defined for bn <= 3 and usable at one thread only).

Factor and psolve are the model's bits at any block count T (the reference-order mode gives T > 1).  Whole solves are the reference's
in every bit in the reference-order mode at T = 1; in the default mode only the dot / nrm2 folds of the Krylov loops differ, so the
iteration counts stay within the slack tests/test_ilu_gpu.py::test_every_served_solver_with_ilu uses.
Not asserted: sign and payload of a NaN -- the zero-pivot case and "twice" at 8 row blocks (a block row without a stored diagonal block,
alone in its row block) produce NaNs on the GPU and in the model on a CPU, and the two units give their default NaN different signs;
everything else, infinities and the places of the NaNs included, is compared in every bit."""
import ctypes as C
import os

import numpy as np
import pytest

import bilu_cases
import bilu_oracle
import ilu_cases
import lis_amd
import lisdrv
import orc
import ssor_cases
from lis_amd import _capi as capi
from test_bilu_cpu import GOLDEN, GOLDEN_CASES, golden_case

pytestmark = pytest.mark.gpu
bits = bilu_cases.bits
SOLVERS = ("-i gmres -restart 30", "-i bicgstab", "-i cg")
SOLVE_CASES = (("p336", 2), ("p336", 3), ("queen_mini", 3))
COMMON = " -tol 1e-12 -maxiter 300 -print mem"


@pytest.fixture(scope="module")
def lib():
    lib = lis_amd.load()
    assert lis_amd.gpu_available(), "no HIP device: the product path has no CPU fallback"
    assert lib.initialize([]) == 0
    lib.dll.lis_amd_set_residency(0)
    lib.dll.lis_amd_matrix_host_modified.argtypes = [capi.PM]
    return lib


class blocks:
    """the library at T row blocks (the reference-order mode) for the duration of a with block"""
    def __init__(self, lib, T):
        self.lib, self.T = lib, T

    def __enter__(self):
        assert self.lib.dll.lis_amd_set_reference_reductions(self.T if self.T > 1 else 0) == 0

    def __exit__(self, *a):
        self.lib.dll.lis_amd_set_reference_reductions(0)


_models = {}


def model(name, bn, fill, T):
    key = (name, bn, fill, T)
    if key not in _models:
        bsr = bilu_cases.system(name, bn)
        f = bilu_oracle.factor(*bsr, fill, T)
        _models[key] = (f, bilu_oracle.psolve(f, bilu_cases.rhs(bsr[4]), T))
    return _models[key]


def untouched(A, bsr):
    bptr, bindex, value, bn, n = bsr
    after = lisdrv.matrix_arrays(A)
    return (not A.contents.is_splited and after["type"] == capi.LIS_MATRIX_BSR and after["bnr"] == bn and after["bnc"] == bn and after["n"] == n
            and np.array_equal(after["bptr"], bptr) and np.array_equal(after["bindex"], bindex) and np.array_equal(bits(after["value"]), bits(value)))


def check_against_model(lib, bsr, fill, T, want, wx, b, tag, nan_payload=False):
    """factor (pattern, order, every bit) and psolve (b apart from x, b aliased with x) of the library at T blocks against the model's;
    a NaN matches a NaN of any sign and payload (see the head of this file), every other value matches in every bit"""
    with blocks(lib, T):
        A = bilu_cases.make_bsr(lib, bsr)
        got = bilu_cases.library_factor(lib, A, fill)
        assert bilu_cases.factor_differences(got, want, nan_payload) == [], tag
        for alias in (False, True):
            err, x = bilu_cases.library_psolve(lib, A, fill, b, alias)
            assert err == 0, tag
            same = bits(x) == bits(wx)
            if not nan_payload:
                same |= np.isnan(x) & np.isnan(wx)
            bad = np.flatnonzero(~same)
            assert bad.size == 0, tag + (alias, int(bad[0]), float(x[bad[0]]), float(wx[bad[0]]))
        assert untouched(A, bsr), tag
        lib.lis_matrix_destroy(A)


@pytest.mark.parametrize("bn", bilu_cases.BNS)
@pytest.mark.parametrize("name", bilu_cases.NAMED)
def test_factor_and_psolve_are_the_model(lib, name, bn):
    """every fill level and every block count; the Poisson sizes leave n % bn = 0, 1 and 2: the padded last block for every residue"""
    bsr = bilu_cases.system(name, bn)
    for fill in bilu_cases.FILLS:
        for T in bilu_cases.THREADS:
            want, wx = model(name, bn, fill, T)
            check_against_model(lib, bsr, fill, T, want, wx, bilu_cases.rhs(bsr[4]), (name, bn, fill, T))


def test_every_residue_of_the_padding_is_covered():
    assert {(bn, bilu_cases.system(name, bn)[4] % bn) for name in ("p100", "p125", "p336") for bn in (2, 3)} == {(2, 0), (2, 1), (3, 0), (3, 1), (3, 2)}


def test_factor_and_psolve_match_the_golden(lib):
    G = np.load(GOLDEN)
    for name, bn, fill in GOLDEN_CASES:
        want, wx = golden_case(G, name, bn, fill)
        bsr = bilu_cases.system(name, bn)
        check_against_model(lib, bsr, fill, 1, want, wx, bilu_cases.rhs(bsr[4]), (name, bn, fill, "golden"))


def converted(lib, name, bn):
    ptr, idx, val = bilu_cases.csr_system(name)
    Ac = lisdrv.make_csr(lib, ptr, idx, val)
    A = lisdrv.convert(lib, Ac, "bsr", bn, bn)
    lib.lis_matrix_destroy(Ac)
    a = lisdrv.matrix_arrays(A)
    assert a["bnr"] == bn and a["bnc"] == bn and a["n"] == len(ptr) - 1
    return A, (a["bptr"], a["bindex"], a["value"], bn, a["n"])


def factor_and_psolve_are_the_model_on(lib, A, bsr, fill, tag):
    want = bilu_oracle.factor(*bsr, fill, 1)
    b = bilu_cases.rhs(bsr[4])
    assert bilu_cases.factor_differences(bilu_cases.library_factor(lib, A, fill), want) == [], tag
    err, x = bilu_cases.library_psolve(lib, A, fill, b)
    assert err == 0 and bilu_cases.same_bits(x, bilu_oracle.psolve(want, b, 1)), tag


@pytest.mark.parametrize("bn", [2, 3])
def test_a_converted_matrix_is_served(lib, bn):
    """lis_matrix_convert of a CSR matrix, in HBM: the factor and psolve of the blocks the conversion made.  A constant-coefficient
    Poisson matrix whose n the block size divides may then be held in its row form (for 2 x 2 blocks at least one is, asserted), so the
    factorisation reads the native upload kept on the entry; the others keep their native arrays in HBM"""
    row_forms = 0
    for name in ("p100", "p336", "nonsym"):
        A, bsr = converted(lib, name, bn)
        n = bsr[4]
        b = bilu_cases.rhs(n)
        assert np.allclose(bilu_cases.spmv(bsr, b), bilu_cases.spmv(bilu_cases.system(name, bn), b), rtol=1e-12, atol=0)      # the same matrix (its blocks perhaps in another order: sums to rounding)
        held_as_rows = lib.dll.lis_amd_matrix_device_type(A) == capi.LIS_MATRIX_CSR        # the row form: bptr / bindex / value are not in HBM
        assert not held_as_rows or (name != "nonsym" and n % bn == 0), (name, bn)           # only constant coefficients without padding
        row_forms += held_as_rows
        factor_and_psolve_are_the_model_on(lib, A, bsr, 1, (name, bn))
        out = lisdrv.solve(lib, A, bilu_cases.spmv(bsr, np.ones(n)), "-i gmres -restart 30 -p ilu" + COMMON)
        assert out["err"] == 0 and out["status"] == 0 and lib.dll.lis_amd_last_solve_ilu_block() == bn
        assert untouched(A, bsr), (name, bn)
        lib.lis_matrix_destroy(A)
    assert bn != 2 or row_forms >= 1, "no 2 x 2 blocking of a stencil was held in row form: the native upload on the entry went unused"


def test_value_edit_on_a_matrix_held_in_row_form(lib):
    """the native upload on the entry dies with the HBM copy: after a host edit the factor is the model's on the edited values.  Scaling
    every value by 3 keeps the coefficients constant (the copy is a row form before and after), a varying edit ends the row form"""
    name, bn = "p336", 2
    A, bsr = converted(lib, name, bn)
    assert bsr[4] % bn == 0 and lib.dll.lis_amd_matrix_device_type(A) == capi.LIS_MATRIX_CSR
    factor_and_psolve_are_the_model_on(lib, A, bsr, 0, (name, bn, "before"))
    live = np.ctypeslib.as_array(A.contents.value, shape=(len(bsr[2]),))
    for step, edit in (("scaled", lambda v: v * 3.0), ("varied", lambda v: v * (1.0 + 0.25 * np.cos(np.arange(len(v)))))):
        live[:] = edit(live.copy())
        assert lib.dll.lis_amd_matrix_host_modified(A) == 0
        edited = (bsr[0], bsr[1], live.copy(), bn, bsr[4])
        factor_and_psolve_are_the_model_on(lib, A, edited, 0, (name, bn, step))
        if step == "scaled":
            assert lib.dll.lis_amd_matrix_device_type(A) == capi.LIS_MATRIX_CSR
    lib.lis_matrix_destroy(A)


def two_copies_one_poisoned(bn):
    """two uncoupled copies of the 6 x 5 x 4 Poisson matrix in bn x bn blocks (n = 120: no padding for bn = 1, 2, 3), the first diagonal
    block of the second copy zeroed: block row 0 of a copy has no pivot before it, so that block is inverted as stored"""
    ptr, idx, val = orc.poisson3d(6, 5, 4)
    n = len(ptr) - 1
    assert n % bn == 0
    bptr, bindex, value = bilu_oracle.csr_to_bsr(ptr, idx, val, bn)
    nr, bs = len(bptr) - 1, bn * bn
    second = value.copy()
    k = [q for q in range(bptr[0], bptr[1]) if bindex[q] == 0][0]
    second[k * bs:(k + 1) * bs] = 0.0
    return (np.concatenate((bptr, bptr[1:] + bptr[-1])), np.concatenate((bindex, bindex + nr)), np.concatenate((value, second)), bn, 2 * n)


@pytest.mark.parametrize("bn", [1, 2, 3])
def test_zero_pivot_block_without_padding(lib, bn):
    """a diagonal block of zeros: lis_array_ge's 1 / 0 = inf (the whole result when bn = 1, NaN from 0 * inf in larger blocks) and what follows
    from it, at the model's places; the uncoupled half stays finite"""
    bsr = two_copies_one_poisoned(bn)
    n = bsr[4]
    for fill in (0, 1):
        want = bilu_oracle.factor(*bsr, fill, 1)
        wx = bilu_oracle.psolve(want, bilu_cases.rhs(n), 1)
        assert (np.isinf(want["D"]).any() if bn == 1 else np.isnan(want["D"]).any()) and np.isnan(wx).any() and np.isfinite(wx[:n // 2]).all()
        check_against_model(lib, bsr, fill, 1, want, wx, bilu_cases.rhs(n), ("zero pivot", bn, fill))


_doors = {}


def two_doors_system(name):
    """(ptr, idx, val) given to the library once as CSR and once as BSR with 1 x 1 blocks.  "handmade": columns stored twice, hence
    `serial`.  "edges": built to order (tests/ssor_cases.py) for the launch edges of the one factorisation kernel -- forward levels of
    1024 rows (the last size that joins a run), 1025 (the first on a launch of its own) and 30 (a run); rows of 63 kept terms (the last
    a thread takes) and of 64 (the first a workgroup takes) in the level on its own launch and in the run.  The rows from 1024 on
    hold no term of U (the backward pattern's first level mirrors onto them), so their L terms are all their kept terms at fill 0"""
    if name not in _doors:
        if name == "handmade":
            _doors[name] = ilu_cases.handmade()
        else:
            fwd = ssor_cases._sizes([1024, 1025, 30], {1: (63, 64), 2: (63, 64, 70)})
            bwd = ssor_cases._sizes([1055, 1024])
            _doors[name] = ssor_cases.matrices(ssor_cases.pattern(fwd, 41), ssor_cases.pattern(bwd, 42), 43)[0]
    return _doors[name]


@pytest.mark.parametrize("fill", [0, 1])
@pytest.mark.parametrize("name", ["handmade", "edges"])
def test_csr_and_bsr_1x1_give_the_same_factor_and_psolve(lib, name, fill):
    """one factorisation behind two doors: the same arrays as a CSR matrix and as a BSR matrix of 1 x 1 blocks give L, U, D
    (lis_amd_ilu_copy) and M^-1 b (lis_amd_ilu_psolve) equal in every bit, in the default mode and in the reference-order mode at 1
    and 3 row blocks.  Each case first shows through lis_amd_ilu_factor_info that it got the launches it is for"""
    from test_ilu_gpu import library_factor as csr_factor
    ptr, idx, val = two_doors_system(name)
    n = len(ptr) - 1
    b = np.random.default_rng(6).uniform(-1.0, 1.0, n)
    for mode in (0, 1, 3):
        assert lib.dll.lis_amd_set_reference_reductions(mode) == 0
        try:
            Ac, Ab = lisdrv.make_csr(lib, ptr, idx, val), bilu_cases.make_bsr(lib, (ptr, idx, val, 1, n))
            fc, fb = (C.c_int * 6)(), (C.c_int * 6)()
            assert lib.dll.lis_amd_ilu_factor_info(Ac, fill, fc) == 0 and lib.dll.lis_amd_ilu_factor_info(Ab, fill, fb) == 0
            assert list(fc) == list(fb), (name, fill, mode, list(fc), list(fb))
            if mode < 3:
                Lc, Uc = bilu_oracle.symbolic(ptr, idx, fill, 1)
                weight = [len(l) + len(u) for l, u in zip(Lc, Uc)]
                sizes = np.bincount(ssor_cases.levels_of([[(c, 0.0) for c in r] for r in Lc], 0)).tolist()
                print("TWO DOORS %s fill %d mode %d factor=%s level sizes=%s longest=%d" % (name, fill, mode, list(fc), sizes[:8], max(weight)))
                if name == "handmade":
                    assert fc[5] == 1                                                  # serial: a column stored twice
                elif fill == 0:
                    assert sizes == [1024, 1025, 30] and fc[:3] == [3, 3, 1]            # run, own launch, run
                    assert 63 in weight[1024:2049] and 64 in weight[1024:2049] and fc[3] == 1       # thread against workgroup on the own launch
                    assert 63 in weight[2049:] and 64 in weight[2049:] and fc[4] == 2 and fc[5] == 0   # and inside the run: the rows of 64 and 70
                else:                                                                  # the fill-in chains the 1025 rows: small levels, one run, longer rows
                    assert fc[0] == len(sizes) > 3 and fc[4] >= 3 and fc[5] == 0 and max(weight) > 2 * ssor_cases.LONG_ROW
            got_c, got_b = csr_factor(lib, Ac, fill), bilu_cases.library_factor(lib, Ab, fill)
            assert bilu_cases.factor_differences(got_b, got_c) == [], (name, fill, mode)
            assert name == "handmade" or np.isfinite(got_c["D"]).all()                 # (handmade at 3 row blocks: a row without a stored diagonal entry alone in its block, 1 / 0)
            for alias in (False, True):
                ec, xc = bilu_cases.library_psolve(lib, Ac, fill, b, alias)
                eb, xb = bilu_cases.library_psolve(lib, Ab, fill, b, alias)
                assert ec == 0 and eb == 0 and bilu_cases.same_bits(xb, xc), (name, fill, mode, alias)
            lib.lis_matrix_destroy(Ac)
            lib.lis_matrix_destroy(Ab)
        finally:
            lib.dll.lis_amd_set_reference_reductions(0)


def last_ilu(lib):
    f, b, l, p = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    r = lib.dll.lis_amd_last_solve_ilu(C.byref(f), C.byref(b), C.byref(l), C.byref(p))
    return r, f.value, b.value, l.value, p.value


_schedules = {}


def expected_last_solve(job):
    """(levels, launches per psolve) lis_amd_last_solve_ilu must report after the job's solve, from the model's pattern at one row block: the
    forward levels of L, and the launches of the forward sweep on L plus those of the backward sweep on U by the rules restated in
    tests/ssor_cases.py (runs of levels of at most SMALL_LEVEL block rows share a launch)"""
    fill = int(job["opts"].split("-ilu_fill ")[1][0])
    key = (job["name"], job["bn"], fill)
    if key not in _schedules:
        bsr = bilu_cases.job_system(job)
        Lc, Uc = bilu_oracle.symbolic(bsr[0], bsr[1], fill, 1)
        fwd = ssor_cases.sweep_stats([[(c, 0.0) for c in r] for r in Lc], 0)["info"]
        bwd = ssor_cases.sweep_stats([[(c, 0.0) for c in r] for r in Uc], 1)["info"]
        _schedules[key] = (fwd[0], fwd[1] + bwd[1])
    return _schedules[key]


def solve_jobs():
    return [dict(kind="solve", name=name, bn=bn, opts="%s -p ilu -ilu_fill %d%s" % (s, fill, COMMON)) for name, bn in SOLVE_CASES for s in SOLVERS for fill in (0, 1)]


@pytest.fixture(scope="module")
def reference_solves():
    """every solve of this file on the reference at one thread, in ONE child process, computed once"""
    if not os.path.exists(orc.REF_SO):
        pytest.skip("oracle/_ref not built")
    jobs = solve_jobs()
    return {(j["name"], j["bn"], j["opts"]): r for j, r in zip(jobs, bilu_cases.reference_jobs(jobs))}


@pytest.mark.parametrize("name,bn", SOLVE_CASES)
def test_reference_order_mode_is_the_reference_at_one_thread(lib, reference_solves, name, bn):
    for job in solve_jobs():
        if (job["name"], job["bn"]) != (name, bn):
            continue
        want = reference_solves[(name, bn, job["opts"])]
        bsr = bilu_cases.job_system(job)
        b = bilu_cases.job_rhs(job, bsr)
        assert lib.dll.lis_amd_set_reference_reductions(1) == 0
        try:
            A = bilu_cases.make_bsr(lib, bsr)
            out = lisdrv.solve(lib, A, b, job["opts"])
            r, fill, blk, lev, la = last_ilu(lib)
            block = lib.dll.lis_amd_last_solve_ilu_block()
            lib.lis_matrix_destroy(A)
        finally:
            lib.dll.lis_amd_set_reference_reductions(0)
        assert out["err"] == 0 and want["err"] == 0 and want["status"] == 0
        assert r == 1 and blk == 1 and block == bn and fill == int(job["opts"].split("-ilu_fill ")[1][0])
        assert (lev, la) == expected_last_solve(job) and lev > 0, (job, lev, la, expected_last_solve(job))
        assert (out["iter"], out["status"]) == (want["iter"], want["status"]), (job, out["iter"], want["iter"])
        diff = np.flatnonzero(bits(out["rhistory"]) != bits(want["rhistory"]))
        assert diff.size == 0, (job, int(diff[0]))
        assert np.array_equal(bits(out["x"]), bits(want["x"])), job


@pytest.mark.parametrize("name,bn", SOLVE_CASES)
def test_solves_default_mode(lib, reference_solves, name, bn):
    for job in solve_jobs():
        if (job["name"], job["bn"]) != (name, bn):
            continue
        r = reference_solves[(name, bn, job["opts"])]
        bsr = bilu_cases.job_system(job)
        A = bilu_cases.make_bsr(lib, bsr)
        a = lisdrv.solve(lib, A, bilu_cases.job_rhs(job, bsr), job["opts"])
        assert last_ilu(lib) == (1, int(job["opts"].split("-ilu_fill ")[1][0]), 1) + expected_last_solve(job), (job, last_ilu(lib), expected_last_solve(job))
        assert lib.dll.lis_amd_last_solve_ilu_block() == bn
        assert lib.dll.lis_amd_last_solve_ssor(None, None, None, None) == 0 and lib.dll.lis_amd_last_solve_renumbered() == 0
        assert untouched(A, bsr), job
        lib.lis_matrix_destroy(A)
        assert a["err"] == 0 and a["status"] == r["status"] == 0, (job, a["status"], r["status"])
        assert abs(a["iter"] - r["iter"]) <= max(3, r["iter"] // 10), (job, a["iter"], r["iter"])
        assert a["resid"] <= 1e-12


def test_block_getter_is_zero_after_a_csr_ilu_solve(lib):
    bsr = bilu_cases.system("p100", 2)
    A = bilu_cases.make_bsr(lib, bsr)
    assert lisdrv.solve(lib, A, bilu_cases.spmv(bsr, np.ones(bsr[4])), "-i cg -p ilu" + COMMON)["err"] == 0
    assert lib.dll.lis_amd_last_solve_ilu_block() == 2
    lib.lis_matrix_destroy(A)
    ptr, idx, val = bilu_cases.csr_system("p100")
    A = lisdrv.make_csr(lib, ptr, idx, val)
    assert lisdrv.solve(lib, A, orc.spmv_csr(ptr, idx, val, np.ones(len(ptr) - 1)), "-i cg -p ilu" + COMMON)["err"] == 0
    assert last_ilu(lib)[0] == 1 and lib.dll.lis_amd_last_solve_ilu_block() == 0
    assert lisdrv.solve(lib, A, orc.spmv_csr(ptr, idx, val, np.ones(len(ptr) - 1)), "-i cg -p none" + COMMON)["err"] == 0
    assert last_ilu(lib)[0] == 0 and lib.dll.lis_amd_last_solve_ilu_block() == 0
    lib.lis_matrix_destroy(A)


def test_value_edit_between_two_solves(lib):
    """the second solve factorises the edited values: its factor is the model's on them, and its answer another one"""
    bptr, bindex, value, bn, n = bsr = bilu_cases.system("nonsym", 3)
    b = bilu_cases.spmv(bsr, np.ones(n))
    opts = "-i bicgstab -p ilu" + COMMON
    A = bilu_cases.make_bsr(lib, bsr)
    first = lisdrv.solve(lib, A, b, opts)
    live = np.ctypeslib.as_array(A.contents.value, shape=(len(value),))
    live *= 1.0 + 0.25 * np.cos(np.arange(len(value)))
    assert lib.dll.lis_amd_matrix_host_modified(A) == 0
    edited = live.copy()
    second = lisdrv.solve(lib, A, b, opts)
    assert first["err"] == 0 and second["err"] == 0 and first["status"] == 0 and second["status"] == 0
    assert not np.array_equal(first["x"], second["x"])
    want = bilu_oracle.factor(bptr, bindex, edited, bn, n, 0, 1)
    assert bilu_cases.factor_differences(bilu_cases.library_factor(lib, A, 0), want) == []
    err, x = bilu_cases.library_psolve(lib, A, 0, bilu_cases.rhs(n))
    assert err == 0 and bilu_cases.same_bits(x, bilu_oracle.psolve(want, bilu_cases.rhs(n), 1))
    lib.lis_matrix_destroy(A)


def rect_bsr():
    """2 x 3 blocks on 12 rows: the diagonal blocks only"""
    n, bnr, bnc = 12, 2, 3
    return n, bnr, bnc, np.arange(7, dtype=np.int32), np.array([0, 0, 1, 1, 2, 3], np.int32), np.ones(6 * 6)


def make_bsr_blocks(lib, n, bnr, bnc, bptr, bindex, value):
    A = capi.PM()
    assert lib.lis_matrix_create(capi.LIS_COMM_WORLD, C.byref(A)) == 0
    assert lib.lis_matrix_set_size(A, n, 0) == 0
    p, i, v = capi.P_INT(), capi.P_INT(), capi.P_DBL()
    assert lib.lis_matrix_malloc_bsr(n, bnr, bnc, len(bindex), C.byref(p), C.byref(i), C.byref(v)) == 0
    C.memmove(p, bptr.ctypes.data, bptr.nbytes)
    C.memmove(i, bindex.ctypes.data, bindex.nbytes)
    C.memmove(v, value.ctypes.data, value.nbytes)
    assert lib.lis_matrix_set_bsr(bnr, bnc, len(bindex), p, i, v, A) == 0
    assert lib.lis_matrix_assemble(A) == 0
    return A


def refused(lib, A, b, opts, says, capfd):
    before = lisdrv.matrix_arrays(A)
    split = bool(A.contents.is_splited)
    capfd.readouterr()
    out = lisdrv.solve(lib, A, b, opts)
    text = "".join(capfd.readouterr())
    assert out["err"] == capi.LIS_ERR_NOT_IMPLEMENTED, (opts, out["err"])
    for s in says + ("(A is untouched)",):
        assert s in text, (opts, s, text[-500:])
    said = [line for line in text.splitlines() if says[0] in line]
    assert said and said[-1].rstrip().endswith("(A is untouched)"), text[-300:]
    after = lisdrv.matrix_arrays(A)
    assert after["type"] == before["type"] and bool(A.contents.is_splited) == split
    for k in ("bptr", "bindex"):
        assert np.array_equal(before[k], after[k])
    assert np.array_equal(bits(before["value"]), bits(after["value"]))


def test_refusals_say_which_and_leave_A_untouched(lib, capfd):
    # blocks that are not square
    n, bnr, bnc, bptr, bindex, value = rect_bsr()
    A = make_bsr_blocks(lib, n, bnr, bnc, bptr, bindex, value)
    refused(lib, A, np.ones(n), "-i gmres -p ilu", ("-p ilu", "2 x 3"), capfd)
    lib.lis_matrix_destroy(A)
    # blocks larger than the reference's w[3]
    ptr, idx, val = bilu_cases.csr_system("p100")
    bsr4 = bilu_oracle.csr_to_bsr(ptr, idx, val, 4)
    A = bilu_cases.make_bsr(lib, bsr4 + (4, len(ptr) - 1))
    refused(lib, A, np.ones(len(ptr) - 1), "-i gmres -p ilu", ("-p ilu", "4 x 4", "w[3]", "1977"), capfd)
    lib.lis_matrix_destroy(A)
    # a split BSR matrix, as an earlier -p bjacobi solve leaves it
    bsr = bilu_cases.system("p100", 2)
    b = bilu_cases.spmv(bsr, np.ones(bsr[4]))
    A = bilu_cases.make_bsr(lib, bsr)
    assert lisdrv.solve(lib, A, b, "-i cg -p bjacobi" + COMMON)["err"] == 0 and A.contents.is_splited
    refused(lib, A, b, "-i cg -p ilu", ("-p ilu", "lis_matrix_merge(A) first"), capfd)
    assert lib.lis_matrix_merge(A) == 0
    out = lisdrv.solve(lib, A, b, "-i cg -p ilu" + COMMON)
    assert out["err"] == 0 and out["status"] == 0 and lib.dll.lis_amd_last_solve_ilu_block() == 2
    # every solver that applies M^-H
    for s in ("bicg", "bicr", "crs", "bicrstab", "gpbicr", "bicrsafe"):
        refused(lib, A, b, "-i %s -p ilu" % s, ("-p ilu", "M^-H", "M^-1", "OpenMP"), capfd)
    # options outside the scope, as for CSR
    for opts, says in (("-p ilu -storage csr", "-storage"), ("-p ilu -scale jacobi", "-scale"), ("-p ilu -adds true", "-adds true"), ("-p ilu -ilu_fill -1", "-ilu_fill -1")):
        refused(lib, A, b, "-i gmres " + opts, (says,), capfd)
    # the tool entry point for M^-H
    err, _ = bilu_cases.library_psolve(lib, A, 0, b, transposed=1)
    assert err == capi.LIS_ERR_NOT_IMPLEMENTED
    err, x = bilu_cases.library_psolve(lib, A, 0, b)
    assert err == 0 and np.isfinite(x).all()
    lib.lis_matrix_destroy(A)


def test_what_stays_refused(lib):
    """-p ilu -storage bsr on a CSR matrix, -p iluc / -p ilut and the Jacobi solver on a BSR matrix"""
    ptr, idx, val = bilu_cases.csr_system("p100")
    A = lisdrv.make_csr(lib, ptr, idx, val)
    out = lisdrv.solve(lib, A, np.ones(len(ptr) - 1), "-i cg -p ilu -storage bsr")
    assert out["err"] == capi.LIS_ERR_NOT_IMPLEMENTED and A.contents.matrix_type == capi.LIS_MATRIX_CSR
    lib.lis_matrix_destroy(A)
    bsr = bilu_cases.system("p100", 2)
    A = bilu_cases.make_bsr(lib, bsr)
    for opts in ("-i cg -p iluc", "-i cg -p ilut", "-i jacobi -p ilu -maxiter 5"):
        assert lisdrv.solve(lib, A, np.ones(bsr[4]), opts)["err"] == capi.LIS_ERR_NOT_IMPLEMENTED, opts
        assert untouched(A, bsr)
    lib.lis_matrix_destroy(A)
