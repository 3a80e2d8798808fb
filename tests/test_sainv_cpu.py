"""tests/sainv_oracle.py (the numpy statement of SAINV -- the build, M^-1, M^-H -- and of the two I+S psolves) held to the reference
library itself at 1, 3 and 8 OpenMP threads; and what liblis_amd shows of -p sainv and -p is without a GPU: the exported symbols, the
options, and every refusal that needs no device -- code 5 with its reason in the message, A and b unchanged.  (The refusal of several ranks is
the same kind of line in the same place; a job of several ranks cannot be made without devices.)

Matrices of fewer than 10 rows are left to the GPU tests' comparison with the model: the reference preallocates n / 10 entries per row."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import lis_amd
import lisdrv
import orc
import sainv_cases as sc
import sainv_oracle as so
from lis_amd import _capi as capi

HERE = os.path.dirname(os.path.abspath(__file__))
needs_ref = pytest.mark.skipif(not os.path.exists(orc.REF_SO), reason="oracle/_ref not built")
CASES = sc.SAINV_CASES + (("p654_fill", "p654", 0.01),)


@pytest.fixture(scope="module")
def lib():
    lib = lis_amd.load()
    assert lib.initialize([]) == 0
    return lib


def test_symbols_are_exported():
    dll = C.CDLL(lis_amd.LIB_PATH)
    amd = ("lis_amd_last_solve_sainv", "lis_amd_sainv_factor", "lis_amd_sainv_copy", "lis_amd_sainv_psolve", "lis_amd_sainv_times", "lis_amd_sainv_info",
           "lis_amd_is_psolve", "lis_amd_last_solve_is")
    hip = ("liship_sainv_gather_scale_f64", "liship_sainv_rows_f64", "liship_is_psolve_f64", "liship_is_psolveh_f64", "liship_is_truncate_f64")
    for name in amd + hip:
        assert hasattr(dll, name), name
    assert all(k in capi._AMD_PROTOS for k in amd) and all(k in lis_amd._LISHIP for k in hip)


def test_nothing_reported_before_any_solve():
    out = subprocess.run([sys.executable, "-c", "import lis_amd; lib = lis_amd.load(); print(lib.dll.lis_amd_last_solve_sainv(None, None, None), lib.dll.lis_amd_last_solve_is(None))"],
                         capture_output=True, text=True, check=True, cwd=os.path.dirname(HERE))
    assert out.stdout.split() == ["0", "0"]


def oracle_against_reference(ref, T):
    """every place where the models at T chunks are not the reference library at T threads: row lengths, index order and every bit of W, Z and d,
    psolve and psolveh of SAINV; psolve and psolveh of I+S"""
    bad = []
    for case, mat, tol in CASES:
        ptr, idx, val = sc.system(mat)
        n = len(ptr) - 1
        if n < 10:
            continue
        vec = sc.inputs(n)
        want = sc.reference_sainv(ref, ptr, idx, val, tol, vec)
        got = so.factor(ptr, idx, val, tol)
        bad += [(case, d) for d in sc.factor_differences(got, want)]
        for tag, b in vec.items():
            if not sc.same_bits(so.psolve(got, b, T), want["psolve"][tag]):
                bad.append((case, "psolve", tag))
            if not sc.same_bits(so.psolveh(got, b, T), want["psolveh"][tag]):
                bad.append((case, "psolveh", tag))
    for mat in sc.IS_MATRICES:
        ptr, idx, val = sc.system(mat)
        vec = sc.inputs(len(ptr) - 1)
        U = so.strict_upper(ptr, idx, val)
        for alpha, m in sc.IS_PARAMS:
            want = sc.reference_is(ref, ptr, idx, val, alpha, m, vec)
            for tag, b in vec.items():
                if not sc.same_bits(so.is_psolve(*U, alpha, m, b), want["psolve"][tag]):
                    bad.append((mat, alpha, m, "is psolve", tag))
                if not sc.same_bits(so.is_psolveh(*U, alpha, m, b, T), want["psolveh"][tag]):
                    bad.append((mat, alpha, m, "is psolveh", tag))
    return bad


def child(T):
    ref = lisdrv.open_lib(orc.REF_SO, threads=T)
    print("RESULT " + json.dumps(oracle_against_reference(ref, T)), flush=True)


@needs_ref
@pytest.mark.parametrize("T", sc.THREADS)
def test_models_are_the_reference_at_T_threads(T):
    """in a child process: the reference reads its thread count once, at initialize"""
    res = subprocess.run([sys.executable, "-c", "import sys; sys.path[:0] = %r; import test_sainv_cpu as t; t.child(%d)" % ([os.path.dirname(HERE), HERE], T)],
                         capture_output=True, text=True, env=dict(os.environ, OMP_NUM_THREADS=str(T)), timeout=900)
    assert res.returncode == 0, res.stderr[-2000:]
    assert json.loads([line for line in res.stdout.splitlines() if line.startswith("RESULT ")][-1][7:]) == []


def test_chunks_are_lis_get_isie():
    assert so.chunks(10, 3) == [(0, 4), (4, 7), (7, 10)] and so.chunks(2, 4) == [(0, 1), (1, 2), (2, 2), (2, 2)] and so.chunks(5, 1) == [(0, 5)]


def test_model_factor_means_what_it_says():
    """without the reference: at drop 0 on a tridiagonal matrix W^T A Z is the diagonal 1 / d to rounding; at a drop nothing passes, W = Z = I"""
    ptr, idx, val = sc.system("tri65")
    n = 65
    A = np.zeros((n, n))
    for i in range(n):
        A[i, idx[ptr[i]:ptr[i + 1]]] = val[ptr[i]:ptr[i + 1]]
    f = so.factor(ptr, idx, val, 0.0)
    W, Z = np.zeros((n, n)), np.zeros((n, n))
    for M, (p, c, v) in ((W, f["W"]), (Z, f["Z"])):
        for i in range(n):
            M[i, c[p[i]:p[i + 1]]] = v[p[i]:p[i + 1]]
            assert c[p[i]] == i and v[p[i]] == 1.0                 # unit diagonal first
    assert np.abs(W @ A @ Z.T - np.diag(1.0 / f["D"])).max() < 1e-12
    b = sc.inputs(n)["wide"]
    x = so.psolve(f, b, 1)
    assert np.abs(A @ x - b).max() <= 1e-9 * np.abs(b).max()      # the full factor is the inverse
    g = so.factor(ptr, idx, val, 10.0)
    assert g["W"][0][-1] == g["Z"][0][-1] == n and np.array_equal(g["D"], 1.0 / np.diag(A))


def test_negative_zero_inputs_give_positive_zero_sums():
    """every sum starts from +0.0: products that are all -0.0 leave +0.0, and x - alpha * (+0.0) keeps x's -0.0"""
    ptr, idx, val = sc.system("p654")
    f = so.factor(ptr, idx, val, 0.01)
    x = so.psolve(f, np.full(120, -0.0), 3)
    assert np.all(x == 0.0) and not np.signbit(x).any()
    y = so.is_psolve(*so.strict_upper(ptr, idx, val), 1.0, 3, np.full(120, -0.0))
    assert np.all(y == 0.0) and np.signbit(y).all()


def test_options_are_parsed(lib):
    S = capi.PS()
    assert lib.lis_solver_create(C.byref(S)) == 0
    s = S.contents
    DROP, ALPHA, M, ISLEVEL = 3, 4, 8, 14            # include/lis.h: LIS_PARAMS_DROP / _ALPHA - LIS_OPTIONS_LEN, LIS_OPTIONS_M, LIS_OPTIONS_ISLEVEL
    assert lib.lis_solver_set_option(b"-p sainv", S) == 0 and s.options[1] == 6
    assert lib.lis_solver_set_option(b"-p is", S) == 0 and s.options[1] == 5
    assert (s.params[DROP], s.params[ALPHA], s.options[M], s.options[ISLEVEL]) == (0.05, 1.0, 3, 1)
    assert lib.lis_solver_set_option(b"-sainv_drop 0.125 -is_alpha 0.75 -is_m 7 -is_level 2", S) == 0
    assert (s.params[DROP], s.params[ALPHA], s.options[M], s.options[ISLEVEL]) == (0.125, 0.75, 7, 2)
    name = C.create_string_buffer(64)
    assert lib.lis_solver_get_preconname(6, name) == 0 and name.value == b"SAINV"
    assert lib.lis_solver_get_preconname(5, name) == 0 and name.value == b"I+S"
    assert lib.lis_solver_destroy(S) == 0


def refused(lib, capfd, A, ptr, idx, val, opts, says):
    b = sc.rhs(ptr, idx, val)
    vb, vx = lisdrv.new_vector(lib, A, b), lisdrv.new_vector(lib, A)
    S = capi.PS()
    assert lib.lis_solver_create(C.byref(S)) == 0 and lib.lis_solver_set_option(opts.encode(), S) == 0
    capfd.readouterr()
    code = lib.lis_solve(A, vb, vx, S)
    text = "".join(capfd.readouterr())
    assert code == capi.LIS_ERR_NOT_IMPLEMENTED == 5, (opts, code)
    assert says in text and "(A is untouched)" in text, (opts, text[-400:])
    assert sc.same_bits(np.ctypeslib.as_array(vb.contents.value, shape=(len(b),)), b)
    lib.lis_solver_destroy(S)
    lib.lis_vector_destroy(vb)
    lib.lis_vector_destroy(vx)


@pytest.mark.parametrize("opts,says", [
    ("-i cg -p sainv -scale jacobi", "-p sainv together with -scale"), ("-i cg -p sainv -adds true", "-p sainv with -adds true"),
    ("-i jacobi -p sainv", "the Jacobi solver with -p sainv"),
    ("-i bicg -p is -is_level 0", "-is_level 0"), ("-i bicg -p is -scale symm_diag", "-p is together with -scale"),
    ("-i bicg -p is -adds true", "-p is with -adds true"), ("-i jacobi -p is", "the Jacobi solver with -p is"),
    ("-i bicg -p is -storage bsr", "-p is is served for CSR storage only")])
def test_refusals_need_no_device(lib, capfd, opts, says):
    ptr, idx, val = sc.system("p654")
    A = lisdrv.make_csr(lib, ptr, idx, val)
    before = lisdrv.matrix_arrays(A)
    refused(lib, capfd, A, ptr, idx, val, opts, says)
    after = lisdrv.matrix_arrays(A)
    assert not A.contents.is_splited and after["type"] == capi.LIS_MATRIX_CSR
    assert np.array_equal(before["ptr"], after["ptr"]) and np.array_equal(before["index"], after["index"]) and sc.same_bits(before["value"], after["value"])
    lib.lis_matrix_destroy(A)


def test_split_and_non_csr_matrices_are_refused_without_a_device(lib, capfd):
    ptr, idx, val = sc.system("p654")
    A = lisdrv.make_csr(lib, ptr, idx, val)
    assert lib.lis_matrix_split(A) == 0
    refused(lib, capfd, A, ptr, idx, val, "-i cg -p sainv", "-p sainv on a split matrix")
    assert A.contents.is_splited
    lib.lis_matrix_destroy(A)
    A = lisdrv.make_csr(lib, ptr, idx, val)
    E = lisdrv.convert(lib, A, "ell")
    before = lisdrv.matrix_arrays(E)
    refused(lib, capfd, E, ptr, idx, val, "-i bicg -p is", "-p is is served for CSR storage only")
    after = lisdrv.matrix_arrays(E)
    assert after["type"] == capi.LIS_MATRIX_ELL and np.array_equal(before["index"], after["index"]) and sc.same_bits(before["value"], after["value"])
    lib.lis_matrix_destroy(E)
    lib.lis_matrix_destroy(A)


def test_hybrid_and_saamg_stay_refused(lib, capfd):
    ptr, idx, val = sc.system("p654")
    A = lisdrv.make_csr(lib, ptr, idx, val)
    for p, number in (("hybrid", 4), ("saamg", 7)):
        b = sc.rhs(ptr, idx, val)
        vb, vx = lisdrv.new_vector(lib, A, b), lisdrv.new_vector(lib, A)
        S = capi.PS()
        assert lib.lis_solver_create(C.byref(S)) == 0 and lib.lis_solver_set_option(("-i cg -p " + p).encode(), S) == 0
        capfd.readouterr()
        assert lib.lis_solve(A, vb, vx, S) == capi.LIS_ERR_NOT_IMPLEMENTED
        text = "".join(capfd.readouterr())
        assert "preconditioner %d is not served" % number in text and "sainv, is" in text
        lib.lis_solver_destroy(S)
        lib.lis_vector_destroy(vb)
        lib.lis_vector_destroy(vx)
    lib.lis_matrix_destroy(A)


def test_kernels_keep_out_of_scratch_memory(tmp_path):
    """sainv.hip compiled to gfx950 assembly with the library's flags (csrc/Makefile, HIPFLAGS): every kernel has a private segment of 0 bytes"""
    import re
    csrc = os.path.join(os.path.dirname(HERE), "lis_amd", "csrc")
    hipcc = os.environ.get("HIPCC") or os.path.join(os.environ.get("ROCM", "/opt/rocm"), "bin", "hipcc")
    asm = str(tmp_path / "sainv.s")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(os.path.dirname(HERE), "include"),
                    "-I" + os.path.join(csrc, "kernels"), "--cuda-device-only", "-S", os.path.join(csrc, "kernels", "sainv.hip"), "-o", asm],
                   check=True, capture_output=True, text=True)
    meta = re.findall(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", open(asm).read())
    sizes = {name: int(size) for name, size in meta}
    assert len([k for k in sizes if "rows_in_order" in k]) == 8 and len(sizes) == 9, sorted(sizes)          # 4 epilogues, chunked or not; the truncation
    assert all(size == 0 for size in sizes.values()), {k: v for k, v in sizes.items() if v}
