"""The eigensolvers of several pairs (-e si | li | ai), the parts that need no GPU: the small dense QR they call (lis_array_qr, lis_array_cgs, lis_array_nrm2,
public as in the reference) against oracle/_ref in every bit, the argument checks of lis_esolve that fire before A or x is touched, and the getters of
several pairs on an esolver that never solved.  The GPU side is tests/test_esolve_multi_gpu.py and tests/test_ritz_tail_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import esolve_drv
import lis_amd
import lisdrv
from lis_amd import _capi as capi

P_DBL, P_INT = capi.P_DBL, capi.P_INT


@pytest.fixture(scope="module")
def lib():
    lib = lis_amd.load()
    assert lib.initialize([]) == 0
    return lib


def _protos(dll):
    dll.lis_array_nrm2.restype, dll.lis_array_nrm2.argtypes = C.c_int, [C.c_int, P_DBL, P_DBL]
    dll.lis_array_cgs.restype, dll.lis_array_cgs.argtypes = C.c_int, [C.c_int, P_DBL, P_DBL, P_DBL]
    dll.lis_array_qr.restype, dll.lis_array_qr.argtypes = C.c_int, [C.c_int, P_DBL, P_DBL, P_DBL, P_INT, P_DBL]
    return dll


def _p(a):
    return a.ctypes.data_as(P_DBL)


# ---------------------------------------------------------------------------------------------- the dense routines
def _matrices():
    """(name, n, column-major n x n): symmetric tridiagonal and upper Hessenberg matrices of sizes 1 .. 6 (what Lanczos and Arnoldi hand to lis_array_qr), one
    whose first subdiagonal entry is already below 1e-12 (one sweep), one rank-deficient (the nrm2 < tol break of lis_array_cgs)."""
    rng = np.random.default_rng(11)
    out = []
    for n in range(1, 7):
        d, o = rng.uniform(1.0, 9.0, n), rng.uniform(0.1, 2.0, max(n - 1, 0))
        out.append(("tridiagonal%d" % n, n, np.diag(d) + np.diag(o, 1) + np.diag(o, -1)))
        out.append(("hessenberg%d" % n, n, np.triu(rng.uniform(-2.0, 2.0, (n, n)), -1) + np.diag(np.arange(n, 0, -1) * 3.0)))
    small = np.triu(rng.uniform(-2.0, 2.0, (4, 4)), -1) + np.diag([9.0, 6.0, 3.0, 1.0])
    small[1, 0] = 3e-13
    out.append(("subdiagonal_below_tol", 4, small))
    deficient = rng.uniform(-1.0, 1.0, (5, 5))
    deficient[:, 2] = 2.0 * deficient[:, 0]            # column 2 is column 0 doubled (exactly): its remainder is 0, classical Gram-Schmidt stops there
    out.append(("rank_deficient", 5, deficient))
    return out


MATRICES = _matrices()


def _flat(m, n, pad):
    a = np.zeros(n * n + pad)
    a[:n * n] = np.asarray(m, np.float64).reshape(n, n).T.reshape(-1)       # column-major
    return a


def _same_bits(a, b, what):
    assert np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64)), what


@pytest.mark.parametrize("name,n,m", MATRICES, ids=[c[0] for c in MATRICES])
def test_dense_qr_cgs_and_nrm2_are_the_reference_in_every_bit(lib, reflib, name, n, m):
    ours, ref = _protos(lib.dll), _protos(reflib.dll)
    results = []
    for dll in (ours, ref):
        # one element of padding behind a: the reference reads a[1] of a 1 x 1 matrix (its stop test); 0.0 there ends both after one sweep
        a = _flat(m, n, 1)
        nrm = C.c_double(-1.0)
        assert dll.lis_array_nrm2(n * n, _p(a), C.byref(nrm)) == 0
        q, r = np.full(n * n, 7.5), np.full(n * n, 7.5)
        a_cgs = a.copy()
        assert dll.lis_array_cgs(n, _p(a_cgs), _p(q), _p(r)) == 0
        q2, r2 = np.full(n * n, 7.5), np.full(n * n, 7.5)
        it, err = C.c_int(-1), C.c_double(-1.0)
        assert dll.lis_array_qr(n, _p(a), _p(q2), _p(r2), C.byref(it), C.byref(err)) == 0
        results.append(dict(nrm2=np.array([nrm.value]), a_after_cgs=a_cgs, q=q, r=r, a=a, q2=q2, r2=r2, iter=it.value, err=np.array([err.value])))
    got, want = results
    assert got["iter"] == want["iter"], (name, got["iter"], want["iter"])
    for k in ("nrm2", "a_after_cgs", "q", "r", "a", "q2", "r2", "err"):
        _same_bits(got[k], want[k], (name, k))
    if name == "subdiagonal_below_tol":
        assert got["iter"] == 1
    if name == "rank_deficient":
        assert np.all(got["q"].reshape(5, 5)[2:] == 0.0) and got["r"][2 + 2 * 5] < 1e-12        # columns 2 .. 4 of Q stay 0: the break


def test_dense_routines_without_the_reference(lib):
    """What holds of them wherever the suite runs: Q R = A with orthonormal Q, and the QR iteration's diagonal are the eigenvalues of a symmetric tridiagonal matrix."""
    dll = _protos(lib.dll)
    n = 5
    m = np.diag([9.0, 7.0, 5.0, 3.0, 1.0]) + np.diag([0.5] * 4, 1) + np.diag([0.5] * 4, -1)
    a = _flat(m, n, 0)
    q, r = np.zeros(n * n), np.zeros(n * n)
    assert dll.lis_array_cgs(n, _p(a), _p(q), _p(r)) == 0
    Q, R = q.reshape(n, n).T, r.reshape(n, n).T
    assert np.allclose(Q @ R, m, atol=1e-13) and np.allclose(Q.T @ Q, np.eye(n), atol=1e-13) and np.allclose(R, np.triu(R))
    it, err = C.c_int(), C.c_double()
    assert dll.lis_array_qr(n, _p(a), _p(q), _p(r), C.byref(it), C.byref(err)) == 0
    assert 1 < it.value < 100000 and err.value < 1e-12
    assert np.allclose(np.sort(a.reshape(n, n).T.diagonal()), np.linalg.eigvalsh(m), atol=1e-9)
    one = np.array([3.0])
    assert dll.lis_array_qr(1, _p(one), _p(q), _p(r), C.byref(it), C.byref(err)) == 0 and (it.value, err.value, one[0]) == (1, 0.0, 3.0)


# ---------------------------------------------------------------------------------------------- argument checks
def _snapshot(lib, A, vx):
    a = lisdrv.matrix_arrays(A)
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in a.items()}, lisdrv.get_vector(lib, vx).copy()


def _same(s1, s2):
    for k in s1[0]:
        assert np.array_equal(s1[0][k], s2[0][k]), k
    assert np.array_equal(s1[1].view(np.int64), s2[1].view(np.int64))


CHECKS = [("-e si -ss 400", capi.LIS_ERR_ILL_ARG), ("-e li -ss 400", capi.LIS_ERR_ILL_ARG), ("-e ai -ss 400", capi.LIS_ERR_ILL_ARG),
          ("-e si -ss 3 -m 3", capi.LIS_ERR_ILL_ARG), ("-e li -ss 3 -m 3", capi.LIS_ERR_ILL_ARG), ("-e ai -ss 3 -m 3", capi.LIS_ERR_ILL_ARG),
          ("-e si -ss 2 -ie rqi", capi.LIS_ERR_NOT_IMPLEMENTED), ("-e si -ss 2 -ie cg", capi.LIS_ERR_NOT_IMPLEMENTED),
          ("-e si -ss 1", capi.LIS_ERR_NOT_IMPLEMENTED), ("-e li -ss 1", capi.LIS_ERR_NOT_IMPLEMENTED), ("-e ai", capi.LIS_ERR_NOT_IMPLEMENTED)]


@pytest.mark.parametrize("text,code", CHECKS)
def test_argument_checks_fire_before_A_or_x_is_touched(lib, text, code, capfd):
    ptr, idx, val = esolve_drv.sym_csr()
    assert len(ptr) - 1 == 343
    A = lisdrv.make_csr(lib, ptr, idx, val)
    vx = lisdrv.new_vector(lib, A, esolve_drv.start_vector(len(ptr) - 1))
    before = _snapshot(lib, A, vx)
    E = capi.PE()
    assert lib.lis_esolver_create(C.byref(E)) == 0
    assert lib.lis_esolver_set_option(text.encode(), E) == 0
    ev = C.c_double(-7.0)
    assert lib.lis_esolve(A, vx, C.byref(ev), E) == code
    assert ev.value == -7.0 and E.contents.retcode == code
    message = capfd.readouterr().out
    if code == capi.LIS_ERR_NOT_IMPLEMENTED:
        assert "not served" in message
    if "-ss 1" in text or text == "-e ai":
        assert "-e pi" in message                           # one pair is what -e pi / -e ii serve, and the message says so
    _same(before, _snapshot(lib, A, vx))
    assert not E.contents.evalue and not E.contents.evector    # nothing was allocated for a refused solve
    lib.lis_esolver_destroy(E)
    lib.lis_vector_destroy(vx)
    lib.lis_matrix_destroy(A)


@pytest.mark.parametrize("e", ["si", "li", "ai"])
def test_getters_of_several_pairs_on_an_esolver_that_never_solved(lib, e, capfd):
    ptr, idx, val = esolve_drv.sym_csr()
    A, M = lisdrv.make_csr(lib, ptr, idx, val), capi.PM()
    assert lib.lis_matrix_create(capi.LIS_COMM_WORLD, C.byref(M)) == 0
    vx = lisdrv.new_vector(lib, A, np.ones(len(ptr) - 1))
    E = capi.PE()
    assert lib.lis_esolver_create(C.byref(E)) == 0
    assert lib.lis_esolver_set_option(("-e %s -ss 3" % e).encode(), E) == 0
    ev, iv = C.c_double(-7.0), C.c_int(-7)
    for call in (lambda: lib.lis_esolver_get_evalues(E, vx), lambda: lib.lis_esolver_get_residualnorms(E, vx), lambda: lib.lis_esolver_get_iters(E, vx),
                 lambda: lib.lis_esolver_get_evectors(E, M), lambda: lib.lis_esolver_get_specific_evalue(E, 0, C.byref(ev)),
                 lambda: lib.lis_esolver_get_specific_evector(E, 0, vx), lambda: lib.lis_esolver_get_specific_residualnorm(E, 0, C.byref(ev)),
                 lambda: lib.lis_esolver_get_specific_iter(E, 0, C.byref(iv))):
        assert call() == capi.LIS_ERR_ILL_ARG
        assert "no eigensolve has filled" in capfd.readouterr().out
    assert (ev.value, iv.value) == (-7.0, -7)
    assert np.array_equal(lisdrv.get_vector(lib, vx), np.ones(len(ptr) - 1)) and M.contents.n == 0
    lib.lis_esolver_destroy(E)
    lib.lis_vector_destroy(vx)
    lib.lis_matrix_destroy(A)
    lib.lis_matrix_destroy(M)


# ---------------------------------------------------------------------------------------------- link check
@pytest.mark.parametrize("driver", ["etest4", "etest5", "etest5b", "etest6"])
def test_the_reference_drivers_of_several_pairs_compile_and_link_against_this_library(tmp_path, driver):
    """The reference's own programs that ask for several eigenpairs (the getters of several pairs, lis_esolver_get_evectors).  Compiles and links only; the
    binaries are not run (they need a GPU)."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join("/root/reference", "test", driver + ".c")
    if not os.path.exists(src):
        pytest.skip("the reference tree is not here")
    exe = tmp_path / (driver + "_amd")
    libdir = os.path.dirname(lis_amd.LIB_PATH)
    done = subprocess.run(["gcc", "-O2", "-w", "-I", os.path.join(root, "include"), src, "-o", str(exe), "-L", libdir, "-llis_amd", "-lm",
                           "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    assert os.path.exists(exe)
