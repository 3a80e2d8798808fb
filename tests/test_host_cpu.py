"""Host-side logic of liblis_amd.so that needs no GPU: ABI, exported symbols, object state machine,
storage-format conversions (bit-exact index work), option parser, error convention, and the loud
failure of every compute entry point when no HIP device exists."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import lis_amd
import lisdrv
import orc
from lis_amd import _capi as capi

HERE = os.path.dirname(os.path.abspath(__file__))

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "lis_ref_golden.npz"))
HAVE_GPU = lis_amd.gpu_available()


@pytest.fixture(scope="module")
def lib():
    lib = lis_amd.load()
    assert lib.initialize([]) == 0
    return lib


# ---------------------------------------------------------------------------------------------- ABI
def _declared_functions(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    names = re.findall(r"\b((?:lis|liship|CHKERR)\w*)\s*\(", txt)
    return sorted({n for n in names if not n.isupper() or n == "CHKERR"} - {"lis_amd_comm_callbacks"})


@pytest.mark.parametrize("header", ["lis.h", "lis_amd.h", "liship.h"])
def test_every_declared_symbol_is_exported(header):
    dll = C.CDLL(lis_amd.LIB_PATH)
    missing = [n for n in _declared_functions(header) if not hasattr(dll, n)]
    assert not missing, missing


LAYOUT_PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "lis.h"
#define F(S, f) printf(#S "." #f " %zu\n", offsetof(struct S, f))
int main(void) {
  printf("sizeof.vector %zu\nsizeof.matrix %zu\nsizeof.solver %zu\nsizeof.precon %zu\nsizeof.commtable %zu\n",
    sizeof(struct LIS_VECTOR_STRUCT), sizeof(struct LIS_MATRIX_STRUCT), sizeof(struct LIS_SOLVER_STRUCT),
    sizeof(struct LIS_PRECON_STRUCT), sizeof(struct LIS_COMMTABLE_STRUCT));
  F(LIS_VECTOR_STRUCT, n); F(LIS_VECTOR_STRUCT, np); F(LIS_VECTOR_STRUCT, ranges); F(LIS_VECTOR_STRUCT, value); F(LIS_VECTOR_STRUCT, intvalue);
  F(LIS_MATRIX_STRUCT, n); F(LIS_MATRIX_STRUCT, matrix_type); F(LIS_MATRIX_STRUCT, nnz); F(LIS_MATRIX_STRUCT, maxnzr);
  F(LIS_MATRIX_STRUCT, ptr); F(LIS_MATRIX_STRUCT, row); F(LIS_MATRIX_STRUCT, index); F(LIS_MATRIX_STRUCT, bptr);
  F(LIS_MATRIX_STRUCT, value); F(LIS_MATRIX_STRUCT, work); F(LIS_MATRIX_STRUCT, L); F(LIS_MATRIX_STRUCT, is_block);
  F(LIS_MATRIX_STRUCT, conv_bnr); F(LIS_MATRIX_STRUCT, options); F(LIS_MATRIX_STRUCT, w_annz); F(LIS_MATRIX_STRUCT, l2g_map);
  F(LIS_MATRIX_STRUCT, commtable);
  F(LIS_SOLVER_STRUCT, rhistory); F(LIS_SOLVER_STRUCT, options); F(LIS_SOLVER_STRUCT, params); F(LIS_SOLVER_STRUCT, retcode);
  F(LIS_SOLVER_STRUCT, iter); F(LIS_SOLVER_STRUCT, resid); F(LIS_SOLVER_STRUCT, time); F(LIS_SOLVER_STRUCT, bnrm); F(LIS_SOLVER_STRUCT, setup);
  F(LIS_PRECON_STRUCT, D); F(LIS_PRECON_STRUCT, commtable);
  F(LIS_COMMTABLE_STRUCT, neibpe); F(LIS_COMMTABLE_STRUCT, export_index); F(LIS_COMMTABLE_STRUCT, wr);
  printf("const %d %d %d %d %d %d\n", LIS_MATRIX_DECIDING_SIZE, LIS_MATRIX_NULL, LIS_OPTIONS_LEN, LIS_PARAMS_RESID, LIS_ERR_NOT_IMPLEMENTED, LIS_MATRIX_BSR);
  return 0;
}
"""


def _probe(include_dir, tmp_path, tag):
    src = tmp_path / f"probe_{tag}.c"
    src.write_text(LAYOUT_PROBE)
    exe = tmp_path / f"probe_{tag}"
    subprocess.run(["gcc", "-I", include_dir, str(src), "-o", str(exe)], check=True)
    return subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout


def test_struct_layout_is_the_reference_abi(tmp_path):
    ours = _probe(os.path.join(ROOT, "include"), tmp_path, "ours")
    golden = open(os.path.join(ROOT, "tests", "golden", "lis_abi_layout.txt")).read()
    assert ours == golden                                     # produced from the reference header (see below)
    ref_inc = "/root/reference/include"
    if os.path.exists(os.path.join(ref_inc, "lis.h")):        # dev container: re-derive from the reference itself
        assert _probe(ref_inc, tmp_path, "ref") == ours


def test_ctypes_mirror_matches_c_layout(tmp_path):
    ours = dict(line.rsplit(" ", 1) for line in _probe(os.path.join(ROOT, "include"), tmp_path, "o2").splitlines()
                if not line.startswith("const"))
    assert C.sizeof(capi.Vector) == int(ours["sizeof.vector"])
    assert C.sizeof(capi.Matrix) == int(ours["sizeof.matrix"])
    assert C.sizeof(capi.Solver) == int(ours["sizeof.solver"])
    assert capi.Matrix.commtable.offset == int(ours["LIS_MATRIX_STRUCT.commtable"])
    assert capi.Solver.resid.offset == int(ours["LIS_SOLVER_STRUCT.resid"])


# ---------------------------------------------------------------------------------------------- state machine
def test_matrix_state_machine_and_errors(lib):
    A = capi.PM()
    assert lib.lis_matrix_create(capi.LIS_COMM_WORLD, C.byref(A)) == 0
    a = A.contents
    assert (a.status, a.matrix_type, a.is_destroy, a.conv_bnr, a.label) == (-256, 1, 1, 2, 1)
    assert lib.lis_matrix_set_size(A, 5, 3) == capi.LIS_ERR_ILL_ARG           # local > global
    assert lib.lis_matrix_set_size(A, -1, 0) == capi.LIS_ERR_ILL_ARG
    assert lib.lis_matrix_set_size(A, 0, 0) == capi.LIS_ERR_ILL_ARG
    assert lib.lis_matrix_assemble(A) == capi.LIS_ERR_ILL_ARG                  # size undefined
    assert lib.lis_matrix_set_size(A, 0, 4) == 0
    assert (a.status, a.n, a.gn, a.np, a.is_, a.ie) == (-257, 4, 4, 4, 0, 4)
    assert lib.lis_matrix_assemble(A) == capi.LIS_ERR_ILL_ARG                  # type undefined
    assert lib.lis_matrix_set_type(A, 99) == capi.LIS_ERR_ILL_ARG
    ptr, idx, val = orc.poisson1d(4)
    p, i, v = capi.P_INT(), capi.P_INT(), capi.P_DBL()
    assert lib.lis_matrix_malloc_csr(4, len(idx), C.byref(p), C.byref(i), C.byref(v)) == 0
    C.memmove(p, ptr.ctypes.data, ptr.nbytes); C.memmove(i, idx.ctypes.data, idx.nbytes); C.memmove(v, val.ctypes.data, val.nbytes)
    assert lib.lis_matrix_set_csr(len(idx), p, i, v, A) == 0
    assert (a.status, a.nnz, a.is_copy) == (-1, len(idx), 0)
    # quirk of the reference: set_<fmt> on a matrix that is not in state NULL succeeds without adopting
    assert lib.lis_matrix_set_csr(1, None, None, None, A) == 0 and a.nnz == len(idx)
    assert lib.lis_matrix_assemble(A) == 0
    assert (a.status, a.matrix_type) == (1, 1)
    assert lib.lis_matrix_set_type(A, capi.LIS_MATRIX_ELL) == capi.LIS_ERR_ILL_ARG   # already assembled
    n, gn, nnz, t = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    assert lib.lis_matrix_get_size(A, C.byref(n), C.byref(gn)) == 0 and (n.value, gn.value) == (4, 4)
    assert lib.lis_matrix_get_nnz(A, C.byref(nnz)) == 0 and nnz.value == len(idx)
    assert lib.lis_matrix_get_type(A, C.byref(t)) == 0 and t.value == 1
    v1 = capi.PV()
    assert lib.lis_vector_duplicate(C.cast(A, C.c_void_p), C.byref(v1)) == 0
    vc = v1.contents
    assert (vc.label, vc.status, vc.n, vc.np, vc.gn) == (0, 1, 4, 4, 4)
    assert lib.lis_vector_set_value(capi.LIS_INS_VALUE, 7, 1.0, v1) == capi.LIS_ERR_ILL_ARG
    assert lib.lis_vector_set_value(capi.LIS_INS_VALUE, 2, 1.5, v1) == 0
    assert lib.lis_vector_set_value(capi.LIS_ADD_VALUE, 2, 1.0, v1) == 0
    out = C.c_double()
    assert lib.lis_vector_get_value(v1, 2, C.byref(out)) == 0 and out.value == 2.5
    assert vc.value[2] == 2.5
    buf = (C.c_double * 4)()
    assert lib.lis_vector_get_values(v1, 1, 4, buf) == capi.LIS_ERR_ILL_ARG     # runs past the end
    assert lib.lis_vector_get_values(v1, 1, 3, buf) == 0 and list(buf)[:3] == [0.0, 2.5, 0.0]
    assert lib.lis_matrix_destroy(A) == 0 and lib.lis_vector_destroy(v1) == 0
    assert lib.lis_matrix_destroy(A) == 0                                       # destroying twice is harmless


def test_set_value_assembly(lib):
    """lis_matrix_set_value -> assemble (test/test4.c): rows in insertion order, duplicates combined."""
    A = capi.PM()
    lib.lis_matrix_create(capi.LIS_COMM_WORLD, C.byref(A))
    lib.lis_matrix_set_size(A, 0, 6)
    for i in range(6):
        if i > 0:
            lib.lis_matrix_set_value(capi.LIS_INS_VALUE, i, i - 1, -1.0, A)
        if i < 5:
            lib.lis_matrix_set_value(capi.LIS_INS_VALUE, i, i + 1, -1.0, A)
        lib.lis_matrix_set_value(capi.LIS_INS_VALUE, i, i, 1.0, A)
        lib.lis_matrix_set_value(capi.LIS_ADD_VALUE, i, i, 1.0, A)
    assert A.contents.status == 0
    assert lib.lis_matrix_assemble(A) == 0
    arrs = lisdrv.matrix_arrays(A)
    ptr, idx, val = orc.poisson1d(6)
    assert np.array_equal(arrs["ptr"], ptr) and np.array_equal(arrs["index"], idx) and np.array_equal(arrs["value"], val)
    lib.lis_matrix_destroy(A)


# ---------------------------------------------------------------------------------------------- conversions
def _check_arrays(fmt, got, want):
    keys = {"csc": ["ptr", "index", "value"], "ell": ["maxnzr", "index", "value"], "dia": ["nnd", "index", "value"],
            "jad": ["maxnzr", "row", "ptr", "index", "value"], "bsr": ["nr", "nc", "bnnz", "pad", "bptr", "bindex", "value"]}[fmt]
    for k in keys:
        w = want[k]
        g = got[k]
        assert np.array_equal(np.atleast_1d(g), np.atleast_1d(w)), (fmt, k)


@pytest.mark.parametrize("name", ["p1d100", "p3d_6x5x4", "p3d_8s", "irr150"])
@pytest.mark.parametrize("fmt", ["csc", "ell", "dia", "jad", "bsr"])
def test_convert_against_golden(lib, name, fmt):
    """lis_matrix_convert produces the arrays the reference produced (tests/golden), bit for bit."""
    ptr, idx, val = (G[f"{name}/{k}"] for k in ("ptr", "idx", "val"))
    A = lisdrv.make_csr(lib, ptr, idx, val)
    B = lisdrv.convert(lib, A, fmt)
    got = lisdrv.matrix_arrays(B)
    want = {k.split("/")[-1]: G[k] for k in G.files if k.startswith(f"{name}/{fmt}/")}
    _check_arrays(fmt, got, want)
    assert B.contents.status == capi.FORMAT_ID[fmt] and B.contents.matrix_type == capi.FORMAT_ID[fmt]
    lib.lis_matrix_destroy(A); lib.lis_matrix_destroy(B)


CASES = {"rand257": lambda: orc.random_csr(257, 9, seed=1), "rand_long": lambda: orc.random_csr(64, 5, seed=2, long_row=60),
         "p3d_7x6x5": lambda: orc.poisson3d(7, 6, 5), "p3d_9_sorted": lambda: orc.poisson3d(9, 9, 9, sort_cols=True)}


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("fmt,bs", [("csc", 0), ("ell", 0), ("dia", 0), ("jad", 0), ("bsr", 2), ("bsr", 3)])
def test_convert_against_reference(lib, reflib, case, fmt, bs):
    ptr, idx, val = CASES[case]()
    out = []
    for L in (lib, reflib):
        A = lisdrv.make_csr(L, ptr, idx, val)
        B = lisdrv.convert(L, A, fmt, bs or 2, bs or 2)
        out.append(lisdrv.matrix_arrays(B))
        L.lis_matrix_destroy(A); L.lis_matrix_destroy(B)
    _check_arrays(fmt, out[0], out[1])


@pytest.mark.parametrize("fmt", ["csc", "ell", "dia", "jad", "bsr"])
def test_round_trip_to_csr(lib, fmt):
    """X -> CSR gives back the matrix (entries by ascending column, explicit zeros of ELL/DIA/BSR dropped)."""
    ptr, idx, val = orc.random_csr(120, 6, seed=5, sort_cols=True)
    A = lisdrv.make_csr(lib, ptr, idx, val)
    B = lisdrv.convert(lib, A, fmt)
    Cm = lisdrv.convert(lib, B, "csr")
    got = lisdrv.matrix_arrays(Cm)
    x = np.random.default_rng(0).uniform(-1, 1, 120)
    sidx, sval = orc.sort_rows(got["ptr"], got["index"], got["value"])
    assert np.array_equal(got["ptr"], ptr) and np.array_equal(sidx, idx) and np.array_equal(sval, val)
    assert np.array_equal(orc.spmv_csr(got["ptr"], sidx, sval, x), orc.spmv_csr(ptr, idx, val, x))
    for M in (A, B, Cm):
        lib.lis_matrix_destroy(M)


def test_diagonal_host_formats(lib):
    if HAVE_GPU:
        pytest.skip("covered on the device path by the gpu tests")
    ptr, idx, val = orc.random_csr(90, 7, seed=6)
    d = orc.csr_diagonal(ptr, idx, val)
    A = lisdrv.make_csr(lib, ptr, idx, val)
    for fmt in ("csr", "csc", "ell", "jad", "bsr"):
        B = A if fmt == "csr" else lisdrv.convert(lib, A, fmt)
        v = lisdrv.new_vector(lib, B)
        assert lib.lis_matrix_get_diagonal(B, v) == 0
        assert np.array_equal(np.ctypeslib.as_array(v.contents.value, shape=(90,)), d), fmt
        lib.lis_vector_destroy(v)


# ---------------------------------------------------------------------------------------------- solver object
def test_solver_defaults_and_options(lib):
    S = capi.PS()
    assert lib.lis_solver_create(C.byref(S)) == 0
    s = S.contents
    assert (s.options[0], s.options[1], s.options[2], s.options[4], s.options[15]) == (2, 0, 1000, 40, 1)   # BiCG, none, 1000, 40, zeros
    assert s.params[0] == 1e-12
    assert lib.lis_solver_set_option(b"-i cg -p jacobi -tol 1.0e-10 -maxiter 77 -print mem -restart 30 -storage ell -initx_zeros false", S) == 0
    assert (s.options[0], s.options[1], s.options[2], s.options[3], s.options[4], s.options[22], s.options[15]) == (1, 1, 77, 1, 30, 5, 0)
    assert s.params[0] == 1e-10
    assert lib.lis_solver_set_option(b"-i 9 -p 0 -conv_cond nrm1_b", S) == 0 and (s.options[0], s.options[1], s.options[24]) == (9, 0, 2)
    assert lib.lis_solver_set_option(b"-i nosuchsolver", S) == capi.LIS_ERR_ILL_ARG
    name = C.create_string_buffer(64)
    assert lib.lis_solver_get_solvername(4, name) == 0 and name.value == b"BiCGSTAB"
    assert lib.lis_solver_get_preconname(1, name) == 0 and name.value == b"Jacobi"
    assert lib.lis_solver_destroy(S) == 0


def test_unserved_paths_say_so(lib):
    ptr, idx, val = orc.poisson1d(10)
    A = lisdrv.make_csr(lib, ptr, idx, val)
    b, x = lisdrv.new_vector(lib, A, np.ones(10)), lisdrv.new_vector(lib, A)
    for opts, code in ((b"-i bicg", 5), (b"-i cg -p ilu", 5), (b"-i cg -f quad", 1), (b"-i cg -maxiter -3", 1)):
        S = capi.PS()
        lib.lis_solver_create(C.byref(S))
        assert lib.lis_solver_set_option(opts, S) == 0
        assert lib.lis_solve(A, b, x, S) == code, opts
        lib.lis_solver_destroy(S)
    B = capi.PM()
    lib.lis_matrix_duplicate(A, C.byref(B))
    lib.lis_matrix_set_type(B, 3)                                   # MSR: in the enum, not served
    assert lib.lis_matrix_convert(A, B) == capi.LIS_ERR_NOT_IMPLEMENTED


@pytest.mark.skipif(HAVE_GPU, reason="needs a box WITHOUT a GPU")
def test_compute_fails_loudly_without_gpu(lib, capfd):
    """No CPU fallback: every compute entry point reports an error instead of silently computing on the host."""
    ptr, idx, val = orc.poisson1d(10)
    A = lisdrv.make_csr(lib, ptr, idx, val)
    x, y = lisdrv.new_vector(lib, A, np.ones(10)), lisdrv.new_vector(lib, A)
    out = C.c_double()
    assert lib.lis_matvec(A, x, y) != 0
    assert lib.lis_vector_dot(x, y, C.byref(out)) != 0
    assert lib.lis_vector_axpy(1.0, x, y) != 0
    S = capi.PS()
    lib.lis_solver_create(C.byref(S))
    lib.lis_solver_set_option(b"-i cg", S)
    assert lib.lis_solve(A, x, y, S) != 0
    assert "no CPU fallback" in capfd.readouterr().err


# ------------------------------------------------------------------ -scale: host arithmetic, no GPU
GS = np.load(os.path.join(ROOT, "tests", "golden", "scale_golden.npz"))


@pytest.mark.parametrize("action", [1, 2])
@pytest.mark.parametrize("fmt", ["csr", "csc", "ell", "dia", "jad", "bsr"])
def test_matrix_scale_matches_reference_bits(lib, fmt, action):
    """lis_matrix_scale: scaled values, b and d are the reference's bits, including its per-format association
    of the two symmetric factors (lis_matrix_csr.c:687 vs lis_matrix_ell.c:821)."""
    ptr, idx, val, b = (GS[k] for k in ("ptr", "idx", "val", "b"))
    n = len(ptr) - 1
    A = lisdrv.make_csr(lib, ptr, idx, val)
    B = A if fmt == "csr" else lisdrv.convert(lib, A, fmt)
    vb, vd = lisdrv.new_vector(lib, B, b), lisdrv.new_vector(lib, B)
    assert lib.lis_matrix_scale(B, vb, vd, action) == 0
    assert B.contents.is_scaled == 1 and vb.contents.is_scaled == 1
    assert np.array_equal(lisdrv.matrix_arrays(B)["value"], GS[f"scale{action}/{fmt}/value"])
    assert np.array_equal(np.ctypeslib.as_array(vb.contents.value, shape=(n,)), GS[f"scale{action}/{fmt}/b"])
    assert np.array_equal(np.ctypeslib.as_array(vd.contents.value, shape=(n,)), GS[f"scale{action}/{fmt}/d"])


def test_set_values_block_and_row_hints(lib):
    """lis_matrix_malloc (capacity hint) + lis_matrix_set_values (dense row-major block) -> the CSR the same
    lis_matrix_set_value calls give (reference lis_matrix.c:592-625, :808-822)."""
    n = 4
    dense = np.arange(1.0, n * n + 1).reshape(n, n)
    A = capi.PM()
    assert lib.lis_matrix_create(0, C.byref(A)) == 0 and lib.lis_matrix_set_size(A, 0, n) == 0
    assert lib.lis_matrix_malloc(A, 4, None) == 0
    assert lib.lis_matrix_set_values(capi.LIS_INS_VALUE, n, dense.ravel().ctypes.data_as(capi.P_DBL), A) == 0
    assert lib.lis_matrix_set_type(A, capi.LIS_MATRIX_CSR) == 0 and lib.lis_matrix_assemble(A) == 0
    arrs = lisdrv.matrix_arrays(A)
    assert np.array_equal(arrs["ptr"], np.arange(0, n * n + 1, n))
    assert np.array_equal(arrs["index"], np.tile(np.arange(n), n)) and np.array_equal(arrs["value"], dense.ravel())
    lib.lis_matrix_destroy(A)


def test_handle_registry_follows_the_live_count(lib):
    """a long create / destroy history (every lis_solve registers a preconditioner) must not grow the handle table"""
    dll = lib.dll
    dll.lisi_registry_slots.restype = C.c_size_t
    keep = []
    for _ in range(100):
        v = capi.PV()
        assert lib.lis_vector_create(0, C.byref(v)) == 0
        keep.append(v)
    before = dll.lisi_registry_slots()
    for _ in range(20000):
        v = capi.PV()
        assert lib.lis_vector_create(0, C.byref(v)) == 0
        assert lib.lis_vector_set_size(v, 4, 0) == 0
        assert lib.lis_vector_destroy(v) == 0
    assert dll.lisi_registry_slots() <= max(before, 1024)
    for v in keep:                                       # the survivors are still known
        assert lib.lis_vector_set_size(v, 3, 0) == 0
        assert lib.lis_vector_destroy(v) == 0


# ---------------------------------------------------------------- coherent semantics by page protection (lis_pages.c), no GPU needed
def _vec(lib, n):
    v = capi.PV()
    assert lib.lis_vector_create(capi.LIS_COMM_WORLD, C.byref(v)) == 0 and lib.lis_vector_set_size(v, n, 0) == 0
    return v


def test_vector_pages_follow_the_flags_through_faults(lib):
    """value[] lives on pages of its own: without access while the HBM copy is newer (any host access faults and the handler brings the
    vector home), read-only while both sides agree (a host write faults once and marks the HBM copy stale), plain memory otherwise.
    Driven here without a GPU: with no HBM buffer the `bring home` step has nothing to copy, the protection and bookkeeping are the same."""
    dll = lib.dll
    for f in (dll.lis_amd_vector_page_state, dll.lis_amd_vector_device_modified, dll.lis_amd_vector_sync_host):
        f.argtypes = [capi.PV]
    dll.lis_amd_vector_page_protect.argtypes = [capi.PV, C.c_int]
    dll.lis_amd_page_faults.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int)]

    def faults():
        r, w = C.c_int(), C.c_int()
        dll.lis_amd_page_faults(C.byref(r), C.byref(w))
        return r.value, w.value
    n = 5000                                    # ten pages
    v = _vec(lib, n)
    val = np.ctypeslib.as_array(v.contents.value, shape=(n,))
    assert dll.lis_amd_vector_page_state(v) == 0 and not val.any()      # fresh pages: zero, writable
    val[:] = np.arange(n)                       # a program poking value[] directly: plain memory, no fault
    r0, w0 = faults()
    assert dll.lis_amd_vector_device_modified(v) == 0                   # "a kernel wrote v": the pages lose all access
    assert dll.lis_amd_vector_page_state(v) == 2
    assert val[4321] == 4321.0                  # the read faults; the handler restores access (and would copy HBM -> host)
    assert faults() == (r0 + 1, w0) and dll.lis_amd_vector_page_state(v) in (0, 1)
    assert dll.lis_amd_vector_page_protect(v, 1) == 0                   # both sides agree: read-only
    assert val[17] == 17.0 and faults() == (r0 + 1, w0)                 # reads are free
    val[17] = -1.0                              # the write faults once: pages writable again, HBM copy stale
    assert faults() == (r0 + 1, w0 + 1) and dll.lis_amd_vector_page_state(v) == 0 and val[17] == -1.0
    val[18] = -2.0
    assert faults() == (r0 + 1, w0 + 1)
    # the API's own writers and readers never fault: they unprotect first
    assert dll.lis_amd_vector_page_protect(v, 1) == 0
    assert lib.lis_vector_set_value(capi.LIS_INS_VALUE, 3, 9.5, v) == 0 and val[3] == 9.5 and dll.lis_amd_vector_page_state(v) == 0
    assert dll.lis_amd_vector_device_modified(v) == 0 and dll.lis_amd_vector_page_state(v) == 2
    out = C.c_double()
    assert lib.lis_vector_get_value(v, 3, C.byref(out)) == 0 and out.value == 9.5
    assert faults() == (r0 + 1, w0 + 1)
    # eager coherence: protection is never raised
    dll.lis_amd_set_coherence(0)
    try:
        w = _vec(lib, 100)
        assert dll.lis_amd_vector_device_modified(w) == 0 and dll.lis_amd_vector_page_state(w) == 0
        lib.lis_vector_destroy(w)
    finally:
        dll.lis_amd_set_coherence(1)
    assert lib.lis_vector_destroy(v) == 0       # (unmaps the pages, whatever their protection)
    # a duplicate sized by a matrix header (np + pad entries) gets its own pages too
    v = _vec(lib, 7)
    d = capi.PV()
    assert lib.lis_vector_duplicate(C.cast(v, C.c_void_p), C.byref(d)) == 0 and dll.lis_amd_vector_page_state(d) == 0
    lib.lis_vector_destroy(d); lib.lis_vector_destroy(v)


def test_matrix_arrays_from_lis_matrix_malloc_are_watched_for_host_writes(lib):
    """lis_matrix_malloc_csr (ref lis_matrix_csr.c:170) hands out pages of the library's own: plain memory until the adopting matrix's HBM copy is built, read-only
    from then on; reads stay free, the first host write to an array opens it and marks the copy stale (the reference reads adopted arrays live on every product,
    lis_matvec_csr.c:97-109).  Driven here without a GPU through lis_amd_matrix_page_test_watch, which protects exactly as an upload does.  Arrays the caller
    malloc'ed cannot be watched; lis_free / lis_matrix_destroy / lis_matrix_unset take the pages back in whatever state they are."""
    dll = lib.dll
    for f in (dll.lis_amd_matrix_page_test_watch, dll.lis_amd_matrix_protected_arrays, dll.lis_amd_matrix_host_written):
        f.argtypes = [capi.PM]
    dll.lis_amd_page_faults.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int)]

    def faults():
        r, w = C.c_int(), C.c_int()
        dll.lis_amd_page_faults(C.byref(r), C.byref(w))
        return r.value, w.value
    ptr, idx, val = orc.poisson3d(12, 10, 8)
    A = lisdrv.make_csr(lib, ptr, idx, val)                      # lis_matrix_malloc_csr + set_csr + assemble
    nnz = len(idx)
    hv = np.ctypeslib.as_array(A.contents.value, shape=(nnz,))
    hi = np.ctypeslib.as_array(A.contents.index, shape=(nnz,))
    hv[3] = 2.5                                                  # before any HBM copy: plain memory
    f0 = faults()
    assert faults() == f0 and dll.lis_amd_matrix_protected_arrays(A) == 0
    assert dll.lis_amd_matrix_page_test_watch(A) == 3 and dll.lis_amd_matrix_protected_arrays(A) == 3
    assert hv[3] == 2.5 and int(hi[5]) == int(idx[5]) and faults() == f0 and dll.lis_amd_matrix_host_written(A) == 0      # reads are free
    hv[7] = -4.0                                                 # the write faults once ...
    assert faults() == (f0[0], f0[1] + 1) and hv[7] == -4.0
    assert dll.lis_amd_matrix_host_written(A) == 1 and dll.lis_amd_matrix_protected_arrays(A) == 2      # ... value[] is open, ptr[] / index[] still watched
    hv[8] = -5.0
    assert faults() == (f0[0], f0[1] + 1)
    hi[0] = int(idx[0])                                          # an index write is seen too
    assert faults() == (f0[0], f0[1] + 2) and dll.lis_amd_matrix_protected_arrays(A) == 1
    assert dll.lis_amd_matrix_page_test_watch(A) == 3 and dll.lis_amd_matrix_host_written(A) == 0         # "uploaded again"
    assert lib.lis_matrix_destroy(A) == 0                        # unmaps protected pages without a fault
    assert faults() == (f0[0], f0[1] + 2)
    # arrays that never reach a matrix go back through lis_free; lis_matrix_unset hands watched arrays back to the program as plain memory
    p, i, v = capi.P_INT(), capi.P_INT(), capi.P_DBL()
    assert lib.lis_matrix_malloc_csr(10, 30, C.byref(p), C.byref(i), C.byref(v)) == 0
    v[29] = 1.0
    dll.lis_free.argtypes = [C.c_void_p]
    dll.lis_free.restype = None
    for a in (p, i, v):
        dll.lis_free(C.cast(a, C.c_void_p))
    A = lisdrv.make_csr(lib, ptr, idx, val)
    keep = [C.cast(a, C.c_void_p).value for a in (A.contents.ptr, A.contents.index, A.contents.value)]      # (addresses: the struct's fields are cleared by unset)
    assert dll.lis_amd_matrix_page_test_watch(A) == 3
    dll.lis_matrix_unset.argtypes = [capi.PM]
    assert dll.lis_matrix_unset(A) == 0 and dll.lis_amd_matrix_protected_arrays(A) == 0
    f1 = faults()
    kv = C.cast(keep[2], capi.P_DBL)
    kv[0] = 9.0                                                  # the program's again: no fault, nobody's matrix
    assert faults() == f1 and kv[0] == 9.0
    assert lib.lis_matrix_destroy(A) == 0
    for a in keep:
        dll.lis_free(a)
    # eager coherence never protects
    dll.lis_amd_set_coherence(0)
    try:
        A = lisdrv.make_csr(lib, ptr, idx, val)
        assert dll.lis_amd_matrix_page_test_watch(A) == 0 and dll.lis_amd_matrix_protected_arrays(A) == 0
        lib.lis_matrix_destroy(A)
    finally:
        dll.lis_amd_set_coherence(1)


def test_a_handler_the_program_installs_later_is_noticed():
    """lazy coherence lives on the SIGSEGV disposition: when the program replaces it, the library's next check opens every protected page for good, declares the
    HBM copies stale and goes on in eager coherence -- with a line on stderr -- instead of leaving pages whose faults nobody serves"""
    import subprocess
    import sys
    code = ("import sys, signal, ctypes as C; sys.path[:0] = [%r, %r]\n"
            "import numpy as np, lis_amd; from lis_amd import _capi as capi\n"
            "lib = lis_amd.load(); assert lib.initialize([]) == 0; dll = lib.dll\n"
            "v = capi.PV(); lib.lis_vector_create(0, C.byref(v)); lib.lis_vector_set_size(v, 5000, 0)\n"
            "dll.lis_amd_vector_page_protect.argtypes = [capi.PV, C.c_int]; dll.lis_amd_vector_page_state.argtypes = [capi.PV]\n"
            "val = np.ctypeslib.as_array(v.contents.value, shape=(5000,)); val[:] = 3.0\n"
            "assert dll.lis_amd_vector_page_protect(v, 1) == 0 and dll.lis_amd_vector_page_state(v) == 1\n"
            "assert dll.lis_amd_check_fault_handler() == 1\n"
            "signal.signal(signal.SIGSEGV, lambda *a: None)        # the program's own handler\n"
            "assert dll.lis_amd_check_fault_handler() == 0\n"
            "assert dll.lis_amd_vector_page_state(v) == 0          # opened for good\n"
            "val[7] = 9.0; assert val[7] == 9.0 and val[8] == 3.0  # plain memory: nobody needs to serve a fault\n"
            "w = capi.PV(); lib.lis_vector_create(0, C.byref(w)); lib.lis_vector_set_size(w, 100, 0)\n"
            "assert dll.lis_amd_vector_page_protect(w, 1) != 0 and dll.lis_amd_vector_page_state(w) == 0      # eager from here on: protection is never raised\n"
            "print('ok', flush=True)\n") % (ROOT, os.path.join(ROOT, "tests"))
    p = subprocess.run([sys.executable, "-X", "faulthandler=0", "-c", code], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "ok" in p.stdout, (p.returncode, p.stdout, p.stderr[-800:])
    assert "lazy coherence on: a SIGSEGV handler" in p.stderr and "was replaced by the program" in p.stderr


def test_foreign_segfaults_still_kill_the_process():
    """the handler only answers for vector pages: any other bad access goes to the previous disposition (here: the default, death by SIGSEGV)"""
    import subprocess
    import sys
    code = ("import sys, ctypes as C; sys.path[:0] = [%r, %r]\n"
            "import lis_amd; from lis_amd import _capi as capi\n"
            "lib = lis_amd.load(); assert lib.initialize([]) == 0\n"
            "v = capi.PV(); lib.lis_vector_create(0, C.byref(v)); lib.lis_vector_set_size(v, 100, 0)\n"
            "lib.dll.lis_amd_vector_page_protect.argtypes = [capi.PV, C.c_int]\n"
            "assert lib.dll.lis_amd_vector_page_protect(v, 2) == 0\n"
            "assert v.contents.value[5] == 0.0          # ours: served\n"
            "print('served', flush=True)\n"
            "C.string_at(8)                              # not ours\n"
            "print('survived', flush=True)\n") % (ROOT, os.path.join(ROOT, "tests"))
    p = subprocess.run([sys.executable, "-X", "faulthandler=0", "-c", code], capture_output=True, text=True, timeout=120)
    assert "served" in p.stdout and "survived" not in p.stdout and p.returncode == -11, (p.returncode, p.stdout, p.stderr[-500:])


# ---------------------------------------------------------------- several threads of the program on one protected vector (tests/c/pages_threads.c)
def build_pages_driver(tmp_path):
    """gcc -fopenmp tests/c/pages_threads.c against include/ and liblis_amd.so (a C program: Python threads would serialise on the GIL)"""
    import subprocess
    root = os.path.dirname(HERE)
    exe = str(tmp_path / "pages_threads")
    libdir = os.path.join(root, "lis_amd", "lib")
    subprocess.run(["gcc", "-O1", "-fopenmp", "-Wall", "-I" + os.path.join(root, "include"), os.path.join(HERE, "c", "pages_threads.c"), "-o", exe,
                    "-L" + libdir, "-llis_amd", "-lm", "-Wl,-rpath," + libdir], check=True)
    return exe


@pytest.mark.parametrize("mode", [("cpu-readers", "8", "4"), ("cpu-readers", "2", "6"), ("cpu-writers", "2"), ("cpu-writers", "8"), ("cpu-fwrite",)])
def test_threads_of_the_program_never_see_a_half_filled_vector(tmp_path, mode):
    """lis_pages.c fills a vector coming home through a second mapping of its pages and opens the program's mapping only when the data is
    complete: T threads that read (or write) disjoint slices of v->value at once -- an OpenMP loop after lis_solve -- all see the data; the
    first fault copies, the others wait.  Several rounds on the same vector with the same thread -> slice mapping: repeated faults at the
    same addresses must neither be mistaken for foreign ones nor remove the handler.  A host buffer plays the HBM copy, copied in two halves
    150 ms apart (lis_amd_vector_page_test_source), so a thread that got through early WOULD read stale entries.  cpu-fwrite pins what page
    protection cannot do (write(2) of a protected buffer: EFAULT) and the documented ways round it."""
    import subprocess
    exe = build_pages_driver(tmp_path)
    out = subprocess.run([exe, *mode], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("ok"), (out.stdout, out.stderr[-2000:])
    if mode[0] == "cpu-readers":
        T, R = int(mode[1]), int(mode[2])
        assert f"read_faults={R} " in out.stdout and f"write_faults=0 " in out.stdout       # one copy per round, whatever the thread count
        waits = int(out.stdout.split("waits=")[1])
        assert 1 <= waits <= (T - 1) * R          # the other threads found the copy in flight and waited (not all of them need to)


def test_second_set_size_releases_the_first_pages(lib):
    """lis_vector_set_size twice (the reference leaks the first array): the first pages leave the fault registry and are unmapped"""
    v = capi.PV()
    assert lib.lis_vector_create(0, C.byref(v)) == 0
    assert lib.lis_vector_set_size(v, 3000, 0) == 0
    first = C.addressof(v.contents.value.contents)
    assert lib.lis_vector_set_size(v, 7000, 0) == 0
    assert v.contents.n == 7000
    val = np.ctypeslib.as_array(v.contents.value, shape=(7000,))
    assert not val.any()
    val[:] = 1.0
    lib.dll.lis_amd_vector_page_state.argtypes = [capi.PV]
    assert lib.dll.lis_amd_vector_page_state(v) == 0
    maps = open("/proc/self/maps").read()
    assert ("%x-" % first) not in maps            # the first mapping is gone
    assert lib.lis_vector_destroy(v) == 0


def test_plain_malloc_arrays_can_be_freed_by_the_program():
    """lis_matrix_malloc_<fmt> hands out pages of the library's own (write-watched once uploaded; lis_free releases them, free() would crash).  With
    LIS_AMD_PLAIN_MALLOC=1 / lis_amd_set_matrix_pages(0) it hands out malloc memory like the reference's lis_malloc: free() takes it, lis_free() too.  In a child:
    a wrong free() aborts the process."""
    import subprocess
    code = ("import sys, ctypes as C; sys.path[:0] = [%r, %r]\n"
            "import lis_amd; from lis_amd import _capi as capi\n"
            "lib = lis_amd.load(); assert lib.initialize([]) == 0; dll = lib.dll\n"
            "libc = C.CDLL(None); libc.free.argtypes = [C.c_void_p]\n"
            "dll.lis_amd_matrix_page_test_watch.argtypes = [capi.PM]\n"
            "def arrays():\n"
            "    p, i, v = capi.P_INT(), capi.P_INT(), capi.P_DBL()\n"
            "    assert lib.lis_matrix_malloc_csr(4, 10, C.byref(p), C.byref(i), C.byref(v)) == 0\n"
            "    return p, i, v\n"
            "p, i, v = arrays()\n"
            "A = capi.PM(); assert lib.lis_matrix_create(0, C.byref(A)) == 0 and lib.lis_matrix_set_size(A, 4, 0) == 0\n"
            "for k in range(5): p[k] = 2 * k if k < 4 else 7\n"
            "for k in range(7): i[k] = k %% 4; v[k] = 1.0\n"
            "assert lib.lis_matrix_set_csr(7, p, i, v, A) == 0 and lib.lis_matrix_assemble(A) == 0\n"
            "print('WATCHED', dll.lis_amd_matrix_page_test_watch(A))\n"
            "assert lib.lis_matrix_destroy(A) == 0\n"
            "assert dll.lis_amd_set_matrix_pages(0) == 0\n"
            "p, i, v = arrays()\n"
            "A = capi.PM(); assert lib.lis_matrix_create(0, C.byref(A)) == 0 and lib.lis_matrix_set_size(A, 4, 0) == 0\n"
            "for k in range(5): p[k] = 2 * k if k < 4 else 7\n"
            "for k in range(7): i[k] = k %% 4; v[k] = 1.0\n"
            "assert lib.lis_matrix_set_csr(7, p, i, v, A) == 0 and lib.lis_matrix_assemble(A) == 0\n"
            "print('PLAIN', dll.lis_amd_matrix_page_test_watch(A))\n"
            "dll.lis_matrix_unset.argtypes = [capi.PM]; assert dll.lis_matrix_unset(A) == 0 and lib.lis_matrix_destroy(A) == 0\n"
            "for a in (p, i, v): libc.free(C.cast(a, C.c_void_p))\n"
            "print('FREED')\n") % (ROOT, os.path.join(ROOT, "tests"))
    import sys
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-500:], p.stderr[-2000:])
    assert "WATCHED 3" in p.stdout and "PLAIN 0" in p.stdout and "FREED" in p.stdout, p.stdout[-500:]


def test_bench_reports_unphysical_fractions_instead_of_dying():
    """bench.py: a side leg whose working set sits in the Infinity Cache may beat the HBM peak (the 128-plane slab's x = 1 leg measured 0.996-0.999 of it): such fractions
    are LISTED in the line (`fracs_outside_0_1`), only the headline's own fraction is a hard rule"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    line = {"roofline": {"frac": 0.75}, "structured_fast_path": {"x_equals_one": {"frac": 1.003}, "roofline": {"frac": 0.84}}, "configs": [{"frac": 0.0}, {"frac": None}, {"frac": 0.5}]}
    bad = []
    bench.collect_unphysical_fracs(line, "line", bad)
    assert bad == [["line.structured_fast_path.x_equals_one", 1.003], ["line.configs[0]", 0.0], ["line.configs[1]", None]]
    bench.assert_fracs_physical({"roofline": line["roofline"]})
    with pytest.raises(AssertionError):
        bench.assert_fracs_physical({"roofline": {"frac": 1.2}})


def test_bench_dump_rows_are_a_fixed_sample_within_64_mb():
    """bench.py --dump-outputs: every row of a short y, a fixed seeded sample of a long one (512^3), ascending and in range; values and rows in float64 stay under 64 MB"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    assert np.array_equal(bench.dump_rows(1000), np.arange(1000))
    n = 512 ** 3
    rows = bench.dump_rows(n)
    assert np.array_equal(rows, bench.dump_rows(n))
    assert 0.99 * bench.DUMP_ROWS < len(rows) <= bench.DUMP_ROWS and rows[0] >= 0 and rows[-1] < n and np.all(np.diff(rows) > 0)
    assert 2 * 8 * bench.DUMP_ROWS <= 64 << 20


def test_bench_rejects_zero_steps():
    """--steps sets the number of timed steps, so it must be at least 1 (refused before any GPU work)"""
    import sys
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 2 and "--steps" in p.stderr and p.stdout == ""
