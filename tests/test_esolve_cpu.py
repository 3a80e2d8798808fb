"""The eigen half of the Lis C API, the parts that need no GPU: the ABI of LIS_ESOLVER_STRUCT, option parsing against the reference's tables, every refusal
(fired before A or x is touched), lis_matrix_shift_diagonal's host path in the six storage formats against tests/esolve_model.py and the reference, the
model's recurrences against the reference in every bit, and the link check: the reference's own test/etest1.c compiles against include/ and links against
liblis_amd.so.  The GPU side is tests/test_esolve_gpu.py, test_shift_gpu.py and test_multidot_gpu.py."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import esolve_drv
import esolve_model as em
import lis_amd
import lisdrv
import orc
from lis_amd import _capi as capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
REF = "/root/reference"


@pytest.fixture(scope="module")
def lib():
    lib = lis_amd.load()
    assert lib.initialize([]) == 0
    return lib


# ---------------------------------------------------------------------------------------------- ABI
LAYOUT_PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "lis.h"
#define F(f) printf("LIS_ESOLVER_STRUCT." #f " %zu\n", offsetof(struct LIS_ESOLVER_STRUCT, f))
int main(void) {
  printf("sizeof.esolver %zu\n", sizeof(struct LIS_ESOLVER_STRUCT));
  F(A); F(B); F(x); F(xx); F(d); F(evalue); F(evector); F(resid); F(work); F(rhistory); F(worklen); F(options); F(params); F(retcode);
  F(iter); F(iter2); F(time); F(nesol); F(itime); F(ptime); F(p_c_time); F(p_i_time); F(eprecision); F(ishift); F(nrm2); F(tol);
  printf("const %d %d %d %d %d %d %d %d %d\n", LIS_EOPTIONS_LEN, LIS_EPARAMS_LEN, LIS_EPARAMS_RESID, LIS_EPARAMS_SHIFT, LIS_EPARAMS_SHIFT_IM,
         LIS_ESOLVER_LEN, LIS_ESOLVER_CR, LIS_ESOLVER_GAI, LIS_EPRINT_ALL);
  printf("eoptions %d %d %d %d %d %d %d %d %d %d %d %d %d\n", LIS_EOPTIONS_ESOLVER, LIS_EOPTIONS_MAXITER, LIS_EOPTIONS_SUBSPACE, LIS_EOPTIONS_MODE,
         LIS_EOPTIONS_OUTPUT, LIS_EOPTIONS_INITGUESS_ONES, LIS_EOPTIONS_INNER_ESOLVER, LIS_EOPTIONS_INNER_GENERALIZED_ESOLVER, LIS_EOPTIONS_STORAGE,
         LIS_EOPTIONS_STORAGE_BLOCK, LIS_EOPTIONS_PRECISION, LIS_EOPTIONS_SWITCH_MAXITER, LIS_EOPTIONS_RVAL);
  return 0;
}
"""


def _probe(include_dir, tmp_path, tag):
    src = tmp_path / f"eprobe_{tag}.c"
    src.write_text(LAYOUT_PROBE)
    exe = tmp_path / f"eprobe_{tag}"
    subprocess.run(["gcc", "-I", include_dir, str(src), "-o", str(exe)], check=True)
    return subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout


def test_esolver_struct_layout_is_the_reference_abi(tmp_path):
    ours = _probe(os.path.join(ROOT, "include"), tmp_path, "ours")
    assert ours == open(os.path.join(GOLDEN, "esolver_abi_layout.txt")).read()      # dumped from the reference header by this probe
    if os.path.exists(os.path.join(REF, "include", "lis.h")):
        assert _probe(os.path.join(REF, "include"), tmp_path, "ref") == ours
    sizes = dict(line.rsplit(" ", 1) for line in ours.splitlines() if line.startswith(("sizeof", "LIS_")))
    assert C.sizeof(capi.ESolver) == int(sizes["sizeof.esolver"])
    for f in ("rhistory", "options", "params", "retcode", "iter", "time", "eprecision", "tol"):
        assert getattr(capi.ESolver, f).offset == int(sizes["LIS_ESOLVER_STRUCT." + f]), f


def test_the_eigen_symbols_are_exported():
    dll = C.CDLL(lis_amd.LIB_PATH)
    for name in capi._PROTOS:
        if name.startswith("lis_esolve") or name in ("lis_gesolve", "lis_matrix_shift_diagonal"):
            assert hasattr(dll, name), name
    assert hasattr(dll, "liship_multidot_f64") and hasattr(dll, "liship_csr_shift_diagonal_f64")


# ---------------------------------------------------------------------------------------------- options
OPTIONS = json.load(open(os.path.join(GOLDEN, "esolve_options.json")))


@pytest.mark.parametrize("text", sorted(OPTIONS["parsed"]))
def test_option_parsing_gives_the_reference_slots(lib, text):
    err, options, params = esolve_drv.parsed(lib, text)
    want = OPTIONS["parsed"][text]
    assert (err, options, [float(p).hex() for p in params]) == (want["err"], want["options"], want["params_hex"])


def test_option_parsing_field_by_field_against_the_reference(lib, reflib):
    for text in esolve_drv.OPTION_TEXTS:
        assert esolve_drv.parsed(lib, text) == esolve_drv.parsed(reflib, text), text


def test_names_and_defaults(lib):
    err, options, params = esolve_drv.parsed(lib, "")
    assert (err, options, params) == (0, [5, 1000, 1, 0, 0, 1, 2, 10, 0, 2, 0, 0, 0], [1.0e-12, 0.0, 0.0])
    buf = C.create_string_buffer(128)
    names = []
    for k in range(1, 17):
        assert lib.lis_esolver_get_esolvername(k, buf) == 0
        names.append(buf.value.decode())
    assert names[:5] == ["Power", "Inverse", "Rayleigh Quotient", "CG", "CR"] and names[15] == "Generalized Arnoldi"
    assert lib.lis_esolver_get_esolvername(0, buf) == -1 and lib.lis_esolver_get_esolvername(17, buf) == -1


# ---------------------------------------------------------------------------------------------- refusals
def _snapshot(lib, A, vx):
    a = lisdrv.matrix_arrays(A)
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in a.items()}, lisdrv.get_vector(lib, vx).copy()


def _same(s1, s2):
    a1, x1 = s1
    a2, x2 = s2
    assert a1.keys() == a2.keys()
    for k in a1:
        assert np.array_equal(a1[k], a2[k]), k
    assert np.array_equal(x1.view(np.int64), x2.view(np.int64))


REFUSED = [("-e si", 5), ("-e li", 5), ("-e ai", 5), ("-e 6", 5), ("-e gpi", 5), ("-e gii", 5), ("-e grqi", 5), ("-e gcg", 5), ("-e gcr", 5), ("-e gsi", 5),
           ("-e gli", 5), ("-e gai", 5), ("-e 16", 5), ("-e 17", 1), ("-e 0", 1), ("-e cr -ef quad", 1), ("-e cr -ef switch", 1), ("-e pi -estorage msr", 5),
           ("-e pi -emaxiter -3", 1)]


@pytest.mark.parametrize("text,code", REFUSED)
def test_refusals_fire_before_A_or_x_is_touched(lib, text, code, capfd):
    ptr, idx, val = esolve_drv.sym_csr()
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
    if code == 5:
        assert "not served" in message
    _same(before, _snapshot(lib, A, vx))
    assert A.contents.matrix_type == capi.LIS_MATRIX_CSR
    lib.lis_esolver_destroy(E)
    lib.lis_vector_destroy(vx)
    lib.lis_matrix_destroy(A)


def test_gesolve_with_a_B_and_the_subspace_getters_are_refused(lib, capfd):
    ptr, idx, val = esolve_drv.sym_csr()
    A, B = lisdrv.make_csr(lib, ptr, idx, val), lisdrv.make_csr(lib, ptr, idx, val)
    vx = lisdrv.new_vector(lib, A, np.ones(len(ptr) - 1))
    before = _snapshot(lib, A, vx)
    E = capi.PE()
    assert lib.lis_esolver_create(C.byref(E)) == 0
    ev, iv = C.c_double(-7.0), C.c_int(-7)
    assert lib.lis_gesolve(A, B, vx, C.byref(ev), E) == capi.LIS_ERR_NOT_IMPLEMENTED
    assert "generalized" in capfd.readouterr().out
    _same(before, _snapshot(lib, A, vx))
    for call in (lambda: lib.lis_esolver_get_evalues(E, vx), lambda: lib.lis_esolver_get_residualnorms(E, vx), lambda: lib.lis_esolver_get_iters(E, vx)):
        assert call() == capi.LIS_ERR_ILL_ARG              # as the reference answers for a solver that is not subspace / Lanczos / Arnoldi (lis_esolver.c:1159-1163)
        assert "Set Subspace" in capfd.readouterr().out
    for call in (lambda: lib.lis_esolver_get_evectors(E, B), lambda: lib.lis_esolver_get_specific_evalue(E, 0, C.byref(ev)),
                 lambda: lib.lis_esolver_get_specific_evector(E, 0, vx), lambda: lib.lis_esolver_get_specific_residualnorm(E, 0, C.byref(ev)),
                 lambda: lib.lis_esolver_get_specific_iter(E, 0, C.byref(iv))):
        assert call() == capi.LIS_ERR_NOT_IMPLEMENTED
        assert "subspace" in capfd.readouterr().out
    assert (ev.value, iv.value) == (-7.0, -7)
    _same(before, _snapshot(lib, A, vx))
    lib.lis_esolver_destroy(E)
    lib.lis_vector_destroy(vx)
    lib.lis_matrix_destroy(A)
    lib.lis_matrix_destroy(B)


def test_an_option_that_is_not_correct_is_an_error(lib):
    for text in ("-e nosuch", "-eprint 7", "-initx_ones maybe", "-ef 2", "-estorage xyz", "-ie nosuch", "-rval 2"):
        assert esolve_drv.parsed(lib, text)[0] == capi.LIS_ERR_ILL_ARG, text


# ---------------------------------------------------------------------------------------------- the shift on the host, six formats
def _matrix(L, fmt, full=False):
    """full: 7-point Poisson on 3^3, every row with a diagonal entry (n = 27: the last 2 x 2 block row of BSR is half padding)"""
    ptr, idx, val = orc.poisson3d(3, 3, 3) if full else em.shift_matrix(twice=(fmt == "csr"))
    A0 = lisdrv.make_csr(L, ptr, idx, val)
    if fmt == "csr":
        return A0
    A = lisdrv.convert(L, A0, fmt)
    L.lis_matrix_destroy(A0)
    return A


def _host_shift(L, fmt, sigmas, split=False):
    """-> (the format's arrays before the shifts, value[] -- or D of the split form -- after them)"""
    A = _matrix(L, fmt, full=split)
    if split:
        assert L.lis_matrix_split(A) == 0
    before = lisdrv.matrix_arrays(A)
    for s in sigmas:
        assert L.lis_matrix_shift_diagonal(A, s) == 0
    out = lisdrv.split_arrays(A)["D"] if split else lisdrv.matrix_arrays(A)["value"]
    L.lis_matrix_destroy(A)
    return before, out


SIGMAS = [(1.5,), (0.0,), (-0.0,), (5e-324,), (float("inf"),), (0.1, -0.1), (1e17, -1e17)]


@pytest.mark.parametrize("fmt", ["csr", "csc", "ell", "dia", "jad", "bsr"])
@pytest.mark.parametrize("sigmas", SIGMAS)
def test_host_shift_is_the_model_in_every_bit(lib, fmt, sigmas):
    """No HBM copy exists (nothing was multiplied): lis_matrix_shift_diagonal edits the host arrays.  shift(s) then shift(-s) keeps the reference's drift."""
    before, got = _host_shift(lib, fmt, sigmas)
    want = before["value"].copy()
    for s in sigmas:
        want = em.shift(fmt, before, want, s)
    assert np.array_equal(got.view(np.int64), want.view(np.int64))
    moved = np.flatnonzero(got.view(np.int64) != before["value"].view(np.int64))
    if sigmas == (1.5,):
        assert len(moved) >= 9                                                              # every row that stores a diagonal entry (ELL: its padding too)
    if sigmas == (1e17, -1e17):
        assert len(moved) > 0                                                               # the drift is there


@pytest.mark.parametrize("fmt", ["csr", "csc", "ell", "bsr"])
def test_host_shift_of_a_split_matrix_moves_D_only(lib, fmt):
    A = _matrix(lib, fmt)
    assert lib.lis_matrix_split(A) == 0
    before = lisdrv.split_arrays(A)
    own = lisdrv.matrix_arrays(A)["value"].copy()
    assert lib.lis_matrix_shift_diagonal(A, 1.5) == 0
    after = lisdrv.split_arrays(A)
    want = before["D"].copy()
    if fmt == "bsr":
        bn = A.contents.bnr
        for i in range(A.contents.nr):
            for j in range(bn):
                want[i * bn * bn + j * bn + j] -= 1.5
    else:
        want -= 1.5                       # every row, diagonal entry stored or not (lis_matrix_csr.c:579-582)
    assert np.array_equal(after["D"].view(np.int64), want.view(np.int64))
    for part in ("L", "U"):
        assert np.array_equal(after[part]["value"], before[part]["value"])
    assert np.array_equal(lisdrv.matrix_arrays(A)["value"], own)
    lib.lis_matrix_destroy(A)


@pytest.mark.parametrize("fmt", ["csr", "csc", "ell", "jad", "bsr"])
def test_host_shift_against_the_reference(lib, reflib, fmt):
    """(DIA is left out: the reference's OpenMP branch, lis_matrix_dia.c:395-412, addresses value[is nnd + j k] -- not the diagonal it found; this library
    and the model follow its serial branch, :414-421)"""
    for sigmas in SIGMAS:
        a, b = _host_shift(lib, fmt, sigmas)[1], _host_shift(reflib, fmt, sigmas)[1]
        assert np.array_equal(a.view(np.int64), b.view(np.int64)), sigmas
    if fmt != "jad":
        # the split form, on a matrix whose every row stores its diagonal: the reference mallocs D and fills the rows that have one, this library starts D at 0 (lis_split.c)
        a, b = _host_shift(lib, fmt, (1.5,), split=True)[1], _host_shift(reflib, fmt, (1.5,), split=True)[1]
        assert np.array_equal(a.view(np.int64), b.view(np.int64))


# ---------------------------------------------------------------------------------------------- the model's recurrences against the reference
MODEL_THREADS = (1, 3, 8)
MODEL_WORKER = r'''
import json, sys
import numpy as np
sys.path[:0] = [%(root)r, %(tests)r]
import esolve_drv, orc
T = int(sys.argv[1])
ref = esolve_drv.open_lib(orc.REF_SO, threads=T)
out = {}
for matrix, opts, given in %(cases)r:
    A = esolve_drv.make_matrix(ref, matrix)
    res = esolve_drv.esolve(ref, A, opts, esolve_drv.start_vector(A.contents.n) if given else None)
    out[matrix + "|" + opts] = {"iter": res["iter"], "status": res["status"], "evalue": float(res["evalue"]).hex(), "resid": float(res["resid"]).hex(),
                                "rhistory": [float(v).hex() for v in res["rhistory"]], "x": [float(v).hex() for v in res["x"]]}
    ref.lis_matrix_destroy(A)
json.dump(out, open(sys.argv[2], "w"))
'''


@pytest.mark.parametrize("T", MODEL_THREADS)
def test_model_recurrences_are_the_reference_in_every_bit(reflib, tmp_path, T):
    """One process per thread count (the OpenMP runtime takes its thread count once).  The model restates lis_esolver_pi.c, _ii.c, _rqi.c, _cg.c with the
    chunked sums of T threads and its own BiCG / CG inner solves (lis_solver_bicg.c, lis_solver_cg.c)."""
    path = tmp_path / ("ref_T%d.json" % T)
    src = MODEL_WORKER % {"root": ROOT, "tests": os.path.join(ROOT, "tests"), "cases": em.MODEL_CASES}
    subprocess.run([os.sys.executable, "-c", src, str(T), str(path)], check=True, env=dict(os.environ, OMP_NUM_THREADS=str(T)), stdout=subprocess.DEVNULL)
    ref = json.load(open(path))
    for matrix, opts, given in em.MODEL_CASES:
        want = ref[matrix + "|" + opts]
        ptr, idx, val = esolve_drv.MATRICES[matrix]()
        got = em.esolve(ptr, idx, val, opts, T=T, x0=esolve_drv.start_vector(len(ptr) - 1) if given else None)
        assert (got["iter"], got["status"]) == (want["iter"], want["status"]), (matrix, opts)
        assert float(got["evalue"]).hex() == want["evalue"] and float(got["resid"]).hex() == want["resid"], (matrix, opts)
        assert [float(v).hex() for v in got["rhistory"]] == want["rhistory"], (matrix, opts)
        assert [float(v).hex() for v in got["x"]] == want["x"], (matrix, opts)


# ---------------------------------------------------------------------------------------------- link check
def test_the_reference_etest1_compiles_and_links_against_this_library(tmp_path):
    """Compiles and links only; the binary is not run (it needs a GPU)."""
    src = os.path.join(REF, "test", "etest1.c")
    if not os.path.exists(src):
        pytest.skip("the reference tree is not here")
    exe = tmp_path / "etest1_amd"
    libdir = os.path.dirname(lis_amd.LIB_PATH)
    done = subprocess.run(["gcc", "-O2", "-w", "-I", os.path.join(ROOT, "include"), src, "-o", str(exe), "-L", libdir, "-llis_amd", "-lm",
                           "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    assert os.path.exists(exe)
