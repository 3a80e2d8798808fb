"""tests/bssor_oracle.py (the model of block SSOR on BSR storage: WD and the six triangular solves) held to the reference library in
every bit at 1 and at 8 OpenMP threads, to the componentwise bound of substitution, and to tests/golden/bssor_bits.npz; and what of the
feature needs no GPU: the exported symbols and the compiled sweep kernels."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import bssor_cases as cases
import bssor_oracle as oracle
import lis_amd
import orc

HERE = os.path.dirname(os.path.abspath(__file__))
TRI = [(name, bn, omega) for name in cases.TRI_NAMES for bn in cases.TRI_BNS for omega in cases.OMEGAS]


def test_block_ssor_symbols_are_exported():
    dll = C.CDLL(lis_amd.LIB_PATH)
    for name in ("liship_bsweep_f64", "liship_bsweep_chunk", "lis_amd_last_solve_ssor_block", "lis_matrix_solve", "lis_matrix_solveh"):
        assert hasattr(dll, name), name
    assert "lis_amd_last_solve_ssor_block" in lis_amd._capi._AMD_PROTOS


def test_no_block_ssor_solve_reported_before_any_solve():
    out = subprocess.run([sys.executable, "-c", "import lis_amd; lib = lis_amd.load(); print(lib.dll.lis_amd_last_solve_ssor_block())"],
                         capture_output=True, text=True, check=True, cwd=os.path.dirname(HERE))
    assert out.stdout.strip() == "0"


def test_chunks_are_the_ones_the_cases_are_built_for():
    """the terms of a long block row that lie in LDS at once, per block size: 16 KB of products at most"""
    dll = C.CDLL(lis_amd.LIB_PATH)
    for bn, chunk in cases.CHUNK.items():
        assert dll.liship_bsweep_chunk(bn) == chunk, bn
        if bn > 1:
            assert chunk * bn * bn * 8 <= 16384 and (chunk == 256 or 2 * chunk * bn * bn * 8 > 16384), bn
    assert dll.liship_bsweep_chunk(0) == 0 and dll.liship_bsweep_chunk(9) == 0


# ---------------------------------------------------------------- the model against the reference library
_reference = {}


def reference(T):
    """every array the reference gives at T threads (a child process: it reads its thread count once), computed once"""
    if T not in _reference:
        with tempfile.TemporaryDirectory() as tmp:
            _reference[T] = cases.reference_in_child(T, os.path.join(tmp, "ref.npz"))
    return _reference[T]


@pytest.mark.skipif(not os.path.exists(orc.REF_SO), reason="oracle/_ref not built")
@pytest.mark.parametrize("T", cases.THREADS)
def test_model_is_the_reference_at_T_threads(T):
    """WD and the twelve solves (B apart from X, B as X) of every triangular case, NaN sign and payload included: both run on this CPU"""
    ref = reference(T)
    bad = [(name, bn, omega, what) for name, bn, omega in TRI for what, v in cases.tri_model(name, bn, omega).items()
           if not cases.same_bits(ref[cases.tri_key(name, bn, omega, what) + "|T%d" % T], v)]
    assert bad == []


@pytest.mark.skipif(not os.path.exists(orc.REF_SO), reason="oracle/_ref not built")
def test_the_reference_sweeps_do_not_depend_on_the_thread_count():
    """lis_matrix_solve_bsr / lis_matrix_solveh_bsr hold no OpenMP pragma: one schedule block at every T"""
    one, eight = reference(1), reference(8)
    keys = [k for k in one if k.startswith("tri|")]
    assert len(keys) == len(TRI) * 13
    assert [k for k in keys if not cases.same_bits(one[k], eight[k[:-1] + "8"])] == []


@pytest.mark.skipif(not os.path.exists(orc.REF_SO), reason="oracle/_ref not built")
@pytest.mark.parametrize("T", cases.THREADS)
def test_golden_whole_solves_are_what_the_reference_computes(T):
    G = np.load(cases.GOLDEN)
    ref = reference(T)
    keys = [k for k in G.files if k.startswith("run|") and "|T%d|" % T in k]
    assert len(keys) == 3 * len(cases.RUNS) * len(cases.SOLVERS)
    assert [k for k in keys if not cases.same_bits(np.asarray(ref[k], np.float64), np.asarray(G[k], np.float64))] == []


# ---------------------------------------------------------------- the model on its own
def test_golden_is_what_the_model_computes():
    G = np.load(cases.GOLDEN)
    assert list(G["model_only"]) == []          # every case came out of the reference the same twice (the file says which did not)
    bad = [(name, bn, omega, what) for name, bn, omega in TRI for what, v in cases.tri_model(name, bn, omega).items()
           if not cases.same_bits(G[cases.tri_key(name, bn, omega, what)], v)]
    assert bad == []


def test_golden_covers_what_it_is_for():
    G = np.load(cases.GOLDEN)
    for T in cases.THREADS:
        for case, bn in cases.RUNS:
            for solver in cases.SOLVERS:
                it, status = G[cases.run_key(case, solver, bn, T, "meta")]
                assert it >= 1 and (status == 0 or (case == "nonsym120" and solver == "-i cg")), (case, solver, bn, T)     # CG on a nonsymmetric matrix runs out of iterations: kept
    assert any(len(cases.system(n)[0]) - 1 == 105 for n in cases.TRI_NAMES) and {b for b in cases.TRI_BNS if 105 % b} == {2, 4, 8}


@pytest.mark.parametrize("name,bn", [(name, bn) for name in cases.TRI_NAMES for bn in cases.TRI_BNS])
def test_model_solves_the_block_triangular_systems(name, bn):
    """meaning, without the reference: LOWER and UPPER of both solves satisfy their block triangular system within the componentwise
    bound of substitution gamma_k (|M| |x|)_i, the bound of tests/test_ssor_cpu.py (bssor_oracle.substitution_residual says which M and which k), in longdouble"""
    ptr, idx, val = cases.system(name)
    n = len(ptr) - 1
    bsr = cases.to_bsr(ptr, idx, val, bn)
    L, U, D = oracle.split(*bsr, bn)
    for omega in cases.OMEGAS:
        res = cases.tri_model(name, bn, omega)
        for what, v in res.items():
            assert np.isfinite(v).all(), (name, bn, omega, what)
        for solve in ("solve", "solveh"):
            for flag in (oracle.LOWER, oracle.UPPER):
                r, bound = oracle.substitution_residual(L, U, D, omega, n, bn, cases.rhs(n), res[cases.solve_tag(solve, flag)], solve, flag)
                worst = int(np.argmax(r - bound))
                assert (r <= bound).all(), (name, bn, omega, solve, flag, worst, float(r[worst]), float(bound[worst]))


def test_block_size_one_is_the_point_model():
    """at bn = 1 every branch is the CSR arithmetic: the block model is tests/ssor_oracle.py on the same matrix, T = 1"""
    import ssor_oracle
    for name in cases.TRI_NAMES:
        ptr, idx, val = cases.system(name)
        n = len(ptr) - 1
        for omega in cases.OMEGAS:
            point = ssor_oracle.all_solves(ptr, idx, val, omega, cases.rhs(n), 1)
            block = cases.tri_model(name, 1, omega)
            assert cases.same_bits(block["wd"], point["wd"])
            for solve, flag in oracle.SOLVES:
                assert cases.same_bits(block[cases.solve_tag(solve, flag)], point[solve, flag]), (name, omega, solve, flag)


def test_start_rule_shows_in_the_sign_of_a_zero():
    """one block row, no terms, every product a -0.0: a sum that starts with its first product (bn <= 3) keeps -0.0, one that starts
    at +0.0 (bn >= 4) gives +0.0 -- in the plain finish and in the transposed one"""
    for bn in (2, 3, 4, 5, 8):
        wd, b = np.full(bn * bn, 3.0), np.full(bn, -0.0)
        for fn in (oracle.solve, oracle.solveh):
            x = fn([[]], [[]], wd, bn, bn, b, oracle.LOWER)
            assert np.signbit(x).all() == (bn <= 3) and (x == 0).all(), (bn, fn.__name__)


def test_valid_groupings_are_all_of_them():
    assert len(cases.valid_groupings([5, 2000, 7, 9])) == 2 * 1 * 5 and [(0, 4, 1)] in cases.valid_groupings([1, 2, 3, 4])
    assert all(g[2] == 0 or all(s <= cases.SMALL_LEVEL for s in [5, 2000, 7, 9][g[0]:g[1]]) for gs in cases.valid_groupings([5, 2000, 7, 9]) for g in gs)


# ---------------------------------------------------------------- the compiled kernels
def test_block_sweep_kernels_are_the_ones_meant_and_use_no_private_memory(tmp_path):
    """kernels/bsptrsv.hip compiled to gfx950 assembly with the library's flags (csrc/Makefile, HIPFLAGS), its kernel metadata read: a
    level and a run kernel for every bn = 2 .. 8 in the four forms (plain MUL and SUB, transposed MUL and SCAT) and nothing else --
    bn = 1 runs the sweeps of sptrsv.hip --, and no kernel with a private segment: a block, t or x_j that leaves the registers shows here"""
    csrc = os.path.join(os.path.dirname(HERE), "lis_amd", "csrc")
    hipcc = os.environ.get("HIPCC") or os.path.join(os.environ.get("ROCM", "/opt/rocm"), "bin", "hipcc")
    asm = str(tmp_path / "bsptrsv.s")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(os.path.dirname(HERE), "include"),
                    "-I" + os.path.join(csrc, "kernels"), "--cuda-device-only", "-S", os.path.join(csrc, "kernels", "bsptrsv.hip"), "-o", asm],
                   check=True, capture_output=True, text=True)
    meta = re.findall(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", open(asm).read())
    sizes = {name: int(size) for name, size in meta}
    forms = ((0, 0), (1, 0), (0, 1), (2, 1))                  # (mode, transposed): MUL, SUB plain; MUL, SCAT transposed
    found = {(k, bn, mode, tr): [s for name, s in sizes.items() if k in name and "BSsorRowsILi%dELi%dELb%dE" % (bn, mode, tr) in name]
             for k in ("level_kernel", "run_kernel") for bn in range(2, 9) for mode, tr in forms}
    assert all(len(v) == 1 for v in found.values()), sorted(sizes)
    assert len(sizes) == 2 * 7 * 4, sorted(sizes)
    print("BSSOR KERNELS private segment:", sizes)
    assert all(size == 0 for (size,) in found.values()), {k: v for k, v in found.items() if v != [0]}
