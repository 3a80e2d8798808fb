"""tests/bjacobi_oracle.py (the independent statement of block Jacobi: the inverse of a block, the padding rule, M^-1 and M^-H) held to the
reference library itself at 1 and 8 OpenMP threads, block sizes 1, 2, 3, 4, 5 and 7; tests/golden/bjacobi_bits.json against the
reference where it exists; and what liblis_amd shows without a GPU: the exported symbols."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bjacobi_cases as cases
import bjacobi_oracle as oracle
import lis_amd
import orc

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "bjacobi_bits.json")
needs_ref = pytest.mark.skipif(not os.path.exists(orc.REF_SO), reason="oracle/_ref not built")


def test_bjacobi_symbols_are_exported():
    dll = C.CDLL(lis_amd.LIB_PATH)
    for name in ("lis_amd_last_solve_bjacobi", "lis_amd_bjacobi_copy", "lis_amd_bjacobi_psolve", "lis_amd_bjacobi_times",
                 "liship_bdiag_inverse_f64", "liship_bdiag_matvec_f64"):
        assert hasattr(dll, name), name
    import lis_amd._capi as capi
    assert all(k in capi._AMD_PROTOS for k in ("lis_amd_last_solve_bjacobi", "lis_amd_bjacobi_copy", "lis_amd_bjacobi_psolve"))
    assert all(k in lis_amd._LISHIP for k in ("liship_bdiag_inverse_f64", "liship_bdiag_matvec_f64"))


def test_no_bjacobi_solve_reported_before_any_solve():
    out = subprocess.run([sys.executable, "-c", "import lis_amd; lib = lis_amd.load(); print(lib.dll.lis_amd_last_solve_bjacobi(None, None, None))"],
                         capture_output=True, text=True, check=True, cwd=os.path.dirname(HERE))
    assert out.stdout.strip() == "0"


def reference_facts(ref):
    """per (matrix, bn, right-hand side): the reference's WD, M^-1 b and M^-H b as hex strings, and what it left of A"""
    out = {}
    for name in cases.NAMED:
        ptr, idx, val = cases.system(name)
        n = len(ptr) - 1
        for bn in cases.BNS:
            for tag, b in (("rhs", cases.rhs(n)), ("negzero", np.full(n, -0.0))):
                r = cases.reference_bjacobi(ref, ptr, idx, val, bn, b)
                out["%s|%d|%s" % (name, bn, tag)] = {"bn": r["bn"], "nr": r["nr"], "type": r["type"], "split": r["split"],
                                                     **{k: [float(v).hex() for v in r[k]] for k in ("WD", "psolve", "psolveh")}}
    return out


def oracle_against(facts):
    """every place where the oracle is not what the reference computed (NaN sign and payload included: both run on this CPU)"""
    from lis_amd import _capi as capi
    bad = []
    for key, r in facts.items():
        name, bn, tag = key.split("|")
        bn = int(bn)
        ptr, idx, val = cases.system(name)
        n = len(ptr) - 1
        b = cases.rhs(n) if tag == "rhs" else np.full(n, -0.0)
        want = {k: np.array([float.fromhex(v) for v in r[k]]) for k in ("WD", "psolve", "psolveh")}
        if (r["bn"], r["nr"], r["type"], r["split"]) != (bn, (n + bn - 1) // bn, capi.LIS_MATRIX_BSR, True):
            bad.append((key, "shape"))
            continue
        wd = oracle.inverse(cases.diagonal_blocks(ptr, idx, val, bn), n, bn)
        if not cases.same_bits(wd, want["WD"]):
            bad.append((key, "WD"))
        if not cases.same_bits(oracle.matvec(wd, b, n, bn), want["psolve"]):
            bad.append((key, "psolve"))
        if not cases.same_bits(oracle.matvech(wd, b, n, bn), want["psolveh"]):
            bad.append((key, "psolveh"))
    return bad


def child(T):
    import lisdrv
    ref = lisdrv.open_lib(orc.REF_SO, threads=T)
    print("RESULT " + json.dumps(reference_facts(ref)), flush=True)


_facts = {}


def facts_at(T):
    """in a child process: the reference reads its thread count once, at initialize"""
    if T not in _facts:
        res = subprocess.run([sys.executable, "-c", "import sys; sys.path[:0] = %r; import test_bjacobi_cpu as t; t.child(%d)" % ([os.path.dirname(HERE), HERE], T)],
                             capture_output=True, text=True, env=dict(os.environ, OMP_NUM_THREADS=str(T)), timeout=900)
        assert res.returncode == 0, res.stderr[-2000:]
        _facts[T] = json.loads([line for line in res.stdout.splitlines() if line.startswith("RESULT ")][-1][7:])
    return _facts[T]


@needs_ref
@pytest.mark.parametrize("T", [1, 8])
def test_oracle_is_the_reference_at_T_threads(T):
    assert oracle_against(facts_at(T)) == []


@needs_ref
def test_block_operations_do_not_depend_on_the_thread_count():
    assert facts_at(1) == facts_at(8)


@needs_ref
def test_negative_zero_case_meets_both_start_rules():
    """b = -0.0 everywhere on the Poisson matrix, whose inverse blocks hold positive entries: every product is -0.0, so a sum that starts with
    the first product is -0.0 and one that starts at +0.0 is +0.0 -- the reference shows each where the rule says"""
    f = facts_at(1)
    neg = lambda bn, k: sum(float.fromhex(v) == 0.0 and v.startswith("-") for v in f["p105|%d|negzero" % bn][k])
    for bn in cases.BNS:
        assert (neg(bn, "psolve") > 0) == (bn <= 4), bn
        assert (neg(bn, "psolveh") > 0) == (bn <= 3), bn


def test_hand_made_negative_zero_blocks():
    for bn in (2, 3, 4, 5):
        d, x, n = cases.negative_zero_case(bn)
        for fn, first in ((oracle.matvec, bn <= 4), (oracle.matvech, bn <= 3)):
            y = fn(d, x, n, bn)
            assert np.all(y == 0.0)
            assert np.signbit(y[:bn]).all() == first and not np.signbit(y[bn:]).any(), (bn, fn.__name__)


def test_oracle_inverse_is_an_inverse_and_pads_the_last_block():
    """meaning, without the reference: WD D = I to rounding on the blocks that lie inside n; the padding of the last block is the identity"""
    ptr, idx, val = cases.system("p105")
    n = len(ptr) - 1
    for bn in (2, 4):
        d = cases.diagonal_blocks(ptr, idx, val, bn)
        wd = oracle.inverse(d, n, bn)
        nr, k = (n + bn - 1) // bn, n % bn
        for b in range(nr - 1):
            D, W = (a[b * bn * bn:(b + 1) * bn * bn].reshape(bn, bn).T for a in (d, wd))
            assert np.abs(W @ D - np.eye(bn)).max() <= 8 * bn * np.finfo(float).eps
        last = wd[(nr - 1) * bn * bn:].reshape(bn, bn).T
        assert np.array_equal(last[k:, k:], np.eye(bn - k)) and not last[:k, k:].any() and not last[k:, :k].any()


def test_zero_pivot_goes_on_as_infinities_and_nans():
    wd = oracle.inverse([0.0, 1.0, 1.0, 2.0, 4.0, 0.0, 0.0, 4.0], 4, 2)
    assert not np.isfinite(wd[:4]).any() and np.array_equal(wd[4:], [0.25, 0.0, 0.0, 0.25])


@pytest.mark.skipif(not os.path.exists(GOLDEN), reason="goldens not made")
def test_golden_covers_every_case():
    G = json.load(open(GOLDEN))
    for T in (1, 8):
        for case in G["cases"]:
            for k in (2, 3, 4, 5):
                assert f"{case}|WD|k{k}|T{T}" in G["solves"]
                for opts in ("-i cg", "-i bicgstab", "-i gmres -restart 30", "-i bicg"):
                    key = f"{case}|{opts}|k{k}|T{T}"
                    assert key in G["solves"] or key in G["dropped"], key
                    if key in G["solves"]:
                        assert G["solves"][key]["status"] == 0
    assert {"poisson7x5x3", "poisson16"} <= set(G["cases"])


@needs_ref
@pytest.mark.skipif(not os.path.exists(GOLDEN), reason="goldens not made")
def test_golden_is_what_the_reference_computes():
    """re-derive T = 1 entries from the reference itself (one thread, in a child process)"""
    G = json.load(open(GOLDEN))
    src = r'''
import sys, json, hashlib, os
import numpy as np
sys.path[:0] = [%r, %r]
import lisdrv, orc, bjacobi_cases as cases
ref = lisdrv.open_lib(orc.REF_SO, threads=1)
ptr, idx, val = orc.poisson3d(16, 16, 16)
sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
out = {}
for k in (3, 5):
    A = lisdrv.make_csr(ref, ptr, idx, val)
    b = lisdrv.matvec(ref, A, np.ones(len(ptr) - 1))
    r = lisdrv.solve(ref, A, b, "-i cg -storage_block %%d " %% k + %r)
    out["cg%%d" %% k] = [r["iter"], sha(r["x"])]
    ref.lis_matrix_destroy(A)
    out["wd%%d" %% k] = sha(cases.reference_bjacobi(ref, ptr, idx, val, k, cases.rhs(len(ptr) - 1))["WD"])
print("RESULT " + json.dumps(out), flush=True)
''' % (os.path.dirname(HERE), HERE, G["common_options"])
    res = subprocess.run([sys.executable, "-c", src], capture_output=True, text=True, check=True, env=dict(os.environ, OMP_NUM_THREADS="1"))
    got = json.loads([line for line in res.stdout.splitlines() if line.startswith("RESULT ")][-1][7:])
    for k in (3, 5):
        want = G["solves"][f"poisson16|-i cg|k{k}|T1"]
        assert tuple(got["cg%d" % k]) == (want["iter"], want["x_sha256"]), k
        assert got["wd%d" % k] == G["solves"][f"poisson16|WD|k{k}|T1"]["sha256"], k


def test_inverse_kernels_keep_their_blocks_in_registers(tmp_path):
    """the compile-time sizes hold the block and its LU copy in registers: bdiag.hip compiled to gfx950 assembly with the library's flags
    (csrc/Makefile, HIPFLAGS) gives every kernel of the file a private segment of 0 bytes -- an index into those arrays that is a run-time
    value (the padding of the last block once was) sends the whole block to scratch memory"""
    import re
    csrc = os.path.join(os.path.dirname(HERE), "lis_amd", "csrc")
    hipcc = os.environ.get("HIPCC") or os.path.join(os.environ.get("ROCM", "/opt/rocm"), "bin", "hipcc")
    asm = str(tmp_path / "bdiag.s")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(os.path.dirname(HERE), "include"),
                    "-I" + os.path.join(csrc, "kernels"), "--cuda-device-only", "-S", os.path.join(csrc, "kernels", "bdiag.hip"), "-o", asm],
                   check=True, capture_output=True, text=True)
    text = open(asm).read()
    meta = re.findall(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", text)
    sizes = {name: int(size) for name, size in meta}
    fixed = [name for name in sizes if "bdiag_inverse_kernelILi" in name]
    assert len(fixed) == 8 and len(sizes) >= 8 + 1 + 18, sorted(sizes)           # bn = 1 .. 8, the generic inverse, 9 products in both forms
    assert all(size == 0 for size in sizes.values()), {k: v for k, v in sizes.items() if v}
