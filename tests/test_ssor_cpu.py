"""tests/golden/ssor_bits.{json,npz} against the reference library where it exists (as tests/test_golden.py does), and the SSOR
entry points of liblis_amd that need no GPU: exported symbols, and refusals that happen before any device work."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import lis_amd
import orc

HERE = os.path.dirname(os.path.abspath(__file__))
G = json.load(open(os.path.join(HERE, "golden", "ssor_bits.json")))


def test_ssor_symbols_are_exported():
    dll = C.CDLL(lis_amd.LIB_PATH)
    for name in ("lis_matrix_solve", "lis_matrix_solveh", "lis_amd_last_solve_ssor", "lis_amd_ssor_schedule_info", "lis_amd_ssor_sweep_info", "liship_sweep_f64"):
        assert hasattr(dll, name), name


def test_no_ssor_solve_reported_before_any_solve():
    out = subprocess.run([sys.executable, "-c", "import lis_amd; lib = lis_amd.load(); print(lib.dll.lis_amd_last_solve_ssor(None, None, None, None))"],
                         capture_output=True, text=True, check=True, cwd=os.path.dirname(HERE))
    assert out.stdout.strip() == "0"


def test_golden_covers_both_thread_counts():
    keys = G["solves"]
    for T in (1, 8):
        for case in ("poisson32", "mm/testmat0.mtx"):
            for solver in ("-i cg", "-i bicgstab", "-i gmres -restart 30", "-i bicg"):
                assert keys[f"{case}|{solver}|T{T}"]["status"] == 0
            for tag in ("wd", "solve", "solveh"):
                assert f"{case}|{tag}|T{T}" in keys
    # the block-Jacobi preconditioner of 8 blocks is weaker: every case needs more iterations at T = 8
    for k, v in keys.items():
        if k.endswith("|T8") and "iter" in v:
            assert v["iter"] >= keys[k[:-1] + "1"]["iter"], k


@pytest.mark.skipif(not os.path.exists(orc.REF_SO), reason="oracle/_ref not built")
def test_golden_is_what_the_reference_computes():
    """re-derive the T = 1 histories from the reference itself (one thread, in a child process)"""
    src = r'''
import sys, json, hashlib, os
import numpy as np
sys.path[:0] = [%r, %r]
import lisdrv, orc
ref = lisdrv.open_lib(orc.REF_SO, threads=1)
ptr, idx, val = orc.poisson3d(32, 32, 32)
out = {}
for solver in ("-i cg", "-i bicg"):
    A = lisdrv.make_csr(ref, ptr, idx, val)
    b = lisdrv.matvec(ref, A, np.ones(len(ptr) - 1))
    r = lisdrv.solve(ref, A, b, solver + " " + %r)
    out[solver] = [r["iter"], hashlib.sha256(r["x"].tobytes()).hexdigest()]
    ref.lis_matrix_destroy(A)
print("RESULT " + json.dumps(out), flush=True)
''' % (os.path.dirname(HERE), HERE, G["common_options"])
    res = subprocess.run([sys.executable, "-c", src], capture_output=True, text=True, check=True, env=dict(os.environ, OMP_NUM_THREADS="1"))
    got = json.loads([line for line in res.stdout.splitlines() if line.startswith("RESULT ")][-1][7:])
    for solver, (it, xs) in got.items():
        want = G["solves"][f"poisson32|{solver}|T1"]
        assert (it, xs) == (want["iter"], want["x_sha256"]), solver


# ------------------------------------------------------------------------------------------------------------------------------
# tests/ssor_oracle.py (the independent statement of the six triangular solves that tests/test_ssor_schedule_gpu.py holds the
# kernels to) against the reference library, and the catalogue of tests/ssor_cases.py against what each case says it is for.
import ssor_cases
import ssor_oracle

FAMILIES = list(ssor_cases.CASES) + ["heavy", "special"]


def _family(name):
    return ssor_cases.special_system() if name == "special" else ssor_cases.system(name)


def oracle_against_reference(ref, T):
    """every place where the oracle at T blocks is not the reference library at T threads, bit for bit (NaN sign and payload
    included: both run on this CPU): WD and the six solves, separate and aliased B / X, of A1 and A2 of every family"""
    bad = []
    for name in FAMILIES:
        s = _family(name)
        for key in ("A1", "A2"):
            if key not in s:
                continue
            A = ssor_cases.library_matrix(ref, *s[key], expect_ok=(name != "special"))
            want = ssor_oracle.all_solves(*s[key], ssor_cases.OMEGA, s["b"], T)
            if ssor_cases.first_difference(ssor_cases.library_wd(A), want["wd"]):
                bad.append((name, key, "wd"))
            for solve, flag in ssor_oracle.SOLVES:
                for alias in (False, True):
                    d = ssor_cases.first_difference(ssor_cases.library_solve(ref, A, solve, flag, s["b"], alias), want[solve, flag])
                    if d:
                        bad.append((name, key, solve, flag, alias) + d)
            ref.lis_matrix_destroy(A)
    return bad


def child(T):
    import lisdrv
    ref = lisdrv.open_lib(orc.REF_SO, threads=T)
    print("RESULT " + json.dumps(oracle_against_reference(ref, T)), flush=True)


@pytest.mark.skipif(not os.path.exists(orc.REF_SO), reason="oracle/_ref not built")
def test_oracle_is_the_reference_at_one_thread(reflib):
    assert oracle_against_reference(reflib, 1) == []


@pytest.mark.skipif(not os.path.exists(orc.REF_SO), reason="oracle/_ref not built")
@pytest.mark.parametrize("T", [3, 8])
def test_oracle_is_the_reference_at_T_threads(T):
    """in a child process: the reference reads its thread count once, at initialize"""
    res = subprocess.run([sys.executable, "-c", "import sys; sys.path[:0] = %r; import test_ssor_cpu as t; t.child(%d)" % ([os.path.dirname(HERE), HERE], T)],
                         capture_output=True, text=True,
                         env=dict(os.environ, OMP_NUM_THREADS=str(T)), timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    assert json.loads([line for line in res.stdout.splitlines() if line.startswith("RESULT ")][-1][7:]) == []


@pytest.mark.parametrize("name", [f for f in FAMILIES if f != "special"])
def test_oracle_solves_the_triangular_systems(name):
    """Meaning, without the reference: LOWER and UPPER of both solves satisfy their triangular system within the componentwise
    bound of substitution, |b - M x|_i <= gamma_k (|M| |x|)_i with k = terms of the row + 2 and u = 2^-53, evaluated in
    numpy.longdouble (ssor_oracle.substitution_residual says which M and why k).  And no result of a case outside the
    special-value case has a non-finite entry."""
    s = _family(name)
    for key in ("A1", "A2"):
        if key not in s:
            continue
        L, U, D = ssor_oracle.split(*s[key])
        res = ssor_oracle.all_solves(*s[key], ssor_cases.OMEGA, s["b"])
        for k, v in res.items():
            assert np.isfinite(v).all(), (name, key, k)
        for solve in ("solve", "solveh"):
            for flag in (ssor_oracle.LOWER, ssor_oracle.UPPER):
                r, bound = ssor_oracle.substitution_residual(L, U, D, ssor_cases.OMEGA, s["b"], res[solve, flag], solve, flag)
                worst = int(np.argmax(r - bound))
                assert (r <= bound).all(), (name, key, solve, flag, worst, float(r[worst]), float(bound[worst]))


def test_special_case_keeps_most_of_every_result_finite():
    """one zero diagonal entry, inf and NaN in b: the poison must reach other rows and still leave at least half of every result
    finite, or the case would compare NaN with NaN and nothing else"""
    s = ssor_cases.special_system()
    n = len(s["b"])
    for key in ("A1", "A2"):
        for T in (1, 3):
            res = ssor_oracle.all_solves(*s[key], ssor_cases.OMEGA, s["b"], T)
            assert np.isinf(res["wd"]).sum() == 1 and res["wd"][s["poisoned"][0]] == np.inf
            for k in ssor_oracle.SOLVES:
                finite = int(np.isfinite(res[k]).sum())
                assert 2 * finite >= n, (key, T, k, finite, n)
                assert n - finite > (3 if T == 1 else 2), (key, T, k, "the poison reached no other row")      # (a block border may stop it)
                assert np.isnan(res[k]).any() and np.isinf(res[k]).any()


def _prescribed(levels):
    sizes = [len(l) for l in levels]
    groups = ssor_cases.grouping(sizes)
    own = [g[0] for g in groups if not g[2]]
    nlong = [sum(c >= ssor_cases.LONG_ROW for c in l) for l in levels]
    return {"sizes": sizes, "counts": [sorted(l) for l in levels],
            "info": [len(sizes), len(groups), len(own), sum(nlong[l] for l in own), sum(nlong) - sum(nlong[l] for l in own), sum(map(sum, levels))]}


@pytest.mark.parametrize("name", list(ssor_cases.CASES))
def test_generated_matrices_have_the_prescribed_schedule(name):
    """the forward sweep on L of A1 and on U^T of A2 have exactly the case's `fwd` levels, row term counts included, the backward
    sweeps on U of A1 and L^T of A2 its `bwd` levels"""
    c, s = ssor_cases.CASES[name], ssor_cases.system(name)
    for key, which in (("A1", (0, 1)), ("A2", (2, 3))):
        sweeps = ssor_cases.sweep_terms(*s[key])
        for w, levels in zip(which, (c["fwd"], c["bwd"])):
            terms, desc = sweeps[w]
            st, want = ssor_cases.sweep_stats(terms, desc), _prescribed(levels)
            assert st["sizes"] == want["sizes"] and st["info"] == want["info"], (name, key, w)
            by_level = [[] for _ in want["sizes"]]
            for i, l in enumerate(st["lev"]):
                by_level[l].append(len(terms[i]))
            assert [sorted(l) for l in by_level] == want["counts"], (name, key, w)


def test_catalogue_reaches_what_it_is_for():
    """the properties the cases exist for, from the restated schedule rules alone"""
    st = {name: [ssor_cases.sweep_stats(t, d) for t, d in ssor_cases.sweep_terms(*ssor_cases.system(name)["A1"])] for name in list(ssor_cases.CASES) + ["heavy"]}
    assert set(st["sizes"][0]["sizes"]) >= {1, 255, 256, 257, 1023, 1024, 1025, 1280, 1281, 5000}
    assert [g[2] for g in st["alternating"][0]["groups"]] == [0, 1, 0, 1, 0, 0, 1, 0]           # large first ... large last
    assert st["alternating"][1]["groups"][0][2] == 1 and st["alternating"][1]["groups"][-1][2] == 0
    assert st["edges_small"][0]["info"][2] == 0 and st["edges_small"][0]["info"][4] == 24       # every long row inside the run
    assert st["edges_large"][0]["info"][3] == 24 and st["edges_large"][0]["info"][4] == 0       # every long row in an own-launch level
    lo = st["long_only"][0]
    assert lo["sizes"][1] == lo["nlong"][1] == 1030                                             # long rows only
    assert (lo["sizes"][2] - lo["nlong"][2], lo["sizes"][3] - lo["nlong"][3], lo["nlong"][4]) == (256, 257, 1)
    for w in (0, 1):                                                                            # heavy: the first levels on their own launch
        assert st["heavy"][w]["sizes"][0] > 1024 and st["heavy"][w]["sizes"][1] > 1024 and st["heavy"][w]["info"][2] >= 2
    # under T blocks: a block-local level of more than 1024 rows, and a long row whose terms reach over a block border
    for name, c in ssor_cases.CASES.items():
        for T in c["T"]:
            ptr, idx, val = ssor_cases.system(name)["A1"]
            n = len(ptr) - 1
            assert n % T != 0
            fwd = ssor_cases.sweep_stats(*ssor_cases.sweep_terms(ptr, idx, val, T)[0])
            assert fwd["info"][2] >= 1, (name, T)
            blk = ssor_cases.row_block(n, T)
            cut = [(int((blk[idx[ptr[i]:ptr[i + 1]]] == blk[i]).sum()) - 1, int(ptr[i + 1] - ptr[i]) - 1) for i in range(n) if ptr[i + 1] - ptr[i] > ssor_cases.LONG_ROW]
            assert any(0 < kept < full for kept, full in cut), (name, T)
