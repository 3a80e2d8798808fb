"""tests/ilu_oracle.py (the independent statement of ILU(k): pattern, term order, factor, M^-1, M^-H) held to the reference library
itself at 1, 3 and 8 OpenMP threads, fill 0, 1 and 2; tests/golden/ilu_bits.json against the reference where it exists; and the
ILU entry points of liblis_amd that need no GPU: the exported symbols."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ilu_cases
import ilu_oracle
import lis_amd
import orc

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "ilu_bits.json")


def test_ilu_symbols_are_exported():
    dll = C.CDLL(lis_amd.LIB_PATH)
    for name in ("lis_amd_last_solve_ilu", "lis_amd_ilu_factor", "lis_amd_ilu_copy", "lis_amd_ilu_psolve", "lis_amd_ilu_times", "lis_amd_ilu_info",
                 "lis_amd_ilu_factor_info", "liship_ilu_factor_f64", "liship_sweep_plain_f64"):
        assert hasattr(dll, name), name


def test_no_ilu_solve_reported_before_any_solve():
    out = subprocess.run([sys.executable, "-c", "import lis_amd; lib = lis_amd.load(); print(lib.dll.lis_amd_last_solve_ilu(None, None, None, None))"],
                         capture_output=True, text=True, check=True, cwd=os.path.dirname(HERE))
    assert out.stdout.strip() == "0"


def oracle_against_reference(ref, T):
    """every place where the oracle at T blocks is not the reference library at T threads: pattern and order of L and U, every bit
    of L, U, D, psolve and psolveh (NaN sign and payload included: both run on this CPU)"""
    bad = []
    for name in ilu_cases.NAMED:
        ptr, idx, val = ilu_cases.system(name)
        b = ilu_cases.rhs(len(ptr) - 1)
        for fill in ilu_cases.FILLS:
            want = ilu_cases.reference_ilu(ref, ptr, idx, val, fill, b)
            got = ilu_oracle.factor(ptr, idx, val, fill, T)
            for d in ilu_cases.factor_differences(got, want):
                bad.append((name, fill, d))
            if not ilu_cases.same_bits(ilu_oracle.psolve(got, b, T), want["psolve"]):
                bad.append((name, fill, "psolve"))
            if not ilu_cases.same_bits(ilu_oracle.psolveh(got, b, T), want["psolveh"]):
                bad.append((name, fill, "psolveh"))
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
    res = subprocess.run([sys.executable, "-c", "import sys; sys.path[:0] = %r; import test_ilu_cpu as t; t.child(%d)" % ([os.path.dirname(HERE), HERE], T)],
                         capture_output=True, text=True, env=dict(os.environ, OMP_NUM_THREADS=str(T)), timeout=900)
    assert res.returncode == 0, res.stderr[-2000:]
    assert json.loads([line for line in res.stdout.splitlines() if line.startswith("RESULT ")][-1][7:]) == []


def test_handmade_matrix_is_what_it_says():
    ptr, idx, val = ilu_cases.system("handmade")
    rows = [idx[ptr[i]:ptr[i + 1]].tolist() for i in range(len(ptr) - 1)]
    assert 4 not in rows[4] and rows[6].count(2) == 2 and rows[3].count(9) == 2 and rows[7].count(7) == 2
    assert any(r != sorted(r) for r in rows)
    for fill in ilu_cases.FILLS:
        f = ilu_oracle.factor(ptr, idx, val, fill)
        assert np.isfinite(f["D"]).all() and np.isfinite(f["L"][2]).all() and np.isfinite(f["U"][2]).all()
        assert f["L"][1][f["L"][0][6]:f["L"][0][7]].tolist().count(2) == 2           # the column held twice stays twice in the pattern


def test_fill_grows_the_pattern_and_zero_fill_keeps_A():
    ptr, idx, val = ilu_cases.system("p3d")
    n = len(ptr) - 1
    sizes = []
    for fill in ilu_cases.FILLS:
        f = ilu_oracle.factor(ptr, idx, val, fill)
        sizes.append(int(f["L"][0][-1] + f["U"][0][-1]))
    assert sizes[0] == int(ptr[-1]) - n and sizes[0] < sizes[1] < sizes[2]


def test_oracle_factor_reproduces_A_on_its_pattern():
    """meaning, without the reference: (L + I) (D^-1 + U) agrees with A on A's pattern for ILU(0) of the Poisson matrix, to rounding"""
    ptr, idx, val = ilu_cases.system("p3d")
    n = len(ptr) - 1
    f = ilu_oracle.factor(ptr, idx, val, 0)
    Lm, Um = np.eye(n), np.diag(1.0 / f["D"])
    for M, part in ((Lm, f["L"]), (Um, f["U"])):
        p, c, v = part
        for i in range(n):
            M[i, c[p[i]:p[i + 1]]] = v[p[i]:p[i + 1]]
    P = Lm @ Um
    for i in range(n):
        for k in range(ptr[i], ptr[i + 1]):
            assert abs(P[i, idx[k]] - val[k]) <= 1e-13 * 6.0, (i, int(idx[k]))


@pytest.mark.skipif(not os.path.exists(GOLDEN), reason="goldens not made")
def test_golden_covers_every_case():
    G = json.load(open(GOLDEN))["solves"]
    for T in (1, 8):
        for case in ("poisson32", "mm/testmat0.mtx"):
            for opts in ("-i cg", "-i bicgstab", "-i gmres -restart 30", "-i bicg", "-i cg -ilu_fill 1", "-i cg -ilu_fill 2"):
                assert G[f"{case}|{opts}|T{T}"]["status"] == 0
            for fill in (0, 1, 2):
                for tag in ("L", "U", "D", "psolve", "psolveh"):
                    assert f"{case}|{tag}|fill{fill}|T{T}" in G


@pytest.mark.skipif(not os.path.exists(orc.REF_SO) or not os.path.exists(GOLDEN), reason="oracle/_ref not built")
def test_golden_is_what_the_reference_computes():
    """re-derive T = 1 entries from the reference itself (one thread, in a child process)"""
    G = json.load(open(GOLDEN))
    src = r'''
import sys, json, hashlib, os
import numpy as np
sys.path[:0] = [%r, %r]
import lisdrv, orc, ilu_cases
ref = lisdrv.open_lib(orc.REF_SO, threads=1)
ptr, idx, val = orc.poisson3d(32, 32, 32)
sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
out = {}
for solver in ("-i cg", "-i cg -ilu_fill 1"):
    A = lisdrv.make_csr(ref, ptr, idx, val)
    b = lisdrv.matvec(ref, A, np.ones(len(ptr) - 1))
    r = lisdrv.solve(ref, A, b, solver + " " + %r)
    out[solver] = [r["iter"], sha(r["x"])]
    ref.lis_matrix_destroy(A)
f = ilu_cases.reference_ilu(ref, ptr, idx, val, 1, ilu_cases.rhs(len(ptr) - 1))
out["factor"] = [sha(f["L"][2]), sha(f["U"][2]), sha(f["D"]), sha(f["psolve"]), sha(f["psolveh"])]
print("RESULT " + json.dumps(out), flush=True)
''' % (os.path.dirname(HERE), HERE, G["common_options"])
    res = subprocess.run([sys.executable, "-c", src], capture_output=True, text=True, check=True, env=dict(os.environ, OMP_NUM_THREADS="1"))
    got = json.loads([line for line in res.stdout.splitlines() if line.startswith("RESULT ")][-1][7:])
    for solver in ("-i cg", "-i cg -ilu_fill 1"):
        want = G["solves"][f"poisson32|{solver}|T1"]
        assert tuple(got[solver]) == (want["iter"], want["x_sha256"]), solver
    assert got["factor"] == [G["solves"][f"poisson32|{tag}|fill1|T1"]["sha256"] for tag in ("L", "U", "D", "psolve", "psolveh")]
