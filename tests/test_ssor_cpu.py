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
    for name in ("lis_matrix_solve", "lis_matrix_solveh", "lis_amd_last_solve_ssor", "lis_amd_ssor_schedule_info", "liship_sweep_f64"):
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
