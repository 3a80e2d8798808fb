"""ILU(k) preconditioner (-p ilu): what it costs and what it buys.  Prints ONE JSON object (a run on an MI355X belongs in profiles/ilu_probe.json).
    python tools/ilu_probe.py [N ...] [--mesh NODES] [--ref-threads 1,16]        (default: 128 256, mesh 2000000, reference at 1 and 16 threads)
Legs:
  cases      7-point Poisson N^3, fill 0 and 1: host seconds of the symbolic step, factorisation and psolve times (device events), levels,
             launches, bytes; the SSOR psolve of the same tree in the same process (ilu0_over_ssor_psolve; above 1.25 the probe says
             "explanation_owed"); CG + ILU(0) against CG + SSOR and CG + Jacobi at tol 1e-12.  liblis_amd reports ptime = 0 for every
             preconditioner (lis_solver_get_timeex): the preconditioner's creation is timed here as create_s (one factorisation with
             the pattern cached, synchronised), itime_s is the library's itime (iterations, psolves included) and
             wall_s_with_precon_create the whole lis_solve.
  reference  the reference library (oracle/_ref) on the host cores at the given thread counts, on the same matrices:
             the wall time of its lis_precon_create (symbolic + numerical, three calls; what it adds to ptime) -- at T threads it factorises T independent row blocks, a
             different and cheaper preconditioner.  Skipped (and said so) where oracle/_ref is absent.
  mesh       the unstructured mesh of tests/perf/irregular_sweep.py (orc.unstructured_mesh) at NODES nodes, fill 0: wide levels;
             levels, factorisation and psolve ms, GMRES(30) + ILU(0) against GMRES(30) + Jacobi.
Times: the first ten samples of every device-event series are warm-up; median, 10th and 90th percentile of the rest."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import lis_amd  # noqa: E402
import lisdrv  # noqa: E402
import orc  # noqa: E402

REPS = 40


def stats(ms):
    t = np.array(ms[10:])
    return {"median_ms": round(float(np.median(t)), 4), "p10_ms": round(float(np.percentile(t, 10)), 4), "p90_ms": round(float(np.percentile(t, 90)), 4),
            "samples": len(t)}


def ilu_times(lib, A, fill, rhs):
    dll = lib.dll
    t0 = time.perf_counter()
    sizes = (C.c_int * 3)()
    assert dll.lis_amd_ilu_factor(A, fill, sizes) == 0
    first_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    assert dll.lis_amd_ilu_factor(A, fill, sizes) == 0
    create_s = time.perf_counter() - t0
    info = (C.c_double * 6)()
    assert dll.lis_amd_ilu_info(A, fill, info) == 0
    fi = (C.c_int * 6)()
    assert dll.lis_amd_ilu_factor_info(A, fill, fi) == 0
    fms, pms = (C.c_double * REPS)(), (C.c_double * REPS)()
    vb, vx = lisdrv.new_vector(lib, A, rhs), lisdrv.new_vector(lib, A)
    assert dll.lis_amd_ilu_times(A, fill, vb, vx, REPS, fms, pms) == 0
    lib.lis_vector_destroy(vb)
    lib.lis_vector_destroy(vx)
    return {"symbolic_s": round(info[0], 4), "first_factor_wall_s": round(first_s, 4), "create_s": round(create_s, 5),
            "nnz_LU": int(info[1]), "levels": int(info[2]), "factor_launches": int(info[3]), "launches_per_psolve": int(info[4]),
            "bytes_per_psolve": int(info[5]), "levels_on_own_launch": fi[2], "rows_by_workgroup": fi[3] + fi[4],
            "factor": stats(list(fms)), "psolve": stats(list(pms))}


def solve_row(lib, A, b, opts):
    lisdrv.solve(lib, A, b, opts + " -maxiter 1")                       # plans, schedules (not timed below)
    t0 = time.perf_counter()
    out = lisdrv.solve(lib, A, b, opts + " -tol 1e-12 -maxiter 5000")
    wall = time.perf_counter() - t0
    return {"iter": out["iter"], "status": out["status"], "resid": out["resid"], "itime_s": round(out["itime"], 4), "wall_s_with_precon_create": round(wall, 4)}


def probe(lib, N, fills):
    dll = lib.dll
    ptr, idx, val = orc.poisson3d(N, N, N)
    n = len(ptr) - 1
    A = lisdrv.make_csr(lib, ptr, idx, val)
    b = lisdrv.matvec(lib, A, np.ones(n))
    row = {"N": N, "n": n, "ilu": {}}
    rhs = np.random.default_rng(1).uniform(-1, 1, n)
    for fill in fills:
        row["ilu"]["fill%d" % fill] = ilu_times(lib, A, fill, rhs)
    for pc in ("jacobi", "ilu", "ssor"):                                  # ssor last: it leaves A split
        row[f"cg_{pc}"] = solve_row(lib, A, b, f"-i cg -p {pc}")
    ms = (C.c_double * REPS)()
    vb, vx = lisdrv.new_vector(lib, A, rhs), lisdrv.new_vector(lib, A)
    assert dll.lis_amd_ssor_psolve_times(A, vb, vx, REPS, ms) == 0
    lib.lis_vector_destroy(vb)
    lib.lis_vector_destroy(vx)
    row["ssor_psolve_same_process"] = stats(list(ms))
    ratio = row["ilu"]["fill0"]["psolve"]["median_ms"] / row["ssor_psolve_same_process"]["median_ms"]
    row["ilu0_over_ssor_psolve"] = round(ratio, 3)
    row["explanation_owed"] = bool(ratio > 1.25)
    row["ilu_over_jacobi_time"] = round(row["cg_ilu"]["itime_s"] / row["cg_jacobi"]["itime_s"], 2)
    lib.lis_matrix_destroy(A)
    return row


def mesh_leg(lib, nodes):
    t0 = time.perf_counter()
    ptr, idx, val = orc.unstructured_mesh(nodes)
    n = len(ptr) - 1
    row = {"nodes": nodes, "nnz": int(ptr[-1]), "generate_s": round(time.perf_counter() - t0, 1)}
    A = lisdrv.make_csr(lib, ptr, idx, val)
    b = lisdrv.matvec(lib, A, np.ones(n))
    row["ilu"] = {"fill0": ilu_times(lib, A, 0, np.random.default_rng(1).uniform(-1, 1, n))}
    for pc in ("jacobi", "ilu"):
        row[f"gmres30_{pc}"] = solve_row(lib, A, b, f"-i gmres -restart 30 -p {pc}")
    lib.lis_matrix_destroy(A)
    return row


REF_CHILD = r'''
import ctypes as C, json, os, sys, time
import numpy as np
sys.path[:0] = [%r, %r]
import lisdrv, orc
from lis_amd import _capi as capi
T = int(sys.argv[1])
ref = lisdrv.open_lib(orc.REF_SO, threads=T)
out = {}
for N in json.loads(sys.argv[2]):
    ptr, idx, val = orc.poisson3d(N, N, N)
    n = len(ptr) - 1
    A = lisdrv.make_csr(ref, ptr, idx, val)
    S = capi.PS()
    ref.lis_solver_create(C.byref(S))
    ref.lis_solver_set_option(b"-p ilu", S)
    S.contents.A = A
    create, destroy = ref.dll.lis_precon_create, ref.dll.lis_precon_destroy
    create.restype, create.argtypes = C.c_int, [capi.PS, C.POINTER(C.c_void_p)]
    destroy.restype, destroy.argtypes = C.c_int, [C.c_void_p]
    walls = []
    for rep in range(3):
        pp = C.c_void_p()
        t0 = time.perf_counter()
        assert create(S, C.byref(pp)) == 0
        walls.append(round(time.perf_counter() - t0, 4))
        destroy(pp)
    out[str(N)] = {"precon_create_wall_s": walls}
    ref.lis_solver_destroy(S); ref.lis_matrix_destroy(A)
print("RESULT " + json.dumps(out), flush=True)
'''


def reference_leg(sizes, threads):
    if not os.path.exists(orc.REF_SO):
        return {"skipped": "oracle/_ref/liblis_ref.so is not built here"}
    out = {"what": "wall time of the reference's lis_precon_create with -p ilu (symbolic + numerical) on the host cores, three calls; at T threads it factorises T independent row blocks"}
    for T in threads:
        src = REF_CHILD % (ROOT, os.path.join(ROOT, "tests"))
        res = subprocess.run([sys.executable, "-c", src, str(T), json.dumps(sizes)], capture_output=True, text=True, env=dict(os.environ, OMP_NUM_THREADS=str(T)), timeout=900)
        lines = [line for line in res.stdout.splitlines() if line.startswith("RESULT ")]
        out["T%d" % T] = json.loads(lines[-1][7:]) if res.returncode == 0 and lines else {"failed": res.stderr[-500:]}
    return out


def main():
    args = sys.argv[1:]
    mesh, threads = 2000000, [1, 16]
    if "--mesh" in args:
        k = args.index("--mesh"); mesh = int(args[k + 1]); del args[k:k + 2]
    if "--ref-threads" in args:
        k = args.index("--ref-threads"); threads = [int(t) for t in args[k + 1].split(",") if t]; del args[k:k + 2]
    sizes = [int(a) for a in args] or [128, 256]
    reference = reference_leg(sizes, threads) if threads else {"skipped": "no thread count given"}      # before the GPU is opened: children on the host cores only
    lib = lis_amd.load()
    assert lib.initialize([]) == 0
    lib.dll.lis_amd_set_residency(1)
    name = (C.c_char * 128)()
    lib.dll.liship_device_name(name, 128)
    doc = {"tool": "tools/ilu_probe.py", "device": name.value.decode(), "cases": [probe(lib, N, (0, 1)) for N in sizes],
           "reference": reference}
    if mesh > 0:
        doc["mesh"] = mesh_leg(lib, mesh)
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
