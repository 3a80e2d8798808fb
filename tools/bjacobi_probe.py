"""Block Jacobi preconditioner (-p bjacobi): what it costs and what it buys.  Prints ONE JSON object (a run on an MI355X belongs in profiles/bjacobi_probe.json).
    python tools/bjacobi_probe.py [--stencil N] [--fem G] [--blocks 2,3,4]        (default: 256, 64, blocks 2,3,4; 0 leaves a case out)
Cases:
  stencil    the 7-point Poisson matrix on N^3 in BSR storage, block sizes 2, 3, 4 (-storage bsr -storage_block k)
  fem        a 3-dof mesh of the Queen class's shape (orc.fem3(G): 27-node connectivity, 3 unknowns per node), 3 x 3 blocks
Per case and block size:
  inverse    the inversion of the nr diagonal blocks (kernel alone, device events): 16 * bn^2 B per block read and written
  psolve     z = WD r: 8 * bn B of WD per row + 16 B of vectors per row
  jacobi     the Jacobi psolve z = r .* dinv of the same length in the same process, 24 B per row: the yardstick.  explanation_owed
             when the psolve's time per byte exceeds 1.25 x that kernel's
  cg / gmres30   -p bjacobi against -p jacobi on the same BSR matrix (split by the first -p bjacobi solve): iterations, iterations / s, seconds
  precon_create_s   per solve, wall time less the iterations' time: with the inverse cached on the HBM copy, a -p bjacobi solve still allocates
             the host WD and copies its nr * bn^2 doubles home (wd_home_bytes); the -p jacobi rows beside it show what a solve costs without that
Times: the first ten samples of every device-event series are warm-up; median, 10th and 90th percentile of the rest."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import lis_amd  # noqa: E402
import lisdrv  # noqa: E402
import orc  # noqa: E402

REPS = 40


def stats(ms, nbytes):
    t = np.array(ms[10:])
    med = float(np.median(t))
    return {"median_ms": round(med, 4), "p10_ms": round(float(np.percentile(t, 10)), 4), "p90_ms": round(float(np.percentile(t, 90)), 4),
            "samples": len(t), "bytes": int(nbytes), "TB_per_s": round(nbytes / (med * 1e-3) / 1e12, 3) if med > 0 else None}


def solve_row(lib, A, b, opts):
    lisdrv.solve(lib, A, b, opts + " -maxiter 1")                       # conversion, split, plans, the inverse (not timed below)
    t0 = time.perf_counter()
    out = lisdrv.solve(lib, A, b, opts + " -tol 1e-12 -maxiter 5000")
    wall = time.perf_counter() - t0
    return {"iter": out["iter"], "status": out["status"], "resid": out["resid"], "itime_s": round(out["itime"], 4),
            "iterations_per_s": round(out["iter"] / out["itime"], 1) if out["itime"] > 0 else None, "wall_s_with_precon_create": round(wall, 4),
            "precon_create_s": round(wall - out["itime"], 4)}


def probe(lib, ptr, idx, val, bn):
    n = len(ptr) - 1
    A = lisdrv.make_csr(lib, ptr, idx, val)
    b = lisdrv.matvec(lib, A, np.ones(n))
    store = f"-storage bsr -storage_block {bn}"
    row = {"bn": bn, "n": n, "nr": (n + bn - 1) // bn, "wd_home_bytes": 8 * bn * bn * ((n + bn - 1) // bn)}
    row["cg_bjacobi"] = solve_row(lib, A, b, f"-i cg -p bjacobi {store}")          # leaves A BSR and split: the other solves run on the same matrix
    row["cg_jacobi"] = solve_row(lib, A, b, f"-i cg -p jacobi {store}")
    row["gmres30_bjacobi"] = solve_row(lib, A, b, f"-i gmres -restart 30 -p bjacobi {store}")
    row["gmres30_jacobi"] = solve_row(lib, A, b, f"-i gmres -restart 30 -p jacobi {store}")
    ims, pms, jms = ((C.c_double * REPS)() for _ in range(3))
    vb, vx = lisdrv.new_vector(lib, A, np.random.default_rng(1).uniform(-1, 1, n)), lisdrv.new_vector(lib, A)
    assert lib.dll.lis_amd_bjacobi_times(A, vb, vx, REPS, ims, pms, jms) == 0
    lib.lis_vector_destroy(vb)
    lib.lis_vector_destroy(vx)
    row["inverse"] = stats(list(ims), 16.0 * bn * bn * row["nr"])
    row["psolve"] = stats(list(pms), (8.0 * bn + 16.0) * n)
    row["jacobi_psolve_same_process"] = stats(list(jms), 24.0 * n)
    per_byte = (row["psolve"]["median_ms"] / row["psolve"]["bytes"]) / (row["jacobi_psolve_same_process"]["median_ms"] / row["jacobi_psolve_same_process"]["bytes"])
    row["psolve_over_jacobi_time_per_byte"] = round(per_byte, 3)
    row["explanation_owed"] = bool(per_byte > 1.25)
    lib.lis_matrix_destroy(A)
    return row


def main():
    args = sys.argv[1:]
    opt = {"--stencil": "256", "--fem": "64", "--blocks": "2,3,4"}
    for k in list(opt):
        if k in args:
            at = args.index(k); opt[k] = args[at + 1]; del args[at:at + 2]
    assert not args, args
    N, G, blocks = int(opt["--stencil"]), int(opt["--fem"]), [int(t) for t in opt["--blocks"].split(",") if t]
    lib = lis_amd.load()
    assert lis_amd.gpu_available(), "no HIP device: nothing here runs without one"
    assert lib.initialize([]) == 0
    lib.dll.lis_amd_set_residency(1)
    name = (C.c_char * 128)()
    lib.dll.liship_device_name(name, 128)
    doc = {"tool": "tools/bjacobi_probe.py", "device": name.value.decode()}
    if N > 0:
        ptr, idx, val = orc.poisson3d(N, N, N)
        doc["stencil"] = {"N": N, "blocks": [probe(lib, ptr, idx, val, bn) for bn in blocks]}
    if G > 0:
        ptr, idx, val = orc.fem3(G, 3)[:3]
        doc["fem"] = {"G": G, "nnz": int(ptr[-1]), "blocks": [probe(lib, ptr, idx, val, 3)]}
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
