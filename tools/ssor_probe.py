"""SSOR preconditioner (-p ssor) on 7-point Poisson N^3: schedule, psolve time against the launch + bandwidth model, and CG + SSOR
against CG + Jacobi.  Prints ONE JSON object (profiles/ssor_probe.json holds a run on an MI355X).
    python tools/ssor_probe.py [N ...]        (default: 128 256)
Model of one psolve: launches x 1.7 us (a dependent kernel boundary on one stream) + bytes / 6 TB/s, bytes from the level-ordered
layout (per sweep: row ids + term offsets, 12 B per term, b / x / wd per row; gathers of x counted as cache hits)."""
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

BOUNDARY_US, HBM_BPS = 1.7, 6.0e12


def probe(lib, N):
    dll = lib.dll
    ptr, idx, val = orc.poisson3d(N, N, N)
    n = len(ptr) - 1
    b = lisdrv.matvec(lib, A0 := lisdrv.make_csr(lib, ptr, idx, val), np.ones(n))
    lib.lis_matrix_destroy(A0)
    row = {"N": N, "n": n}
    for pc in ("jacobi", "ssor"):
        A = lisdrv.make_csr(lib, ptr, idx, val)
        lisdrv.solve(lib, A, b, f"-i cg -p {pc} -maxiter 1")            # plan, split, schedule (not timed below)
        t0 = time.perf_counter()
        out = lisdrv.solve(lib, A, b, f"-i cg -p {pc} -tol 1e-10 -maxiter 5000")
        wall = time.perf_counter() - t0
        row[f"cg_{pc}"] = {"iter": out["iter"], "status": out["status"], "resid": out["resid"], "solve_s": round(out["itime"], 4),
                           "wall_s": round(wall, 4), "it_per_s": round(out["iter"] / out["itime"], 1)}
        if pc == "ssor":
            blk, lf, lb, la = C.c_int(), C.c_int(), C.c_int(), C.c_int()
            dll.lis_amd_last_solve_ssor(C.byref(blk), C.byref(lf), C.byref(lb), C.byref(la))
            info = (C.c_double * 4)()
            assert dll.lis_amd_ssor_schedule_info(A, info) == 0
            reps = 60
            ms = (C.c_double * reps)()
            vb, vx = lisdrv.new_vector(lib, A, np.random.default_rng(1).uniform(-1, 1, n)), lisdrv.new_vector(lib, A)
            assert dll.lis_amd_ssor_psolve_times(A, vb, vx, reps, ms) == 0
            lib.lis_vector_destroy(vb)
            lib.lis_vector_destroy(vx)
            t = np.array(ms[10:])                                          # the first ten: warm-up
            med = float(np.median(t))
            launch_ms, bytes_ms = la.value * BOUNDARY_US * 1e-3, info[1] / HBM_BPS * 1e3
            row["schedule"] = {"blocks": blk.value, "levels_fwd": lf.value, "levels_bwd": lb.value, "launches_per_psolve": la.value,
                               "bytes_per_psolve": int(info[1]), "build_s": round(info[0], 4)}
            row["psolve"] = {"median_ms": round(med, 4), "p10_ms": round(float(np.percentile(t, 10)), 4), "p90_ms": round(float(np.percentile(t, 90)), 4),
                             "samples": len(t), "model_ms": round(launch_ms + bytes_ms, 4), "model_launch_ms": round(launch_ms, 4),
                             "model_bytes_ms": round(bytes_ms, 4), "ratio": round(med / (launch_ms + bytes_ms), 3),
                             "us_per_launch_if_bytes_at_6TBps": round((med - bytes_ms) * 1e3 / la.value, 3)}
        lib.lis_matrix_destroy(A)
    row["ssor_over_jacobi_time"] = round(row["cg_ssor"]["solve_s"] / row["cg_jacobi"]["solve_s"], 3)
    return row


def main():
    sizes = [int(a) for a in sys.argv[1:]] or [128, 256]
    lib = lis_amd.load()
    assert lib.initialize([]) == 0
    lib.dll.lis_amd_set_residency(1)
    rows = [probe(lib, N) for N in sizes]
    print(json.dumps({"tool": "tools/ssor_probe.py", "model": {"boundary_us": BOUNDARY_US, "hbm_TBps": HBM_BPS / 1e12}, "cases": rows}, indent=1))


if __name__ == "__main__":
    main()
