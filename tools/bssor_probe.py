"""Block SSOR on BSR storage (-p ssor on a BSR matrix): what it costs and what it buys.  Prints ONE JSON object (a run on an MI355X belongs in
profiles/bssor_probe.json).
    python tools/bssor_probe.py [--fem G] [--queen mini|none] [--stencil N]       (default: 64, mini, 256; 0 / none leaves a case out)
Cases, each as the CSR matrix and as the BSR matrix lis_matrix_convert makes of it:
  fem        the Queen-class stand-in orc.fem3(G): 3 unknowns per node of a G^3 grid, 27-node connectivity; BSR 3 x 3
  queen      queen_class "mini" (tests/golden/gen_queen_class.c through tests/queen_class.py); BSR 3 x 3
  stencil    the 7-point stencil on N^3; BSR 2 x 2
Per case, for the point graph (CSR) and the block graph (BSR):
  schedule   levels and launches of the two sweeps of a psolve, bytes one psolve streams (lisi_sweep_bytes_places: the level-ordered layout)
  psolve     device-event times (lis_amd_ssor_psolve_times) beside the model of DESIGN 8a -- launches x 1.7 us + bytes / 6 TB/s -- as a ratio;
             the first ten samples are warm-up; median, 10th and 90th percentile of the rest
  product    lis_matvec on the same (split) matrix: wall time of a batch between two lis_amd_synchronize divided by its length
and for the BSR matrix GMRES(30) and CG at tol 1e-12 with -p ssor against -p none, -p ilu and -p bjacobi: iterations, seconds."""
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
REPS, BATCH = 40, 50


def product_ms(lib, A, x):
    vx, vy = lisdrv.new_vector(lib, A, x), lisdrv.new_vector(lib, A)
    samples = []
    for rep in range(6):                                               # the first batch is warm-up
        lib.dll.lis_amd_synchronize()
        t0 = time.perf_counter()
        for _ in range(BATCH):
            assert lib.lis_matvec(A, vx, vy) == 0
        lib.dll.lis_amd_synchronize()
        samples.append((time.perf_counter() - t0) * 1e3 / BATCH)
    lib.lis_vector_destroy(vx)
    lib.lis_vector_destroy(vy)
    t = np.array(samples[1:])
    return {"median_ms": round(float(np.median(t)), 4), "min_ms": round(float(t.min()), 4), "max_ms": round(float(t.max()), 4), "batches": len(t), "batch": BATCH}


def ssor_side(lib, A, b, rhs):
    """schedule, psolve and product of a matrix after its first -p ssor solve (which converts nothing: A is what the caller made)"""
    dll = lib.dll
    out = lisdrv.solve(lib, A, b, "-i cg -p ssor -maxiter 1")
    assert out["err"] == 0, out["err"]
    blk, lf, lb, la = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    dll.lis_amd_last_solve_ssor(C.byref(blk), C.byref(lf), C.byref(lb), C.byref(la))
    info = (C.c_double * 4)()
    assert dll.lis_amd_ssor_schedule_info(A, info) == 0
    terms = []
    for w in (0, 1):
        si = (C.c_int * 6)()
        assert dll.lis_amd_ssor_sweep_info(A, w, si) == 0
        terms.append(si[5])
    ms = (C.c_double * REPS)()
    vb, vx = lisdrv.new_vector(lib, A, rhs), lisdrv.new_vector(lib, A)
    assert dll.lis_amd_ssor_psolve_times(A, vb, vx, REPS, ms) == 0
    lib.lis_vector_destroy(vb)
    lib.lis_vector_destroy(vx)
    t = np.array(ms[10:])
    med = float(np.median(t))
    launch_ms, bytes_ms = la.value * BOUNDARY_US * 1e-3, info[1] / HBM_BPS * 1e3
    return {"block": dll.lis_amd_last_solve_ssor_block(), "schedule_blocks": blk.value, "levels_fwd": lf.value, "levels_bwd": lb.value,
            "launches_per_psolve": la.value, "terms_fwd": terms[0], "terms_bwd": terms[1], "bytes_per_psolve": int(info[1]), "build_s": round(info[0], 4),
            "psolve": {"median_ms": round(med, 4), "p10_ms": round(float(np.percentile(t, 10)), 4), "p90_ms": round(float(np.percentile(t, 90)), 4),
                       "samples": len(t), "model_ms": round(launch_ms + bytes_ms, 4), "model_launch_ms": round(launch_ms, 4),
                       "model_bytes_ms": round(bytes_ms, 4), "ratio": round(med / (launch_ms + bytes_ms), 3)},
            "product": product_ms(lib, A, rhs)}


def solve_row(lib, A, b, opts):
    first = lisdrv.solve(lib, A, b, opts + " -maxiter 1")               # plans, schedules, WD, the first factorisation (not timed below)
    if first["err"] != 0:
        return {"err": first["err"]}
    t0 = time.perf_counter()
    out = lisdrv.solve(lib, A, b, opts + " -tol 1e-12 -maxiter 5000")
    wall = time.perf_counter() - t0
    return {"iter": out["iter"], "status": out["status"], "resid": out["resid"], "itime_s": round(out["itime"], 4),
            "iterations_per_s": round(out["iter"] / out["itime"], 1) if out["itime"] > 0 else None, "wall_s_with_precon_create": round(wall, 4)}


def note(text):
    print("bssor_probe: " + text, file=sys.stderr, flush=True)


def probe(lib, ptr, idx, val, bn):
    n = len(ptr) - 1
    note("n = %d, nnz = %d, blocks of %d" % (n, int(ptr[-1]), bn))
    rhs = np.random.default_rng(1).uniform(-1, 1, n)
    Ac = lisdrv.make_csr(lib, ptr, idx, val)
    b = lisdrv.matvec(lib, Ac, np.ones(n))
    A = lisdrv.convert(lib, Ac, "bsr", bn, bn)
    row = {"n": n, "nnz": int(ptr[-1]), "bn": bn, "block_rows": A.contents.nr, "blocks": A.contents.bnnz, "solves": {}}
    for solver in ("-i gmres -restart 30", "-i cg"):                    # unsplit first: -p ilu refuses a split matrix
        tag = solver.split()[1]
        row["solves"][tag + "_none"] = solve_row(lib, A, b, solver + " -p none")
        row["solves"][tag + "_ilu"] = solve_row(lib, A, b, solver + " -p ilu")
    for solver in ("-i gmres -restart 30", "-i cg"):
        row["solves"][solver.split()[1] + "_bjacobi"] = solve_row(lib, A, b, solver + " -p bjacobi")
    note("solves without SSOR done")
    row["point"] = ssor_side(lib, Ac, b, rhs)
    note("point sweeps done")
    row["blocked"] = ssor_side(lib, A, b, rhs)
    assert row["point"]["block"] == 1 and row["blocked"]["block"] == bn
    note("block sweeps done")
    for solver in ("-i gmres -restart 30", "-i cg"):
        row["solves"][solver.split()[1] + "_ssor"] = solve_row(lib, A, b, solver + " -p ssor")
        row["solves"][solver.split()[1] + "_ssor_csr"] = solve_row(lib, Ac, b, solver + " -p ssor")
    row["block_over_point_psolve"] = round(row["blocked"]["psolve"]["median_ms"] / row["point"]["psolve"]["median_ms"], 3)
    lib.lis_matrix_destroy(A)
    lib.lis_matrix_destroy(Ac)
    return row


def main():
    args = sys.argv[1:]
    opt = {"--fem": "64", "--queen": "mini", "--stencil": "256"}
    for k in list(opt):
        if k in args:
            at = args.index(k); opt[k] = args[at + 1]; del args[at:at + 2]
    assert not args, args
    lib = lis_amd.load()
    assert lis_amd.gpu_available(), "no HIP device: nothing here runs without one"
    assert lib.initialize([]) == 0
    lib.dll.lis_amd_set_residency(1)
    name = (C.c_char * 128)()
    lib.dll.liship_device_name(name, 128)
    doc = {"tool": "tools/bssor_probe.py", "device": name.value.decode(), "model": {"boundary_us": BOUNDARY_US, "hbm_TBps": HBM_BPS / 1e12},
           "sizes": {k[2:]: v for k, v in opt.items()}}
    if int(opt["--fem"]) > 0:
        G = int(opt["--fem"])
        doc["fem"] = dict(G=G, **probe(lib, *orc.fem3(G, 3)[:3], 3))
    if opt["--queen"] != "none":
        import ilu_cases
        import queen_class
        path, rows, _ = queen_class.generate(opt["--queen"])
        try:
            ptr, idx, val = ilu_cases.read_mtx(path)
        finally:
            os.unlink(path)
        doc["queen"] = dict(case=opt["--queen"], **probe(lib, ptr, idx, val, 3))
    if int(opt["--stencil"]) > 0:
        N = int(opt["--stencil"])
        doc["stencil"] = dict(N=N, **probe(lib, *orc.poisson3d(N, N, N), 2))
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
