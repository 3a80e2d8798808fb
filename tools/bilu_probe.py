"""Block ILU(k) on BSR storage (-p ilu on a BSR matrix): what it costs and what it buys.  Prints ONE JSON object (a run on an MI355X belongs in
profiles/bilu_probe.json).
    python tools/bilu_probe.py [--fem G] [--queen mini|none] [--fills 0,1]        (default: 64, mini, fill 0 and 1; --fem 0 leaves the case out)
Cases, both in BSR 3 x 3 made by lis_matrix_convert from the CSR matrix:
  fem        the Queen-class stand-in orc.fem3(G): 3 unknowns per node of a G^3 grid, 27-node connectivity
  queen      queen_class "mini" (tests/golden/gen_queen_class.c through tests/queen_class.py)
Per case and fill level:
  symbolic_s        host seconds of the symbolic step on the block graph and of the L and U layouts
  levels, launches  forward levels (= those of the factorisation), launches of one factorisation and of one psolve, block rows by workgroup
  factor, psolve    device-event times of the factorisation and of one psolve; product: lis_matvec on the same BSR matrix, wall time of a
                    batch between two lis_amd_synchronize divided by its length (the yardstick beside the psolve)
  gmres30_*         GMRES(30) at tol 1e-12 with -p ilu against -p none and -p bjacobi (last: it leaves A split): iterations, iterations / s
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
BATCH = 50


def stats(ms):
    t = np.array(ms[10:])
    return {"median_ms": round(float(np.median(t)), 4), "p10_ms": round(float(np.percentile(t, 10)), 4), "p90_ms": round(float(np.percentile(t, 90)), 4),
            "samples": len(t)}


def ilu_times(lib, A, fill, rhs):
    dll = lib.dll
    sizes = (C.c_int * 3)()
    t0 = time.perf_counter()
    assert dll.lis_amd_ilu_factor(A, fill, sizes) == 0
    first_s = time.perf_counter() - t0
    info, fi = (C.c_double * 6)(), (C.c_int * 6)()
    assert dll.lis_amd_ilu_info(A, fill, info) == 0 and dll.lis_amd_ilu_factor_info(A, fill, fi) == 0
    fms, pms = (C.c_double * REPS)(), (C.c_double * REPS)()
    vb, vx = lisdrv.new_vector(lib, A, rhs), lisdrv.new_vector(lib, A)
    assert dll.lis_amd_ilu_times(A, fill, vb, vx, REPS, fms, pms) == 0
    lib.lis_vector_destroy(vb)
    lib.lis_vector_destroy(vx)
    return {"symbolic_s": round(info[0], 4), "first_factor_wall_s": round(first_s, 4), "block_rows": sizes[0], "blocks_L": sizes[1], "blocks_U": sizes[2],
            "levels": int(info[2]), "factor_launches": int(info[3]), "launches_per_psolve": int(info[4]), "bytes_per_psolve": int(info[5]),
            "levels_on_own_launch": fi[2], "block_rows_by_workgroup": fi[3] + fi[4], "factor": stats(list(fms)), "psolve": stats(list(pms))}


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


def solve_row(lib, A, b, opts):
    lisdrv.solve(lib, A, b, opts + " -maxiter 1")                       # plans, schedules, the first factorisation (not timed below)
    t0 = time.perf_counter()
    out = lisdrv.solve(lib, A, b, opts + " -tol 1e-12 -maxiter 5000")
    wall = time.perf_counter() - t0
    return {"iter": out["iter"], "status": out["status"], "resid": out["resid"], "itime_s": round(out["itime"], 4),
            "iterations_per_s": round(out["iter"] / out["itime"], 1) if out["itime"] > 0 else None, "wall_s_with_precon_create": round(wall, 4)}


def probe(lib, ptr, idx, val, fills):
    n = len(ptr) - 1
    Ac = lisdrv.make_csr(lib, ptr, idx, val)
    A = lisdrv.convert(lib, Ac, "bsr", 3, 3)
    lib.lis_matrix_destroy(Ac)
    b = lisdrv.matvec(lib, A, np.ones(n))
    rhs = np.random.default_rng(1).uniform(-1, 1, n)
    row = {"n": n, "nnz": int(ptr[-1]), "bn": 3, "block_rows": A.contents.nr, "blocks": A.contents.bnnz, "product": product_ms(lib, A, rhs), "ilu": {}}
    for fill in fills:
        row["ilu"]["fill%d" % fill] = ilu_times(lib, A, fill, rhs)
        row["ilu"]["fill%d" % fill]["psolve_over_product"] = round(row["ilu"]["fill%d" % fill]["psolve"]["median_ms"] / row["product"]["median_ms"], 2)
    row["gmres30_none"] = solve_row(lib, A, b, "-i gmres -restart 30 -p none")
    for fill in fills:
        row["gmres30_ilu_fill%d" % fill] = solve_row(lib, A, b, "-i gmres -restart 30 -p ilu -ilu_fill %d" % fill)
        assert lib.dll.lis_amd_last_solve_ilu_block() == 3
    row["gmres30_bjacobi"] = solve_row(lib, A, b, "-i gmres -restart 30 -p bjacobi")          # last: it leaves A split
    lib.lis_matrix_destroy(A)
    return row


def main():
    args = sys.argv[1:]
    opt = {"--fem": "64", "--queen": "mini", "--fills": "0,1"}
    for k in list(opt):
        if k in args:
            at = args.index(k); opt[k] = args[at + 1]; del args[at:at + 2]
    assert not args, args
    G, fills = int(opt["--fem"]), [int(t) for t in opt["--fills"].split(",") if t]
    lib = lis_amd.load()
    assert lis_amd.gpu_available(), "no HIP device: nothing here runs without one"
    assert lib.initialize([]) == 0
    lib.dll.lis_amd_set_residency(1)
    name = (C.c_char * 128)()
    lib.dll.liship_device_name(name, 128)
    doc = {"tool": "tools/bilu_probe.py", "device": name.value.decode()}
    if G > 0:
        doc["fem"] = dict(G=G, **probe(lib, *orc.fem3(G, 3)[:3], fills))
    if opt["--queen"] != "none":
        import ilu_cases
        import queen_class
        path, rows, _ = queen_class.generate(opt["--queen"])
        try:
            ptr, idx, val = ilu_cases.read_mtx(path)
        finally:
            os.unlink(path)
        doc["queen"] = dict(case=opt["--queen"], **probe(lib, ptr, idx, val, fills))
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
