"""SAINV and I+S (-p sainv, -p is): what one application costs and what the preconditioner buys.  Prints ONE JSON object (a run on an MI355X
belongs in profiles/sainv_probe.json).
    python tools/sainv_probe.py [N ...] [--drops 0.05,0.01]        (default: 128 256; the default drop, and 0.01 for a factor with fill-in)
Per 7-point Poisson matrix N^3 and drop tolerance:
  build      host seconds of the factor's build (lis_amd_sainv_info), nnz(W), nnz(Z)
  psolve     ms of one M^-1 b by device events, the bytes it streams, and that time over bytes / the box's streaming yardstick
             (liship_stream_yardstick, 13 reads : 1 write, measured in the same process)
  beside it  one lis_matvec of A and one SSOR psolve (lis_amd_ssor_psolve_times) in the same process, with the same figures, and one I+S psolve
  solves     CG to tol 1e-12 with -p none | jacobi | sainv | ssor: iterations, the library's itime, the wall time with the preconditioner's creation
Times: the first ten samples of every device-event series are warm-up; median, 10th and 90th percentile of the 30 that follow."""
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
from lis_amd import DeviceArray as DA, check  # noqa: E402

REPS = 40


def stats(ms, nbytes=None, yard=None):
    t = np.array(ms[10:])
    med = float(np.median(t))
    out = {"median_ms": round(med, 4), "p10_ms": round(float(np.percentile(t, 10)), 4), "p90_ms": round(float(np.percentile(t, 90)), 4), "samples": len(t)}
    if nbytes is not None:
        out.update(bytes=int(nbytes), TB_per_s=round(nbytes / (med * 1e-3) / 1e12, 3) if med > 0 else None)
        if yard:
            out["time_over_bytes_over_yardstick"] = round(med / (nbytes / (yard * 1e12) * 1e3), 3)
    return out


class Timer:
    """device events on a stream"""
    def __init__(self, lib, stream):
        self.lib, self.stream, self.t = lib, stream, C.c_void_p()
        check(lib.liship_timer_create(C.byref(self.t)))

    def time(self, fn):
        ms = C.c_float()
        check(self.lib.liship_timer_start(self.t, self.stream))
        fn()
        check(self.lib.liship_timer_stop(self.t, self.stream))
        check(self.lib.liship_stream_synchronize(self.stream))
        check(self.lib.liship_timer_elapsed_ms(self.t, C.byref(ms)))
        return ms.value


def yardstick(lib):
    n = 512 * 65536
    timer = Timer(lib, None)
    src, dst = DA.zeros(13 * n, np.float64), DA.zeros(n, np.float64)
    ms = [timer.time(lambda: check(lib.liship_stream_yardstick(13, n, src.ptr, dst.ptr, 0, None))) for _ in range(REPS)]
    src.free()
    dst.free()
    return stats(ms, 14 * 8 * n)


def solve_row(lib, A, b, opts):
    lisdrv.solve(lib, A, b, opts + " -maxiter 1")                       # plans, factor, schedules (not timed below)
    t0 = time.perf_counter()
    out = lisdrv.solve(lib, A, b, opts + " -tol 1e-12 -maxiter 5000")
    wall = time.perf_counter() - t0
    return {"iter": out["iter"], "status": out["status"], "resid": out["resid"], "itime_s": round(out["itime"], 4), "wall_s": round(wall, 4)}


def probe(lib, N, drops, yard):
    dll = lib.dll
    ptr, idx, val = orc.poisson3d(N, N, N)
    n, nnz = len(ptr) - 1, len(idx)
    A = lisdrv.make_csr(lib, ptr, idx, val)
    b = lisdrv.matvec(lib, A, np.ones(n))
    rhs = np.random.default_rng(1).uniform(-1, 1, n)
    row = {"N": N, "n": n, "nnz": nnz, "sainv": {}}
    vb, vx = lisdrv.new_vector(lib, A, rhs), lisdrv.new_vector(lib, A)
    dll.lis_amd_stream.restype = C.c_void_p
    timer = Timer(lib, dll.lis_amd_stream())
    ms = [timer.time(lambda: lib.lis_matvec(A, vb, vx)) for _ in range(REPS)]
    row["matvec"] = stats(ms, 16 * n, yard)           # x read, y written: what the marching form of this constant-coefficient matrix moves, its values held as records
    for drop in drops:
        info, pms, build = (C.c_double * 6)(), (C.c_double * REPS)(), C.c_double()
        t0 = time.perf_counter()
        assert dll.lis_amd_sainv_info(A, drop, info) == 0
        first = time.perf_counter() - t0
        assert dll.lis_amd_sainv_times(A, drop, vb, vx, REPS, C.byref(build), pms) == 0
        r = {"drop": drop, "build_s": round(info[0], 3), "first_use_wall_s": round(first, 3), "nnz_W": int(info[1]), "nnz_Z": int(info[2]),
             "launches_per_psolve": int(info[4]), "psolve": stats(list(pms), info[3], yard)}
        r["psolve_over_matvec"] = round(r["psolve"]["median_ms"] / row["matvec"]["median_ms"], 3)
        r["cg_sainv"] = solve_row(lib, A, b, "-i cg -p sainv -sainv_drop %r" % drop)
        row["sainv"]["drop_%g" % drop] = r
    for pc in ("none", "jacobi", "ssor"):                                  # ssor last: it leaves A split
        row[f"cg_{pc}"] = solve_row(lib, A, b, f"-i cg -p {pc}")
    sms = (C.c_double * REPS)()
    assert dll.lis_amd_ssor_psolve_times(A, vb, vx, REPS, sms) == 0
    row["ssor_psolve"] = stats(list(sms))
    u_nnz = int(np.count_nonzero(idx > np.repeat(np.arange(n, dtype=idx.dtype), np.diff(ptr))))      # rows of U hold up to 3 entries here: m + 1 = 4 keeps them all
    ims = [timer.time(lambda: dll.lis_amd_is_psolve(A, 1.0, 3, vb, vx, 0)) for _ in range(REPS)]     # (A is split: what -p is asks for)
    row["is_psolve"] = stats(ims, 12 * u_nnz + 4 * (n + 1) + 16 * n, yard)
    first_drop = row["sainv"]["drop_%g" % drops[0]]
    row["sainv_over_ssor_psolve"] = round(first_drop["psolve"]["median_ms"] / row["ssor_psolve"]["median_ms"], 4)
    row["cg_time_sainv_over_jacobi"] = round(first_drop["cg_sainv"]["itime_s"] / row["cg_jacobi"]["itime_s"], 3)
    lib.lis_vector_destroy(vb)
    lib.lis_vector_destroy(vx)
    lib.lis_matrix_destroy(A)
    return row


def main():
    args = sys.argv[1:]
    drops = [0.05, 0.01]
    if "--drops" in args:
        k = args.index("--drops"); drops = [float(t) for t in args[k + 1].split(",") if t]; del args[k:k + 2]
    sizes = [int(a) for a in args] or [128, 256]
    lib = lis_amd.load()
    if not lis_amd.gpu_available():
        raise SystemExit("sainv_probe: no HIP device -- nothing here is measured without one")
    assert lib.initialize([]) == 0
    lib.dll.lis_amd_set_residency(1)
    name = (C.c_char * 128)()
    lib.dll.liship_device_name(name, 128)
    yard = yardstick(lib)
    doc = {"tool": "tools/sainv_probe.py", "device": name.value.decode(), "yardstick_13_reads_1_write": yard,
           "cases": [probe(lib, N, drops, yard["TB_per_s"]) for N in sizes]}
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
