"""-f quad on the device: what the double-double kernels of kernels/quad.hip cost beside their double forms.  Writes profiles/quad_probe.json and prints it.
    python tools/quad_probe.py [--grid 256]
One process, the 7-point Poisson matrix on grid^3 as plain CSR arrays (8 B values and 4 B indices streamed: no index codes, row patterns or value records):
yardstick   the box's streaming rate (liship_stream_yardstick, 13 reads : 1 write)
spmv        liship_spmv_csr_dd_f64 beside liship_spmv_csr_f64 (the row-gather product) on the same arrays; bytes = the matrix once + x and y once per part
vector      axpy, xpay, axpyz, muld (Jacobi's psolve) and the dot beside liship_axpy_f64, _xpay_, _axpyz_, _pmul_ and _dot_
solve       lis_solve -i cg -p jacobi: -f quad (switch on, -tol 1e-25) beside the unfused double loop (-tol 1e-12): iterations, wall seconds, iterations / s
Kernel times by device events: 3 warm-up samples, then the median of 10 with the 10th / 90th percentile."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import lis_amd  # noqa: E402
import lisdrv  # noqa: E402
import vbr_probe  # noqa: E402
from lis_amd import DeviceArray as DA, _capi as capi, check  # noqa: E402

WARM, REPS = 3, 13
I32, F64 = np.int32, np.float64


def stats(ms, nbytes=None):
    t = np.array(ms[WARM:])
    out = {"median_ms": round(float(np.median(t)), 4), "p10_ms": round(float(np.percentile(t, 10)), 4), "p90_ms": round(float(np.percentile(t, 90)), 4), "samples": len(t)}
    if nbytes:
        out["bytes"] = int(nbytes)
        out["TB_per_s"] = round(nbytes / (out["median_ms"] * 1e-3) / 1e12, 3)
    return out


def beside(dd, dbl):
    return {"quad": dd, "double": dbl, "quad_over_double_time": round(dd["median_ms"] / dbl["median_ms"], 2)}


def main():
    args = sys.argv[1:]
    N = int(args[args.index("--grid") + 1]) if "--grid" in args else 256
    lib = lis_amd.load()
    if not lis_amd.gpu_available():
        raise SystemExit("quad_probe: no HIP device -- nothing here is measured without one")
    assert lib.initialize([]) == 0
    dll = lib.dll
    dll.lis_amd_matrix_poisson3d.argtypes = [capi.PM, C.c_int, C.c_int, C.c_int, C.c_int]
    name = (C.c_char * 128)()
    dll.liship_device_name(name, 128)
    for f in (lib.liship_spmv_csr_set_index_codes, lib.liship_spmv_csr_set_row_patterns, lib.liship_spmv_csr_set_row_values):
        check(f(0))
    timer = vbr_probe.Timer(lib, None)
    yard = vbr_probe.yardstick(lib)
    doc = {"tool": "tools/quad_probe.py", "device": name.value.decode(), "grid": N, "yardstick_13_reads_1_write": yard}

    n = N ** 3
    nnz = int(lib.liship_poisson3d_nnz(N, N, N, 0, n))
    ptr, idx, val = DA(n + 1, I32), DA(nnz, I32), DA(nnz, F64)
    check(lib.liship_poisson3d_csr(N, N, N, 0, n, 1, ptr.ptr, idx.ptr, val.ptr, None))
    rng = np.random.default_rng(0)
    v = [DA.from_host(rng.uniform(-1, 1, n)) for _ in range(2)] + [DA.zeros(n, F64) for _ in range(4)]
    xh, xl, yh, yl, zh, zl = (a.ptr for a in v)
    check(lib.liship_memcpy_d2d(yh, xh, 8 * n, None))
    res, work = DA.zeros(4, F64), DA(max(lib.liship_reduce_work_bytes(), lib.liship_dot_dd_work_bytes()) // 8, F64)
    run = lambda fn: [timer.time(lambda: check(fn())) for _ in range(REPS)]      # noqa: E731

    plan = C.c_void_p()
    check(lib.liship_csr_plan_create(C.byref(plan), n, ptr.ptr, None))
    mat = 12 * nnz + 4 * (n + 1)
    doc["spmv"] = beside(stats(run(lambda: lib.liship_spmv_csr_dd_f64(n, ptr.ptr, idx.ptr, val.ptr, xh, xl, zh, zl, None)), mat + 32 * n),
                         stats(run(lambda: lib.liship_spmv_csr_f64(plan, ptr.ptr, idx.ptr, val.ptr, xh, zh, None)), mat + 16 * n))
    check(lib.liship_csr_plan_destroy(plan))
    a = (0.75, 2.0 ** -56)
    doc["vector"] = {
        "axpy": beside(stats(run(lambda: lib.liship_axpy_dd_f64(n, a[0] * 1e-3, a[1] * 1e-3, xh, xl, yh, yl, None)), 48 * n),
                       stats(run(lambda: lib.liship_axpy_f64(n, 1e-3, xh, zh, None)), 24 * n)),
        "xpay": beside(stats(run(lambda: lib.liship_xpay_dd_f64(n, xh, xl, a[0], a[1], yh, yl, None)), 48 * n),
                       stats(run(lambda: lib.liship_xpay_f64(n, xh, 0.75, zh, None)), 24 * n)),
        "axpyz": beside(stats(run(lambda: lib.liship_axpyz_dd_f64(n, a[0], a[1], xh, xl, yh, yl, zh, zl, None)), 48 * n),
                        stats(run(lambda: lib.liship_axpyz_f64(n, 0.75, xh, yh, zh, None)), 24 * n)),
        "muld_jacobi": beside(stats(run(lambda: lib.liship_muld_dd_f64(n, xh, xl, yh, zh, zl, None)), 40 * n),
                              stats(run(lambda: lib.liship_pmul_f64(n, xh, yh, zh, None)), 24 * n)),
        "dot": beside(stats(run(lambda: lib.liship_dot_dd_f64(n, xh, xl, yh, yl, res.ptr, work.ptr, None)), 32 * n),
                      stats(run(lambda: lib.liship_dot_f64(n, xh, yh, res.ptr, work.ptr, None)), 16 * n)),
    }
    for d in v + [ptr, idx, val, res, work]:
        d.free()

    A = capi.PM()
    assert lib.lis_matrix_create(capi.LIS_COMM_WORLD, C.byref(A)) == 0 and lib.lis_matrix_set_size(A, 0, n) == 0
    assert dll.lis_amd_matrix_poisson3d(A, N, N, N, 1) == 0
    b = np.ones(n)
    doc["solve"] = {}
    for tag, quad, opts in (("double_unfused", 0, "-i cg -p jacobi -tol 1e-12 -maxiter 5000"), ("quad", 1, "-i cg -p jacobi -f quad -tol 1e-25 -maxiter 5000")):
        dll.lis_amd_set_quad_precision(quad)
        dll.lis_amd_set_loop_mode(2)
        best = None
        for _ in range(2):                                   # the first solve uploads the matrix and builds its plan
            t0 = time.perf_counter()
            r = lisdrv.solve(lib, A, b, opts)
            secs = time.perf_counter() - t0
            best = secs if best is None else min(best, secs)
        assert r["err"] == 0 and r["status"] == 0 and dll.lis_amd_last_solve_quad() == quad
        doc["solve"][tag] = {"options": opts, "iterations": r["iter"], "relative_residual": r["resid"], "lis_solve_itime_s": round(r["itime"], 4),
                             "iterations_per_s": round(r["iter"] / r["itime"], 1), "wall_s_with_vector_setup": round(best, 4)}
    dll.lis_amd_set_quad_precision(0)
    dll.lis_amd_set_loop_mode(0)
    lib.lis_matrix_destroy(A)
    text = json.dumps(doc, indent=1)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "quad_probe.json"), "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
