"""The generalized eigensolvers (lis_gesolve) on an MI355X: what lis_matrix_shift_matrix and an outer iteration of -e grqi cost.  Prints ONE JSON object (a
run belongs in profiles/gesolve_probe.json).
    python tools/gesolve_probe.py [--grid 256] [--inner-tol 1e-6]
The pencil: A = the 7-point Poisson matrix of N^3 generated in HBM with 2 added to its diagonal, B on the same pattern with diagonal 1 and off-diagonals 0.05
(A's values mapped affinely on the device).  Both live in HBM only: no matrix array exists on the host, none crosses the bus.
  in_place   one lis_matrix_shift_matrix that keeps A's layout (rows ascending, one pattern), +sigma and -sigma alternating: the one launch alone
             (liship_csr_shift_matrix_try_f64, device events), the whole call (host clock, stream drained), refresh_ms = whole call - launch: the flag's
             read-back, dropping what hung on the old values and making the plan again (lisd_mat_values_changed)
  rebuilt    the same on a matrix whose rows are NOT in ascending column order (every row merged into new arrays): the three steps alone (try, scan, fill),
             the whole call on a fresh matrix per sample, refresh_ms as above
  bytes      what each form has to stream -- in place: A's and B's indices and values once and A's values back, 32 nnz + 16 n; rebuilt: both matrices twice
             (count, fill) and the result once, 60 nnz + 28 n -- priced at the box's streaming yardstick (liship_stream_yardstick, 13 reads : 1 write, what
             bench.py's box_yardstick measures) taken in the same process: ratio = measured / (bytes / yardstick)
  grqi       ms per outer iteration of -e grqi (lis_esolver_get_time / iterations, 2 iterations after one untimed), the two shifts of an iteration from the
             rows above, and the iteration without them (the difference).  The inner BiCG runs to --inner-tol (given to lis_initialize, as a program's
             command line would)
The reference cannot produce a number at this size: its lis_matrix_shift_matrix goes through two dense n x n copies, 2 n^2 doubles -- 4.5 PB at 256^3.
Times: device events or a drained host clock; the first samples of a series are warm-up; median, 10th and 90th percentile of the rest."""
import argparse
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
from lis_amd import DeviceArray as DA, check  # noqa: E402
from lis_amd import _capi as capi  # noqa: E402

REPS = 24
WARM = 4


def stats(ms, nbytes=None, yard_TBs=None):
    t = np.array(ms[WARM:] if len(ms) > 2 * WARM else ms)
    med = float(np.median(t))
    out = {"median_ms": round(med, 4), "p10_ms": round(float(np.percentile(t, 10)), 4), "p90_ms": round(float(np.percentile(t, 90)), 4), "samples": len(t)}
    if nbytes is not None:
        out.update(bytes=int(nbytes), TB_per_s=round(nbytes / (med * 1e-3) / 1e12, 3) if med > 0 else None)
        if yard_TBs:
            out["ratio_to_bytes_over_yardstick"] = round(med / (nbytes / (yard_TBs * 1e12) * 1e3), 3)
    return out


class Timer:
    def __init__(self, lib):
        self.lib, self.t = lib, C.c_void_p()
        check(lib.liship_timer_create(C.byref(self.t)))

    def time(self, fn):
        ms = C.c_float()
        check(self.lib.liship_timer_start(self.t, None))
        fn()
        check(self.lib.liship_timer_stop(self.t, None))
        check(self.lib.liship_timer_elapsed_ms(self.t, C.byref(ms)))
        return ms.value


def device_csr(lib, A):
    fn = lib.dll.lis_amd_matrix_device_csr
    fn.restype, fn.argtypes = C.c_int, [capi.PM, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    p, i, v = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert fn(A, C.byref(p), C.byref(i), C.byref(v)) == 0
    return p.value, i.value, v.value


def poisson_hbm(lib, N, sorted_rows):
    """the 7-point matrix of N^3 born in HBM; sorted_rows: columns ascending, else the order of test/test3.c (the diagonal last)"""
    A = capi.PM()
    assert lib.lis_matrix_create(0, C.byref(A)) == 0 and lib.lis_matrix_set_size(A, 0, N ** 3) == 0
    lib.dll.lis_amd_matrix_poisson3d.argtypes = [capi.PM, C.c_int, C.c_int, C.c_int, C.c_int]
    assert lib.dll.lis_amd_matrix_poisson3d(A, N, N, N, 1 if sorted_rows else 0) == 0
    return A


def pencil(lib, N, sorted_rows=True):
    """A = Poisson + 2 I on its diagonal through lis_matrix_shift_diagonal(-2); B: a copy of the Poisson arrays with v -> (0.95 / 7) v + (0.05 + 0.95 / 7)"""
    A = poisson_hbm(lib, N, sorted_rows)
    n, nnz = A.contents.n, A.contents.nnz
    p, i, v = device_csr(lib, A)
    bp, bi, bv = DA(n + 1, np.int32), DA(nnz, np.int32), DA(nnz, np.float64)
    check(lib.liship_memcpy_d2d(bp.ptr, p, 4 * (n + 1), None))
    check(lib.liship_memcpy_d2d(bi.ptr, i, 4 * nnz, None))
    alpha = 0.95 / 7.0
    check(lib.liship_set_all_f64(nnz, 0.05 + alpha, bv.ptr, None))
    check(lib.liship_axpy_f64(nnz, alpha, v, bv.ptr, None))
    check(lib.liship_device_synchronize())
    B = capi.PM()
    assert lib.lis_matrix_create(0, C.byref(B)) == 0 and lib.lis_matrix_set_size(B, n, 0) == 0
    fn = lib.dll.lis_amd_matrix_set_csr_device
    fn.restype, fn.argtypes = C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, capi.PM]
    assert fn(nnz, n, bp.ptr, bi.ptr, bv.ptr, B) == 0
    bp.ptr = bi.ptr = bv.ptr = None                                                       # owned by B now
    assert lib.lis_matrix_shift_diagonal(A, -2.0) == 0
    return A, B


def whole_call(lib, A, B, sigma):
    check(lib.liship_device_synchronize())
    t0 = time.perf_counter()
    assert lib.dll.lis_matrix_shift_matrix(A, B, C.c_double(sigma)) == 0
    check(lib.liship_device_synchronize())
    return 1e3 * (time.perf_counter() - t0)


def last_shift(lib):
    info = (C.c_int * 3)()
    lib.dll.lis_amd_last_shift_matrix(info)
    return list(info)


def in_place_rows(lib, N, timer, yard):
    A, B = pencil(lib, N)
    n, nnz = A.contents.n, A.contents.nnz
    ap, bp = device_csr(lib, A), device_csr(lib, B)
    work = DA.zeros(2 * n + 2, np.int32)
    count, done, flag = work.ptr, work.ptr + 4 * n, work.ptr + 8 * n
    launch = [timer.time(lambda: check(lib.liship_csr_shift_matrix_try_f64(n, *ap, *bp, 0.25 if k % 2 == 0 else -0.25, count, done, flag, None))) for k in range(REPS)]
    left = int(work.to_host()[2 * n])
    whole = [whole_call(lib, A, B, 0.25 if k % 2 == 0 else -0.25) for k in range(REPS)]
    info = last_shift(lib)
    work.free()
    lib.lis_matrix_destroy(A)
    lib.lis_matrix_destroy(B)
    nbytes = 32 * nnz + 16 * n
    k, w = stats(launch, nbytes, yard), stats(whole, nbytes, yard)
    return {"rows": n, "nnz": nnz, "rows_left_to_a_rebuild": left, "last_shift_info": info, "launch": k, "whole_call": w, "refresh_ms": round(w["median_ms"] - k["median_ms"], 4)}


def rebuilt_rows(lib, N, timer, yard):
    samples, steps, info = [], {"try": [], "scan": [], "fill": []}, None
    for s in range(6):
        A, B = pencil(lib, N, sorted_rows=False)
        n, nnz = A.contents.n, A.contents.nnz
        if s < 3:                                                                          # the three steps alone, on A's own arrays (no row qualifies: the try writes nothing)
            ap, bp = device_csr(lib, A), device_csr(lib, B)
            work = DA.zeros(2 * n + 2, np.int32)
            count, done, flag = work.ptr, work.ptr + 4 * n, work.ptr + 8 * n
            nptr, scratch, total = DA(n + 1, np.int32), DA(n // 4096 + 2, np.int64), C.c_int()
            steps["try"].append(timer.time(lambda: check(lib.liship_csr_shift_matrix_try_f64(n, *ap, *bp, 0.25, count, done, flag, None))))
            steps["scan"].append(timer.time(lambda: check(lib.liship_csr_shift_matrix_scan(n, count, nptr.ptr, scratch.ptr, C.byref(total), None))))
            nidx, nval = DA(total.value, np.int32), DA(total.value, np.float64)
            steps["fill"].append(timer.time(lambda: check(lib.liship_csr_shift_matrix_fill_f64(n, *ap, *bp, 0.25, done, nptr.ptr, nidx.ptr, nval.ptr, None))))
            for d in (work, nptr, scratch, nidx, nval):
                d.free()
        samples.append(whole_call(lib, A, B, 0.25))
        info = last_shift(lib)
        lib.lis_matrix_destroy(A)
        lib.lis_matrix_destroy(B)
    nbytes = 60 * nnz + 28 * n
    kernels = {k: round(float(np.median(v)), 4) for k, v in steps.items()}
    kernels["sum_ms"] = round(sum(kernels.values()), 4)
    w = stats(samples[1:], nbytes, yard)
    return {"rows": n, "nnz": nnz, "last_shift_info": info, "steps_alone_ms": kernels, "whole_call": w, "refresh_ms": round(w["median_ms"] - kernels["sum_ms"], 4),
            "steps_ratio_to_bytes_over_yardstick": round(kernels["sum_ms"] / (nbytes / (yard * 1e12) * 1e3), 3) if yard else None}


def grqi_rows(lib, N, shift_ms):
    import gesolve_drv as gd
    A, B = pencil(lib, N)
    gd.gesolve(lib, A, B, "-e grqi -emaxiter 1 -etol 1e-30")                              # plans, the transposed copy, work vectors: not timed
    E = capi.PE()
    assert lib.lis_esolver_create(C.byref(E)) == 0 and lib.lis_esolver_set_option(b"-e grqi -emaxiter 2 -etol 1e-30", E) == 0
    vx = lisdrv.new_vector(lib, A)
    ev, t, it = C.c_double(), C.c_double(), C.c_int()
    err = lib.lis_gesolve(A, B, vx, C.byref(ev), E)
    out = {"err": err}
    if err == 0:
        lib.lis_esolver_get_time(E, C.byref(t))
        lib.lis_esolver_get_iter(E, C.byref(it))
        per = 1e3 * t.value / max(it.value, 1)
        out.update(outer_iterations=it.value, seconds=round(t.value, 4), ms_per_outer_iteration=round(per, 3), two_shifts_ms=round(2 * shift_ms, 3),
                   ms_per_outer_iteration_without_the_shifts=round(per - 2 * shift_ms, 3), shifts_share=round(2 * shift_ms / per, 4) if per > 0 else None, evalue=ev.value,
                   last_shift_info=last_shift(lib))
    lib.lis_esolver_destroy(E)
    lib.lis_vector_destroy(vx)
    lib.lis_matrix_destroy(A)
    lib.lis_matrix_destroy(B)
    return out


def yardstick(lib, timer):
    n = 512 * 65536
    src, dst = DA.zeros(13 * n, np.float64), DA.zeros(n, np.float64)
    ms = [timer.time(lambda: check(lib.liship_stream_yardstick(13, n, src.ptr, dst.ptr, 0, None))) for _ in range(REPS)]
    src.free()
    dst.free()
    return stats(ms, 14 * 8 * n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--inner-tol", default="1e-6")
    args = ap.parse_args()
    lib = lis_amd.load()
    if not lis_amd.gpu_available():
        raise SystemExit("gesolve_probe: no HIP device -- nothing here is measured without one")
    assert lib.initialize(["-tol", args.inner_tol]) == 0
    lib.dll.lis_matrix_shift_matrix.argtypes = [capi.PM, capi.PM, C.c_double]
    name = C.create_string_buffer(256)
    lib.liship_device_name(name, 256)
    timer = Timer(lib)
    yard = yardstick(lib, timer)
    N = args.grid
    out = {"device": name.value.decode(), "grid": N, "yardstick_13_reads_1_write": yard, "inner_tol": args.inner_tol,
           "reference": "no number at this size: lis_matrix_shift_matrix of the reference needs two dense n x n copies, 2 n^2 doubles = %.3g bytes" % (16.0 * float(N) ** 6)}
    for key, fn in (("in_place", lambda: in_place_rows(lib, N, timer, yard["TB_per_s"])), ("rebuilt", lambda: rebuilt_rows(lib, N, timer, yard["TB_per_s"]))):
        try:
            out[key] = fn()
        except Exception as e:                                                             # a probe reports what it could not measure
            out[key] = {"error": repr(e)}
    try:
        out["grqi"] = grqi_rows(lib, N, out["in_place"]["whole_call"]["median_ms"])
    except Exception as e:
        out["grqi"] = {"error": repr(e)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
