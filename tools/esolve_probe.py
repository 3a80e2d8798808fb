"""The eigensolvers (lis_esolve) on an MI355X: what an outer iteration, a diagonal shift and a Gram block cost.  Prints ONE JSON object (a run belongs in
profiles/esolve_probe.json).
    python tools/esolve_probe.py [--grids 128,256] [--shift-grid 256]
  esolve     ms per outer iteration of -e pi | ii | rqi | cg | cr on the 7-point Poisson matrix of N^3, born in HBM: lis_esolver_get_time / iterations, the
             outer iterations capped (pi, cg, cr: 20; ii, rqi: 3 -- each of theirs is a whole inner BiCG solve)
  shift      one lis_matrix_shift_diagonal of a resident CSR matrix (N = --shift-grid): the kernel alone (device events on the HBM arrays), the whole call
             on a matrix that lives in HBM only and the whole call on a host-backed one (host clock, stream drained).  plan_rebuild_ms = HBM-only call -
             kernel: dropping what hung on the old values and making the plan again from the HBM arrays; host_edit_ms = host-backed call - HBM-only
             call: the same edit of the host arrays
  multidot   the A/B the issue asks for: liship_multidot_f64 of CR's 5-pair block (3 vectors), of CG's own 12-pair block and of a 15-pair block over its 6 vectors against the same
             sums as separate liship_dot_f64 launches (a kernel this probe's subject does not touch), alternating the two in one process; bytes are what each
             form has to read (V n 8 against 2 K n 8 -- a self pair reads one array -- ), and each time is set against bytes / the box's streaming yardstick
             (liship_stream_yardstick, 13 reads : 1 write) measured in the same process.  explanation_owed: the fused pass is not faster at the largest grid.
Times: device events, the first ten samples of a series are warm-up; median, 10th and 90th percentile of the rest."""
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
import orc  # noqa: E402
from lis_amd import DeviceArray as DA, check  # noqa: E402
from lis_amd import _capi as capi  # noqa: E402

REPS = 40
CR5 = [(0, 2), (0, 1), (2, 2), (1, 2), (1, 1)]
CG12 = [(0, 3), (1, 3), (2, 3), (1, 4), (2, 4), (2, 5), (0, 0), (1, 0), (2, 0), (1, 1), (2, 1), (2, 2)]      # lis_ecg's Gram block over (w x p Aw Ax Ap)
CG15 = CG12 + [(1, 4), (3, 3), (5, 4)]                                                                       # and three more: tests/test_multidot_gpu.py's list


def stats(ms, nbytes=None):
    t = np.array(ms[10:])
    med = float(np.median(t))
    out = {"median_ms": round(med, 4), "p10_ms": round(float(np.percentile(t, 10)), 4), "p90_ms": round(float(np.percentile(t, 90)), 4), "samples": len(t)}
    if nbytes is not None:
        out.update(bytes=int(nbytes), TB_per_s=round(nbytes / (med * 1e-3) / 1e12, 3) if med > 0 else None)
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


def poisson_hbm(lib, N):
    A = capi.PM()
    assert lib.lis_matrix_create(0, C.byref(A)) == 0 and lib.lis_matrix_set_size(A, 0, N ** 3) == 0
    lib.dll.lis_amd_matrix_poisson3d.argtypes = [capi.PM, C.c_int, C.c_int, C.c_int, C.c_int]
    assert lib.dll.lis_amd_matrix_poisson3d(A, N, N, N, 0) == 0
    return A


def esolve_rows(lib, N):
    import esolve_drv
    rows = {}
    for e, cap in (("pi", 20), ("ii", 3), ("rqi", 3), ("cg", 20), ("cr", 20)):
        A = poisson_hbm(lib, N)
        esolve_drv.esolve(lib, A, "-e %s -emaxiter 1 -etol 1e-30" % e)                    # plans, transposed copy, work vectors: not timed
        E = capi.PE()
        assert lib.lis_esolver_create(C.byref(E)) == 0
        assert lib.lis_esolver_set_option(("-e %s -emaxiter %d -etol 1e-30" % (e, cap)).encode(), E) == 0
        vx = lisdrv.new_vector(lib, A)
        ev, t, it = C.c_double(), C.c_double(), C.c_int()
        err = lib.lis_esolve(A, vx, C.byref(ev), E)
        lib.lis_esolver_get_time(E, C.byref(t))
        lib.lis_esolver_get_iter(E, C.byref(it))
        rows[e] = {"err": err, "outer_iterations": it.value, "seconds": round(t.value, 4), "ms_per_outer_iteration": round(1e3 * t.value / max(it.value, 1), 3),
                   "evalue": ev.value}
        lib.lis_esolver_destroy(E)
        lib.lis_vector_destroy(vx)
        lib.lis_matrix_destroy(A)
    return rows


def shift_rows(lib, N, timer):
    ptr, idx, val = orc.poisson3d(N, N, N)
    n = len(ptr) - 1
    dptr, didx, dval = DA.from_host(ptr, np.int32), DA.from_host(idx, np.int32), DA.from_host(val, np.float64)
    kernel = [timer.time(lambda: check(lib.liship_csr_shift_diagonal_f64(n, dptr.ptr, didx.ptr, dval.ptr, 0.25 if k % 2 == 0 else -0.25, None))) for k in range(REPS)]
    for d in (dptr, didx, dval):
        d.free()
    A = lisdrv.make_csr(lib, ptr, idx, val)
    lisdrv.matvec(lib, A, np.ones(n))                                                     # resident from here on
    whole = []
    for k in range(REPS // 2):
        check(lib.liship_device_synchronize())
        t0 = time.perf_counter()
        assert lib.lis_matrix_shift_diagonal(A, 0.25 if k % 2 == 0 else -0.25) == 0
        check(lib.liship_device_synchronize())
        whole.append(1e3 * (time.perf_counter() - t0))
    written = lib.dll.lis_amd_matrix_host_written(A)
    lib.lis_matrix_destroy(A)
    A = poisson_hbm(lib, N)                                                               # the same matrix, born in HBM: no host arrays to edit
    lisdrv.matvec(lib, A, np.ones(n))
    hbm = []
    for k in range(REPS // 2):
        check(lib.liship_device_synchronize())
        t0 = time.perf_counter()
        assert lib.lis_matrix_shift_diagonal(A, 0.25 if k % 2 == 0 else -0.25) == 0
        check(lib.liship_device_synchronize())
        hbm.append(1e3 * (time.perf_counter() - t0))
    lib.lis_matrix_destroy(A)
    k, w, h = stats(kernel, 12 * n + 4 * len(idx)), stats(whole), stats(hbm)
    # (the kernel reads ptr, walks a row's columns up to its diagonal and rewrites one value: between 20 n bytes and the whole index array)
    return {"grid": N, "rows": n, "nnz": int(len(idx)), "kernel": k, "whole_call_hbm_only": h, "whole_call_host_backed": w,
            "plan_rebuild_ms": round(h["median_ms"] - k["median_ms"], 4), "host_edit_ms": round(w["median_ms"] - h["median_ms"], 4),
            "host_written_after": int(written)}


def multidot_rows(lib, N, timer, yard_TBs):
    n = N ** 3
    rng = np.random.default_rng(N)
    vecs = [DA.from_host(rng.uniform(-1.0, 1.0, n), np.float64) for _ in range(6)]
    work = DA(lib.liship_reduce_work_bytes() // 8, np.float64)
    res = DA.zeros(64, np.float64)
    out = {}
    for name, V, pairs in (("cr_5_pairs_3_vectors", 3, CR5), ("cg_12_pairs_6_vectors", 6, CG12), ("cg_15_pairs_6_vectors", 6, CG15)):
        K = len(pairs)
        ptrs = (C.c_void_p * V)(*[v.ptr for v in vecs[:V]])
        cp = (C.c_int * (2 * K))(*[i for p in pairs for i in p])

        def fused():
            check(lib.liship_multidot_f64(n, V, ptrs, K, cp, res.ptr, work.ptr, None))

        def separate():
            for k, (a, b) in enumerate(pairs):
                check(lib.liship_dot_f64(n, vecs[a].ptr, vecs[b].ptr, res.ptr + 8 * k, work.ptr, None))

        fused()
        f0 = res.to_host()[:K].copy()
        separate()
        same = bool(np.array_equal(f0.view(np.int64), res.to_host()[:K].view(np.int64)))
        tf, ts = [], []
        for _ in range(REPS):                                                             # alternating: both see the same neighbours on the box
            tf.append(timer.time(fused))
            ts.append(timer.time(separate))
        bytes_f = 8 * n * V
        bytes_s = 8 * n * sum(1 if a == b else 2 for a, b in pairs)
        f, s = stats(tf, bytes_f), stats(ts, bytes_s)
        for row, nbytes in ((f, bytes_f), (s, bytes_s)):
            row["ratio_to_bytes_over_yardstick"] = round(row["median_ms"] / (nbytes / (yard_TBs * 1e12) * 1e3), 3) if yard_TBs else None
        out[name] = {"K": K, "V": V, "same_bits": same, "fused": f, "separate_dots": s, "speedup": round(s["median_ms"] / f["median_ms"], 3) if f["median_ms"] > 0 else None}
    for v in vecs:
        v.free()
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
    ap.add_argument("--grids", default="128,256")
    ap.add_argument("--shift-grid", type=int, default=256)
    args = ap.parse_args()
    grids = [int(g) for g in args.grids.split(",") if int(g) > 0]
    lib = lis_amd.load()
    if not lis_amd.gpu_available():
        raise SystemExit("esolve_probe: no HIP device -- nothing here is measured without one")
    assert lib.initialize([]) == 0
    name = C.create_string_buffer(256)
    lib.liship_device_name(name, 256)
    timer = Timer(lib)
    yard = yardstick(lib, timer)
    out = {"device": name.value.decode(), "yardstick_13_reads_1_write": yard, "esolve": {}, "multidot": {}}
    for N in grids:
        out["multidot"]["n_%d_cubed" % N] = multidot_rows(lib, N, timer, yard["TB_per_s"])
    if args.shift_grid > 0:
        out["shift"] = shift_rows(lib, args.shift_grid, timer)
    for N in grids:
        out["esolve"]["poisson_%d_cubed" % N] = esolve_rows(lib, N)
    last = out["multidot"].get("n_%d_cubed" % grids[-1], {}) if grids else {}
    out["explanation_owed"] = [k for k, v in last.items() if v["speedup"] is not None and v["speedup"] <= 1.0]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
