"""Several pairs of the generalized problem (-e gsi): what the two pair passes cost against the separate calls they replace, and what one outer iteration costs
fused and unfused, with the share of it spent inside the inner solves.  Prints ONE JSON object (a run on an MI355X belongs in profiles/gesolve_multi_probe.json).
    python tools/gesolve_multi_probe.py [N] [--ss 4] [--iters 3] [--inner-maxiter 200]
Workload (default N = 256): the 7-point A on N^3 and B on the same pattern with diagonal 1 and off-diagonals 0.05, both adopted from arrays in HBM (no host copy).
  pair_passes  ms by device events, beside the stream model:
                 scale2_inv_sqrt (in place: 4 n-vector streams, 1 launch) against liship_scale_inv_norm_f64 twice (4 streams, 2 launches);
                 scale2_to (out of place: 4 streams, 1 launch) against copy, copy, scale, scale (8 streams, 4 launches).
               The first ten samples are warm-up; median, 10th and 90th percentile of the 30 that follow; the two forms alternate sample by sample.
  iteration    -e gsi -ss <ss> -ige gii with -etol 1e-30 -emaxiter <iters>: ms per outer iteration by mode, fused and unfused (lis_amd_set_loop_mode), from the
               library's own per-mode elapsed time (the "Generalized Subspace: elapsed time" line of -eprint mem, which holds the mode's
               lis_vector_duplicate, preconditioner and copy as well) over the mode's iterations; and mode 0's share inside the inner solves: the inner
               solver's own times, which the loop adds up over mode 0 (lis_esolver_get_timeex: itime), over mode 0's elapsed time.  The inner BiCG solves
               are capped at --inner-maxiter iterations through the command line's -maxiter, which the inner solver honours (lis_solver_set_optionC): what is
               compared is the time outside them, and an uncapped solve on this A only lengthens the part both forms share."""
import ctypes as C
import json
import os
import re
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import gesolve_drv as gd  # noqa: E402
import lis_amd  # noqa: E402
import lisdrv  # noqa: E402
import orc  # noqa: E402
from lis_amd import DeviceArray as DA, check  # noqa: E402
from lis_amd import _capi as capi  # noqa: E402

REPS = 40
LOOP_FUSED, LOOP_UNFUSED = 0, 2


def stats(ms, nbytes):
    t = np.array(ms[10:])
    med = float(np.median(t))
    return {"median_ms": round(med, 4), "p10_ms": round(float(np.percentile(t, 10)), 4), "p90_ms": round(float(np.percentile(t, 90)), 4), "samples": len(t),
            "bytes": int(nbytes), "TB_per_s": round(nbytes / (med * 1e-3) / 1e12, 3) if med > 0 else None}


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


def captured(fn):
    """what the C library printed on stdout while fn ran"""
    libc = C.CDLL(None)
    sys.stdout.flush()
    libc.fflush(None)
    keep = os.dup(1)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 1)
        try:
            out = fn()
            libc.fflush(None)
        finally:
            os.dup2(keep, 1)
            os.close(keep)
        tmp.seek(0)
        return out, tmp.read().decode(errors="replace")


def pair_pass_times(lib, n):
    rng = np.random.default_rng(3)
    v, w, r, q = (DA.from_host(rng.uniform(0.5, 1.5, n)) for _ in range(4))
    s = DA.from_host(np.array([1.0]))                       # 1 / sqrt(1) = 1: the in-place forms leave their data as it was, sample after sample
    timer = Timer(lib, None)

    def inv_fused():
        check(lib.liship_scale2_inv_sqrt_f64(n, s.ptr, v.ptr, w.ptr, None))

    def inv_separate():
        check(lib.liship_scale_inv_norm_f64(n, s.ptr, v.ptr, None))
        check(lib.liship_scale_inv_norm_f64(n, s.ptr, w.ptr, None))

    def to_fused():
        check(lib.liship_scale2_to_f64(n, 0.5, r.ptr, q.ptr, w.ptr, v.ptr, None))

    def to_separate():                                       # copy r -> w, copy q -> v, scale w, scale v
        check(lib.liship_memcpy_d2d(w.ptr, r.ptr, 8 * n, None))
        check(lib.liship_memcpy_d2d(v.ptr, q.ptr, 8 * n, None))
        check(lib.liship_scale_f64(n, 0.5, w.ptr, None))
        check(lib.liship_scale_f64(n, 0.5, v.ptr, None))

    out = {}
    for name, fused, separate, sf, ss_, lf, ls in (("scale2_inv_sqrt", inv_fused, inv_separate, 4, 4, 1, 2), ("scale2_to", to_fused, to_separate, 4, 8, 1, 4)):
        a, b = [], []
        for _ in range(REPS):                                # alternating, so that both see the same neighbours on the machine
            a.append(timer.time(fused))
            b.append(timer.time(separate))
        row = {"fused": dict(stats(a, sf * 8 * n), launches=lf, streams=sf), "separate": dict(stats(b, ss_ * 8 * n), launches=ls, streams=ss_)}
        row["fused_over_separate"] = round(row["fused"]["median_ms"] / row["separate"]["median_ms"], 3)
        row["stream_model_fused_over_separate"] = round(sf / ss_, 3)
        out[name] = row
    for d in (v, w, r, q, s):
        d.free()
    return out


def iteration_times(lib, A, B, ss, iters, loop_mode):
    """-> {mode: {...}} from the library's per-mode lines, and mode 0's share inside the inner solves"""
    vx = lisdrv.new_vector(lib, A)
    E = capi.PE()
    assert lib.lis_esolver_create(C.byref(E)) == 0
    assert lib.lis_esolver_set_option(("-e gsi -ss %d -ige gii -etol 1e-30 -emaxiter %d -eprint mem" % (ss, iters)).encode(), E) == 0
    ev = C.c_double()
    lib.dll.lis_amd_set_loop_mode(loop_mode)
    try:
        err, text = captured(lambda: lib.lis_gesolve(A, B, vx, C.byref(ev), E))
    finally:
        lib.dll.lis_amd_set_loop_mode(LOOP_FUSED)
    assert err == 0, err
    modes = [int(m) for m in re.findall(r"Generalized Subspace: mode number\s+= (\d+)", text)]
    secs = [float(s) for s in re.findall(r"Generalized Subspace: elapsed time\s+= (\S+) sec", text)]
    its = [int(k) for k in re.findall(r"Generalized Subspace: number of iterations = (\d+)", text)]
    assert modes == list(range(ss)) and len(secs) == ss and len(its) == ss, text[-2000:]
    t = [C.c_double() for _ in range(5)]
    lib.dll.lis_esolver_get_timeex.argtypes = [capi.PE] + [C.POINTER(C.c_double)] * 5
    assert lib.dll.lis_esolver_get_timeex(E, *[C.byref(x) for x in t]) == 0
    lib.lis_esolver_destroy(E)
    lib.lis_vector_destroy(vx)
    out = {m: {"iterations": k, "ms_per_iteration": round(s / k * 1e3, 4)} for m, s, k in zip(modes, secs, its)}
    out[0]["ms_per_iteration_inside_inner_solves"] = round(t[1].value / its[0] * 1e3, 4)
    out[0]["share_inside_inner_solves"] = round(t[1].value / secs[0], 4)
    return out


def main():
    args = sys.argv[1:]
    opt = {"--ss": 4, "--iters": 3, "--inner-maxiter": 200}
    for flag in list(opt):
        if flag in args:
            k = args.index(flag)
            opt[flag] = int(args[k + 1])
            del args[k:k + 2]
    ss, iters, inner = opt["--ss"], opt["--iters"], opt["--inner-maxiter"]
    N = int(args[0]) if args else 256
    lib = lis_amd.load()
    if not lis_amd.gpu_available():
        raise SystemExit("gesolve_multi_probe: no HIP device -- nothing here is measured without one")
    assert lib.initialize(["-maxiter", str(inner)]) == 0
    lib.dll.lis_amd_set_residency(1)
    name = (C.c_char * 128)()
    lib.dll.liship_device_name(name, 128)
    ptr, idx, val = orc.poisson3d(N, N, N)
    n = len(ptr) - 1
    rows = np.repeat(np.arange(n, dtype=np.int32), np.diff(ptr))
    bval = np.where(idx == rows, 1.0, 0.05)
    del rows
    doc = {"tool": "tools/gesolve_multi_probe.py", "device": name.value.decode(), "N": N, "n": n, "nnz": len(idx),
           "pencil": "7-point A (diagonal 6, off-diagonals -1), B on the same pattern with diagonal 1 and off-diagonals 0.05, both in HBM only",
           "pair_passes": pair_pass_times(lib, n)}
    A, B = gd.make_hbm(lib, (ptr, idx, val)), gd.make_hbm(lib, (ptr, idx, bval))
    iteration_times(lib, A, B, 2, 1, LOOP_FUSED)            # plans and pools (not timed below)
    fused, unfused = iteration_times(lib, A, B, ss, iters, LOOP_FUSED), iteration_times(lib, A, B, ss, iters, LOOP_UNFUSED)
    lib.lis_matrix_destroy(A)
    lib.lis_matrix_destroy(B)
    doc["options"] = "-e gsi -ss %d -ige gii -etol 1e-30 -emaxiter %d; inner solves: -i bicg -p none -maxiter %d" % (ss, iters, inner)
    doc["iteration"] = {"mode_%d" % m: {"fused": fused[m], "unfused": unfused[m],
                                        "fused_over_unfused": round(fused[m]["ms_per_iteration"] / unfused[m]["ms_per_iteration"], 3)} for m in range(ss)}
    m0 = doc["iteration"]["mode_0"]
    for k in ("fused", "unfused"):
        m0[k]["ms_per_iteration_outside_inner_solves"] = round(m0[k]["ms_per_iteration"] - m0[k]["ms_per_iteration_inside_inner_solves"], 4)
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
