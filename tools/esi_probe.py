"""Subspace iteration (-e si): what one iteration costs at the first and at the last mode, with the device chains and the fused tail and with the plain
lis_vector_* calls, and what the tail alone costs.  Prints ONE JSON object (a run on an MI355X belongs in profiles/esi_probe.json).
    python tools/esi_probe.py [N] [--ss 4] [--iters 20]        (default: the 7-point Poisson matrix on 256^3, -e si -ss 4 -ie pi)
  iteration  ms per iteration of mode 0 and of mode ss - 1, fused and unfused (lis_amd_set_loop_mode): the library's own per-mode elapsed time (the
             "Subspace: elapsed time" line of -eprint mem, which holds the mode's lis_vector_duplicate and copy as well) over the mode's iterations.  An
             iteration of mode j is j orthogonalisation pairs, one product and the tail, and it waits for the host once (fused) or 3 + j times (unfused)
  tail       ms by device events of {liship_multidot_f64, liship_ritz_tail_f64} and of the six calls they replace -- sumsq, dot, axpyz, sumsq, scale, copy --
             launched back to back WITHOUT the three read-backs the unfused loop makes between them, beside the model: 6 against 11 n-vector streams
Times of the tail: the first ten samples are warm-up; median, 10th and 90th percentile of the 30 that follow."""
import ctypes as C
import json
import os
import re
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
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


def iteration_times(lib, A, ss, iters, loop_mode):
    """-> {mode: ms per iteration} from the library's per-mode lines"""
    vx = lisdrv.new_vector(lib, A)
    E = capi.PE()
    assert lib.lis_esolver_create(C.byref(E)) == 0
    assert lib.lis_esolver_set_option(("-e si -ss %d -ie pi -etol 1e-30 -emaxiter %d -eprint mem" % (ss, iters)).encode(), E) == 0
    ev = C.c_double()
    lib.dll.lis_amd_set_loop_mode(loop_mode)
    try:
        err, text = captured(lambda: lib.lis_esolve(A, vx, C.byref(ev), E))
    finally:
        lib.dll.lis_amd_set_loop_mode(LOOP_FUSED)
    assert err == 0, err
    modes = [int(m) for m in re.findall(r"Subspace: mode number\s+= (\d+)", text)]
    secs = [float(s) for s in re.findall(r"Subspace: elapsed time\s+= (\S+) sec", text)]
    its = [int(k) for k in re.findall(r"Subspace: number of iterations = (\d+)", text)]
    assert modes == list(range(ss)) and len(secs) == ss and len(its) == ss, text[-2000:]
    lib.lis_esolver_destroy(E)
    lib.lis_vector_destroy(vx)
    return {m: {"iterations": k, "ms_per_iteration": round(s / k * 1e3, 4)} for m, s, k in zip(modes, secs, its)}


def tail_times(lib, n):
    rng = np.random.default_rng(3)
    r, v, q = DA.from_host(rng.uniform(-1, 1, n)), DA.from_host(rng.uniform(-1, 1, n)), DA.zeros(n, np.float64)
    work, res = DA(lib.liship_reduce_work_bytes() // 8, np.float64), DA.zeros(4, np.float64)
    timer = Timer(lib, None)
    vecs = (C.c_void_p * 2)(r.ptr, v.ptr)
    pairs = ((C.c_int * 2) * 2)((0, 0), (1, 0))

    def fused():
        check(lib.liship_multidot_f64(n, 2, vecs, 2, pairs, res.ptr, work.ptr, None))
        check(lib.liship_ritz_tail_f64(n, res.ptr, r.ptr, v.ptr, res.ptr + 16, work.ptr, None))

    def separate():                                          # the scalars by value, as lis_vector_* take them (their size does not matter to the time)
        check(lib.liship_sumsq_f64(n, r.ptr, res.ptr, work.ptr, None))
        check(lib.liship_dot_f64(n, v.ptr, r.ptr, res.ptr + 8, work.ptr, None))
        check(lib.liship_axpyz_f64(n, -0.5, v.ptr, r.ptr, q.ptr, None))
        check(lib.liship_sumsq_f64(n, q.ptr, res.ptr + 16, work.ptr, None))
        check(lib.liship_scale_f64(n, 1.0, r.ptr, None))
        check(lib.liship_memcpy_d2d(v.ptr, r.ptr, 8 * n, None))

    out = {"fused_2_launches": stats([timer.time(fused) for _ in range(REPS)], 6 * 8 * n),
           "separate_6_launches": stats([timer.time(separate) for _ in range(REPS)], 11 * 8 * n)}
    out["fused_over_separate"] = round(out["fused_2_launches"]["median_ms"] / out["separate_6_launches"]["median_ms"], 3)
    out["stream_model_fused_over_separate"] = round(6 / 11, 3)
    for d in (r, v, q, work, res):
        d.free()
    return out


def main():
    args = sys.argv[1:]
    ss, iters = 4, 20
    for flag in ("--ss", "--iters"):
        if flag in args:
            k = args.index(flag)
            if flag == "--ss":
                ss = int(args[k + 1])
            else:
                iters = int(args[k + 1])
            del args[k:k + 2]
    N = int(args[0]) if args else 256
    lib = lis_amd.load()
    if not lis_amd.gpu_available():
        raise SystemExit("esi_probe: no HIP device -- nothing here is measured without one")
    assert lib.initialize([]) == 0
    lib.dll.lis_amd_set_residency(1)
    name = (C.c_char * 128)()
    lib.dll.liship_device_name(name, 128)
    ptr, idx, val = orc.poisson3d(N, N, N)
    n = len(ptr) - 1
    A = lisdrv.make_csr(lib, ptr, idx, val)
    iteration_times(lib, A, 2, 2, LOOP_FUSED)               # plans and pools (not timed below)
    fused, unfused = iteration_times(lib, A, ss, iters, LOOP_FUSED), iteration_times(lib, A, ss, iters, LOOP_UNFUSED)
    lib.lis_matrix_destroy(A)
    doc = {"tool": "tools/esi_probe.py", "device": name.value.decode(), "N": N, "n": n, "nnz": len(idx), "options": "-e si -ss %d -ie pi" % ss,
           "iteration": {"mode_0": {"fused": fused[0], "unfused": unfused[0]}, "mode_%d" % (ss - 1): {"fused": fused[ss - 1], "unfused": unfused[ss - 1]}},
           "tail": tail_times(lib, n)}
    for k, row in doc["iteration"].items():
        row["fused_over_unfused"] = round(row["fused"]["ms_per_iteration"] / row["unfused"]["ms_per_iteration"], 3)
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
