"""COO and DNS storage: what the two dense kernels reach and what the COO row form costs.  Prints ONE JSON object (a run on an MI355X belongs in
profiles/coo_dns_probe.json).
    python tools/coo_dns_probe.py [--dns 8192,16384] [--coo 256]
DNS   liship_spmv_dns_f64 and liship_spmv_dns_t_f64 (T = 1) at n = np: ms by device events, over 8 n np bytes, and that time over bytes / the box's streaming
      yardstick (liship_stream_yardstick, 13 reads : 1 write, measured in the same process).  0.5 GiB and 2 GiB at the default sizes: beyond the Infinity Cache.
COO   the 7-point Poisson matrix on N^3 as triplets: host seconds of liship_coo_rows_f64 (it ends in a synchronize) for the triplets in row order (ptr from
      the row starts, col / value in place) and shuffled (the stable grouping), the arrays in HBM before the clock starts; then lis_matvec of the matrix in
      COO storage beside the same matrix in CSR storage -- the same plan and kernel are expected -- by device events.
Times: the first five samples of every series are warm-up; median, 10th and 90th percentile of the 20 that follow."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import coo_dns_drv as drv  # noqa: E402
import lis_amd  # noqa: E402
import lisdrv  # noqa: E402
import orc  # noqa: E402
from lis_amd import DeviceArray as DA, check  # noqa: E402

WARM, REPS = 5, 25


def stats(ms, nbytes=None, yard=None):
    t = np.array(ms[WARM:])
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


def dns_case(lib, n, yard):
    timer = Timer(lib, None)
    count = n * n
    value = DA(count, np.float64)
    chunk = np.random.default_rng(n).uniform(-1, 1, min(count, 1 << 22))           # random values, laid end to end
    for at in range(0, count, len(chunk)):
        part = chunk[:min(len(chunk), count - at)]
        check(lib.liship_memcpy_h2d(value.ptr + 8 * at, part.ctypes.data, part.nbytes, None))
    check(lib.liship_device_synchronize())
    x, y = DA.from_host(np.random.default_rng(1).uniform(-1, 1, n)), DA.zeros(n, np.float64)
    fwd = [timer.time(lambda: check(lib.liship_spmv_dns_f64(n, n, value.ptr, x.ptr, y.ptr, None))) for _ in range(REPS)]
    tr = [timer.time(lambda: check(lib.liship_spmv_dns_t_f64(n, n, 1, value.ptr, x.ptr, y.ptr, None))) for _ in range(REPS)]
    for a in (value, x, y):
        a.free()
    return {"n": n, "np": n, "GiB": round(8 * count / 2**30, 3), "forward": stats(fwd, 8 * count, yard), "transposed": stats(tr, 8 * count, yard)}


def coo_case(lib, N, yard):
    dll = lib.dll
    ptr, idx, val = orc.poisson3d(N, N, N)
    n, nnz = len(ptr) - 1, len(idx)
    row = np.repeat(np.arange(n, dtype=np.int32), np.diff(ptr))
    out = {"N": N, "n": n, "nnz": nnz}
    p = np.random.default_rng(N).permutation(nnz)
    for tag, (r, c, v) in (("sorted", (row, idx, val)), ("shuffled", (row[p], idx[p], val[p]))):
        dr, dc, dv, dptr = DA.from_host(r), DA.from_host(c), DA.from_host(v), DA(n + 1, np.int32)
        secs, in_place = [], None
        for _ in range(3):
            pi, pv = C.c_void_p(), C.c_void_p()
            check(lib.liship_device_synchronize())
            t0 = time.perf_counter()
            check(lib.liship_coo_rows_f64(n, nnz, dr.ptr, dc.ptr, dv.ptr, dptr.ptr, C.byref(pi), C.byref(pv), None))
            secs.append(time.perf_counter() - t0)
            in_place = pi.value == dc.ptr
            if not in_place:
                check(lib.liship_free(pi))
                check(lib.liship_free(pv))
        out["row_form_" + tag] = {"in_place": bool(in_place), "seconds": [round(s, 4) for s in secs], "best_s": round(min(secs), 4)}
        for a in (dr, dc, dv, dptr):
            a.free()
    del p
    dll.lis_amd_stream.restype = C.c_void_p
    timer = Timer(lib, dll.lis_amd_stream())
    x = np.random.default_rng(2).uniform(-1, 1, n)
    for tag, A in (("csr", lisdrv.make_csr(lib, ptr, idx, val)), ("coo", drv.make_coo(lib, n, row, idx, val))):
        vx, vy = lisdrv.new_vector(lib, A, x), lisdrv.new_vector(lib, A)
        t0 = time.perf_counter()
        assert lib.lis_matvec(A, vx, vy) == 0                                       # the upload, the row form, the plan
        check(lib.liship_stream_synchronize(dll.lis_amd_stream()))
        first = time.perf_counter() - t0
        ms = [timer.time(lambda: lib.lis_matvec(A, vx, vy)) for _ in range(REPS)]
        out["matvec_" + tag] = dict(stats(ms, 16 * n, yard), first_product_wall_s=round(first, 3))
        lib.lis_vector_destroy(vx)
        lib.lis_vector_destroy(vy)
        lib.lis_matrix_destroy(A)
    out["matvec_coo_over_csr"] = round(out["matvec_coo"]["median_ms"] / out["matvec_csr"]["median_ms"], 3)
    return out


def sizes(args, flag, default):
    if flag in args:
        return [int(t) for t in args[args.index(flag) + 1].split(",") if t]
    return default


def main():
    args = sys.argv[1:]
    lib = lis_amd.load()
    if not lis_amd.gpu_available():
        raise SystemExit("coo_dns_probe: no HIP device -- nothing here is measured without one")
    assert lib.initialize([]) == 0
    name = (C.c_char * 128)()
    lib.dll.liship_device_name(name, 128)
    info = (C.c_int * 4)()
    check(lib.liship_dns_tile_info(info))
    yard = yardstick(lib)
    doc = {"tool": "tools/coo_dns_probe.py", "device": name.value.decode(), "yardstick_13_reads_1_write": yard, "dns_tiles": list(info),
           "dns": [dns_case(lib, n, yard["TB_per_s"]) for n in sizes(args, "--dns", [8192, 16384])],
           "coo": [coo_case(lib, N, yard["TB_per_s"]) for N in sizes(args, "--coo", [256])]}
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
