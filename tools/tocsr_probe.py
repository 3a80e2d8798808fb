"""X -> CSR in HBM: what the count and fill kernels of kernels/convert.hip reach and what lis_matrix_convert gains by them.  Writes profiles/tocsr_probe.json
and prints it.
    python tools/tocsr_probe.py [--grid 256] [--dns 8192] [--side 578]
Workloads: the 7-point Poisson matrix on grid^3 in ELL, DIA and BSR 2 x 2; a dense matrix of dns^2 entries, one in twenty of them non-zero; the finite-element
mesh of tools/vbr_probe.py (3 unknowns per node) in VBR.
kernels   liship_<fmt>_csr_count and liship_<fmt>_to_csr on device arrays, ms by device events (the count entry ends in a synchronize: its time holds the scan
          and the read-back of the total).  bytes = the source read twice + the CSR arrays written once; the ratio is (count + fill) over the time the box's
          streaming yardstick (liship_stream_yardstick, 13 reads : 1 write, measured in the same process) needs for those bytes.
convert   wall seconds of one lis_matrix_convert(X, CSR), the stream drained before and after, four ways in this order:
            hbm_lazy    X made by a conversion in HBM, its host arrays never read -- the HBM path;
            host_first  the same call with lis_amd_set_device_convert(0): X's arrays come home over the bus, then the host routine, then the upload of the result;
            host_again  once more: the arrays are at home now, the host routine and the upload alone;
            hbm_home    the HBM path again, X's arrays at home (read from X's native copy, or uploaded into temporaries where the copy is a row form);
            hbm_no_copy the HBM path with X's arrays at home and X's copy dropped first: every source array crosses the bus into a temporary.
          DNS and VBR sources are made from host arrays (no conversion builds them lazily: hbm_lazy is absent, host_first has nothing to bring home).
shift     one lis_matrix_shift_matrix(X, I, 0.5) on the grid^3 matrix in ELL made in HBM: X -> CSR -> shift -> X.  The switch covers both directions, so
          with it off the way back to ELL runs on the host too.
Times: kernels, the first 3 samples are warm-up and the median of the 10 that follow is reported with the 10th / 90th percentile; conversions are single calls."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import coo_dns_drv  # noqa: E402
import lis_amd  # noqa: E402
import lisdrv  # noqa: E402
import vbr_drv  # noqa: E402
import vbr_probe  # noqa: E402
from lis_amd import DeviceArray as DA, _capi as capi, check  # noqa: E402

WARM, REPS = 3, 13
I32, F64 = np.int32, np.float64


def stats(ms):
    t = np.array(ms[WARM:])
    return {"median_ms": round(float(np.median(t)), 4), "p10_ms": round(float(np.percentile(t, 10)), 4), "p90_ms": round(float(np.percentile(t, 90)), 4), "samples": len(t)}


def kernels(lib, count_fn, fill_fn, source_bytes, n, yard):
    """count_fn(count, rptr, scratch, nnz_ref), fill_fn(rptr, ridx, rval) on device arrays -> the record of one workload"""
    timer = vbr_probe.Timer(lib, None)
    nnz = C.c_int(0)
    work = count_fn(None)                                            # cells the count entry counts over
    count, rptr, scratch = DA(work, I32), DA(n + 1, I32), DA(work // 4096 + 4, np.int64)
    extra = DA(work + 1, I32)
    cms = [timer.time(lambda: check(count_fn((count, extra, rptr, scratch, C.byref(nnz))))) for _ in range(REPS)]
    ridx, rval = DA(max(nnz.value, 1), I32), DA(max(nnz.value, 1), F64)
    fms = [timer.time(lambda: check(fill_fn((extra, rptr, ridx, rval)))) for _ in range(REPS)]
    nbytes = 2 * source_bytes + 12 * nnz.value + 4 * (n + 1)
    c, f = stats(cms), stats(fms)
    ideal_ms = nbytes / (yard * 1e12) * 1e3
    for a in (count, rptr, scratch, extra, ridx, rval):
        a.free()
    return {"n": n, "csr_nnz": nnz.value, "count": c, "fill": f, "bytes": int(nbytes), "yardstick_ms_for_bytes": round(ideal_ms, 4),
            "time_over_bytes_over_yardstick": round((c["median_ms"] + f["median_ms"]) / ideal_ms, 3)}


def poisson_csr(lib, N):
    n = N ** 3
    nnz = lib.liship_poisson3d_nnz(N, N, N, 0, n)
    ptr, idx, val = DA(n + 1, I32), DA(nnz, I32), DA(nnz, F64)
    check(lib.liship_poisson3d_csr(N, N, N, 0, n, 1, ptr.ptr, idx.ptr, val.ptr, None))
    check(lib.liship_device_synchronize())
    return n, int(nnz), ptr, idx, val


def grid_kernels(lib, N, yard):
    n, nnz, ptr, idx, val = poisson_csr(lib, N)
    out = {}
    # ELL
    mx = 7
    eidx, ev = DA(n * mx, I32), DA(n * mx, F64)
    check(lib.liship_csr_to_ell(n, mx, ptr.ptr, idx.ptr, val.ptr, eidx.ptr, ev.ptr, None))
    out["ell"] = kernels(lib, lambda a: n if a is None else lib.liship_ell_csr_count(n, mx, ev.ptr, a[0].ptr, a[2].ptr, a[3].ptr, a[4], None),
                         lambda a: lib.liship_ell_to_csr(n, mx, eidx.ptr, ev.ptr, a[1].ptr, a[2].ptr, a[3].ptr, None), 12 * n * mx, n, yard)
    eidx.free(); ev.free()
    # DIA
    used, slot, scratch, nnd = DA(2 * n, I32), DA(2 * n + 1, I32), DA(2 * n // 4096 + 4, np.int64), C.c_int(0)
    check(lib.liship_csr_dia_offsets(n, n, ptr.ptr, idx.ptr, used.ptr, slot.ptr, scratch.ptr, C.byref(nnd), None))
    offs, dv = DA(nnd.value, I32), DA(n * nnd.value, F64)
    check(lib.liship_csr_to_dia(n, n, nnd.value, ptr.ptr, idx.ptr, val.ptr, used.ptr, slot.ptr, offs.ptr, dv.ptr, None))
    for a in (used, slot, scratch):
        a.free()
    out["dia"] = kernels(lib, lambda a: n if a is None else lib.liship_dia_csr_count(n, n, nnd.value, offs.ptr, dv.ptr, a[0].ptr, a[2].ptr, a[3].ptr, a[4], None),
                         lambda a: lib.liship_dia_to_csr(n, n, nnd.value, offs.ptr, dv.ptr, a[1].ptr, a[2].ptr, a[3].ptr, None), 8 * n * nnd.value, n, yard)
    offs.free(); dv.free()
    # BSR 2 x 2
    nr = n // 2
    cnt, bptr, scratch, bnnz = DA(nr + 1, I32), DA(nr + 1, I32), DA(nr // 4096 + 4, np.int64), C.c_int(0)
    check(lib.liship_csr_bsr_count(n, n, 2, 2, ptr.ptr, idx.ptr, cnt.ptr, bptr.ptr, scratch.ptr, C.byref(bnnz), None))
    bidx, bv = DA(bnnz.value, I32), DA(4 * bnnz.value, F64)
    check(lib.liship_csr_to_bsr(n, 2, 2, bnnz.value, ptr.ptr, idx.ptr, val.ptr, bptr.ptr, bidx.ptr, bv.ptr, None))
    out["bsr2x2"] = kernels(lib, lambda a: n if a is None else lib.liship_bsr_csr_count(n, 2, 2, bptr.ptr, bidx.ptr, bv.ptr, a[0].ptr, a[2].ptr, a[3].ptr, a[4], None),
                            lambda a: lib.liship_bsr_to_csr(n, 2, 2, bptr.ptr, bidx.ptr, bv.ptr, a[1].ptr, a[2].ptr, a[3].ptr, None),
                            36 * bnnz.value + 4 * (nr + 1), n, yard)
    for a in (cnt, bptr, scratch, bidx, bv, ptr, idx, val):
        a.free()
    return out


def dense(n):
    rng = np.random.default_rng(n)
    d = rng.uniform(-1, 1, n * n)
    d[rng.uniform(size=n * n) >= 0.05] = 0.0
    return d


def dns_kernels(lib, n, d, slab, yard):
    dv = DA.from_host(d)
    cells = n * ((n + slab - 1) // slab)
    out = kernels(lib, lambda a: cells if a is None else lib.liship_dns_csr_count(n, n, dv.ptr, a[0].ptr, a[1].ptr, a[2].ptr, a[3].ptr, a[4], None),
                  lambda a: lib.liship_dns_to_csr(n, n, dv.ptr, a[0].ptr, a[2].ptr, a[3].ptr, None), 8 * n * n, n, yard)
    dv.free()
    return out


def vbr_kernels(lib, v, yard):
    n = v["n"]
    d = {f: DA.from_host(v[f]) for f in ("row", "col", "ptr", "bptr", "bindex", "value")}
    flags, brow = C.c_int(-1), DA(n + 4, I32)
    check(lib.liship_vbr_check(n, n, v["nnz"], v["nr"], v["nc"], v["bnnz"], d["row"].ptr, d["col"].ptr, d["ptr"].ptr, d["bptr"].ptr, d["bindex"].ptr, C.byref(flags), None))
    assert flags.value == 0
    check(lib.liship_vbr_block_rows(n, v["nr"], d["row"].ptr, brow.ptr, None))
    six = [d[f].ptr for f in ("row", "col", "ptr", "bptr", "bindex")] + [brow.ptr, d["value"].ptr]
    src = 8 * v["nnz"] + 4 * (2 * v["bnnz"] + 1) + 8 * (v["nr"] + 1) + 4 * (v["nc"] + 1) + 4 * n
    out = kernels(lib, lambda a: n if a is None else lib.liship_vbr_csr_count(n, *six, a[0].ptr, a[2].ptr, a[3].ptr, a[4], None),
                  lambda a: lib.liship_vbr_to_csr(n, *six, a[1].ptr, a[2].ptr, a[3].ptr, None), src, n, yard)
    for a in list(d.values()) + [brow]:
        a.free()
    return out


def convert_s(lib, X, on):
    """wall seconds of X -> CSR with the switch on / off, and which way lis_amd_convert_stats says it went"""
    dll = lib.dll
    before = (C.c_int * 2)()
    after = (C.c_int * 2)()
    dll.lis_amd_set_device_convert(1 if on else 0)
    dll.lis_amd_convert_stats(before)
    check(lib.liship_stream_synchronize(dll.lis_amd_stream()))
    t0 = time.perf_counter()
    err, B = coo_dns_drv.convert(lib, X, "csr")
    check(lib.liship_stream_synchronize(dll.lis_amd_stream()))
    secs = time.perf_counter() - t0
    dll.lis_amd_set_device_convert(1)
    dll.lis_amd_convert_stats(after)
    assert err == 0
    lib.lis_matrix_destroy(B)
    return {"seconds": round(secs, 4), "served": "hbm" if after[0] > before[0] else "host"}


def four_ways(lib, X, lazy):
    out = {}
    if lazy:
        assert lib.dll.lis_amd_matrix_lazy_arrays(X) > 0
        out["hbm_lazy"] = convert_s(lib, X, True)
        out["hbm_lazy_again"] = convert_s(lib, X, True)
    out["host_first"] = convert_s(lib, X, False)
    out["host_again"] = convert_s(lib, X, False)
    out["hbm_home"] = convert_s(lib, X, True)
    out["hbm_home_again"] = convert_s(lib, X, True)
    assert lib.dll.lis_amd_matrix_host_modified(X) == 0              # X's HBM copy is dropped: every array is uploaded into a temporary
    out["hbm_no_copy"] = convert_s(lib, X, True)
    hbm = [out[k]["seconds"] for k in out if k.startswith("hbm")]
    out["host_again_over_best_hbm"] = round(out["host_again"]["seconds"] / min(hbm), 2)
    out["host_again_over_worst_hbm"] = round(out["host_again"]["seconds"] / max(hbm), 2)
    return out


def poisson_matrix(lib, N):
    A = capi.PM()
    assert lib.lis_matrix_create(capi.LIS_COMM_WORLD, C.byref(A)) == 0 and lib.lis_matrix_set_size(A, 0, N ** 3) == 0
    assert lib.dll.lis_amd_matrix_poisson3d(A, N, N, N, 1) == 0
    return A


def shift_s(lib, X, B, on):
    dll = lib.dll
    dll.lis_amd_set_device_convert(1 if on else 0)
    check(lib.liship_stream_synchronize(dll.lis_amd_stream()))
    t0 = time.perf_counter()
    err = dll.lis_matrix_shift_matrix(X, B, 0.5)
    check(lib.liship_stream_synchronize(dll.lis_amd_stream()))
    secs = time.perf_counter() - t0
    dll.lis_amd_set_device_convert(1)
    assert err == 0
    return round(secs, 4)


def arg(args, flag, default):
    return int(args[args.index(flag) + 1]) if flag in args else default


def main():
    args = sys.argv[1:]
    N, nd, side = arg(args, "--grid", 256), arg(args, "--dns", 8192), arg(args, "--side", 578)
    lib = lis_amd.load()
    if not lis_amd.gpu_available():
        raise SystemExit("tocsr_probe: no HIP device -- nothing here is measured without one")
    assert lib.initialize([]) == 0
    dll = lib.dll
    dll.lis_amd_stream.restype = C.c_void_p
    dll.lis_amd_matrix_lazy_arrays.argtypes = [capi.PM]
    dll.lis_amd_matrix_host_modified.argtypes = [capi.PM]
    dll.lis_amd_matrix_poisson3d.argtypes = [capi.PM, C.c_int, C.c_int, C.c_int, C.c_int]
    dll.lis_matrix_shift_matrix.restype, dll.lis_matrix_shift_matrix.argtypes = capi.LIS_INT, [capi.PM, capi.PM, C.c_double]
    name = (C.c_char * 128)()
    dll.liship_device_name(name, 128)
    info = (C.c_int * 3)()
    check(lib.liship_tocsr_tile_info(info))
    yard = vbr_probe.yardstick(lib)
    doc = {"tool": "tools/tocsr_probe.py", "device": name.value.decode(), "yardstick_13_reads_1_write": yard, "tocsr_tiles": list(info), "grid": N, "dns_n": nd,
           "vbr_side": side, "kernels": {}, "convert": {}}
    Y = yard["TB_per_s"]
    doc["kernels"].update(grid_kernels(lib, N, Y))
    d = dense(nd)
    doc["kernels"]["dns"] = dns_kernels(lib, nd, d, info[1], Y)
    v, _ = vbr_probe.mesh_vbr(side, np.full(side * side, 3), side)
    doc["kernels"]["vbr"] = vbr_kernels(lib, v, Y)
    # lis_matrix_convert
    A = poisson_matrix(lib, N)
    for tag, fmt in (("ell", "ell"), ("dia", "dia"), ("bsr2x2", "bsr")):
        X = lisdrv.convert(lib, A, fmt)
        doc["convert"][tag] = four_ways(lib, X, True)
        lib.lis_matrix_destroy(X)
    X = coo_dns_drv.make_dns(lib, nd, d)
    del d
    doc["convert"]["dns"] = four_ways(lib, X, False)
    lib.lis_matrix_destroy(X)
    X = vbr_drv.make_vbr(lib, v)
    doc["convert"]["vbr"] = four_ways(lib, X, False)
    lib.lis_matrix_destroy(X)
    # lis_matrix_shift_matrix on the ELL matrix
    n = N ** 3
    B = lisdrv.make_csr(lib, np.arange(n + 1, dtype=I32), np.arange(n, dtype=I32), np.ones(n))
    X = lisdrv.convert(lib, A, "ell")
    doc["shift_matrix_ell"] = {"hbm_s": [shift_s(lib, X, B, True) for _ in range(2)], "switch_off_s": [shift_s(lib, X, B, False) for _ in range(2)]}
    for M in (X, B, A):
        lib.lis_matrix_destroy(M)
    text = json.dumps(doc, indent=1)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "tocsr_probe.json"), "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
