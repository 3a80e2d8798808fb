"""VBR storage: what the lane-per-row kernel reaches beside the other layouts of the same matrix.  Prints ONE JSON object and writes it to
profiles/vbr_probe.json.
    python tools/vbr_probe.py [--side 578]
Matrices: the finite-element class of tests/vbr_cases.py at about a million rows -- a side x side mesh of nodes, 5-point couplings, a dense block per
coupling -- once with 3 unknowns per node (`fem3`: uniform 3 x 3 blocks) and once with 1 .. 3 (`fem123`: variable blocks, about the same n).
Times, all in this process beside liship_stream_yardstick (13 reads : 1 write): liship_spmv_vbr_f64 on the six arrays; lis_matvec of the matrix in VBR
storage (the same kernel behind the dispatcher), of the same matrix in CSR storage under the default plan and in the reference layout
(lis_amd_set_reference_layout: the row-gather product on ptr / index / value as they stand), and -- the uniform case -- in BSR 3 x 3 storage.
Each: ms by device events, the bytes the kernel is asked to move (arrays once, x once, y once), and that time over bytes / the yardstick's rate.
The first five samples of every series are warm-up; median, 10th and 90th percentile of the 20 that follow."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import lis_amd  # noqa: E402
import lisdrv  # noqa: E402
import vbr_drv as drv  # noqa: E402
from lis_amd import DeviceArray as DA, check  # noqa: E402

WARM, REPS = 5, 25


def stats(ms, nbytes, yard=None):
    t = np.array(ms[WARM:])
    med = float(np.median(t))
    out = {"median_ms": round(med, 4), "p10_ms": round(float(np.percentile(t, 10)), 4), "p90_ms": round(float(np.percentile(t, 90)), 4), "samples": len(t),
           "bytes": int(nbytes), "TB_per_s": round(nbytes / (med * 1e-3) / 1e12, 3) if med > 0 else None}
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


def mesh_vbr(side, unknowns, seed):
    """the VBR arrays of the mesh, blocks of a block row in the order below, left, self, right, above; random values, a dominant diagonal"""
    nodes = side * side
    start = np.concatenate([[0], np.cumsum(unknowns)]).astype(np.int64)
    a = np.arange(nodes)
    i, j = a // side, a % side
    nb = np.stack([np.where(i > 0, a - side, -1), np.where(j > 0, a - 1, -1), a, np.where(j < side - 1, a + 1, -1), np.where(i < side - 1, a + side, -1)], axis=1)
    have = nb >= 0
    bptr = np.concatenate([[0], np.cumsum(have.sum(axis=1))]).astype(np.int32)
    bindex = nb[have].astype(np.int32)
    of_row = np.repeat(a, have.sum(axis=1))
    size = unknowns[of_row].astype(np.int64) * unknowns[bindex]
    ptr = np.concatenate([[0], np.cumsum(size)])
    assert ptr[-1] < 2**31
    value = np.random.default_rng(seed).uniform(-1, 1, int(ptr[-1]))
    return dict(n=int(start[-1]), nr=nodes, nc=nodes, bnnz=len(bindex), nnz=int(ptr[-1]), row=start.astype(np.int32), col=start.astype(np.int32),
                ptr=ptr.astype(np.int32), bptr=bptr, bindex=bindex, value=value), of_row


def csr_of(v, of_row):
    """the same matrix as CSR rows, a row's entries block after block in stored order, a block's columns ascending (what vbr2csr gives without the zero test)"""
    h = np.diff(v["row"])[of_row].astype(np.int64)
    blk = np.repeat(np.arange(v["bnnz"]), np.diff(v["ptr"]))
    off = np.arange(v["nnz"]) - v["ptr"][blk]
    ii, jj = off % h[blk], off // h[blk]
    r = v["row"][of_row][blk] + ii
    order = np.lexsort((jj, blk, r))
    ptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=v["n"]))]).astype(np.int32)
    return ptr, (v["col"][v["bindex"]][blk] + jj)[order].astype(np.int32), v["value"][order]


def case(lib, tag, side, unknowns, yard):
    dll = lib.dll
    v, of_row = mesh_vbr(side, unknowns, side)
    csr = csr_of(v, of_row)
    n, nnz = v["n"], v["nnz"]
    x = np.random.default_rng(2).uniform(-1, 1, n)
    out = {"matrix": tag, "side": side, "n": n, "stored_values": nnz, "blocks": v["bnnz"], "block_rows": v["nr"]}
    vbr_bytes = 8 * nnz + 4 * (2 * v["bnnz"] + 1) + 4 * 2 * (v["nr"] + 1) + 4 * (v["nc"] + 1) + 4 * n + 16 * n
    # the kernel on the six arrays
    d = {f: DA.from_host(v[f]) for f in ("row", "col", "ptr", "bptr", "bindex", "value")}
    flags = C.c_int(-1)
    check(lib.liship_vbr_check(n, n, nnz, v["nr"], v["nc"], v["bnnz"], d["row"].ptr, d["col"].ptr, d["ptr"].ptr, d["bptr"].ptr, d["bindex"].ptr, C.byref(flags), None))
    assert flags.value == 0
    brow, dx, dy = DA(n, np.int32), DA.from_host(x), DA.zeros(n, np.float64)
    check(lib.liship_vbr_block_rows(n, v["nr"], d["row"].ptr, brow.ptr, None))
    timer = Timer(lib, None)
    ms = [timer.time(lambda: check(lib.liship_spmv_vbr_f64(n, d["row"].ptr, d["col"].ptr, d["ptr"].ptr, d["bptr"].ptr, d["bindex"].ptr, brow.ptr, d["value"].ptr,
                                                          dx.ptr, dy.ptr, None))) for _ in range(REPS)]
    out["liship_spmv_vbr_f64"] = stats(ms, vbr_bytes, yard)
    y_kernel = dy.to_host()
    for a in list(d.values()) + [brow, dx, dy]:
        a.free()
    # the same matrix behind lis_matvec, in four storages
    dll.lis_amd_stream.restype = C.c_void_p
    dll.lis_amd_set_reference_layout.argtypes = [C.c_int]
    timer = Timer(lib, dll.lis_amd_stream())
    runs = [("vbr", 0, vbr_bytes), ("csr_default_plan", 0, 12 * nnz + 4 * (n + 1) + 16 * n), ("csr_reference_layout", 1, 12 * nnz + 4 * (n + 1) + 16 * n)]
    if len(set(unknowns.tolist())) == 1:
        runs.append(("bsr_3x3", 0, 8 * nnz + 4 * v["bnnz"] + 4 * (v["nr"] + 1) + 16 * n))
    for name, ref_layout, nbytes in runs:
        assert dll.lis_amd_set_reference_layout(ref_layout) == 0
        if name == "vbr":
            A = drv.make_vbr(lib, v)
        else:
            A = lisdrv.make_csr(lib, *csr)
            if name == "bsr_3x3":
                B = lisdrv.convert(lib, A, "bsr", 3, 3)
                lib.lis_matrix_destroy(A)
                A = B
        vx, vy = lisdrv.new_vector(lib, A, x), lisdrv.new_vector(lib, A)
        assert lib.lis_matvec(A, vx, vy) == 0
        ms = [timer.time(lambda: lib.lis_matvec(A, vx, vy)) for _ in range(REPS)]
        y = lisdrv.get_vector(lib, vy, n)
        out["lis_matvec_" + name] = dict(stats(ms, nbytes, yard), same_bits_as_the_vbr_kernel=bool(y.tobytes() == y_kernel.tobytes()))
        lib.lis_vector_destroy(vx)
        lib.lis_vector_destroy(vy)
        lib.lis_matrix_destroy(A)
    assert dll.lis_amd_set_reference_layout(0) == 0
    out["vbr_over_csr_default_plan"] = round(out["liship_spmv_vbr_f64"]["median_ms"] / out["lis_matvec_csr_default_plan"]["median_ms"], 3)
    out["vbr_over_csr_reference_layout"] = round(out["liship_spmv_vbr_f64"]["median_ms"] / out["lis_matvec_csr_reference_layout"]["median_ms"], 3)
    return out


def main():
    args = sys.argv[1:]
    side = int(args[args.index("--side") + 1]) if "--side" in args else 578
    lib = lis_amd.load()
    if not lis_amd.gpu_available():
        raise SystemExit("vbr_probe: no HIP device -- nothing here is measured without one")
    assert lib.initialize([]) == 0
    name = (C.c_char * 128)()
    lib.dll.liship_device_name(name, 128)
    info = (C.c_int * 2)()
    check(lib.liship_vbr_tile_info(info))
    yard = yardstick(lib)
    side123 = int(round(side * (3 / 2) ** 0.5))
    doc = {"tool": "tools/vbr_probe.py", "device": name.value.decode(), "yardstick_13_reads_1_write": yard, "vbr_tiles": list(info),
           "cases": [case(lib, "fem3", side, np.full(side * side, 3), yard["TB_per_s"]),
                     case(lib, "fem123", side123, 1 + np.random.default_rng(3).integers(0, 3, side123 * side123), yard["TB_per_s"])]}
    text = json.dumps(doc, indent=1)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "vbr_probe.json"), "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
