"""One rank of a multi-process test of the distributed layer (row-block partition, ghost renumbering, halo
tables, halo exchange, cross-rank folds).  Launched by tests/test_distributed.py with RANK / WORLD_SIZE /
MASTER_ADDR / MASTER_PORT in the environment; collectives go through torch.distributed (gloo) installed
into the library as host-memory callbacks (lis_amd_comm_init_callbacks).

    python tests/dist_worker.py host     # CPU only: tables + host halo exchange + local products by the oracle
    python tests/dist_worker.py device   # GPU box: lis_matvec / lis_solve on every rank's HBM slice
    python tests/dist_worker.py rccl     # >= WORLD_SIZE GPUs: the same checks with an RCCL communicator, one GPU per rank --
                                         # grouped ncclSend/ncclRecv halos, ncclAllGather + rank-order folds, the overlap stream
    python tests/dist_worker.py renumber # GPU box: every rank renumbers ITS rows and owned columns inside its plan (ghost columns kept apart) and lis_solve
                                         # iterates in those numberings -- the halo export lists renumbered with them
"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

import lis_amd  # noqa: E402
import lisdrv  # noqa: E402
import orc  # noqa: E402
from lis_amd import _capi as capi  # noqa: E402

from lis_amd._hostcomm import Callbacks, make_callbacks  # noqa: E402,F401


def isie(rank, world, n):
    q, r = divmod(n, world)
    if rank < r:
        return (q + 1) * rank, (q + 1) * rank + q + 1
    return q * rank + r, q * rank + r + q


def local_rows(ptr, idx, val, is_, ie):
    p = (ptr[is_:ie + 1] - ptr[is_]).astype(np.int32)
    return p, idx[ptr[is_]:ptr[ie]].copy(), val[ptr[is_]:ptr[ie]].copy()


def main():
    mode = sys.argv[1]
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    lib = lis_amd.load()
    if mode == "rccl":
        # rank 0's unique id travels over the gloo control plane; the data plane of everything below is RCCL over xGMI
        uid = [None]
        if rank == 0:
            buf = (C.c_char * 128)()
            assert lib.dll.lis_amd_comm_get_unique_id(buf) == 0
            uid[0] = bytes(buf)
        dist.broadcast_object_list(uid, src=0)
        assert lib.dll.lis_amd_comm_init_rccl(uid[0], rank, world, int(os.environ.get("LOCAL_RANK", rank))) == 0
        assert lib.dll.lis_amd_comm_kind() == 1
        mode = "device"
        tag = "rccl"
    else:
        tag = mode
        cb = make_callbacks(world)
        lib.dll.lis_amd_comm_init_callbacks.argtypes = [C.POINTER(Callbacks), C.c_int, C.c_int]
        assert lib.dll.lis_amd_comm_init_callbacks(C.byref(cb), rank, world) == 0
    assert lib.initialize([]) == 0
    assert lib.dll.lis_amd_comm_rank() == rank and lib.dll.lis_amd_comm_size() == world
    lib.dll.lis_amd_halo_exchange_host.argtypes = [capi.PM, capi.P_DBL]
    if mode == "renumber":
        renumber_checks(lib, rank, world)
        dist.barrier()
        print(f"rank {rank}/{world} {tag} OK", flush=True)
        dist.destroy_process_group()
        return

    cases = {
        "poisson_unaligned": orc.poisson3d(5, 4, 3),                  # 60 rows: slabs cut through planes
        "poisson_planes": orc.poisson3d(2 * world, 5, 4),
        "irregular": orc.random_csr(211, 7, seed=3),                  # far-away ghosts, empty rows
        "block_diagonal": (np.arange(41, dtype=np.int32), np.arange(40, dtype=np.int32), np.full(40, 2.0)),  # no ghosts at all
    }
    for name, (ptr, idx, val) in cases.items():
        gn = len(ptr) - 1
        is_, ie = isie(rank, world, gn)
        n = ie - is_
        lp, li, lv = local_rows(ptr, idx, val, is_, ie)
        A = lisdrv.make_csr(lib, lp, li, lv, n=0, gn=gn)             # set_size(A, 0, gn): LIS_GET_ISIE split
        a = A.contents
        assert (a.n, a.gn, a.is_, a.ie, a.nprocs, a.my_rank) == (n, gn, is_, ie, world, rank), name
        if world > 1:
            assert list(a.ranges[:world + 1]) == [isie(r, world, gn)[0] for r in range(world)] + [gn]

        # ghost renumbering: owned g -> g - is, ghosts -> n + rank among the sorted distinct ghost columns
        ghosts = np.unique(li[(li < is_) | (li >= ie)])
        assert a.np == n + len(ghosts), name
        want = np.where((li >= is_) & (li < ie), li - is_, n + np.searchsorted(ghosts, li)).astype(np.int32)
        got = lisdrv.matrix_arrays(A)
        assert np.array_equal(got["index"], want), name
        if len(ghosts):
            assert np.array_equal(np.ctypeslib.as_array(a.l2g_map, shape=(len(ghosts),)), ghosts), name

        # halo tables: neighbours ascending, import slots contiguous per owner, exports = what the peer imports
        t = a.commtable.contents
        nb = t.neibpetot
        neib = list(t.neibpe[:nb])
        assert neib == sorted(neib) and rank not in neib
        owners = np.searchsorted(np.array([isie(r, world, gn)[1] for r in range(world)]), ghosts, side="right")
        assert t.imnnz == len(ghosts)
        for i, p in enumerate(neib):
            assert t.import_ptr[i + 1] - t.import_ptr[i] == int(np.sum(owners == p)), name
        assert list(t.import_index[:t.imnnz]) == list(range(n, n + len(ghosts)))
        all_ghosts = [None] * world
        dist.all_gather_object(all_ghosts, ghosts)
        for i, p in enumerate(neib):
            mine = all_ghosts[p][(all_ghosts[p] >= is_) & (all_ghosts[p] < ie)] - is_
            assert list(t.export_index[t.export_ptr[i]:t.export_ptr[i + 1]]) == list(mine), name

        # halo exchange + local product == the rows of the global product, bit for bit
        xg = np.random.default_rng(17).uniform(-1, 1, gn)
        xl = np.zeros(a.np)
        xl[:n] = xg[is_:ie]
        if tag == "rccl":
            xl[n:] = xg[ghosts]                                        # the host-array exchange belongs to the callback communicator
        else:
            assert lib.dll.lis_amd_halo_exchange_host(A, xl.ctypes.data_as(capi.P_DBL)) == 0
            assert np.array_equal(xl[n:], xg[ghosts]), name
        yg = orc.spmv_csr(ptr, idx, val, xg)
        assert np.array_equal(orc.spmv_csr(got["ptr"], got["index"], got["value"], xl), yg[is_:ie]), name

        # BSR of the local block: ghost columns start on a fresh block column (lis_matrix_bsr.c:425-428), i.e. they are
        # shifted by pad = (bnc - n % bnc) % bnc, and the halo lands at x[n + pad ...) (commtable->pad)
        for bs in (2, 3):
            B = lisdrv.convert(lib, A, "bsr", bs, bs)
            g = lisdrv.matrix_arrays(B)
            pad = (bs - n % bs) % bs
            assert g["pad"] == pad + ((bs - len(ghosts) % bs) % bs if len(ghosts) else 0), (name, bs, g["pad"], pad)   # front + back padding (:97-102)
            xb = np.zeros(max(g["nc"] * bs, a.np + pad))
            xb[:n] = xg[is_:ie]
            xb[n + pad:n + pad + len(ghosts)] = xg[ghosts]
            yb = orc.spmv_bsr(n, g["nr"], bs, bs, g["bptr"], g["bindex"], g["value"], xb)
            sc = orc.spmv_csr(ptr, idx, np.abs(val), np.abs(xg))[is_:ie] + 1e-300
            assert np.all(np.abs(yb - yg[is_:ie]) <= 1e-13 * sc), (name, bs)
            lib.lis_matrix_destroy(B)

        # a solve the multi-rank job cannot serve is refused BEFORE A and b are touched: -scale jacobi -storage bsr retypes, splits and scales A in place and scales b,
        # and the solvers that multiply by A^T would then fail at their first transposed product of the split matrix (one rank only, lis_matvech.c)
        if world > 1 and False:       # round 6: served now (lis_matvech.c: the split walk's transposed rows + the reverse halo) -- device_checks solves it instead
            S = capi.PS()
            assert lib.lis_solver_create(C.byref(S)) == 0
            assert lib.lis_solver_set_option(b"-i bicg -p none -scale jacobi -storage bsr -maxiter 5 -print none", S) == 0
            vb, vs = lisdrv.new_vector(lib, A, None), lisdrv.new_vector(lib, A, None)
            assert lib.lis_vector_set_values2(capi.LIS_INS_VALUE, is_, n, np.ascontiguousarray(yg[is_:ie]).ctypes.data_as(capi.P_DBL), vb) == 0
            devnull, saved = os.open(os.devnull, os.O_WRONLY), os.dup(2)       # (the refusal prints the reference's "file(line) : func : error" line)
            os.dup2(devnull, 2)
            try:
                rc = lib.lis_solve(A, vb, vs, S)
            finally:
                os.dup2(saved, 2); os.close(devnull); os.close(saved)
            assert rc == capi.LIS_ERR_NOT_IMPLEMENTED, (name, rc)
            assert a.matrix_type == 1 and a.is_splited == 0 and a.is_scaled == 0, (name, a.matrix_type)      # still the CSR matrix it was
            after = lisdrv.matrix_arrays(A)
            assert np.array_equal(after["value"], got["value"]) and np.array_equal(after["index"], got["index"]), name
            bvals = np.empty(n)
            assert lib.lis_vector_get_values(vb, is_, n, bvals.ctypes.data_as(capi.P_DBL)) == 0 and np.array_equal(bvals, yg[is_:ie]), name
            lib.lis_solver_destroy(S); lib.lis_vector_destroy(vb); lib.lis_vector_destroy(vs)

        # vectors of the partition: ranges, gather, infinity norm (host-side collectives)
        v = lisdrv.new_vector(lib, A, None)
        assert (v.contents.n, v.contents.np, v.contents.gn, v.contents.is_) == (n, a.np, gn, is_)
        for i in range(n):
            assert lib.lis_vector_set_value(capi.LIS_INS_VALUE, is_ + i, float(xg[is_ + i]), v) == 0    # global indices
        assert lib.lis_vector_set_value(capi.LIS_INS_VALUE, (ie) % gn if world > 1 else gn, 1.0, v) == capi.LIS_ERR_ILL_ARG
        full = np.zeros(gn)
        assert lib.lis_vector_gather(v, full.ctypes.data_as(capi.P_DBL)) == 0
        assert np.array_equal(full, xg), name
        out = C.c_double()
        assert lib.lis_vector_nrmi(v, C.byref(out)) == 0 and out.value == np.abs(xg).max()

        if mode == "device":
            device_checks(lib, name, A, ptr, idx, val, xg, yg, is_, ie, gn)
        lib.lis_vector_destroy(v)
        lib.lis_matrix_destroy(A)

    io_checks(lib, rank, world)
    if mode == "device":
        device_poisson_generator(lib, rank, world)
    dist.barrier()
    if tag == "rccl":
        assert lib.dll.lis_amd_comm_finalize() == 0
    print(f"rank {rank}/{world} {tag} OK", flush=True)
    dist.destroy_process_group()


def io_checks(lib, rank, world):
    """Matrix Market in a multi-rank job (lis_input_mm.c: every rank reads the file and keeps its rows; the writers take
    turns in rank order): local rows / vectors equal the slices of the single-process golden arrays, and the files the
    ranks write together are the bytes one process writes."""
    import tempfile
    here = os.path.dirname(os.path.abspath(__file__))
    G = np.load(os.path.join(here, "golden", "mm_golden.npz"))
    path = [None]
    if rank == 0:
        path[0] = tempfile.mkdtemp(prefix="lis_dist_io_")
    dist.broadcast_object_list(path, src=0)
    for fname in ("gen_general_b.mtx", "gen_symmetric_bx.mtx", "gen_binary_bx.mtx", "testmat.mtx", "gen_general_shuffled.mtx"):
        A, b, x = capi.PM(), capi.PV(), capi.PV()
        assert lib.lis_matrix_create(0, C.byref(A)) == 0
        assert lib.lis_vector_create(0, C.byref(b)) == 0 and lib.lis_vector_create(0, C.byref(x)) == 0
        assert lib.lis_input(A, b, x, os.path.join(here, "golden", "mm", fname).encode()) == 0, fname
        a = A.contents
        gptr, gidx, gval = G[f"{fname}/ptr"], G[f"{fname}/index"], G[f"{fname}/value"]
        gn = len(gptr) - 1
        is_, ie = isie(rank, world, gn)
        assert (a.n, a.gn, a.is_, a.ie) == (ie - is_, gn, is_, ie), fname
        got = lisdrv.matrix_arrays(A)
        l2g = np.ctypeslib.as_array(a.l2g_map, shape=(a.np - a.n,)) if a.np > a.n else np.zeros(0, np.int32)
        cols = np.where(got["index"] < a.n, got["index"] + is_, l2g[np.maximum(got["index"] - a.n, 0)] if len(l2g) else 0)
        lo, hi = gptr[is_], gptr[ie]
        assert np.array_equal(got["ptr"], gptr[is_:ie + 1] - lo), fname
        assert np.array_equal(cols, gidx[lo:hi]) and np.array_equal(got["value"], gval[lo:hi]), fname
        for tag, v in (("b", b), ("x", x)):
            if f"{fname}/{tag}" in G.files:
                vals = np.empty(ie - is_)
                assert lib.lis_vector_get_values(v, is_, ie - is_, vals.ctypes.data_as(capi.P_DBL)) == 0
                assert np.array_equal(vals, G[f"{fname}/{tag}"][is_:ie]), (fname, tag)
        out = os.path.join(path[0], f"{fname}.out")
        assert lib.lis_output_matrix(A, 2, out.encode()) == 0
        dist.barrier()
        if rank == 0:
            assert np.array_equal(np.frombuffer(open(out, "rb").read(), np.uint8), G[f"{fname}/out_matrix"]), fname
        dist.barrier()
        if f"{fname}/b" in G.files:
            for fmt, tag in ((1, "plain"), (2, "mm")):
                assert lib.lis_output_vector(b, fmt, out.encode()) == 0
                dist.barrier()
                if rank == 0:
                    assert np.array_equal(np.frombuffer(open(out, "rb").read(), np.uint8), G[f"{fname}/out_b_{tag}"]), (fname, tag)
                dist.barrier()
        lib.lis_matrix_destroy(A); lib.lis_vector_destroy(b); lib.lis_vector_destroy(x)
    dist.barrier()
    if rank == 0:
        import shutil
        shutil.rmtree(path[0], ignore_errors=True)


def device_checks(lib, name, A, ptr, idx, val, xg, yg, is_, ie, gn):
    """Every rank drives its HBM slice: lis_matvec with the halo exchange, global reductions, lis_solve."""
    n = ie - is_
    vx, vy = lisdrv.new_vector(lib, A, None), lisdrv.new_vector(lib, A, None)
    assert lib.lis_vector_set_values2(capi.LIS_INS_VALUE, is_, n, np.ascontiguousarray(xg[is_:ie]).ctypes.data_as(capi.P_DBL), vx) == 0
    assert lib.lis_matvec(A, vx, vy) == 0
    y = np.empty(n)
    assert lib.lis_vector_get_values(vy, is_, n, y.ctypes.data_as(capi.P_DBL)) == 0
    assert np.array_equal(y, yg[is_:ie]), name                        # distributed SpMV: bit-identical rows
    out = C.c_double()
    assert lib.lis_vector_dot(vx, vy, C.byref(out)) == 0
    assert abs(out.value - float(np.dot(xg, yg))) <= 1e-13 * float(np.abs(xg * yg).sum()), name
    assert lib.lis_vector_nrm2(vy, C.byref(out)) == 0 and abs(out.value - np.linalg.norm(yg)) <= 1e-13 * np.linalg.norm(yg)
    # a vector that was NOT made from the matrix (no room for ghosts) grows inside lis_matvec like the reference's lis_realloc (include/lis_matvec.h:32-43):
    # the header AND the host array -- a program may read X->value[n .. np) afterwards
    vs = capi.PV()
    assert lib.lis_vector_create(capi.LIS_COMM_WORLD, C.byref(vs)) == 0 and lib.lis_vector_set_size(vs, n, 0) == 0
    assert vs.contents.np == n
    assert lib.lis_vector_set_values2(capi.LIS_INS_VALUE, is_, n, np.ascontiguousarray(xg[is_:ie]).ctypes.data_as(capi.P_DBL), vs) == 0
    assert lib.lis_matvec(A, vs, vy) == 0
    assert lib.lis_vector_get_values(vy, is_, n, y.ctypes.data_as(capi.P_DBL)) == 0 and np.array_equal(y, yg[is_:ie]), name
    a_np, a_pad = A.contents.np, A.contents.pad
    assert vs.contents.np == a_np and vs.contents.pad == a_pad
    host = np.ctypeslib.as_array(vs.contents.value, shape=(a_np + a_pad,))
    assert np.array_equal(host[:n], xg[is_:ie])                        # the owned entries kept their place (and the memory beyond them exists)
    assert host[a_np + a_pad - 1] == host[a_np + a_pad - 1]
    lib.lis_vector_destroy(vs)
    # distributed A^T x: local transposed rows + ghost contributions sent back to their owners (lis_reduce);
    # the cross-rank adds change the association, so 1e-13 relative instead of bit equality
    yt = orc.spmvh_csr(ptr, idx, val, xg)
    assert lib.lis_matvech(A, vx, vy) == 0
    assert lib.lis_vector_get_values(vy, is_, n, y.ctypes.data_as(capi.P_DBL)) == 0
    scale = orc.spmvh_csr(ptr, idx, np.abs(val), np.abs(xg))[is_:ie] + 1e-300
    assert np.all(np.abs(y - yt[is_:ie]) <= 1e-13 * scale), name
    scale_y = orc.spmv_csr(ptr, idx, np.abs(val), np.abs(xg))[is_:ie] + 1e-300
    # the NATIVE ELL / DIA kernels behind the overlapped halo (interior rows while it travels, boundary rows after), overlap on and off:
    # with the row form switched off a constant-coefficient matrix keeps its layout.
    if name.startswith("poisson"):
        lib.dll.lis_amd_set_row_form(0)
        try:
            for fmt in ("ell", "dia"):
                for overlap in (0, 1):
                    lib.dll.lis_amd_set_overlap(overlap)
                    Ac = lisdrv.convert(lib, A, "csr")          # (a copy: csr2dia sorts the rows of its INPUT)
                    B = lisdrv.convert(lib, Ac, fmt)
                    lib.lis_matrix_destroy(Ac)
                    vb2, vy2 = lisdrv.new_vector(lib, B, None), lisdrv.new_vector(lib, B, None)
                    assert lib.lis_vector_set_values2(capi.LIS_INS_VALUE, is_, n, np.ascontiguousarray(xg[is_:ie]).ctypes.data_as(capi.P_DBL), vb2) == 0
                    assert lib.lis_matvec(B, vb2, vy2) == 0, (name, fmt)
                    assert lib.lis_vector_get_values(vy2, is_, n, y.ctypes.data_as(capi.P_DBL)) == 0
                    assert np.all(np.abs(y - yg[is_:ie]) <= 1e-13 * scale_y), (name, fmt, overlap)
                    if fmt == "ell":
                        assert np.array_equal(y, yg[is_:ie]), (name, fmt, overlap)
                    lib.lis_vector_destroy(vb2); lib.lis_vector_destroy(vy2); lib.lis_matrix_destroy(B)
        finally:
            lib.dll.lis_amd_set_row_form(1)
            lib.dll.lis_amd_set_overlap(1)
    # the same product from every other storage format of the local block (ghost columns included): same rows to
    # 1e-13 relative (CSC / BSR / DIA add a row's terms in another order), every format behind the halo exchange
    for fmt in ("csc", "ell", "jad", "bsr", "dia"):
        if fmt == "dia" and not name.startswith("poisson"):
            continue
        B = lisdrv.convert(lib, A, fmt)
        vb2, vy2 = lisdrv.new_vector(lib, B, None), lisdrv.new_vector(lib, B, None)
        assert lib.lis_vector_set_values2(capi.LIS_INS_VALUE, is_, n, np.ascontiguousarray(xg[is_:ie]).ctypes.data_as(capi.P_DBL), vb2) == 0
        assert lib.lis_matvec(B, vb2, vy2) == 0, (name, fmt)
        assert lib.lis_vector_get_values(vy2, is_, n, y.ctypes.data_as(capi.P_DBL)) == 0
        assert np.all(np.abs(y - yg[is_:ie]) <= 1e-13 * scale_y), (name, fmt)
        if fmt in ("ell", "jad"):
            assert np.array_equal(y, yg[is_:ie]), (name, fmt)
        # A^T x through the same format: the local transposed rows + the reverse halo (ghost sums back to their owners)
        assert lib.lis_matvech(B, vb2, vy2) == 0, (name, fmt)
        assert lib.lis_vector_get_values(vy2, is_, n, y.ctypes.data_as(capi.P_DBL)) == 0
        assert np.all(np.abs(y - yt[is_:ie]) <= 1e-13 * scale), (name, fmt, "A^T x")
        if fmt == "bsr":                                               # 3 x 3 blocks: n % 3 != 0 on some rank puts the ghost block columns `pad` entries behind the owned ones
            B3 = lisdrv.convert(lib, A, "bsr", 3, 3)
            vb3, vy3 = lisdrv.new_vector(lib, B3, None), lisdrv.new_vector(lib, B3, None)
            assert lib.lis_vector_set_values2(capi.LIS_INS_VALUE, is_, n, np.ascontiguousarray(xg[is_:ie]).ctypes.data_as(capi.P_DBL), vb3) == 0
            assert lib.lis_matvech(B3, vb3, vy3) == 0, (name, "bsr3")
            assert lib.lis_vector_get_values(vy3, is_, n, y.ctypes.data_as(capi.P_DBL)) == 0
            assert np.all(np.abs(y - yt[is_:ie]) <= 1e-13 * scale), (name, "bsr 3x3", "A^T x")
            assert lib.lis_matvec(B3, vb3, vy3) == 0 and lib.lis_vector_get_values(vy3, is_, n, y.ctypes.data_as(capi.P_DBL)) == 0
            assert np.all(np.abs(y - yg[is_:ie]) <= 1e-13 * scale_y), (name, "bsr 3x3", "A x")
            lib.lis_vector_destroy(vb3); lib.lis_vector_destroy(vy3); lib.lis_matrix_destroy(B3)
            assert lib.lis_matvec(B, vb2, vy2) == 0 and lib.lis_vector_get_values(vy2, is_, n, y.ctypes.data_as(capi.P_DBL)) == 0
        if fmt == "bsr":                                               # the block rows without ghost blocks under the halo, the others behind it: the bits of exchange-first
            y_overlapped = y.copy()
            lib.dll.lis_amd_set_overlap(0)
            assert lib.lis_matvec(B, vb2, vy2) == 0, (name, fmt)
            lib.dll.lis_amd_set_overlap(1)
            assert lib.lis_vector_get_values(vy2, is_, n, y.ctypes.data_as(capi.P_DBL)) == 0
            assert np.array_equal(y, y_overlapped), (name, fmt, "overlap")
        lib.lis_vector_destroy(vb2); lib.lis_vector_destroy(vy2); lib.lis_matrix_destroy(B)
    if name == "block_diagonal":
        # a SPLIT JAD matrix on ranks without ghost columns: its HBM copy is two CSR halves and a diagonal with no row-range form, so it must not take the
        # CSR branch that runs the interior rows under the halo (that returned L x alone).  One term per row: the bits of the single-process product
        B = lisdrv.convert(lib, A, "jad")
        assert lib.lis_matrix_split(B) == 0 and B.contents.is_splited and B.contents.np == B.contents.n
        vb2, vy2 = lisdrv.new_vector(lib, B, None), lisdrv.new_vector(lib, B, None)
        assert lib.lis_vector_set_values2(capi.LIS_INS_VALUE, is_, n, np.ascontiguousarray(xg[is_:ie]).ctypes.data_as(capi.P_DBL), vb2) == 0
        assert lib.lis_matvec(B, vb2, vy2) == 0, (name, "split jad")
        assert lib.lis_vector_get_values(vy2, is_, n, y.ctypes.data_as(capi.P_DBL)) == 0
        assert np.array_equal(y, yg[is_:ie]), (name, "split jad", y[:4], yg[is_:is_ + 4])
        lib.lis_vector_destroy(vb2); lib.lis_vector_destroy(vy2); lib.lis_matrix_destroy(B)
    if name.startswith("poisson"):
        bg = orc.spmv_csr(ptr, idx, val, np.ones(gn))
        vb, vs = lisdrv.new_vector(lib, A, None), lisdrv.new_vector(lib, A, None)
        assert lib.lis_vector_set_values2(capi.LIS_INS_VALUE, is_, n, np.ascontiguousarray(bg[is_:ie]).ctypes.data_as(capi.P_DBL), vb) == 0
        for solver, precon, ref in (("cg", "jacobi", orc.cg), ("bicgstab", "none", orc.bicgstab), ("gmres", "none", orc.gmres),
                                    ("bicg", "jacobi", orc.bicg)):
            S = capi.PS()
            lib.lis_solver_create(C.byref(S))
            lib.lis_solver_set_option(f"-i {solver} -p {precon} -tol 1e-12 -maxiter 500 -restart 20".encode(), S)
            assert lib.lis_solve(A, vb, vs, S) == 0
            xs = np.empty(n)
            assert lib.lis_vector_get_values(vs, is_, n, xs.ctypes.data_as(capi.P_DBL)) == 0
            kw = {"restart": 20} if solver == "gmres" else {}
            xo, it, rc, resid, _ = ref(ptr, idx, val, bg, precon=precon, maxiter=500, **kw)
            assert S.contents.retcode == 0 and S.contents.resid <= 1e-12, (name, solver)
            if solver in ("cg", "bicg"):
                assert S.contents.iter == it, (name, solver, S.contents.iter, it)
            else:
                assert abs(S.contents.iter - it) <= max(3, it // 10), (name, solver, S.contents.iter, it)
            assert np.allclose(xs, xo[is_:ie], rtol=0, atol=1e-9), (name, solver)
            lib.lis_solver_destroy(S)
        # the solvers on the other storage formats of the same partition (BiCG also needs their A^T with the reverse halo)
        xo, it, _, _, _ = orc.cg(ptr, idx, val, bg, precon="jacobi", maxiter=500)
        for fmt in ("ell", "jad", "bsr", "csc", "dia"):
            B = lisdrv.convert(lib, A, fmt)
            for opts in ("-i cg -p jacobi", "-i bicg -p none", "-i bicgstab -p jacobi"):
                vb2, vs2 = lisdrv.new_vector(lib, B, None), lisdrv.new_vector(lib, B, None)
                assert lib.lis_vector_set_values2(capi.LIS_INS_VALUE, is_, n, np.ascontiguousarray(bg[is_:ie]).ctypes.data_as(capi.P_DBL), vb2) == 0
                S = capi.PS()
                lib.lis_solver_create(C.byref(S))
                lib.lis_solver_set_option(f"{opts} -tol 1e-12 -maxiter 500".encode(), S)
                assert lib.lis_solve(B, vb2, vs2, S) == 0, (name, fmt, opts)
                xs = np.empty(n)
                assert lib.lis_vector_get_values(vs2, is_, n, xs.ctypes.data_as(capi.P_DBL)) == 0
                assert S.contents.retcode == 0 and S.contents.resid <= 1e-12, (name, fmt, opts, S.contents.retcode, S.contents.resid)
                assert abs(S.contents.iter - it) <= max(3, it // 4) or "bicgstab" in opts, (name, fmt, opts, S.contents.iter, it)
                assert np.allclose(xs, xo[is_:ie], rtol=0, atol=1e-9), (name, fmt, opts)
                lib.lis_solver_destroy(S); lib.lis_vector_destroy(vb2); lib.lis_vector_destroy(vs2)
            lib.lis_matrix_destroy(B)
        # the other short-recurrence solvers share the collective vector kernels: spot-check a few per family
        for opts in ("-i cgs", "-i cr", "-i gpbicg", "-i tfqmr", "-i bicgsafe", "-i orthomin -restart 10", "-i bicr", "-i crs",
                     "-i bicrstab", "-i fgmres -restart 20", "-i minres", "-i idrs -irestart 2", "-i bicgstabl -ell 2", "-i jacobi"):
            vs2 = lisdrv.new_vector(lib, A, None)
            S = capi.PS()
            lib.lis_solver_create(C.byref(S))
            lib.lis_solver_set_option(f"{opts} -p none -tol 1e-11 -maxiter 3000".encode(), S)
            assert lib.lis_solve(A, vb, vs2, S) == 0, (name, opts)
            xs = np.empty(n)
            assert lib.lis_vector_get_values(vs2, is_, n, xs.ctypes.data_as(capi.P_DBL)) == 0
            assert S.contents.retcode == 0, (name, opts, S.contents.retcode, S.contents.iter, S.contents.resid)
            assert np.allclose(xs, xo[is_:ie], rtol=0, atol=1e-7), (name, opts, np.abs(xs - xo[is_:ie]).max())
            lib.lis_solver_destroy(S); lib.lis_vector_destroy(vs2)
        # round 6: A^T x of a SPLIT matrix in a multi-rank job (ref src/matvec/lis_matvec.c:191-349: lis_matvech_<fmt> of the split parts + LIS_MATVEC_REDUCE) -- by hand
        # on a split CSR copy, and through the solver options that reach it: -scale jacobi -storage bsr retypes, splits and block-scales A, BiCG then multiplies by its A^T
        B = lisdrv.convert(lib, A, "csr")
        assert lib.lis_matrix_split(B) == 0 and B.contents.is_splited
        vb2, vy2 = lisdrv.new_vector(lib, B, None), lisdrv.new_vector(lib, B, None)
        assert lib.lis_vector_set_values2(capi.LIS_INS_VALUE, is_, n, np.ascontiguousarray(xg[is_:ie]).ctypes.data_as(capi.P_DBL), vb2) == 0
        assert lib.lis_matvech(B, vb2, vy2) == 0, name
        assert lib.lis_vector_get_values(vy2, is_, n, y.ctypes.data_as(capi.P_DBL)) == 0
        assert np.all(np.abs(y - yt[is_:ie]) <= 1e-13 * scale), (name, "split A^T x")
        assert lib.lis_matvec(B, vb2, vy2) == 0 and lib.lis_vector_get_values(vy2, is_, n, y.ctypes.data_as(capi.P_DBL)) == 0
        assert np.all(np.abs(y - yg[is_:ie]) <= 1e-13 * scale_y), (name, "split A x")
        lib.lis_vector_destroy(vb2); lib.lis_vector_destroy(vy2); lib.lis_matrix_destroy(B)
        for opts in ("-i bicg -p none -scale jacobi -storage bsr", "-i bicg -p none -scale jacobi -storage bsr -storage_block 3"):
            B = lisdrv.convert(lib, A, "csr")
            vb2, vs2 = lisdrv.new_vector(lib, B, None), lisdrv.new_vector(lib, B, None)
            assert lib.lis_vector_set_values2(capi.LIS_INS_VALUE, is_, n, np.ascontiguousarray(bg[is_:ie]).ctypes.data_as(capi.P_DBL), vb2) == 0
            S = capi.PS()
            lib.lis_solver_create(C.byref(S))
            lib.lis_solver_set_option(f"{opts} -tol 1e-12 -maxiter 500 -print none".encode(), S)
            assert lib.lis_solve(B, vb2, vs2, S) == 0, (name, opts)
            xs = np.empty(n)
            assert lib.lis_vector_get_values(vs2, is_, n, xs.ctypes.data_as(capi.P_DBL)) == 0
            assert S.contents.retcode == 0 and B.contents.is_splited and B.contents.matrix_type == capi.LIS_MATRIX_BSR, (name, opts, S.contents.retcode)
            assert np.allclose(xs, xo[is_:ie], rtol=0, atol=1e-8), (name, opts, np.abs(xs - xo[is_:ie]).max())
            lib.lis_solver_destroy(S); lib.lis_vector_destroy(vb2); lib.lis_vector_destroy(vs2); lib.lis_matrix_destroy(B)
        # -scale in a distributed job: symm_diag needs the diagonal of the ghost columns (one halo of d)
        for scale, opts in (("symm_diag", "-i cg -p none"), ("jacobi", "-i bicgstab -p none")):
            B = lisdrv.convert(lib, A, "csr")                       # scaling rewrites the matrix: work on a copy
            vb2, vs2 = lisdrv.new_vector(lib, B, None), lisdrv.new_vector(lib, B, None)
            assert lib.lis_vector_set_values2(capi.LIS_INS_VALUE, is_, n, np.ascontiguousarray(bg[is_:ie]).ctypes.data_as(capi.P_DBL), vb2) == 0
            S = capi.PS()
            lib.lis_solver_create(C.byref(S))
            lib.lis_solver_set_option(f"{opts} -scale {scale} -tol 1e-12 -maxiter 500".encode(), S)
            assert lib.lis_solve(B, vb2, vs2, S) == 0, (name, scale)
            xs = np.empty(n)
            assert lib.lis_vector_get_values(vs2, is_, n, xs.ctypes.data_as(capi.P_DBL)) == 0
            assert S.contents.retcode == 0, (name, scale, S.contents.retcode)
            assert np.allclose(xs, xo[is_:ie], rtol=0, atol=1e-8), (name, scale, np.abs(xs - xo[is_:ie]).max())
            lib.lis_solver_destroy(S); lib.lis_vector_destroy(vb2); lib.lis_vector_destroy(vs2); lib.lis_matrix_destroy(B)


def renumber_checks(lib, rank, world):
    """Round 6: the plan-time renumbering on several ranks.  A 3-dof mesh (81 entries per row) cut into row blocks, the NODES of every block
    numbered at random inside it -- a partitioned mesh whose local numbering has no locality.  Every rank's plan renumbers its rows and owned columns on the device
    (ghost columns keep their numbers, the rows that read one go behind the others), lis_matvec keeps the bits of the single-process product, and lis_solve iterates
    in the ranks' own numberings: b, x0, 1/diag gathered once, the export lists of the halo renumbered with the rows, x scattered back -- the counts and the
    solution of the run in the caller's numbering (sums fold in another order), with the overlap of interior rows and halo on and off."""
    dll = lib.dll
    dll.lis_amd_set_reorder_after.argtypes = [C.c_longlong]
    dll.lis_amd_matrix_reordered.argtypes = [capi.PM]; dll.lis_amd_matrix_reordered.restype = C.c_longlong
    for case in ("fem3", "mesh"):
        _renumber_case(lib, rank, world, case)


def _renumber_matrix(case, world):
    if case == "mesh":
        # round 6, second half: ONE unknown per node, ragged rows of 7 .. 32 entries -- short rows, whose plans try block-local columns since then.  201 600 nodes along
        # a Morton curve of 4^3 cells (the row blocks of the ranks are pieces of space), numbered at random inside a cell: the lists fail, the ordering's six landmarks
        # and the block-local kernel on P A P^T take over -- with ghost columns in every rank's lists
        return orc.unstructured_mesh(201600, cells=4)
    G = 42                                                         # 74 088 nodes, 222 264 rows: >= 65 536 rows on each of 2 or 3 ranks, nodes divisible by both
    ptr, idx, val = orc.fem3(G, 3)[:3]
    gn = len(ptr) - 1
    nodes = gn // 3
    assert nodes % world == 0
    rng = np.random.default_rng(77)
    pn = np.concatenate([r * (nodes // world) + rng.permutation(nodes // world) for r in range(world)])
    perm = (3 * pn[:, None] + np.arange(3)[None, :]).reshape(-1)
    inv = np.empty(gn, np.int64); inv[perm] = np.arange(gn)
    lens = np.diff(ptr)[perm]
    p2 = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    src = np.repeat(np.asarray(ptr[:-1], np.int64)[perm] - p2[:-1], lens) + np.arange(p2[-1])
    return p2, inv[idx[src]].astype(np.int32), val[src]


def _renumber_case(lib, rank, world, case):
    dll = lib.dll
    ptr, idx, val = _renumber_matrix(case, world)
    gn = len(ptr) - 1
    is_, ie = isie(rank, world, gn)
    n = ie - is_
    assert n >= 65536
    lp, li, lv = local_rows(ptr, idx, val, is_, ie)
    xg = np.random.default_rng(19).uniform(-1, 1, gn)
    yg = orc.spmv_csr(ptr, idx, val, xg)
    xt = np.cos(np.arange(gn) * 0.37) + 1.5
    bg = orc.spmv_csr(ptr, idx, val, xt)
    dll.lis_amd_set_reorder_after(0)                               # the renumbered form at plan time (the default builds it after 4096 products)
    try:
        A = lisdrv.make_csr(lib, lp, li, lv, n=0, gn=gn)
        assert A.contents.np > A.contents.n                        # (there are ghost columns)
        vx, vy, vb, vs = (lisdrv.new_vector(lib, A, None) for _ in range(4))
        assert lib.lis_vector_set_values2(capi.LIS_INS_VALUE, is_, n, np.ascontiguousarray(xg[is_:ie]).ctypes.data_as(capi.P_DBL), vx) == 0
        assert lib.lis_vector_set_values2(capi.LIS_INS_VALUE, is_, n, np.ascontiguousarray(bg[is_:ie]).ctypes.data_as(capi.P_DBL), vb) == 0
        y = np.empty(n)
        assert lib.lis_matvec(A, vx, vy) == 0 and lib.lis_vector_get_values(vy, is_, n, y.ctypes.data_as(capi.P_DBL)) == 0
        assert np.array_equal(y.view(np.uint64), yg[is_:ie].view(np.uint64))
        listed = dll.lis_amd_matrix_reordered(A)
        assert listed > 0, "the rank's plan holds no renumbered form"
        runs = {}
        for opts in ("-i cg -p jacobi", "-i bicgstab -p none", "-i gmres -restart 30 -p jacobi", "-i bicg -p none"):
            for on, overlap in ((1, 1), (1, 0), (0, 1)):
                lib.liship_spmv_csr_set_reorder(on)
                dll.lis_amd_set_overlap(overlap)
                S = capi.PS()
                lib.lis_solver_create(C.byref(S))
                lib.lis_solver_set_option(f"{opts} -tol 1e-11 -maxiter 800 -initx_zeros true -print none".encode(), S)
                assert lib.lis_solve(A, vb, vs, S) == 0, (opts, on, overlap)
                want = 1 if on else 0                                          # (BiCG too: (P A P^T)^T of the rank's rows, the reverse halo at the renumbered export rows)
                assert dll.lis_amd_last_solve_renumbered() == want, (opts, on, overlap, dll.lis_amd_last_solve_renumbered())
                xs = np.empty(n)
                assert lib.lis_vector_get_values(vs, is_, n, xs.ctypes.data_as(capi.P_DBL)) == 0
                assert S.contents.retcode == 0, (case, opts, on, overlap, S.contents.retcode, S.contents.iter)
                runs[(opts, on, overlap)] = (S.contents.iter, xs)
                lib.lis_solver_destroy(S)
            lib.liship_spmv_csr_set_reorder(1)
            dll.lis_amd_set_overlap(1)
            it0, x0 = runs[(opts, 0, 1)]
            for key in ((opts, 1, 1), (opts, 1, 0)):
                it, xs = runs[key]
                slack = it0 // 7 if "bicgstab" in opts else it0 // 50
                assert abs(it - it0) <= max(1, slack), (key, it, it0)
                assert np.linalg.norm(xs - x0) <= 1e-8 * np.linalg.norm(x0) and np.linalg.norm(xs - xt[is_:ie]) <= 1e-7 * np.linalg.norm(xt[is_:ie]), key
        # the product after the solves: the caller's tables are back (the bits of the single-process product)
        assert lib.lis_matvec(A, vx, vy) == 0 and lib.lis_vector_get_values(vy, is_, n, y.ctypes.data_as(capi.P_DBL)) == 0
        assert np.array_equal(y.view(np.uint64), yg[is_:ie].view(np.uint64))
        for v in (vx, vy, vb, vs):
            lib.lis_vector_destroy(v)
        lib.lis_matrix_destroy(A)
    finally:
        dll.lis_amd_set_reorder_after(4096)
    if rank == 0:
        print(f"{case}: renumbered form on every rank; rank 0 lists {listed} columns", flush=True)


def device_poisson_generator(lib, rank, world):
    """lis_amd_matrix_poisson3d: HBM-generated slab + closed-form halo tables == the host path on the same rows."""
    l, m, n = 3 * world, 6, 5
    gn = l * m * n
    A = capi.PM()
    assert lib.lis_matrix_create(capi.LIS_COMM_WORLD, C.byref(A)) == 0
    assert lib.lis_matrix_set_size(A, 0, gn) == 0
    lib.dll.lis_amd_matrix_poisson3d.argtypes = [capi.PM, C.c_int, C.c_int, C.c_int, C.c_int]
    assert lib.dll.lis_amd_matrix_poisson3d(A, l, m, n, 0) == 0
    is_, ie = A.contents.is_, A.contents.ie
    ptr, idx, val = orc.poisson3d(l, m, n)
    xg = np.random.default_rng(5).uniform(-1, 1, gn)
    yg = orc.spmv_csr(ptr, idx, val, xg)
    vx, vy = lisdrv.new_vector(lib, A, None), lisdrv.new_vector(lib, A, None)
    nl = ie - is_
    assert lib.lis_vector_set_values2(capi.LIS_INS_VALUE, is_, nl, np.ascontiguousarray(xg[is_:ie]).ctypes.data_as(capi.P_DBL), vx) == 0
    assert lib.lis_matvec(A, vx, vy) == 0
    y = np.empty(nl)
    assert lib.lis_vector_get_values(vy, is_, nl, y.ctypes.data_as(capi.P_DBL)) == 0
    assert np.array_equal(y, yg[is_:ie])
    # The form a 512^3 slab takes (x beyond the Infinity Cache): the two-rows-per-lane value-record kernels, forced here, on a
    # partitioned matrix -- ghost columns at constant offsets keep the rows on a few (offsets, values) patterns -- through the
    # overlapped interior / boundary launches and the fused dots of CG: the bits of the one-row kernels
    l, m, n = 4 * world, 24, 20
    gn = l * m * n
    B = capi.PM()
    assert lib.lis_matrix_create(capi.LIS_COMM_WORLD, C.byref(B)) == 0
    assert lib.lis_matrix_set_size(B, 0, gn) == 0
    assert lib.dll.lis_amd_matrix_poisson3d(B, l, m, n, 0) == 0
    is_, ie = B.contents.is_, B.contents.ie
    nl = ie - is_
    ptr, idx, val = orc.poisson3d(l, m, n)
    xg = np.random.default_rng(6).uniform(-1, 1, gn)
    yg = orc.spmv_csr(ptr, idx, val, xg)
    bx, by, bb, bs = (lisdrv.new_vector(lib, B, None) for _ in range(4))
    assert lib.lis_vector_set_values2(capi.LIS_INS_VALUE, is_, nl, np.ascontiguousarray(xg[is_:ie]).ctypes.data_as(capi.P_DBL), bx) == 0
    assert lib.lis_vector_set_values2(capi.LIS_INS_VALUE, is_, nl, np.ascontiguousarray(yg[is_:ie]).ctypes.data_as(capi.P_DBL), bb) == 0
    got = {}
    for variant in (0, 0x4000):
        lib.liship_spmv_csr_set_variant(variant)
        assert lib.lis_matvec(B, bx, by) == 0
        yy = np.empty(nl)
        assert lib.lis_vector_get_values(by, is_, nl, yy.ctypes.data_as(capi.P_DBL)) == 0
        assert np.array_equal(yy, yg[is_:ie]), variant
        S = capi.PS()
        assert lib.lis_solver_create(C.byref(S)) == 0
        assert lib.lis_solver_set_option(b"-i cg -p jacobi -tol 1e-12 -maxiter 500 -initx_zeros true", S) == 0
        assert lib.lis_solve(B, bb, bs, S) == 0
        it = C.c_int()
        lib.lis_solver_get_iter(S, C.byref(it))
        xs = np.empty(nl)
        assert lib.lis_vector_get_values(bs, is_, nl, xs.ctypes.data_as(capi.P_DBL)) == 0
        got[variant] = (it.value, xs)
        lib.lis_solver_destroy(S)
    lib.liship_spmv_csr_set_variant(0)
    assert lib.dll.lis_amd_matrix_value_records(B) == 1
    # 0x4000: the fused dots as the row blocks' partial sums; 0: a partial per tile of the dominant-pattern product -- the same sums to rounding,
    # so the same count (give or take one at the tolerance) and the same solution to the tolerance
    assert abs(got[0][0] - got[0x4000][0]) <= 1 and 10 < got[0][0] < 500 and np.allclose(got[0][1], got[0x4000][1], rtol=0, atol=1e-9)
    assert np.allclose(got[0][1], xg[is_:ie], rtol=0, atol=1e-8)


if __name__ == "__main__":
    main()
