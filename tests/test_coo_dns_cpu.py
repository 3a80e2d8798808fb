"""COO and DNS storage without a device: the API (set / malloc / duplicate / copy / unset / get_diagonal / scale / shift), the host conversions in both
directions with the in-place sort of a COO source, the restated quicksort, every refusal, array-format input into DNS and the write watch -- all held,
bit for bit, to the reference's own results in tests/golden/coo_dns_bits.npz (tests/golden/make_golden_coo_dns.py).  The numpy models of
tests/coo_dns_cases.py, from which the GPU tests take their kernel-level expectations, are held to the same fixture here."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import coo_dns_cases as cc
import coo_dns_drv as drv
import lis_amd
import lisdrv
from lis_amd import _capi as capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", cc.FIXTURE))
COO, DNS, CSR = drv.COO, drv.DNS, capi.LIS_MATRIX_CSR
NOT_IMPLEMENTED = capi.LIS_ERR_NOT_IMPLEMENTED


@pytest.fixture(scope="module")
def lib():
    lib = lis_amd.load()
    assert lib.initialize([]) == 0
    return lib


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def build(lib, m, fmt):
    """matrix m in COO / DNS storage, through lis_matrix_malloc_<fmt> + lis_matrix_set_<fmt> from the fixture's arrays"""
    n = len(cc.matrix(m)[0]) - 1
    if fmt == "coo":
        return drv.make_coo(lib, n, G[m + "|coo|row"], G[m + "|coo|col"], G[m + "|coo|value"])
    return drv.make_dns(lib, n, G[m + "|dns|value"])


# ---------------------------------------------------------------------------------------------- the models against the fixture
@pytest.mark.parametrize("m", cc.MATRICES)
def test_models_give_the_reference_arrays_and_products(m):
    ptr, idx, val = cc.matrix(m)
    n = len(ptr) - 1
    x = cc.xvec(n)
    row, col, v = cc.csr2coo(ptr, idx, val)
    assert same(row, G[m + "|coo|row"]) and same(col, G[m + "|coo|col"]) and same(v, G[m + "|coo|value"])
    dns = cc.csr2dns(ptr, idx, val)
    assert same(dns, G[m + "|dns|value"])
    for got, key in zip(cc.dns2csr(n, n, dns), ("ptr", "index", "value")):
        assert same(got, G["%s|dns|csr|%s" % (m, key)]), key
    assert same(cc.coo_matvec(n, row, col, v, x), G[m + "|coo|y"]) and same(cc.dns_matvec(n, n, dns, x), G[m + "|dns|y"])
    for T in cc.THREADS:
        assert same(cc.coo_matvech(n, row, col, v, x), G["%s|coo|yt|T%d" % (m, T)])         # serial in every build: the same bits at every T
        assert same(cc.dns_matvech(n, n, dns, x, T), G["%s|dns|yt|T%d" % (m, T)])
    assert same(cc.coo_diagonal(n, row, col, v, np.full(n, 7.0)), G[m + "|coo|diag"])
    assert same(dns[np.arange(n) * (n + 1)], G[m + "|dns|diag"])
    if m != "rand301":
        assert same(cc.coo_shift(row, col, v, cc.SHIFT), G[m + "|coo|shift|value"]) and same(cc.dns_shift(n, dns, cc.SHIFT), G[m + "|dns|shift|value"])
    if m not in cc.UNSCALED:
        for tag, symm in (("jacobi", False), ("symm_diag", True)):
            assert same(cc.coo_scale(row, col, v, G["%s|coo|scale_%s|d" % (m, tag)], symm), G["%s|coo|scale_%s|value" % (m, tag)])
            assert same(cc.dns_scale(n, n, dns, G["%s|dns|scale_%s|d" % (m, tag)], symm), G["%s|dns|scale_%s|value" % (m, tag)])


@pytest.mark.parametrize("t", cc.TRIPLETS)
def test_model_sort_and_grouping_against_the_fixture(t):
    n, row, col, val = cc.triplets(t)
    x = cc.xvec(n)
    (ptr, idx, v), (srow, scol, sval) = cc.coo2csr(n, row, col, val)
    assert same(ptr, G[t + "|csr|ptr"]) and same(srow, G[t + "|after|row"]) and same(scol, G[t + "|after|col"]) and same(sval, G[t + "|after|value"])
    assert same(cc.coo_matvec(n, row, col, val, x), G[t + "|y_before"]) and same(cc.coo_matvec(n, srow, scol, sval, x), G[t + "|y_after"])
    assert not same(G[t + "|y_before"], G[t + "|y_after"])           # the sort moves entries inside rows: the reference's own product changes its bits
    # the row form in HBM is a STABLE grouping: its row sums are the serial walk's
    gptr, gidx, gval = cc.group_by_key(n, row, col, val)
    y = np.array([sum_chain(gval[gptr[r]:gptr[r + 1]] * x[gidx[gptr[r]:gptr[r + 1]]]) for r in range(n)])
    assert same(y, G[t + "|y_before"])


def sum_chain(terms):
    t = np.float64(0.0)
    for v in terms:
        t = t + v
    return t


# ---------------------------------------------------------------------------------------------- the API
@pytest.mark.parametrize("fmt", ["coo", "dns"])
@pytest.mark.parametrize("m", cc.MATRICES)
def test_set_duplicate_copy_diagonal_shift(lib, m, fmt):
    A = build(lib, m, fmt)
    a = A.contents
    n = a.n
    assert a.status == capi.FORMAT_ID[fmt] and a.matrix_type == capi.FORMAT_ID[fmt] and a.np == n
    assert a.nnz == (len(G[m + "|coo|row"]) if fmt == "coo" else 0)      # (DNS: lis_matrix_set_dns leaves nnz alone, as the reference does)
    t = C.c_int()
    assert lib.lis_matrix_get_type(A, C.byref(t)) == 0 and t.value == capi.FORMAT_ID[fmt]
    # duplicate: sized, unassembled; copy: the same arrays in every bit, at other addresses
    B = drv.duplicate_as(lib, A, fmt)
    assert B.contents.n == n and B.contents.status == -257
    assert lib.lis_matrix_copy(A, B) == 0
    got, want = drv.arrays(B), drv.arrays(A)
    for f in ("row", "col", "value"):
        if f in want:
            assert same(got[f], want[f]), f
    assert C.cast(B.contents.value, C.c_void_p).value != C.cast(a.value, C.c_void_p).value
    # the diagonal: COO keeps what the vector held where a row stores no (i,i)
    err, d = drv.diagonal(lib, A, np.full(n, 7.0))
    assert err == 0 and same(d, G["%s|%s|diag" % (m, fmt)])
    if m != "rand301":
        assert lib.lis_matrix_shift_diagonal(B, cc.SHIFT) == 0
        assert same(drv.arrays(B)["value"], G["%s|%s|shift|value" % (m, fmt)])
    assert lib.lis_matrix_destroy(B) == 0
    # unset: the arrays are the caller's again, the matrix is unassembled
    keep = [C.cast(p, C.c_void_p).value for p in (a.row, a.col, a.value) if p]
    assert lib.lis_matrix_unset(A) == 0 and A.contents.status == -257 and not A.contents.value and not A.contents.row and not A.contents.col
    lib.dll.lis_free.argtypes, lib.dll.lis_free.restype = [C.c_void_p], None
    for p in keep:
        lib.dll.lis_free(p)
    assert lib.lis_matrix_destroy(A) == 0


@pytest.mark.parametrize("fmt", ["coo", "dns"])
@pytest.mark.parametrize("m", [m for m in cc.MATRICES if m not in cc.UNSCALED])
@pytest.mark.parametrize("tag,action", [("jacobi", 1), ("symm_diag", 2)])
def test_scale(lib, m, fmt, tag, action):
    A = build(lib, m, fmt)
    err, b, d = drv.scale(lib, A, np.ones(A.contents.n), action)
    key = "%s|%s|scale_%s|" % (m, fmt, tag)
    assert err == 0 and same(drv.arrays(A)["value"], G[key + "value"]) and same(b, G[key + "b"]) and same(d, G[key + "d"])
    assert A.contents.is_scaled
    lib.lis_matrix_destroy(A)


def test_set_on_an_assembled_matrix_adopts_nothing_and_arguments_are_checked(lib):
    A = build(lib, "one", "coo")
    keep = C.cast(A.contents.value, C.c_void_p).value
    assert lib.lis_matrix_set_coo(5, None, None, None, A) == 0 and C.cast(A.contents.value, C.c_void_p).value == keep and A.contents.nnz == 1
    assert lib.lis_matrix_set_dns(None, A) == 0 and A.contents.matrix_type == COO
    lib.lis_matrix_destroy(A)
    v = capi.P_DBL()
    assert lib.lis_matrix_malloc_dns(-1, 3, C.byref(v)) == capi.LIS_ERR_ILL_ARG and not v
    assert lib.lis_matrix_malloc_dns(0, 0, C.byref(v)) == 0 and v
    lib.dll.lis_free.argtypes, lib.dll.lis_free.restype = [C.c_void_p], None
    lib.dll.lis_free(C.cast(v, C.c_void_p))
    assert "coo" in capi.FORMAT_ID and "dns" in capi.FORMAT_ID and capi.FORMAT_ID["coo"] == 10 and capi.FORMAT_ID["dns"] == 11


# ---------------------------------------------------------------------------------------------- conversions
@pytest.mark.parametrize("m", cc.MATRICES)
def test_csr_to_coo_and_dns_and_back(lib, m):
    ptr, idx, val = cc.matrix(m)
    A = lisdrv.make_csr(lib, ptr, idx, val)
    for fmt in ("coo", "dns"):
        err, B = drv.convert(lib, A, fmt)
        assert err == 0 and B.contents.matrix_type == capi.FORMAT_ID[fmt]
        a = drv.arrays(B)
        assert a["nnz"] == int(G["%s|%s|nnz" % (m, fmt)][0])
        for f in ("row", "col", "value"):
            if f in a:
                assert same(a[f], G["%s|%s|%s" % (m, fmt, f)]), (fmt, f)
        if (m, fmt) != ("rand301", "coo"):
            err, back = drv.convert(lib, B, "csr")
            assert err == 0
            c = lisdrv.matrix_arrays(back)
            for f in ("ptr", "index", "value"):
                assert same(c[f], G["%s|%s|csr|%s" % (m, fmt, f)]), (fmt, f)
            lib.lis_matrix_destroy(back)
        # through CSR to another format and between the two, as the reference's dispatcher goes
        err, E = drv.convert(lib, B, "ell")
        assert err == 0 and E.contents.matrix_type == capi.FORMAT_ID["ell"]
        lib.lis_matrix_destroy(E)
        other = "dns" if fmt == "coo" else "coo"
        err, O = drv.convert(lib, B, other)
        assert err == 0 and O.contents.matrix_type == capi.FORMAT_ID[other]
        if fmt == "coo":              # the dense form does not depend on the order of the triplets (the conversion sorts B on its way) -- but for
            assert m == "dups" or same(drv.arrays(O)["value"], G[m + "|dns|value"])      # duplicates, of which the last in the SORTED order wins
        else:                         # the triplets of the rows the dense form converts to: columns ascending, zeros gone
            n = len(ptr) - 1
            for f, want in zip(("row", "col", "value"), cc.csr2coo(*cc.dns2csr(n, n, G[m + "|dns|value"]))):
                assert same(drv.arrays(O)[f], want), f
        lib.lis_matrix_destroy(O)
        lib.lis_matrix_destroy(B)
    lib.lis_matrix_destroy(A)


@pytest.mark.parametrize("t", cc.TRIPLETS)
def test_coo_to_csr_sorts_the_source_in_place_as_the_reference_does(lib, t):
    n, row, col, val = cc.triplets(t)
    A = drv.make_coo(lib, n, row, col, val)
    err, B = drv.convert(lib, A, "csr")
    assert err == 0
    c, a = lisdrv.matrix_arrays(B), drv.arrays(A)
    assert same(c["ptr"], G[t + "|csr|ptr"]) and same(c["index"], G[t + "|after|col"]) and same(c["value"], G[t + "|after|value"])
    for f in ("row", "col", "value"):
        assert same(a[f], G["%s|after|%s" % (t, f)]), f
    assert A.contents.matrix_type == COO and A.contents.nnz == len(row)
    lib.lis_matrix_destroy(B)
    lib.lis_matrix_destroy(A)


def test_restated_sort_against_the_reference_on_keys_with_many_ties(lib, reflib):
    """lisi_sort_iid (host/lis_convert.c) and the reference's lis_sort_iid on 1000 seeded key arrays: the same permutation, element for element"""
    mine, theirs = lib.dll.lisi_sort_iid, reflib.dll.lis_sort_iid
    for f in (mine, theirs):
        f.restype, f.argtypes = None, [C.c_int, C.c_int, capi.P_INT, capi.P_INT, capi.P_DBL]
    rng = np.random.default_rng(1000)
    for case in range(1000):
        count = int(rng.integers(0, 300))
        keys = rng.integers(0, max(1, int(rng.integers(1, 12))), count).astype(np.int32)
        if case % 7 == 0:
            keys.sort()
        if case % 11 == 0:
            keys = keys[::-1].copy()
        out = []
        for f in (mine, theirs):
            k, tag, v = keys.copy(), np.arange(count, dtype=np.int32), np.arange(count, dtype=np.float64)
            f(0, count - 1, k.ctypes.data_as(capi.P_INT), tag.ctypes.data_as(capi.P_INT), v.ctypes.data_as(capi.P_DBL))
            out.append((k, tag, v))
        assert all(same(a, b) for a, b in zip(*out)), (case, count)
        assert same(out[0][0], np.sort(keys)) and same(out[0][1].astype(np.float64), out[0][2])
        for got, model in zip(out[0], cc.sort_iid(keys, np.arange(count, dtype=np.int32), np.arange(count, dtype=np.float64))):
            assert case % 50 or same(got, model)                     # (the numpy model is slow: every 50th case)


# ---------------------------------------------------------------------------------------------- refusals
def untouched(A, before):
    now = drv.arrays(A)
    return now["type"] == before["type"] and all(same(now[f], before[f]) for f in ("row", "col", "value") if f in before) and not A.contents.is_splited


@pytest.mark.parametrize("fmt", ["coo", "dns"])
def test_refusals_leave_the_matrix_alone(lib, fmt, capfd):
    m = "dups"
    ptr, idx, val = cc.matrix(m)
    n = len(ptr) - 1
    name = fmt.upper()
    A = build(lib, m, fmt)
    before = drv.arrays(A)
    capfd.readouterr()
    # lis_matrix_split
    assert lib.lis_matrix_split(A) == NOT_IMPLEMENTED and untouched(A, before)
    assert "lis_matrix_split: %s storage is not split" % name in capfd.readouterr().out
    # the preconditioners that rest on the split, on a matrix in this storage and on a CSR matrix asked to become it
    for holder, extra in ((A, ""), (None, " -storage " + fmt)):
        M = holder if holder is not None else lisdrv.make_csr(lib, ptr, idx, val)
        held = drv.arrays(M)
        for p, text in (("ssor", "-p ssor is served for CSR and BSR storage only"), ("is", "-p is is served for CSR storage only")):
            b, x = lisdrv.new_vector(lib, M, np.ones(n)), lisdrv.new_vector(lib, M, np.full(n, 3.0))
            S = capi.PS()
            assert lib.lis_solver_create(C.byref(S)) == 0 and lib.lis_solver_set_option(("-i cg -p %s%s" % (p, extra)).encode(), S) == 0
            assert lib.lis_solve(M, b, x, S) == NOT_IMPLEMENTED
            err = capfd.readouterr().out
            assert text in err and "A is untouched" in err, err
            if p == "ssor" and fmt == "coo":
                assert "the reference itself fails" in err
            now = drv.arrays(M)
            assert now["type"] == held["type"] and same(now["value"], held["value"]) and not M.contents.is_splited
            assert same(lisdrv.get_vector(lib, b), np.ones(n)) and same(lisdrv.get_vector(lib, x), np.full(n, 3.0))
            lib.lis_solver_destroy(S); lib.lis_vector_destroy(b); lib.lis_vector_destroy(x)
        if holder is None:
            lib.lis_matrix_destroy(M)
    # lis_matrix_shift_matrix with A or B in this storage
    Bc = lisdrv.make_csr(lib, ptr, idx, val)
    held = lisdrv.matrix_arrays(Bc)
    for first, second in ((A, Bc), (Bc, A)):
        assert lib.lis_matrix_shift_matrix(first, second, 0.5) == NOT_IMPLEMENTED
        assert "lis_matrix_shift_matrix: %s storage is not shifted by a matrix" % name in capfd.readouterr().out
        assert untouched(A, before) and same(lisdrv.matrix_arrays(Bc)["value"], held["value"])
    # lis_gesolve with A or B in this storage, or asked into it
    for first, second, extra in ((A, Bc, ""), (Bc, A, ""), (Bc, Bc, " -estorage " + fmt)):
        x = lisdrv.new_vector(lib, first, np.full(n, 3.0))
        E, ev = capi.PE(), C.c_double(0.0)
        assert lib.lis_esolver_create(C.byref(E)) == 0 and lib.lis_esolver_set_option(("-e gpi" + extra).encode(), E) == 0
        assert lib.lis_gesolve(first, second, x, C.byref(ev), E) == NOT_IMPLEMENTED
        assert "lis_gesolve: A and B in COO or DNS storage" in capfd.readouterr().out
        assert untouched(A, before) and same(lisdrv.matrix_arrays(Bc)["value"], held["value"]) and same(lisdrv.get_vector(lib, x), np.full(n, 3.0))
        lib.lis_esolver_destroy(E); lib.lis_vector_destroy(x)
    # MSR stays refused, from these storages too
    err, B = drv.convert(lib, A, "csr")
    assert err == 0
    lib.lis_matrix_destroy(B)
    M = capi.PM()
    lib.lis_matrix_duplicate(A, C.byref(M)); lib.lis_matrix_set_type(M, 3)
    assert lib.lis_matrix_convert(A, M) == NOT_IMPLEMENTED
    lib.lis_matrix_destroy(M); lib.lis_matrix_destroy(Bc); lib.lis_matrix_destroy(A)


RANKS_WORKER = r'''
import ctypes as C, os, sys
import numpy as np
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
import coo_dns_cases as cc, coo_dns_drv as drv, lis_amd, lisdrv
from lis_amd import _capi as capi
ALLGATHER = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t)
EXCHANGE = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_int))
class Callbacks(C.Structure):                      # lis_amd_comm_callbacks (include/lis_amd.h)
    _fields_ = [("allgather", ALLGATHER), ("neighbor_exchange", EXCHANGE), ("ctx", C.c_void_p)]
reached = []
def allgather(ctx, send, recv, nbytes): reached.append("allgather"); return 1
def exchange(ctx, nneib, neib, sendbuf, sptr, recvbuf, rptr): reached.append("exchange"); return 1
lib = lis_amd.load()
assert lib.initialize([]) == 0
ptr, idx, val = cc.matrix("dups")
n = len(ptr) - 1
row, col, v = cc.csr2coo(ptr, idx, val)
A = {"coo": drv.make_coo(lib, n, row, col, v), "dns": drv.make_dns(lib, n, cc.csr2dns(ptr, idx, val)), "csr": lisdrv.make_csr(lib, ptr, idx, val)}
vx, vy = lisdrv.new_vector(lib, A["csr"], np.ones(n)), lisdrv.new_vector(lib, A["csr"], np.full(n, 3.0))
before = {f: drv.arrays(A[f]) for f in A}
# the matrices were made by a job of one rank; from here on the library believes it is rank 0 of 2 (no callback is ever reached: every call below is refused first)
cb = Callbacks(ALLGATHER(allgather), EXCHANGE(exchange), None)
lib.dll.lis_amd_comm_init_callbacks.argtypes = [C.POINTER(Callbacks), C.c_int, C.c_int]
assert lib.dll.lis_amd_comm_init_callbacks(C.byref(cb), 0, 2) == 0
for fmt in ("coo", "dns"):
    assert lib.lis_matvec(A[fmt], vx, vy) == 5 and lib.lis_matvech(A[fmt], vx, vy) == 5
    B = drv.duplicate_as(lib, A[fmt], "csr")
    assert lib.lis_matrix_convert(A[fmt], B) == 5
    B = drv.duplicate_as(lib, A["csr"], fmt)
    assert lib.lis_matrix_convert(A["csr"], B) == 5
    for M, opts in ((A[fmt], "-i cg"), (A["csr"], "-i cg -storage " + fmt)):
        S = capi.PS()
        assert lib.lis_solver_create(C.byref(S)) == 0 and lib.lis_solver_set_option(opts.encode(), S) == 0
        assert lib.lis_solve(M, vx, vy, S) == 5
for f in A:
    now = drv.arrays(A[f])
    assert now["type"] == before[f]["type"] and now["value"].tobytes() == before[f]["value"].tobytes()
assert lisdrv.get_vector(lib, vy).tobytes() == np.full(n, 3.0).tobytes()
assert not reached, reached
print("REFUSED")
'''


def test_several_ranks_are_refused_before_anything_is_touched():
    out = subprocess.run([sys.executable, "-c", RANKS_WORKER % {"root": ROOT}], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "REFUSED" in out.stdout, out.stderr[-3000:]
    assert out.stdout.count("storage is served on one rank only (this job has 2)") >= 12, out.stderr[-3000:]


# ---------------------------------------------------------------------------------------------- input, write watch
def test_array_file_into_dns(lib, tmp_path):
    ptr, idx, val = cc.matrix("dups")
    n = len(ptr) - 1
    dns = cc.csr2dns(ptr, idx, val)
    path = tmp_path / "dense.mtx"
    path.write_text("%%%%MatrixMarket matrix array real general\n%d %d\n" % (n, n) + "".join("%s\n" % repr(float(v)) for v in dns))
    A = capi.PM()
    assert lib.lis_matrix_create(capi.LIS_COMM_WORLD, C.byref(A)) == 0 and lib.lis_matrix_set_type(A, DNS) == 0
    assert lib.lis_input_matrix(A, str(path).encode()) == 0
    a = drv.arrays(A)
    assert a["type"] == DNS and a["n"] == n and same(a["value"], dns)
    lib.lis_matrix_destroy(A)
    B = capi.PM()                                                # any other type: the CSR the dense values convert to, as before
    assert lib.lis_matrix_create(capi.LIS_COMM_WORLD, C.byref(B)) == 0
    assert lib.lis_input_matrix(B, str(path).encode()) == 0 and B.contents.matrix_type == CSR
    for got, want in zip((lisdrv.matrix_arrays(B)[f] for f in ("ptr", "index", "value")), cc.dns2csr(n, n, dns)):
        assert same(got, want)
    lib.lis_matrix_destroy(B)


def test_write_watch_sees_edits_of_coo_row_and_dns_value(lib):
    dll = lib.dll
    for f in (dll.lis_amd_matrix_page_test_watch, dll.lis_amd_matrix_protected_arrays, dll.lis_amd_matrix_host_written):
        f.argtypes = [capi.PM]
    A = build(lib, "stencil", "coo")
    assert dll.lis_amd_matrix_page_test_watch(A) == 3 and dll.lis_amd_matrix_protected_arrays(A) == 3 and dll.lis_amd_matrix_host_written(A) == 0
    hr = np.ctypeslib.as_array(A.contents.row, shape=(A.contents.nnz,))
    assert int(hr[4]) == int(G["stencil|coo|row"][4]) and dll.lis_amd_matrix_host_written(A) == 0      # reads are free
    hr[0] = int(hr[0])
    assert dll.lis_amd_matrix_host_written(A) == 1 and dll.lis_amd_matrix_protected_arrays(A) == 2
    lib.lis_matrix_destroy(A)
    A = build(lib, "stencil", "dns")
    n = A.contents.n
    assert dll.lis_amd_matrix_page_test_watch(A) == 1 and dll.lis_amd_matrix_protected_arrays(A) == 1
    hv = np.ctypeslib.as_array(A.contents.value, shape=(n * n,))
    hv[n * n - 1] = 2.0                                          # the last element of the n * n array lies on a watched page
    assert dll.lis_amd_matrix_host_written(A) == 1 and dll.lis_amd_matrix_protected_arrays(A) == 0 and hv[n * n - 1] == 2.0
    lib.lis_matrix_destroy(A)
