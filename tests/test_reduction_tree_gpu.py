"""Every sum of the default mode against tests/reduction_model.py, bit for bit: the fixed reduction tree of kernels/vector_ops.hip
(reduce_level1, block_sum / wave_sum, reduce_fold, reduce_final, finish_kernel) through every reduction entry point of liship.h,
and the chunked A^T x of kernels/transpose.hip.  tests/test_reduction_model_cpu.py pins the model to recorded MI355X bits and to
the reference's lis_matvech, and asserts what the alignment cases need: the two level-1 layouts give different bits on this data.

There is no tolerance in this module.  Comparisons are on uint64 views; a NaN the model computes has to be a NaN on the device
(IEEE 754 leaves sign and payload of a NaN result open) -- any NaN but the sentinel that marks memory nobody may write.  The work
buffer is filled with NaN before every call, so stale scratch cannot reach a result unseen; vectors are allocated over-long with
sentinels around the n elements, which have to survive the fused forms' stores."""
import ctypes as C

import numpy as np
import pytest

import lis_amd
import orc
import reduction_cases as rc
import reduction_model as rm
from lis_amd import DeviceArray as DA, check

pytestmark = pytest.mark.gpu
ERR_ARG = -1
SENT = np.uint64(0x7FF8DEAD0000BEEF)              # a quiet NaN no arithmetic here produces
NAN_BITS = np.float64(np.nan).view(np.uint64)
PAD = 6                                           # sentinels behind every vector


@pytest.fixture(scope="module")
def lib():
    lib = lis_amd.load()
    assert lis_amd.gpu_available(), "no HIP device: the product path has no CPU fallback"
    assert not lib.liship_missing
    return lib


@pytest.fixture(scope="module")
def work(lib):
    return DA(lib.liship_reduce_work_bytes() // 8, np.float64)


@pytest.fixture(scope="module")
def scal(lib):
    """the scalars the entry points take: by value, and the block in HBM the `_dev` forms and the Gram-Schmidt step read"""
    block = DA.from_host(rc.SCALARS)
    s = {"a": rc.A, "c": rc.DC, "block": block}
    s.update({name: block.ptr + 8 * k for k, name in enumerate(("pa", "psp", "pcb", "pcc"))})
    return s


@pytest.fixture(autouse=True)
def defaults(lib):
    """the tree is the DEFAULT mode: no guard, no announced step, no reference order -- before and after every test"""
    def reset():
        lib.liship_krylov_guard(None)
        lib.liship_krylov_chain(0, None, None)
        lib.liship_set_reference_reductions(0)
    reset()
    yield
    reset()
    lib.liship_device_synchronize()


def sentinels(k):
    return np.full(k, SENT, np.uint64).view(np.float64)


def canon(a):
    """bits with every NaN except the sentinel mapped to one NaN"""
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    b = a.view(np.uint64).copy()
    b[np.isnan(a) & (b != SENT)] = NAN_BITS
    return b


def differing(got, want):
    return np.nonzero(canon(got) != canon(want))[0][:8].tolist()


def poison(lib, work):
    check(lib.liship_memset(work.ptr, 0xFF, work.nbytes, None))          # every double a NaN


class Vec:
    """n doubles in HBM, `off` doubles (8 B each) past a 16 B aligned address, sentinels before and behind"""
    def __init__(self, host, off=0):
        self.n, self.off = len(host), off
        full = sentinels(off + self.n + PAD)
        full[off:off + self.n] = host
        self.da = DA.from_host(full)
        assert self.da.ptr % 16 == 0
        self.ptr = self.da.ptr + 8 * off

    def read(self):
        full = self.da.to_host()
        inside = full[self.off:self.off + self.n]
        outside = np.concatenate([full[:self.off], full[self.off + self.n:]])
        return inside, bool((outside.view(np.uint64) == SENT).all())


def run_case(lib, work, scal, entry, data, off_role=None):
    """one call of `entry` on `data` (role -> host array) with the array of `off_role` moved off 16 B alignment; -> what differs from the model"""
    n = len(data["x"])
    vecs = {role: Vec(data[role], 1 if role == off_role else 0) for role in entry.roles}
    res = DA.from_host(sentinels(4))
    poison(lib, work)
    check(entry.call(lib, n, {role: v.ptr for role, v in vecs.items()}, scal, res.ptr, work.ptr))
    check(lib.liship_device_synchronize())
    want, stored = rc.expected(entry, data, vector=off_role is None)
    got = res.to_host()
    bad = []
    if differing(got[:entry.nres], want):
        bad.append(("result", [hex(b) for b in canon(got[:entry.nres])], [hex(b) for b in canon(want)]))
    if not (got[entry.nres:].view(np.uint64) == SENT).all():
        bad.append(("result: written past its %d doubles" % entry.nres,))
    for role, v in vecs.items():
        inside, intact = v.read()
        if differing(inside, stored[role]):
            bad.append((role, differing(inside, stored[role])))
        if not intact:
            bad.append((role, "sentinel overwritten"))
    return bad


# ------------------------------------------------------------------------------------------------ every entry point, every edge
@pytest.mark.parametrize("entry", rc.ENTRIES, ids=repr)
def test_entry_point_gives_the_models_bits(lib, work, scal, entry):
    """aligned arrays (the vector path) at the lane, wavefront, block and odd-tail edges: results and stored vectors"""
    bad = {n: b for n in rc.SIZES for b in [run_case(lib, work, scal, entry, rc.case_data(entry, n))] if b}
    assert bad == {}


@pytest.mark.parametrize("entry", rc.ENTRIES, ids=repr)
def test_any_operand_off_alignment_takes_the_scalar_layout(lib, work, scal, entry):
    """each array in turn 8 B off (the in-place outputs are the arrays they overwrite): the scalar-path model's bits, which the CPU
    test shows to be other bits than the vector path's; with everything aligned again, the vector path's"""
    bad = {}
    for n in rc.ALIGN_SIZES:
        data = rc.case_data(entry, n)
        for role in entry.roles + "-":
            b = run_case(lib, work, scal, entry, data, None if role == "-" else role)
            if b:
                bad[(n, role)] = b
    assert bad == {}


@pytest.mark.parametrize("kind", rc.SPECIAL_KINDS)
def test_special_values(lib, work, scal, kind):
    bad = {name: b for name in rc.SPECIAL_ENTRIES for b in [run_case(lib, work, scal, rc.BY_NAME[name], rc.special_data(rc.BY_NAME[name], kind))] if b}
    assert bad == {}


@pytest.mark.parametrize("n", [1, 2048, 2049, 65537])
def test_nrm2_takes_the_root_once_of_the_final_sum(lib, work, n):
    """one block applies it in level 1, more blocks in the last fold: never to a partial"""
    x = rc.wide(np.random.default_rng(n), n)
    v, res = Vec(x), DA.from_host(sentinels(2))
    poison(lib, work)
    check(lib.liship_nrm2_f64(n, v.ptr, res.ptr, work.ptr, None))
    got = res.to_host()
    total = rm.tree(x * x)
    assert got[:1].view(np.uint64)[0] == np.sqrt(total).view(np.uint64) and got[1:].view(np.uint64)[0] == SENT
    partials = rm.level1_vector(x * x)
    assert len(partials) == {1: 1, 2048: 1, 2049: 2, 65537: 33}[n]
    if np.count_nonzero(partials) > 1:                                  # (2049: the second block holds no pair, and block 0 adds the tail)
        assert rm.fold(np.sqrt(partials)) != np.sqrt(total)             # a root per partial could not pass


# ------------------------------------------------------------------------------------------------ the folds alone
def slot_count(lib):
    return lib.liship_reduce_work_bytes() // 32


@pytest.mark.parametrize("want_sumsq", [0, 1])
def test_fold_of_partials_the_test_wrote(lib, work, want_sumsq):
    """finish_kernel (1), reduce_final (up to 2^14), reduce_fold + reduce_final (more) and the per-result strides, with no product
    kernel involved: wide-range partials at work[0, s) and work[slots, slots + s), NaN everywhere else"""
    slots = slot_count(lib)
    rng = np.random.default_rng(77)
    p0, p1 = rc.wide(rng, slots), rc.wide(rng, slots)
    bad = {}
    for used in (0, 1, 2, 1023, 1024, 1025, 16384, 16385, 18432, 18433, slots):
        host = np.full(4 * slots, np.nan)
        host[:used], host[slots:slots + used] = p0[:used], p1[:used]
        work.upload(host)
        res = DA.from_host(sentinels(3))
        check(lib.liship_spmv_csr_dot_finish_f64(used, want_sumsq, res.ptr, work.ptr, None))
        got = res.to_host()
        want = [rm.fold(p0[:used]) if used else 0.0] + ([rm.fold(p1[:used]) if used else 0.0] if want_sumsq else [])
        if differing(got[:len(want)], want) or got.view(np.uint64)[2] != SENT or (used and not want_sumsq and got.view(np.uint64)[1] != SENT):
            bad[used] = ([hex(b) for b in canon(got)], [hex(b) for b in canon(want)])
    assert bad == {}


def test_fold_refuses_more_slots_than_the_scratch_has(lib, work):
    res = DA.from_host(sentinels(2))
    assert lib.liship_spmv_csr_dot_finish_f64(slot_count(lib) + 1, 1, res.ptr, work.ptr, None) == ERR_ARG
    assert lib.liship_spmv_csr_dot_finish_f64(-1, 1, res.ptr, work.ptr, None) == ERR_ARG
    check(lib.liship_device_synchronize())
    assert (res.to_host().view(np.uint64) == SENT).all()


@pytest.mark.parametrize("name,matrix", [("p3d_64", lambda: orc.poisson3d(64, 64, 64)), ("rand_5000", lambda: orc.random_csr(5000, 11, seed=1))],
                         ids=["p3d_64", "rand_5000"])
def test_fold_of_the_fused_products_partials(lib, work, name, matrix):
    """the product in three row ranges parks its partials; the finish returns the model's fold of exactly those, for both results"""
    ptr, idx, val = matrix()
    n = len(ptr) - 1
    rng = np.random.default_rng(12)
    x, w = rc.wide(rng, max(n, int(idx.max()) + 1)), rc.wide(rng, n)
    dptr, didx, dval = DA.from_host(ptr, np.int32), DA.from_host(idx, np.int32), DA.from_host(val, np.float64)
    dx, dw, dy = DA.from_host(x, np.float64), DA.from_host(w, np.float64), DA.from_host(np.full(n, np.nan), np.float64)
    plan = C.c_void_p()
    check(lib.liship_csr_plan_create(C.byref(plan), n, dptr.ptr, None))
    slots, lo, hi = slot_count(lib), n // 10, n - n // 7
    try:
        for want_sumsq in (1, 0):
            poison(lib, work)
            total, used = 0, C.c_int()
            for a, b in ((lo, hi), (0, lo), (hi, n)):
                check(lib.liship_spmv_csr_rows_dot_f64(plan, a, b, dptr.ptr, didx.ptr, dval.ptr, dx.ptr, dy.ptr, dw.ptr, want_sumsq, work.ptr, total,
                                                       C.byref(used), None))
                total += used.value
            parked = work.to_host()
            parts = [parked[:total]] + ([parked[slots:slots + total]] if want_sumsq else [])
            assert total >= 3 and not any(np.isnan(p).any() for p in parts)
            assert np.isnan(parked[total:slots]).all() and np.isnan(parked[slots + (total if want_sumsq else 0):]).all()
            res = DA.from_host(sentinels(3))
            check(lib.liship_spmv_csr_dot_finish_f64(total, want_sumsq, res.ptr, work.ptr, None))
            got = res.to_host()
            assert differing(got[:len(parts)], [rm.fold(p) for p in parts]) == []
            assert (got[len(parts):].view(np.uint64) == SENT).all()
    finally:
        check(lib.liship_csr_plan_destroy(plan))


# ------------------------------------------------------------------------------------------------ the large shapes
N_FLAT = 32 << 20                 # 16384 partials: the last size without a fold level, the last without non-temporal loads
N_NT = N_FLAT + 3                 # non-temporal loads, 16385 partials (reduce_fold, then reduce_final over 9), an odd tail


class Big:
    def __init__(self):
        rng = np.random.default_rng(2025)
        decades = 10.0 ** np.arange(-8, 8)
        self.host = {k: rng.uniform(-1.0, 1.0, N_NT) * decades[rng.integers(0, 16, N_NT)] for k in "xyv"}
        self.dev = {k: DA(N_NT + PAD, np.float64) for k in "xyv"}
        for k in "xyv":
            self.restore(k)

    def restore(self, k):
        self.dev[k].upload(np.concatenate([self.host[k], sentinels(PAD)]))

    def unchanged(self, k, want, n):
        """the first n elements are `want`, the rest of the array and the sentinels behind it as uploaded"""
        got = self.dev[k].to_host()
        return differing(got[:n], want) == [] and differing(got[n:], np.concatenate([self.host[k][n:], sentinels(PAD)])) == []


@pytest.fixture(scope="module")
def big(lib):
    b = Big()
    yield b
    for d in b.dev.values():
        d.free()
    b.host.clear()


def big_sums(lib, work, big, n):
    x, y, v = (big.host[k][:n] for k in "xyv")
    res = DA.from_host(sentinels(3))
    poison(lib, work)
    check(lib.liship_dot_f64(n, big.dev["x"].ptr, big.dev["y"].ptr, res.ptr, work.ptr, None))
    dot = res.to_host()
    poison(lib, work)
    check(lib.liship_nrm2_f64(n, big.dev["x"].ptr, res.ptr, work.ptr, None))
    nrm2 = res.to_host()
    assert dot.view(np.uint64)[0] == rm.tree(x * y).view(np.uint64) and (dot.view(np.uint64)[1:] == SENT).all()
    assert nrm2.view(np.uint64)[0] == rm.root(rm.tree(x * x)).view(np.uint64) and (nrm2.view(np.uint64)[1:] == SENT).all()
    poison(lib, work)
    check(lib.liship_axpy_sumsq_dot_f64(n, rc.A, big.dev["x"].ptr, big.dev["y"].ptr, big.dev["v"].ptr, res.ptr, work.ptr, None))
    got = res.to_host()
    oy = y + rc.A * x
    try:
        assert differing(got[:2], [rm.tree(oy * oy), rm.tree(v * oy)]) == [] and got.view(np.uint64)[2] == SENT
        assert big.unchanged("y", oy, n) and big.unchanged("x", x, n) and big.unchanged("v", v, n)
    finally:
        big.restore("y")


def test_largest_size_without_a_fold_level(lib, work, big):
    assert rm.grid_for(N_FLAT) == rm.FINAL_MAX and N_FLAT == rm.NT_ELEMS
    big_sums(lib, work, big, N_FLAT)


def test_non_temporal_loads_and_the_fold_level(lib, work, big):
    assert rm.grid_for(N_NT) == rm.FINAL_MAX + 1 and N_NT > rm.NT_ELEMS and N_NT & 1
    big_sums(lib, work, big, N_NT)


def test_non_temporal_element_wise_kernels(lib, scal, big):
    """axpy, xpay, axpy2 and the CG direction update at a size that loads past the caches: one rounded multiply, one rounded add each"""
    n, a, b = N_NT, rc.A, rc.CB
    x, y, v = (big.host[k] for k in "xyv")
    dx, dy, dv = (big.dev[k].ptr for k in "xyv")
    try:
        check(lib.liship_axpy_f64(n, a, dx, dy, None))
        assert big.unchanged("y", y + a * x, n)
        big.restore("y")
        check(lib.liship_xpay_f64(n, dx, a, dy, None))
        assert big.unchanged("y", x + a * y, n)
        big.restore("y")
        check(lib.liship_axpy2_f64(n, a, dx, b, dv, dy, None))
        assert big.unchanged("y", (y + a * x) + b * v, n)
        big.restore("y")
        # x: the iterate, y: p, v: r;  alpha = *pa, beta = *pcb:  x += alpha*p (the old p), p = r + beta*p
        check(lib.liship_cg_direction_dev_f64(n, scal["pa"], scal["pcb"], dv, None, dy, dx, None))
        assert big.unchanged("y", v + b * y, n) and big.unchanged("x", x + a * y, n) and big.unchanged("v", v, n)
    finally:
        big.restore("y")
        big.restore("x")


# ------------------------------------------------------------------------------------------------ chunked A^T x
@pytest.mark.parametrize("T", rc.CHUNK_T)
def test_chunked_transposed_product_gives_the_models_bits(lib, T):
    """nsrc < T (empty chunks), nsrc % T != 0, more transposed rows than source rows, empty rows, a row living in the last chunk only,
    products that are -0.0"""
    bad = {}
    for nsrc in rc.CHUNK_NSRC:
        rows, tptr, tidx, tval, x = rc.chunked_case(nsrc, T)
        dptr, didx, dval, dx = DA.from_host(tptr, np.int32), DA.from_host(tidx, np.int32), DA.from_host(tval, np.float64), DA.from_host(x, np.float64)
        y = Vec(np.full(rows, np.nan))
        check(lib.liship_spmv_csr_transposed_chunked_f64(rows, nsrc, T, dptr.ptr, didx.ptr, dval.ptr, dx.ptr, y.ptr, None))
        check(lib.liship_device_synchronize())
        got, intact = y.read()
        want = rm.spmv_transposed_chunked(rows, nsrc, T, tptr, tidx, tval, x)
        if differing(got, want) or np.isnan(got).any() or not intact:
            bad[nsrc] = (differing(got, want), intact)
    assert bad == {}


def test_chunked_transposed_product_edges(lib):
    rows, tptr, tidx, tval, x = rc.chunked_case(13, 3)
    dptr, didx, dval, dx = DA.from_host(tptr, np.int32), DA.from_host(tidx, np.int32), DA.from_host(tval, np.float64), DA.from_host(x, np.float64)
    y = Vec(sentinels(rows))
    for T in (0, -1):
        assert lib.liship_spmv_csr_transposed_chunked_f64(rows, 13, T, dptr.ptr, didx.ptr, dval.ptr, dx.ptr, y.ptr, None) == ERR_ARG
    assert lib.liship_spmv_csr_transposed_chunked_f64(-1, 13, 3, dptr.ptr, didx.ptr, dval.ptr, dx.ptr, y.ptr, None) == ERR_ARG
    check(lib.liship_spmv_csr_transposed_chunked_f64(0, 13, 3, dptr.ptr, didx.ptr, dval.ptr, dx.ptr, y.ptr, None))       # no rows: nothing written
    check(lib.liship_device_synchronize())
    got, intact = y.read()
    assert (got.view(np.uint64) == SENT).all() and intact
