"""The code that carries a device-driven Krylov loop, kernel by kernel, against tests/krylov_model.py (which
tests/test_krylov_model_cpu.py pins to the CPU oracle): the one-lane scalar steps, the `_dev` forms of the vector kernels,
the guard behind which a batch of iterations is enqueued blind, and the chain that lets a step ride in a reduction's last kernel.

Comparisons are bit for bit (uint64).  One exception is written down in canon(): IEEE 754 leaves the sign and the payload of
a NaN *result* to the implementation, so a NaN the model computes has to be a NaN on the device -- any NaN but the sentinel
that marks memory nobody wrote.

g_guard and g_chain are process globals holding raw device pointers: the autouse fixture below removes both after every test,
passed or failed, and only then lets go of the buffers they pointed at."""
import ctypes as C

import numpy as np
import pytest

import krylov_model as km
import lis_amd
import orc
from krylov_model import (KS_ALPHA, KS_BETA, KS_DONE, KS_DOT0, KS_ITER, KS_LEN, KS_NALPHA, KS_NOMEGA, KS_NOT_HALF, KS_OMEGA,
                          KS_STATUS, KS_SUM0, KS_SUM1)
from lis_amd import DeviceArray as DA, check

pytestmark = pytest.mark.gpu
ERR_ARG = -1
SENT = np.uint64(0x7FF8DEAD0000BEEF)              # a quiet NaN no arithmetic here produces
NAN_BITS = np.float64(np.nan).view(np.uint64)
HIST = 20


@pytest.fixture(scope="module")
def lib():
    lib = lis_amd.load()
    assert lis_amd.gpu_available(), "no HIP device: the product path has no CPU fallback"
    assert not lib.liship_missing
    return lib


@pytest.fixture(scope="module")
def work(lib):
    return DA.zeros(lib.liship_reduce_work_bytes() // 8, np.float64)


@pytest.fixture(autouse=True)
def keep(lib):
    """Buffers a guard or a chain points at go into this list; they are released after the globals are cleared."""
    held = []
    yield held
    lib.liship_krylov_guard(None)
    lib.liship_krylov_chain(0, None, None)
    lib.liship_set_reference_reductions(0)
    lib.liship_device_synchronize()
    del held[:]


def sentinels(k):
    return np.full(k, SENT, np.uint64).view(np.float64)


def u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(-1).view(np.uint64)


def same(a, b):
    return np.array_equal(u64(a), u64(b))


def canon(a):
    """bits with every NaN except the sentinel mapped to one NaN"""
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    b = a.view(np.uint64).copy()
    b[np.isnan(a) & (b != SENT)] = NAN_BITS
    return b


def differing(a, b):
    return np.nonzero(canon(a) != canon(b))[0].tolist()


def sync(lib):
    check(lib.liship_device_synchronize())


def base_state(**slots):
    """an ordinary mid-solve state; NOT_HALF starts lowered so that every case also sees the step re-arm it; the slots no
    step owns carry values that must survive"""
    st = km.new_state(rho=0.7310585786300049, rho_old=1.3, alpha=0.37, nalpha=-0.37, beta=0.5, omega=0.61, nomega=-0.61,
                      dot0=0.9, dot1=1.7, sum0=2.25e-6, sum1=0.45, nrm2=0.125, bnrm=3.0, tol=1e-12, iter=3.0, nhist=3.0,
                      not_half=0.0)
    st[19:] = np.arange(19, KS_LEN) + 0.5
    for k, v in slots.items():
        st[getattr(km, "KS_" + k.upper())] = v
    return st


CONVERGENCE_STEPS = (km.STEP_CG_RESID, km.STEP_CG_RESID_PRE, km.STEP_BICGSTAB_HALF, km.STEP_BICGSTAB_RESID, km.STEP_BICG_RESID)


def step_cases(kind):
    cases = {
        "ordinary": {}, "history_null": {}, "done": {"done": 1.0}, "done_negative": {"done": -1.0},
        "sum0_nan": {"sum0": np.nan}, "sum0_inf": {"sum0": np.inf},
        "iter0": {"iter": 0.0, "nhist": 0.0}, "iter15": {"iter": 15.0, "nhist": 15.0},
    }
    zeros = {"pos": 0.0, "neg": -0.0}
    for sign, z in zeros.items():
        if kind == km.STEP_CG_ALPHA:
            cases["dot0_zero_" + sign] = {"dot0": z}
        if kind == km.STEP_BICGSTAB_ALPHA:
            cases["rho_zero_" + sign] = {"rho": z}
            cases["dot0_zero_" + sign] = {"dot0": z}              # the reference does not test <rtld,v>: alpha = +-inf, no breakdown
        if kind == km.STEP_BICGSTAB_RESID:
            cases["omega_zero_" + sign] = {"omega": z, "nomega": -z}
            cases["omega_zero_converged_" + sign] = {"omega": z, "nomega": -z, "tol": 1.0}   # convergence is tested first
        if kind == km.STEP_BICG_ALPHA:
            cases["rho_zero_" + sign] = {"rho": z}
            cases["dot0_zero_" + sign] = {"dot0": z}
    if kind in CONVERGENCE_STEPS:
        st = base_state()
        nrm2 = np.sqrt(st[KS_SUM0]) * st[km.KS_BNRM]
        cases["nrm2_equals_tol"] = {"tol": nrm2}
        cases["nrm2_one_ulp_below_tol"] = {"tol": np.nextafter(nrm2, np.inf)}
        cases["nrm2_one_ulp_above_tol"] = {"tol": np.nextafter(nrm2, 0.0)}
    return cases


def run_step(lib, kind, st, hist, gathered=None, nranks=0):
    dst = DA.from_host(st)
    dh = DA.from_host(hist) if hist is not None else None
    dg = DA.from_host(gathered) if gathered is not None else None
    rc = lib.liship_krylov_step(kind, dst.ptr, dh.ptr if dh else None, dg.ptr if dg else None, nranks, None)
    sync(lib)
    return rc, dst.to_host(), (dh.to_host() if dh else None)


STEP_CASES = [(kind, name) for kind in km.STEPS for name in step_cases(kind)]


# ------------------------------------------------------------------------------------------------ a. scalar steps
@pytest.mark.parametrize("kind,name", STEP_CASES, ids=["%s-%s" % (km.STEP_NAMES[k], n) for k, n in STEP_CASES])
def test_step_matches_the_model(lib, kind, name):
    st = base_state(**step_cases(kind)[name])
    hist = None if name == "history_null" else sentinels(HIST)
    exp, exph = st.copy(), (None if hist is None else hist.copy())
    km.step(kind, exp, exph)
    rc, got, goth = run_step(lib, kind, st, hist)
    assert rc == 0
    assert differing(got, exp) == [], (got, exp)
    if hist is not None:
        assert differing(goth, exph) == []
    if name.startswith("done"):                         # only NOT_HALF may have changed
        st[KS_NOT_HALF] = 1.0
        assert same(got, st)
    if "zero" in name and "converged" not in name and not (kind == km.STEP_BICGSTAB_ALPHA and name.startswith("dot0")):
        assert got[KS_STATUS] == km.STATUS_BREAKDOWN and got[KS_DONE] == 1.0
    if name == "nrm2_equals_tol" or name == "nrm2_one_ulp_below_tol":
        assert got[KS_STATUS] == km.STATUS_CONVERGED and got[KS_DONE] == 1.0 and got[KS_ITER] == 4.0
    if name == "nrm2_one_ulp_above_tol":
        assert got[KS_STATUS] == km.STATUS_RUNNING and got[KS_DONE] == 0.0


# per-rank sums whose rank-order sum differs from any other order: {1e16, 1, -1e16, 1} gives 1e16, 1e16, 0, 1 after 1, 2, 3, 4 ranks
# (left to right) and 2 exactly; the second result's sequence never sums to 0, so no step divides 0 by 0
RANK_SUMS = (np.array([1e16, 1.0, -1e16, 1.0]), np.array([3.0, 1e16, 1.0, -1e16]))


def gathered_sums(nranks, count):
    g = np.empty(nranks * count)
    for r in range(nranks):
        for k in range(count):
            g[r * count + k] = RANK_SUMS[k % 2][(r + k // 2) % 4]
    return g


@pytest.mark.parametrize("nranks", [1, 2, 3, 8])
@pytest.mark.parametrize("kind", km.STEPS, ids=[km.STEP_NAMES[k] for k in km.STEPS])
def test_step_folds_the_gathered_sums_in_rank_order(lib, kind, nranks):
    slot, count = km.FOLD[kind]
    g = gathered_sums(nranks, count)
    st, hist = base_state(), sentinels(HIST)
    exp, exph = st.copy(), hist.copy()
    km.step(kind, exp, exph, g, nranks)
    assert same(exp[slot:slot + count], km.rank_fold(g, nranks, count))
    rc, got, goth = run_step(lib, kind, st, hist, g, nranks)
    assert rc == 0 and differing(got, exp) == [] and differing(goth, exph) == []
    if nranks == 8:                                     # the order matters for these values: folded from the last rank down, the first sum is 0.0, not 1.0
        backwards = np.ascontiguousarray(g.reshape(nranks, count)[::-1]).reshape(-1)
        assert km.rank_fold(backwards, nranks, count)[0] != km.rank_fold(g, nranks, count)[0]


@pytest.mark.parametrize("kind", km.STEPS, ids=[km.STEP_NAMES[k] for k in km.STEPS])
def test_step_without_a_gathered_array_folds_nothing(lib, kind):
    st, hist = base_state(), sentinels(HIST)
    exp, exph = st.copy(), hist.copy()
    km.step(kind, exp, exph)
    rc, got, goth = run_step(lib, kind, st, hist, None, 3)
    assert rc == 0 and differing(got, exp) == [] and differing(goth, exph) == []


def test_step_and_chain_argument_errors(lib, keep):
    st = base_state()
    dst, dh = DA.from_host(st), DA.from_host(sentinels(HIST))
    keep += [dst, dh]
    for bad in (0, 11, -1):
        assert lib.liship_krylov_step(bad, dst.ptr, dh.ptr, None, 0, None) == ERR_ARG
    assert lib.liship_krylov_step(km.STEP_CG_ALPHA, None, dh.ptr, None, 0, None) == ERR_ARG
    assert lib.liship_krylov_chain(km.STEP_CG_ALPHA, None, dh.ptr) == ERR_ARG
    assert lib.liship_krylov_chain(11, dst.ptr, dh.ptr) == ERR_ARG
    assert lib.liship_krylov_chain(-1, dst.ptr, dh.ptr) == ERR_ARG
    check(lib.liship_krylov_chain_flush(None))          # none of the refused calls announced anything
    sync(lib)
    assert same(dst.to_host(), st) and same(dh.to_host(), sentinels(HIST))


@pytest.mark.parametrize("nranks", [1, 2, 8])
@pytest.mark.parametrize("count", [1, 2, 64])
def test_rank_fold(lib, count, nranks):
    g = gathered_sums(nranks, count)
    dg, out = DA.from_host(g), DA.from_host(sentinels(66))
    check(lib.liship_rank_fold_f64(count, dg.ptr, nranks, out.ptr, None))
    sync(lib)
    got = out.to_host()
    assert same(got[:count], km.rank_fold(g, nranks, count))
    assert same(got[count:], sentinels(66 - count))


def test_rank_fold_argument_errors(lib):
    dg, out = DA.from_host(np.ones(66 * 2)), DA.from_host(sentinels(66))
    assert lib.liship_rank_fold_f64(0, dg.ptr, 2, out.ptr, None) == ERR_ARG
    assert lib.liship_rank_fold_f64(65, dg.ptr, 2, out.ptr, None) == ERR_ARG
    assert lib.liship_rank_fold_f64(2, dg.ptr, 0, out.ptr, None) == ERR_ARG
    assert lib.liship_rank_fold_f64(2, None, 2, out.ptr, None) == ERR_ARG
    assert lib.liship_rank_fold_f64(2, dg.ptr, 2, None, None) == ERR_ARG
    sync(lib)
    assert same(out.to_host(), sentinels(66))


# ------------------------------------------------------------------------------------------------ b. the chain
def ride(lib, keep, kind, slot, nres, launch, st=None):
    """Announce `kind`, run the reduction `launch(result_ptr)` into the state block: the state must be the model's step applied to
    the state that holds what the same reduction gives unchained.  A second, unannounced run must only rewrite its sums."""
    scratch = DA.from_host(sentinels(4))
    launch(scratch.ptr)
    sync(lib)
    sums = scratch.to_host()[:nres]
    assert same(scratch.to_host()[nres:], sentinels(4 - nres))
    st = base_state() if st is None else st
    dst, dh = DA.from_host(st), DA.from_host(sentinels(HIST))
    keep += [dst, dh]
    check(lib.liship_krylov_chain(kind, dst.ptr, dh.ptr))
    launch(dst.ptr + 8 * slot)
    sync(lib)
    exp, exph = st.copy(), sentinels(HIST)
    exp[slot:slot + nres] = sums
    km.step(kind, exp, exph)
    got, goth = dst.to_host(), dh.to_host()
    assert differing(got, exp) == [], (got, exp)
    assert differing(goth, exph) == []
    launch(dst.ptr + 8 * slot)                          # nothing announced: ITER and all the rest stay
    check(lib.liship_krylov_chain_flush(None))          # and nothing is left to flush
    sync(lib)
    got[slot:slot + nres] = sums
    assert same(dst.to_host(), got) and same(dh.to_host(), goth)
    return sums


@pytest.mark.parametrize("n", [1, 2047, 2048, 2049, 4097])
def test_chain_rides_in_the_tree_reductions(lib, keep, work, n):
    """one workgroup (its own launch behind level 1) up to 2048, reduce_final beyond"""
    x = np.random.default_rng(n).uniform(-1, 1, n)
    dx = DA.from_host(x)
    sums = ride(lib, keep, km.STEP_CG_RESID, KS_SUM0, 1,
                lambda res: check(lib.liship_sumsq_f64(n, dx.ptr, res, work.ptr, None)))
    ref = km.exact_sum(x * x)
    assert abs(sums[0] - ref) <= 1e-14 * ref * max(1.0, np.log2(n + 1))
    dy = DA.from_host(np.random.default_rng(n + 1).uniform(-1, 1, n))
    ride(lib, keep, km.STEP_BICGSTAB_OMEGA, KS_DOT0, 2,
         lambda res: check(lib.liship_dot2_f64(n, dx.ptr, dy.ptr, res, work.ptr, None)))


def test_chain_rides_behind_a_fold_level(lib, keep, work):
    """more than 2^14 level-1 partials: reduce_fold, then reduce_final carries the step.  Every term is 0.25, so the sum is
    exact in any order."""
    n = 16385 * 2048 - 3
    dx = DA(n, np.float64)
    check(lib.liship_set_all_f64(n, 0.5, dx.ptr, None))
    sums = ride(lib, keep, km.STEP_CG_RESID, KS_SUM0, 1,
                lambda res: check(lib.liship_sumsq_f64(n, dx.ptr, res, work.ptr, None)))
    assert sums[0] == 0.25 * n
    dx.free()


def test_chain_rides_in_the_finish_kernel_of_a_fused_product(lib, keep, work):
    """a matrix of one row block leaves a single partial: finish_kernel carries the step"""
    ptr, idx, val = orc.poisson1d(100)
    n = len(ptr) - 1
    rng = np.random.default_rng(8)
    x, w = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    dptr, didx, dval, dx, dw = (DA.from_host(a) for a in (ptr, idx, val, x, w))
    dy = DA.from_host(sentinels(n))
    plan = C.c_void_p()
    check(lib.liship_csr_plan_create(C.byref(plan), n, dptr.ptr, None))
    pn, pnnz, pnb = C.c_int(), C.c_longlong(), C.c_int()
    check(lib.liship_csr_plan_info(plan, C.byref(pn), C.byref(pnnz), C.byref(pnb)))
    assert pnb.value == 1
    try:
        for want_sumsq, kind in ((0, km.STEP_CG_ALPHA), (1, km.STEP_BICGSTAB_OMEGA)):
            sums = ride(lib, keep, kind, KS_DOT0, 1 + want_sumsq,
                        lambda res: check(lib.liship_spmv_csr_dot_f64(plan, dptr.ptr, didx.ptr, dval.ptr, dx.ptr, dy.ptr, dw.ptr,
                                                                      want_sumsq, res, work.ptr, None)))
            y = orc.spmv_csr(ptr, idx, val, x)
            assert same(dy.to_host(), y)
            assert abs(sums[0] - km.exact_sum(w * y)) <= 1e-13 * np.abs(w * y).sum()
    finally:
        lib.liship_krylov_chain(0, None, None)
        sync(lib)
        check(lib.liship_csr_plan_destroy(plan))


@pytest.mark.parametrize("T", [1, 3, 8])
@pytest.mark.parametrize("n", [5, 4097])
def test_chain_rides_in_the_reference_order_reductions(lib, keep, work, n, T):
    rng = np.random.default_rng(n + T)
    x, y = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    dx, dy = DA.from_host(x), DA.from_host(y)
    check(lib.liship_set_reference_reductions(T))
    sums = ride(lib, keep, km.STEP_CG_RESID, KS_SUM0, 1,
                lambda res: check(lib.liship_sumsq_f64(n, dx.ptr, res, work.ptr, None)))
    assert same(sums, [km.chunked_sum(x * x, T)])
    sums = ride(lib, keep, km.STEP_BICGSTAB_OMEGA, KS_DOT0, 2,
                lambda res: check(lib.liship_dot2_f64(n, dx.ptr, dy.ptr, res, work.ptr, None)))
    assert same(sums, [km.chunked_sum(x * y, T), km.chunked_sum(x * x, T)])


def test_chain_flush_and_withdrawal(lib, keep, work):
    st = base_state()
    dst, dh = DA.from_host(st), DA.from_host(sentinels(HIST))
    keep += [dst, dh]
    exp, exph = st.copy(), sentinels(HIST)
    check(lib.liship_krylov_chain_flush(None))                      # nothing announced: a no-op
    sync(lib)
    assert same(dst.to_host(), exp) and same(dh.to_host(), exph)
    check(lib.liship_krylov_chain(km.STEP_BICG_RESID, dst.ptr, dh.ptr))
    check(lib.liship_krylov_chain_flush(None))                      # announced, no reduction: the flush runs it
    sync(lib)
    km.step(km.STEP_BICG_RESID, exp, exph)
    assert exp[KS_ITER] == 4.0
    assert same(dst.to_host(), exp) and same(dh.to_host(), exph)
    check(lib.liship_krylov_chain_flush(None))                      # ... once
    sync(lib)
    assert same(dst.to_host(), exp) and same(dh.to_host(), exph)
    x = np.random.default_rng(2).uniform(-1, 1, 4097)
    dx, scratch = DA.from_host(x), DA.from_host(sentinels(2))
    check(lib.liship_krylov_chain(km.STEP_BICG_RESID, dst.ptr, dh.ptr))
    check(lib.liship_krylov_chain(0, None, None))                   # withdrawn: neither a reduction nor a flush runs it
    check(lib.liship_sumsq_f64(4097, dx.ptr, scratch.ptr, work.ptr, None))
    check(lib.liship_krylov_chain_flush(None))
    sync(lib)
    assert same(dst.to_host(), exp) and same(dh.to_host(), exph)
    check(lib.liship_krylov_chain(km.STEP_BICG_RESID, dst.ptr, dh.ptr))
    check(lib.liship_sumsq_f64(4097, dx.ptr, scratch.ptr, work.ptr, None))     # the reduction takes the step along ...
    check(lib.liship_krylov_chain_flush(None))                                 # ... and the flush finds nothing
    sync(lib)
    km.step(km.STEP_BICG_RESID, exp, exph)
    assert exp[KS_ITER] == 5.0
    assert same(dst.to_host(), exp) and same(dh.to_host(), exph)


# ------------------------------------------------------------------------------------------------ c. the _dev kernels
class Vecs:
    """named host vectors and their device copies, `off` elements into an allocation with a sentinel on either side (off = 1:
    8-byte aligned only, which takes the kernels' scalar path)"""
    NAMES = ("x", "y", "w", "d", "p", "q", "r", "t", "v", "it")

    def __init__(self, n, seed, off=0):
        rng = np.random.default_rng(seed)
        self.n, self.off = n, off
        self.h = {k: rng.uniform(-1, 1, n) for k in self.NAMES}
        self.h["d"] = rng.uniform(0.5, 2.0, n)
        for k in ("y", "r", "it"):                     # zeros of both signs, where a -0.0 or subnormal product shows
            self.h[k][0::7] = 0.0
            self.h[k][3::7] = -0.0
        self.d = {k: DA(n + off + 1, np.float64) for k in self.NAMES}
        self.reset()

    def reset(self, *names):
        for k in names or self.NAMES:
            self.d[k].upload(np.concatenate((sentinels(self.off), self.h[k], sentinels(1))))

    def ptr(self, k):
        return self.d[k].ptr + 8 * self.off

    def get(self, k):
        a = self.d[k].to_host()
        assert same(a[:self.off], sentinels(self.off)) and same(a[-1:], sentinels(1)), "wrote outside " + k
        return a[self.off:-1]

    def untouched(self, *names):
        return all(same(self.get(k), self.h[k]) for k in names or self.NAMES)


SHAPES = [(1, 0), (2, 0), (3, 0), (2047, 0), (2048, 0), (2049, 0), (4097, 0), (1001, 1)]
SHAPE_IDS = ["n%d%s" % (n, "_unaligned" if off else "") for n, off in SHAPES]
# (a, b): ordinary; -0.0; a subnormal coefficient, whose product with any |x| < 1 is subnormal
COEFS = {"ordinary": (0.37120000000000003, -1.6180339887498949), "negative_zero": (-0.0, -0.0),
         "subnormal_products": (2.0 ** -1030, -3.0 * 2.0 ** -1040)}


def coef_state(a, b):
    """coefficients where the solver keeps them: a in ALPHA / NALPHA, b in BETA and OMEGA / NOMEGA"""
    return base_state(alpha=a, nalpha=-a, beta=b, omega=b, nomega=-b)


def slot(dst, k):
    return dst.ptr + 8 * k


def elementwise_kernels(lib, V, dst, a, b):
    """(name, outputs, device-coefficient call, host-coefficient twin or None, model of the outputs)"""
    n, H, P = V.n, V.h, V.ptr
    dc = 0.8125
    return [
        ("xpay_dev", ("y",), lambda: lib.liship_xpay_dev_f64(n, P("x"), slot(dst, KS_BETA), P("y"), None),
         lambda: lib.liship_xpay_f64(n, P("x"), b, P("y"), None), lambda: (km.xpay(H["x"], b, H["y"]),)),
        ("pmul_xpay_dev", ("y",), lambda: lib.liship_pmul_xpay_dev_f64(n, P("x"), P("d"), slot(dst, KS_BETA), P("y"), None),
         lambda: lib.liship_pmul_xpay_f64(n, P("x"), P("d"), b, P("y"), None), lambda: (km.pmul_xpay(H["x"], H["d"], b, H["y"]),)),
        ("axpy_dev", ("y",), lambda: lib.liship_axpy_dev_f64(n, slot(dst, KS_ALPHA), P("x"), P("y"), None),
         lambda: lib.liship_axpy_f64(n, a, P("x"), P("y"), None), lambda: (km.axpy(a, H["x"], H["y"]),)),
        ("axpy2_dev", ("y",), lambda: lib.liship_axpy2_dev_f64(n, slot(dst, KS_ALPHA), P("x"), slot(dst, KS_OMEGA), P("w"), P("y"), None),
         lambda: lib.liship_axpy2_f64(n, a, P("x"), b, P("w"), P("y"), None), lambda: (km.axpy2(a, H["x"], b, H["w"], H["y"]),)),
        ("axpy_xpay_dev", ("y",), lambda: lib.liship_axpy_xpay_dev_f64(n, slot(dst, KS_NALPHA), P("x"), P("w"), slot(dst, KS_BETA), P("y"), None),
         lambda: lib.liship_axpy_xpay_f64(n, -a, P("x"), P("w"), b, P("y"), None), lambda: (km.axpy_xpay(-a, H["x"], H["w"], b, H["y"]),)),
        ("cg_direction_dev", ("p", "it"),
         lambda: lib.liship_cg_direction_dev_f64(n, slot(dst, KS_ALPHA), slot(dst, KS_BETA), P("r"), None, P("p"), P("it"), None),
         None, lambda: km.cg_direction(a, b, H["r"], None, H["p"], H["it"])),
        ("cg_direction_dev_jacobi", ("p", "it"),
         lambda: lib.liship_cg_direction_dev_f64(n, slot(dst, KS_ALPHA), slot(dst, KS_BETA), P("r"), P("d"), P("p"), P("it"), None),
         None, lambda: km.cg_direction(a, b, H["r"], H["d"], H["p"], H["it"])),
        ("cg_direction_dev_first", ("p", "it"),
         lambda: lib.liship_cg_direction_dev_f64(n, None, slot(dst, KS_BETA), P("r"), P("d"), P("p"), P("it"), None),
         None, lambda: km.cg_direction(None, b, H["r"], H["d"], H["p"], H["it"])),
        ("cg_direction_uniform_dev", ("p", "it"),
         lambda: lib.liship_cg_direction_uniform_dev_f64(n, slot(dst, KS_ALPHA), slot(dst, KS_BETA), P("r"), dc, P("p"), P("it"), None),
         None, lambda: km.cg_direction(a, b, H["r"], None, H["p"], H["it"], dc=dc)),
        ("cg_direction_uniform_dev_first", ("p", "it"),
         lambda: lib.liship_cg_direction_uniform_dev_f64(n, None, slot(dst, KS_BETA), P("r"), dc, P("p"), P("it"), None),
         None, lambda: km.cg_direction(None, b, H["r"], None, H["p"], H["it"], dc=dc)),
        # the plain kernels the loops launch under a guard
        ("pmul", ("t",), lambda: lib.liship_pmul_f64(n, P("x"), P("d"), P("t"), None), None, lambda: (km.pmul(H["x"], H["d"]),)),
        ("axpy", ("y",), lambda: lib.liship_axpy_f64(n, a, P("x"), P("y"), None), None, lambda: (km.axpy(a, H["x"], H["y"]),)),
    ]


@pytest.mark.parametrize("coef", list(COEFS))
@pytest.mark.parametrize("n,off", SHAPES, ids=SHAPE_IDS)
def test_elementwise_dev_kernels_match_model_and_twin(lib, n, off, coef):
    a, b = COEFS[coef]
    V = Vecs(n, 100 + n, off)
    st = coef_state(a, b)
    dst = DA.from_host(st)
    for name, outs, dev, twin, model in elementwise_kernels(lib, V, dst, a, b):
        exp = model()
        for which, call in (("dev", dev), ("twin", twin)):
            if call is None:
                continue
            V.reset(*outs)
            check(call())
            sync(lib)
            for k, e in zip(outs, exp):
                assert same(V.get(k), e), (name, which, k)
            assert V.untouched(*[k for k in V.NAMES if k not in outs]), (name, which)
            V.reset(*outs)
    assert same(dst.to_host(), st)
    if coef != "ordinary":                              # the edge really is visible in the result: the model's axpy differs from y
        assert not same(km.axpy(a, V.h["x"], V.h["y"]), V.h["y"]) or n < 4


def fused_kernels(lib, V, dst, a, b, res, work):
    """(name, vector outputs, device-coefficient call, twin or None, model -> (vectors..., terms))"""
    n, H, P, W = V.n, V.h, V.ptr, work.ptr
    dc = 0.8125

    def m_update(dinv):
        x, r, terms = km.cg_update(a, H["p"], H["q"], dinv, H["it"], H["r"])
        return (x, r), terms

    def m_axpy_sumsq():
        y, terms = km.axpy_sumsq(-a, H["x"], H["y"])
        return (y,), terms

    def m_axpy_sumsq_dot():
        y, terms = km.axpy_sumsq_dot(-b, H["x"], H["y"], H["v"])
        return (y,), terms

    def m_end():
        x, r, terms = km.bicgstab_end(a, b, -b, H["p"], H["t"], H["v"], H["it"], H["r"])
        return (x, r), terms

    def m_resid(uniform):
        r, terms = km.cg_residual_jacobi(-a, H["q"], H["d"], H["r"], dc=dc if uniform else None)
        return (r,), terms

    return [
        ("cg_update_dev", ("it", "r"),
         lambda: lib.liship_cg_update_dev_f64(n, slot(dst, KS_ALPHA), P("p"), P("q"), None, P("it"), P("r"), res, W, None),
         lambda: lib.liship_cg_update_f64(n, a, P("p"), P("q"), P("it"), P("r"), res, W, None), lambda: m_update(None)),
        ("cg_update_dev_jacobi", ("it", "r"),
         lambda: lib.liship_cg_update_dev_f64(n, slot(dst, KS_ALPHA), P("p"), P("q"), P("d"), P("it"), P("r"), res, W, None),
         lambda: lib.liship_cg_update_jacobi_f64(n, a, P("p"), P("q"), P("d"), P("it"), P("r"), res, W, None), lambda: m_update(H["d"])),
        ("axpy_sumsq_dev", ("y",),
         lambda: lib.liship_axpy_sumsq_dev_f64(n, slot(dst, KS_NALPHA), P("x"), P("y"), res, W, None),
         lambda: lib.liship_axpy_sumsq_f64(n, -a, P("x"), P("y"), res, W, None), m_axpy_sumsq),
        ("axpy_sumsq_dot_dev", ("y",),
         lambda: lib.liship_axpy_sumsq_dot_dev_f64(n, slot(dst, KS_NOMEGA), P("x"), P("y"), P("v"), res, W, None),
         lambda: lib.liship_axpy_sumsq_dot_f64(n, -b, P("x"), P("y"), P("v"), res, W, None), m_axpy_sumsq_dot),
        ("bicgstab_end_dev", ("it", "r"),
         lambda: lib.liship_bicgstab_end_dev_f64(n, slot(dst, KS_ALPHA), slot(dst, KS_OMEGA), slot(dst, KS_NOMEGA), P("p"), P("t"), P("v"),
                                                 P("it"), P("r"), res, W, None),
         None, m_end),
        ("cg_residual_jacobi_dev", ("r",),
         lambda: lib.liship_cg_residual_jacobi_dev_f64(n, slot(dst, KS_NALPHA), P("q"), P("d"), P("r"), res, W, None),
         None, lambda: m_resid(False)),
        ("cg_residual_jacobi_uniform_dev", ("r",),
         lambda: lib.liship_cg_residual_jacobi_uniform_dev_f64(n, slot(dst, KS_NALPHA), P("q"), dc, P("r"), res, W, None),
         None, lambda: m_resid(True)),
    ]


def close(a, b, ref_mag, n):
    """the bar test_kernels_gpu.test_reductions applies to a tree sum"""
    return abs(a - b) <= 1e-14 * max(ref_mag, 1e-300) * max(1.0, np.log2(n + 1))


@pytest.mark.parametrize("coef", list(COEFS))
@pytest.mark.parametrize("n,off", SHAPES, ids=SHAPE_IDS)
def test_fused_dev_passes_match_model_and_twin(lib, work, n, off, coef):
    a, b = COEFS[coef]
    V = Vecs(n, 200 + n, off)
    st = coef_state(a, b)
    dst, dres = DA.from_host(st), DA.from_host(sentinels(4))
    for T in (0, 1, 3):
        check(lib.liship_set_reference_reductions(T))
        for name, outs, dev, twin, model in fused_kernels(lib, V, dst, a, b, dres.ptr, work):
            exp, terms = model()
            got = {}
            for which, call in (("dev", dev), ("twin", twin)):
                if call is None:
                    continue
                V.reset(*outs)
                dres.upload(sentinels(4))
                check(call())
                sync(lib)
                for k, e in zip(outs, exp):
                    assert same(V.get(k), e), (name, which, k, T)
                assert V.untouched(*[k for k in V.NAMES if k not in outs]), (name, which, T)
                V.reset(*outs)
                res = dres.to_host()
                assert same(res[len(terms):], sentinels(4 - len(terms))), (name, which, T)
                got[which] = res[:len(terms)]
            if "twin" in got:
                assert same(got["dev"], got["twin"]), (name, T)
            for s, t in zip(got["dev"], terms):
                if T == 0:
                    assert close(s, km.exact_sum(t), np.abs(t).sum(), n), (name, s, km.exact_sum(t))
                else:
                    assert u64(s)[0] == u64(km.chunked_sum(t, T))[0], (name, T, s, km.chunked_sum(t, T))
    check(lib.liship_set_reference_reductions(0))
    assert same(dst.to_host(), st)


def test_dev_kernels_with_no_elements_touch_nothing(lib, work):
    """n = 0: every call answers 0; no vector changes.  A fused pass still reports the sum of no terms, 0.0, the reference's
    value for an empty vector (lis_vector_ops.c: the sums start from 0.0)."""
    a, b = COEFS["ordinary"]
    V = Vecs(3, 1)
    st = coef_state(a, b)
    dst, dres = DA.from_host(st), DA.from_host(sentinels(4))
    V.n = 0
    for name, outs, dev, twin, model in elementwise_kernels(lib, V, dst, a, b):
        assert dev() == 0, name
    for name, outs, dev, twin, model in fused_kernels(lib, V, dst, a, b, dres.ptr, work):
        dres.upload(sentinels(4))
        assert dev() == 0, name
        sync(lib)
        res, nres = dres.to_host(), (1 if name in ("cg_update_dev", "axpy_sumsq_dev") else 2)
        assert same(res[:nres], np.zeros(nres)) and same(res[nres:], sentinels(4 - nres)), name
    sync(lib)
    V.n = 3
    assert V.untouched() and same(dst.to_host(), st)


def test_dev_kernels_refuse_a_missing_coefficient(lib, work):
    n = 5
    V = Vecs(n, 2)
    st = coef_state(*COEFS["ordinary"])
    dst, dres = DA.from_host(st), DA.from_host(sentinels(4))
    P, pa, W, res = V.ptr, slot(dst, KS_ALPHA), work.ptr, dres.ptr
    calls = [
        lib.liship_xpay_dev_f64(n, P("x"), None, P("y"), None),
        lib.liship_pmul_xpay_dev_f64(n, P("x"), P("d"), None, P("y"), None),
        lib.liship_axpy_dev_f64(n, None, P("x"), P("y"), None),
        lib.liship_axpy2_dev_f64(n, None, P("x"), pa, P("w"), P("y"), None),
        lib.liship_axpy2_dev_f64(n, pa, P("x"), None, P("w"), P("y"), None),
        lib.liship_axpy_xpay_dev_f64(n, None, P("x"), P("w"), pa, P("y"), None),
        lib.liship_axpy_xpay_dev_f64(n, pa, P("x"), P("w"), None, P("y"), None),
        lib.liship_cg_update_dev_f64(n, None, P("p"), P("q"), None, P("it"), P("r"), res, W, None),
        lib.liship_axpy_sumsq_dev_f64(n, None, P("x"), P("y"), res, W, None),
        lib.liship_axpy_sumsq_dot_dev_f64(n, None, P("x"), P("y"), P("v"), res, W, None),
        lib.liship_bicgstab_end_dev_f64(n, None, pa, pa, P("p"), P("t"), P("v"), P("it"), P("r"), res, W, None),
        lib.liship_bicgstab_end_dev_f64(n, pa, None, pa, P("p"), P("t"), P("v"), P("it"), P("r"), res, W, None),
        lib.liship_bicgstab_end_dev_f64(n, pa, pa, None, P("p"), P("t"), P("v"), P("it"), P("r"), res, W, None),
        lib.liship_cg_direction_dev_f64(n, pa, None, P("r"), None, P("p"), P("it"), None),
    ]
    assert calls == [ERR_ARG] * len(calls)
    sync(lib)
    assert V.untouched() and same(dres.to_host(), sentinels(4)) and same(dst.to_host(), st)


# ------------------------------------------------------------------------------------------------ d. the guard
GUARD_N = 4097
LOWERED = {"zero": 0.0, "negative_zero": -0.0}
RAISED = {"one": 1.0, "minus_one": -1.0, "nan": np.nan}


@pytest.mark.parametrize("flag", list(LOWERED) + list(RAISED))
def test_guard_on_elementwise_kernels(lib, keep, flag):
    """a lowered flag (0.0 or -0.0) changes nothing relative to no guard; behind a raised one (anything else, NaN included) no
    output element changes"""
    a, b = COEFS["ordinary"]
    V = Vecs(GUARD_N, 300)
    st = coef_state(a, b)
    dst = DA.from_host(st)
    dflag = DA.from_host(np.array([{**LOWERED, **RAISED}[flag], 7.0]))
    keep += [dflag, dst]
    for name, outs, dev, twin, model in elementwise_kernels(lib, V, dst, a, b):
        V.reset(*outs)
        check(lib.liship_krylov_guard(dflag.ptr))
        check(dev())
        check(lib.liship_krylov_guard(None))
        sync(lib)
        exp = model() if flag in LOWERED else [V.h[k] for k in outs]
        for k, e in zip(outs, exp):
            assert same(V.get(k), e), (name, k)
        assert V.untouched(*[k for k in V.NAMES if k not in outs]), name
        V.reset(*outs)


@pytest.mark.parametrize("T", [0, 1, 3], ids=["tree", "ref1", "ref3"])
@pytest.mark.parametrize("flag", list(LOWERED) + list(RAISED))
def test_guard_on_fused_passes_with_a_step_chained(lib, keep, work, flag, T):
    """The guard is the state's DONE slot, as in the solver, and a step is announced.  Lowered: vectors and state are what the
    unguarded pass and the model's step give.  Raised: no vector changes, the step re-arms NOT_HALF and nothing else, the history
    stays; the pass's own result slots are unspecified then (include/liship.h: the folds of a multi-workgroup reduction are not
    guarded and rewrite them from stale partials)."""
    a, b = COEFS["ordinary"]
    value = {**LOWERED, **RAISED}[flag]
    V = Vecs(GUARD_N, 400)
    check(lib.liship_set_reference_reductions(T))
    nres_of = {"cg_update_dev": 1, "axpy_sumsq_dev": 1}
    for index in range(7):
        st = coef_state(a, b)
        st[KS_DONE] = value
        dst, dh = DA.from_host(st), DA.from_host(sentinels(HIST))
        keep += [dst, dh]
        name, outs, dev, twin, model = fused_kernels(lib, V, dst, a, b, slot(dst, KS_SUM0), work)[index]
        nres = nres_of.get(name, 2)
        kind = km.STEP_CG_RESID if nres == 1 else km.STEP_BICGSTAB_RESID
        if flag in LOWERED:                              # what the pass gives unguarded and unchained, into a scratch buffer
            V.reset(*outs)
            scratch = DA.from_host(sentinels(4))
            check(fused_kernels(lib, V, dst, a, b, scratch.ptr, work)[index][2]())
            sync(lib)
            sums = scratch.to_host()[:nres]
        V.reset(*outs)
        check(lib.liship_krylov_guard(slot(dst, KS_DONE)))
        check(lib.liship_krylov_chain(kind, dst.ptr, dh.ptr))
        check(dev())
        check(lib.liship_krylov_chain_flush(None))
        check(lib.liship_krylov_guard(None))
        sync(lib)
        got, goth = dst.to_host(), dh.to_host()
        exp, exph = st.copy(), sentinels(HIST)
        if flag in LOWERED:
            exp[KS_SUM0:KS_SUM0 + nres] = sums
            km.step(kind, exp, exph)
            vectors = model()[0]
        else:
            km.step(kind, exp, exph)                     # DONE is raised: NOT_HALF only
            exp[KS_SUM0:KS_SUM0 + nres] = got[KS_SUM0:KS_SUM0 + nres]
            vectors = [V.h[k] for k in outs]
            assert exp[KS_NOT_HALF] == 1.0 and same(exph, sentinels(HIST))
        assert differing(got, exp) == [], (name, got, exp)
        assert differing(goth, exph) == [], name
        for k, e in zip(outs, vectors):
            assert same(V.get(k), e), (name, k)
        assert V.untouched(*[k for k in V.NAMES if k not in outs]), name
        V.reset(*outs)


@pytest.mark.parametrize("flag", list(LOWERED) + list(RAISED))
def test_guard_on_the_fused_product(lib, keep, work, flag):
    value = {**LOWERED, **RAISED}[flag]
    ptr, idx, val = orc.poisson3d(12, 10, 8)
    n = len(ptr) - 1
    rng = np.random.default_rng(9)
    x, w = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    dptr, didx, dval, dx, dw = (DA.from_host(a) for a in (ptr, idx, val, x, w))
    dy = DA.from_host(sentinels(n))
    st = base_state(done=value)
    dst, dh = DA.from_host(st), DA.from_host(sentinels(HIST))
    keep += [dst, dh]
    plan = C.c_void_p()
    check(lib.liship_csr_plan_create(C.byref(plan), n, dptr.ptr, None))
    try:
        check(lib.liship_krylov_guard(slot(dst, KS_DONE)))
        check(lib.liship_krylov_chain(km.STEP_CG_ALPHA, dst.ptr, dh.ptr))
        check(lib.liship_spmv_csr_dot_f64(plan, dptr.ptr, didx.ptr, dval.ptr, dx.ptr, dy.ptr, dw.ptr, 0, slot(dst, KS_DOT0), work.ptr, None))
        check(lib.liship_krylov_chain_flush(None))
        check(lib.liship_krylov_guard(None))
        sync(lib)
        got, exp, exph = dst.to_host(), st.copy(), sentinels(HIST)
        if flag in LOWERED:
            y = orc.spmv_csr(ptr, idx, val, x)
            assert same(dy.to_host(), y)
            assert abs(got[KS_DOT0] - km.exact_sum(w * y)) <= 1e-13 * np.abs(w * y).sum()
        else:
            assert same(dy.to_host(), sentinels(n))
        exp[KS_DOT0] = got[KS_DOT0]                      # lowered: checked above; raised: unspecified
        km.step(km.STEP_CG_ALPHA, exp, exph)
        assert differing(got, exp) == [] and differing(dh.to_host(), exph) == []
    finally:
        lib.liship_krylov_guard(None)
        lib.liship_krylov_chain(0, None, None)
        sync(lib)
        check(lib.liship_csr_plan_destroy(plan))


@pytest.mark.parametrize("converges", [True, False])
def test_not_half_protocol(lib, keep, work, converges):
    """bicgstab_batch's half step: r += (-alpha) v with ||s||^2 into SUM0 and BICGSTAB_HALF riding along, then x += alpha*phat
    guarded on NOT_HALF.  x moves exactly when the half step converged, and not again when the same pair is replayed behind the
    raised DONE flag: the replayed step re-arms NOT_HALF."""
    n = GUARD_N
    V = Vecs(n, 500)
    a = 0.37120000000000003
    st = base_state(alpha=a, nalpha=-a, tol=(1e300 if converges else 1e-300), not_half=1.0)
    dst, dh = DA.from_host(st), DA.from_host(sentinels(HIST))
    keep += [dst, dh]

    def pair():
        check(lib.liship_krylov_guard(slot(dst, KS_DONE)))
        check(lib.liship_krylov_chain(km.STEP_BICGSTAB_HALF, dst.ptr, dh.ptr))
        check(lib.liship_axpy_sumsq_dev_f64(n, slot(dst, KS_NALPHA), V.ptr("v"), V.ptr("r"), slot(dst, KS_SUM0), work.ptr, None))
        check(lib.liship_krylov_chain_flush(None))
        check(lib.liship_krylov_guard(slot(dst, KS_NOT_HALF)))
        check(lib.liship_axpy_dev_f64(n, slot(dst, KS_ALPHA), V.ptr("p"), V.ptr("it"), None))
        check(lib.liship_krylov_guard(slot(dst, KS_DONE)))
        sync(lib)

    pair()
    r, terms = km.axpy_sumsq(-a, V.h["v"], V.h["r"])
    exp, exph = st.copy(), sentinels(HIST)
    exp[KS_SUM0] = dst.to_host()[KS_SUM0]
    assert close(exp[KS_SUM0], km.exact_sum(terms[0]), np.abs(terms[0]).sum(), n)
    km.step(km.STEP_BICGSTAB_HALF, exp, exph)
    x = km.axpy(a, V.h["p"], V.h["it"]) if converges else V.h["it"]
    assert (exp[KS_NOT_HALF] == 0.0) == converges and (exp[KS_DONE] == 1.0) == converges
    assert differing(dst.to_host(), exp) == [] and differing(dh.to_host(), exph) == []
    assert same(V.get("r"), r) and same(V.get("it"), x)
    if not converges:
        return
    pair()                                               # behind the raised flag: r stays, the step re-arms NOT_HALF, x stays
    got = dst.to_host()
    exp[KS_NOT_HALF] = 1.0
    exp[KS_SUM0] = got[KS_SUM0]                           # unspecified behind a raised flag
    assert differing(got, exp) == [] and differing(dh.to_host(), exph) == []
    assert same(V.get("r"), r) and same(V.get("it"), x)


# ------------------------------------------------------------------------------------------------ e. halo pack / unpack
def test_gather_and_scatter_add_past_the_grid_cap(lib):
    """4096 workgroups of 256 lanes is the cap of both launches: one element more and the grid-stride loop takes a second turn"""
    count = 4096 * 256 + 5
    ny = count + 1000
    rng = np.random.default_rng(12)
    index = rng.permutation(ny)[:count].astype(np.int32)
    x, wr, y = rng.uniform(-1, 1, ny), rng.uniform(-1, 1, count), rng.uniform(-1, 1, ny)
    dindex, dx, dwr, dy = DA.from_host(index), DA.from_host(x), DA.from_host(wr), DA.from_host(y)
    out = DA.from_host(sentinels(count + 1))
    check(lib.liship_gather_f64(count, dindex.ptr, dx.ptr, out.ptr, None))
    sync(lib)
    got = out.to_host()
    assert same(got[:count], km.gather(index, x)) and same(got[count:], sentinels(1))
    check(lib.liship_scatter_add_f64(count, dindex.ptr, dwr.ptr, dy.ptr, None))
    sync(lib)
    assert same(dy.to_host(), km.scatter_add(index, wr, y))
    # no elements: nothing moves; a negative count is refused
    out.upload(sentinels(count + 1))
    dy.upload(y)
    assert lib.liship_gather_f64(0, dindex.ptr, dx.ptr, out.ptr, None) == 0
    assert lib.liship_scatter_add_f64(0, dindex.ptr, dwr.ptr, dy.ptr, None) == 0
    assert lib.liship_gather_f64(-1, dindex.ptr, dx.ptr, out.ptr, None) == ERR_ARG
    assert lib.liship_scatter_add_f64(-1, dindex.ptr, dwr.ptr, dy.ptr, None) == ERR_ARG
    sync(lib)
    assert same(out.to_host(), sentinels(count + 1)) and same(dy.to_host(), y)
