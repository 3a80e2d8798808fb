"""liship_ritz_tail_f64 (kernels/vector_ops.hip, the reduction op RED_RITZ_TAIL), the fused tail of a subspace iteration, against a numpy model built from
tests/reduction_model.py: the new r, the new v and the sum of q^2 in every bit, in the tree mode (T = 0) and in the reference-order mode (T chunks summed left to
right, the partials in chunk order), at every size where the launch takes another shape; guard words behind both arrays; the refusals; the six separate
liship_* calls it replaces; and an announced liship_krylov_chain step, which it runs wherever liship_sumsq_f64 runs it."""
import numpy as np
import pytest

import lis_amd
import reduction_cases as rc
import reduction_model as rm
from lis_amd import DeviceArray as DA, check

pytestmark = pytest.mark.gpu
ERR_ARG = -1
SENT = np.uint64(0x7FF8DEAD0000BEEF)              # a quiet NaN no arithmetic here produces
PAD = 6                                           # guard words behind every vector
# one block with one lane, one pair, a pair and the odd tail; the last lane of a wavefront / workgroup row; one block full, one element more (two blocks:
# the fold), the odd tail beside two blocks; three blocks; 49 blocks with an odd tail
SIZES = [1, 2, 3, 255, 256, 257, 2047, 2048, 2049, 4097, 100003]
THREADS = [0, 1, 2, 3, 8]


@pytest.fixture(scope="module")
def lib():
    lib = lis_amd.load()
    assert lis_amd.gpu_available(), "no HIP device: the product path has no CPU fallback"
    assert not lib.liship_missing
    return lib


@pytest.fixture(scope="module")
def work(lib):
    return DA(lib.liship_reduce_work_bytes() // 8, np.float64)


@pytest.fixture(autouse=True)
def defaults(lib):
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


class Vec:
    """n doubles in HBM, `off` doubles past a 16 B aligned address, guard words before and behind"""
    def __init__(self, host, off=0):
        self.n, self.off = len(host), off
        full = sentinels(off + self.n + PAD)
        full[off:off + self.n] = host
        self.da = DA.from_host(full)
        assert self.da.ptr % 16 == 0
        self.ptr = self.da.ptr + 8 * off

    def read(self):
        full = self.da.to_host()
        outside = np.concatenate([full[:self.off], full[self.off + self.n:]])
        return full[self.off:self.off + self.n], bool((outside.view(np.uint64) == SENT).all())


def ordered_sum(terms, T):
    """the sum of `terms` as the library forms it: the tree (T = 0), or chunk k of T = LIS_GET_ISIE(k, T, n) summed left to right from 0.0 and the T partials
    added in chunk order from 0.0 (liship_set_reference_reductions)"""
    if T == 0:
        return np.float64(rm.tree(terms, True))
    total = np.float64(0.0)
    for k in range(T):
        lo, hi = rm.get_isie(k, T, len(terms))
        s = np.float64(0.0)
        for t in terms[lo:hi]:
            s = s + t
        total = total + s
    return total


_CASES = {}


def case(n, T):
    """data and the model's results for (n, T), made once: r, v of mixed magnitudes, the two sums the kernel reads, the new r (= new v), the sum of q^2"""
    if (n, T) not in _CASES:
        rng = np.random.default_rng([n, 17])
        r, v = rc.wide(rng, n), rc.wide(rng, n)
        with np.errstate(all="ignore"):
            sums = np.array([ordered_sum(r * r, T), ordered_sum(v * r, T)])
            ntheta = -sums[1]
            inv = np.float64(1.0) / np.sqrt(sums[0])
            t = ntheta * v                                # each product and each sum rounded once
            q = t + r
            want_sum = ordered_sum(q * q, T)
            s = inv * r
        for a in (r, v, sums, s):
            a.setflags(write=False)
        _CASES[(n, T)] = (r, v, sums, s, want_sum)
    return _CASES[(n, T)]


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).reshape(-1).view(np.uint64), np.asarray(b, np.float64).reshape(-1).view(np.uint64))


@pytest.mark.parametrize("T", THREADS)
@pytest.mark.parametrize("n", SIZES)
def test_kernel_gives_the_models_bits(lib, work, n, T):
    r, v, sums, s, want_sum = case(n, T)
    dr, dv = Vec(r), Vec(v)
    dsums, res = DA.from_host(np.array(sums)), DA.from_host(sentinels(3))
    check(lib.liship_memset(work.ptr, 0xFF, work.nbytes, None))          # every double of the scratch a NaN
    check(lib.liship_set_reference_reductions(T))
    check(lib.liship_ritz_tail_f64(n, dsums.ptr, dr.ptr, dv.ptr, res.ptr, work.ptr, None))
    check(lib.liship_device_synchronize())
    got = res.to_host()
    print(n, T, float(got[0]).hex(), float(want_sum).hex())
    assert same_bits(got[:1], [want_sum]), (float(got[0]).hex(), float(want_sum).hex())
    assert (got[1:].view(np.uint64) == SENT).all()                       # one result, nothing behind it
    for name, d in (("r", dr), ("v", dv)):
        inside, intact = d.read()
        assert same_bits(inside, s), (name, np.flatnonzero(inside.view(np.uint64) != s.view(np.uint64))[:8])
        assert intact, name + ": guard word overwritten"
    assert same_bits(dsums.to_host(), sums)


def test_the_sum_is_the_one_liship_sumsq_forms(lib, work):
    """the contract by the library's own reduction: q formed by liship_axpyz_f64, then liship_sumsq_f64 on it, at a size with a fold"""
    n = 4097
    for T in (0, 3):
        r, v, sums, s, want_sum = case(n, T)
        dr, dv, dq, res = Vec(r), Vec(v), Vec(np.zeros(n)), DA.from_host(sentinels(2))
        check(lib.liship_set_reference_reductions(T))
        check(lib.liship_axpyz_f64(n, -sums[1], dv.ptr, dr.ptr, dq.ptr, None))
        check(lib.liship_sumsq_f64(n, dq.ptr, res.ptr, work.ptr, None))
        check(lib.liship_device_synchronize())
        assert same_bits(res.to_host()[:1], [want_sum])


@pytest.mark.parametrize("T", [0, 3])
@pytest.mark.parametrize("n", [3, 4097])                    # one workgroup (no fold to ride in), a fold
def test_an_announced_step_runs_as_behind_liship_sumsq(lib, work, n, T):
    """liship.h: "a pending liship_krylov_chain step rides in the fold, as in liship_sumsq_f64" -- with one workgroup and in the reference-order mode too.
    The state block after {announce, ritz_tail into SUM0} equals, in every bit, the block after {announce, liship_sumsq_f64 of the stored q into SUM0},
    and nothing stays pending: a flush behind it changes nothing."""
    import krylov_model as km
    r, v, sums, s, want_sum = case(n, T)
    st = km.new_state(rho=0.7310585786300049, rho_old=1.3, bnrm=3.0, tol=1e-300, iter=3.0, nhist=3.0, nrm2=0.125, not_half=0.0)
    st[19:] = np.arange(19, km.KS_LEN) + 0.5
    hist = 8
    check(lib.liship_set_reference_reductions(T))

    def after(launch):
        dst, dh = DA.from_host(st), DA.from_host(sentinels(hist))
        check(lib.liship_krylov_chain(km.STEP_CG_RESID, dst.ptr, dh.ptr))
        launch(dst.ptr + 8 * km.KS_SUM0)
        check(lib.liship_device_synchronize())
        return dst, dh, dst.to_host(), dh.to_host()

    dr, dv, dq, dsums = Vec(r), Vec(v), Vec(np.zeros(n)), DA.from_host(np.array(sums))
    check(lib.liship_axpyz_f64(n, -sums[1], dv.ptr, dr.ptr, dq.ptr, None))          # q, stored
    _, _, want, want_hist = after(lambda res: check(lib.liship_sumsq_f64(n, dq.ptr, res, work.ptr, None)))
    dst, dh, got, got_hist = after(lambda res: check(lib.liship_ritz_tail_f64(n, dsums.ptr, dr.ptr, dv.ptr, res, work.ptr, None)))
    assert same_bits(want[km.KS_SUM0:km.KS_SUM0 + 1], [want_sum]) and want[km.KS_ITER] == 4.0          # the step ran behind liship_sumsq_f64
    assert same_bits(got, want), np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
    assert same_bits(got_hist, want_hist)
    check(lib.liship_krylov_chain_flush(None))
    check(lib.liship_device_synchronize())
    assert same_bits(dst.to_host(), got) and same_bits(dh.to_host(), got_hist)


@pytest.mark.parametrize("T", [0, 8])
def test_fused_tail_and_the_six_separate_calls_give_equal_bits(lib, work, T):
    """multidot + ritz_tail against nrm2 (as sumsq), dot, axpyz, nrm2 (as sumsq), scale, copy on the same data"""
    import ctypes as C
    n = 100003
    r, v = case(n, T)[:2]
    check(lib.liship_set_reference_reductions(T))
    # fused: two passes
    fr, fv, fres = Vec(r), Vec(v), DA.from_host(sentinels(4))
    vecs = (C.c_void_p * 2)(fr.ptr, fv.ptr)
    pairs = ((C.c_int * 2) * 2)((0, 0), (1, 0))
    check(lib.liship_multidot_f64(n, 2, vecs, 2, pairs, fres.ptr, work.ptr, None))
    check(lib.liship_ritz_tail_f64(n, fres.ptr, fr.ptr, fv.ptr, fres.ptr + 16, work.ptr, None))
    check(lib.liship_device_synchronize())
    fused = fres.to_host()
    # separate: six passes, the scalars through the host as lis_vector_* take them
    ur, uv, uq, ures = Vec(r), Vec(v), Vec(np.zeros(n)), DA.from_host(sentinels(4))
    check(lib.liship_sumsq_f64(n, ur.ptr, ures.ptr, work.ptr, None))
    check(lib.liship_dot_f64(n, uv.ptr, ur.ptr, ures.ptr + 8, work.ptr, None))
    check(lib.liship_device_synchronize())
    sumsq, theta = ures.to_host()[:2]
    check(lib.liship_axpyz_f64(n, -theta, uv.ptr, ur.ptr, uq.ptr, None))
    check(lib.liship_sumsq_f64(n, uq.ptr, ures.ptr + 16, work.ptr, None))
    check(lib.liship_scale_f64(n, 1.0 / np.sqrt(sumsq), ur.ptr, None))
    check(lib.liship_memcpy_d2d(uv.ptr, ur.ptr, 8 * n, None))
    check(lib.liship_device_synchronize())
    unfused = ures.to_host()
    assert same_bits(fused[:3], unfused[:3]) and (fused[3:].view(np.uint64) == SENT).all()
    for a, b in ((fr, ur), (fv, uv)):
        (ia, oka), (ib, okb) = a.read(), b.read()
        assert same_bits(ia, ib) and oka and okb
    assert same_bits(fr.read()[0], fv.read()[0])


def test_refusals_write_nothing(lib, work):
    n = 2049
    r, v, sums = case(n, 0)[:3]
    dsums = DA.from_host(np.array(sums))

    def refused(n_, rp, vp, vecs):
        res = DA.from_host(sentinels(2))
        assert lib.liship_ritz_tail_f64(n_, dsums.ptr, rp, vp, res.ptr, work.ptr, None) == ERR_ARG
        check(lib.liship_device_synchronize())
        assert (res.to_host().view(np.uint64) == SENT).all()
        for d, host in vecs:
            inside, intact = d.read()
            assert same_bits(inside, host) and intact

    a, b = Vec(r), Vec(v)
    a8, b8 = Vec(r, off=1), Vec(v, off=1)
    refused(n, a8.ptr, b.ptr, [(a8, r), (b, v)])            # r only 8 B aligned
    refused(n, a.ptr, b8.ptr, [(a, r), (b8, v)])            # v only 8 B aligned
    refused(n, a.ptr, a.ptr, [(a, r)])                      # r and v the same array: each is read and written by its lane, refused
    refused(n - 16, a.ptr, a.ptr + 64, [(a, r)])            # overlapping
    refused(0, a.ptr, b.ptr, [(a, r), (b, v)])
    refused(-3, a.ptr, b.ptr, [(a, r), (b, v)])
    for args in ((None, a.ptr, b.ptr), (dsums.ptr, None, b.ptr), (dsums.ptr, a.ptr, None)):
        assert lib.liship_ritz_tail_f64(n, args[0], args[1], args[2], dsums.ptr, work.ptr, None) == ERR_ARG
    assert lib.liship_ritz_tail_f64(n, dsums.ptr, a.ptr, b.ptr, None, work.ptr, None) == ERR_ARG
    assert lib.liship_ritz_tail_f64(n, dsums.ptr, a.ptr, b.ptr, dsums.ptr, None, None) == ERR_ARG
