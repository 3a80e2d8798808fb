"""The two pair passes (liship_scale2_inv_sqrt_f64, liship_scale2_to_f64; kernels/vector_ops.hip, functors over vector_pass<NT, VEC, 2, 2>) against the numpy
model tests/pair_pass_model.py in every bit: at every size where the walk takes another shape (one lane, the odd tail taken by lane 0 of block 0, the tile
edge, a second workgroup), with every operand 16 B aligned and with one operand 8 B off (the scalar walk), in place and out of place, guard words before and
behind every array; the refusals, with the outputs untouched; the special values of *s; and the separate calls they replace."""
import numpy as np
import pytest

import lis_amd
import pair_pass_model as ppm
import reduction_cases as rc
from lis_amd import DeviceArray as DA, check

pytestmark = pytest.mark.gpu
ERR_ARG = -1
SENT = np.uint64(0x7FF8DEAD0000BEEF)              # a quiet NaN no arithmetic here produces
PAD = 6                                           # guard words behind every vector
SIZES = [1, 2, 3, 255, 256, 257, 2047, 2048, 2049, 4097]
# which of the four arrays (in0, in1, out0, out1) lies 8 B past a 16 B aligned address; None: all aligned (the 16 B walk)
OFFSETS = [None, 0, 1, 2, 3]


@pytest.fixture(scope="module")
def lib():
    lib = lis_amd.load()
    assert lis_amd.gpu_available(), "no HIP device: the product path has no CPU fallback"
    assert not lib.liship_missing
    return lib


@pytest.fixture(autouse=True)
def defaults(lib):
    lib.liship_krylov_guard(None)
    yield
    lib.liship_krylov_guard(None)
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


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).reshape(-1).view(np.uint64), np.asarray(b, np.float64).reshape(-1).view(np.uint64))


_DATA = {}


def data(n):
    if n not in _DATA:
        rng = np.random.default_rng([n, 23])
        v, w = rc.wide(rng, n), rc.wide(rng, n)
        v.setflags(write=False); w.setflags(write=False)
        _DATA[n] = (v, w)
    return _DATA[n]


ALPHA = 0.37
S = 5.3


@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("n", SIZES)
def test_scale2_to_out_of_place_gives_the_models_bits(lib, n, off):
    v, w = data(n)
    offs = [1 if off == k else 0 for k in range(4)]
    want0, want1 = ppm.scale2_to(ALPHA, v, w, vec=off is None)
    i0, i1, o0, o1 = Vec(v, offs[0]), Vec(w, offs[1]), Vec(sentinels(n), offs[2]), Vec(sentinels(n), offs[3])
    check(lib.liship_scale2_to_f64(n, ALPHA, i0.ptr, i1.ptr, o0.ptr, o1.ptr, None))
    for vec, want in ((o0, want0), (o1, want1), (i0, v), (i1, w)):
        got, guards = vec.read()
        assert same_bits(got, want) and guards


@pytest.mark.parametrize("off", [None, 0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_scale2_to_in_place_gives_the_models_bits(lib, n, off):
    v, w = data(n)
    want0, want1 = ppm.scale2_to(ALPHA, v, w, vec=off is None)
    a, b = Vec(v, 1 if off == 0 else 0), Vec(w, 1 if off == 1 else 0)
    check(lib.liship_scale2_to_f64(n, ALPHA, a.ptr, b.ptr, a.ptr, b.ptr, None))
    for vec, want in ((a, want0), (b, want1)):
        got, guards = vec.read()
        assert same_bits(got, want) and guards
    # one array in place, the other out of place
    a, b, o = Vec(v), Vec(w), Vec(sentinels(n))
    check(lib.liship_scale2_to_f64(n, ALPHA, a.ptr, b.ptr, a.ptr, o.ptr, None))
    assert same_bits(a.read()[0], want0) and same_bits(o.read()[0], want1) and same_bits(b.read()[0], w) and a.read()[1] and o.read()[1]


@pytest.mark.parametrize("off", [None, 0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_scale2_inv_sqrt_gives_the_models_bits(lib, n, off):
    v, w = data(n)
    want0, want1 = ppm.scale2_inv_sqrt(S, v, w, vec=off is None)
    a, b, s = Vec(v, 1 if off == 0 else 0), Vec(w, 1 if off == 1 else 0), Vec(np.array([S]))
    check(lib.liship_scale2_inv_sqrt_f64(n, s.ptr, a.ptr, b.ptr, None))
    for vec, want in ((a, want0), (b, want1), (s, [S])):
        got, guards = vec.read()
        assert same_bits(got, want) and guards


@pytest.mark.parametrize("s", [0.0, -0.0, -1.0, np.inf, -np.inf, np.nan, 5e-324, 1.7e308])
def test_special_values_of_s(lib, s):
    """*s = 0 gives inf, and 0 * inf NaN; *s < 0 gives NaN everywhere (no fabs: the NaN of -e gsi); *s = +inf gives 0 and 0 * inf NaN"""
    n = 2049
    v, w = np.array(data(n)[0]), np.array(data(n)[1])
    v[:4] = [0.0, -0.0, np.inf, 1.0]
    w[-3:] = [np.nan, -np.inf, 0.0]
    want0, want1 = ppm.scale2_inv_sqrt(s, v, w)
    if s == 0.0 and not np.signbit(s):
        assert np.isposinf(want0[3]) and np.isnan(want0[0])
    if s == -1.0:
        assert np.isnan(want0).all() and np.isnan(want1).all()
    if s == np.inf:
        assert want0[3] == 0.0 and np.isnan(want0[2])
    a, b, ds = Vec(v), Vec(w), Vec(np.array([s]))
    check(lib.liship_scale2_inv_sqrt_f64(n, ds.ptr, a.ptr, b.ptr, None))
    for vec, want in ((a, want0), (b, want1)):
        got, guards = vec.read()
        assert np.array_equal(np.isnan(got), np.isnan(want)) and guards         # where the model has NaN the kernel has; which NaN is not compared
        keep = ~np.isnan(want)
        assert same_bits(got[keep], want[keep])


@pytest.mark.parametrize("n", [1, 3, 257, 2049, 4097])
def test_the_separate_calls_give_the_same_bits(lib, n):
    v, w = data(n)
    # liship_scale_inv_norm_f64 twice
    a, b, s = Vec(v), Vec(w), Vec(np.array([S]))
    check(lib.liship_scale_inv_norm_f64(n, s.ptr, a.ptr, None))
    check(lib.liship_scale_inv_norm_f64(n, s.ptr, b.ptr, None))
    fa, fb = Vec(v), Vec(w)
    check(lib.liship_scale2_inv_sqrt_f64(n, s.ptr, fa.ptr, fb.ptr, None))
    assert same_bits(fa.read()[0], a.read()[0]) and same_bits(fb.read()[0], b.read()[0])
    # copy + scale, twice
    r, q, wj, vj = Vec(v), Vec(w), Vec(sentinels(n)), Vec(sentinels(n))
    for src, dst in ((r, wj), (q, vj)):
        check(lib.liship_memcpy_d2d(dst.ptr, src.ptr, 8 * n, None))
    for dst in (wj, vj):
        check(lib.liship_scale_f64(n, ALPHA, dst.ptr, None))
    fw, fv = Vec(sentinels(n)), Vec(sentinels(n))
    check(lib.liship_scale2_to_f64(n, ALPHA, r.ptr, q.ptr, fw.ptr, fv.ptr, None))
    assert same_bits(fw.read()[0], wj.read()[0]) and same_bits(fv.read()[0], vj.read()[0])


def test_refusals_launch_nothing(lib):
    n = 300
    v, w = data(n)
    big = Vec(np.concatenate([v, w, v]))                      # three spans of n inside one allocation, to overlap at will
    a, b, o, p, s = Vec(v), Vec(w), Vec(sentinels(n)), Vec(sentinels(n)), Vec(np.array([S]))
    at = lambda k: big.ptr + 8 * k

    def untouched():
        lib.liship_device_synchronize()
        got, guards = big.read()
        assert same_bits(got, np.concatenate([v, w, v])) and guards
        for vec, want in ((a, v), (b, w), (o, sentinels(n)), (p, sentinels(n))):
            assert same_bits(vec.read()[0], want)

    to = lambda i0, i1, o0, o1, n_=n: lib.liship_scale2_to_f64(n_, ALPHA, i0, i1, o0, o1, None)
    assert to(a.ptr, b.ptr, o.ptr, o.ptr) == ERR_ARG                       # the two outputs are one array
    assert to(a.ptr, b.ptr, at(0), at(n - 1)) == ERR_ARG                   # ... overlap by one element
    assert to(a.ptr, b.ptr, b.ptr, a.ptr) == ERR_ARG                       # an output is the OTHER input
    assert to(a.ptr, b.ptr, b.ptr, o.ptr) == ERR_ARG
    assert to(at(0), b.ptr, at(1), o.ptr) == ERR_ARG                       # an output overlaps its own input, shifted
    assert to(a.ptr, at(n), o.ptr, at(n - 8)) == ERR_ARG
    assert to(a.ptr, a.ptr, a.ptr, a.ptr) == ERR_ARG
    assert to(a.ptr, b.ptr, o.ptr, p.ptr, 0) == ERR_ARG and to(a.ptr, b.ptr, o.ptr, p.ptr, -4) == ERR_ARG
    for args in ((None, b.ptr, o.ptr, p.ptr), (a.ptr, None, o.ptr, p.ptr), (a.ptr, b.ptr, None, p.ptr), (a.ptr, b.ptr, o.ptr, None)):
        assert to(*args) == ERR_ARG
    inv = lambda sp, x, y, n_=n: lib.liship_scale2_inv_sqrt_f64(n_, sp, x, y, None)
    assert inv(s.ptr, a.ptr, a.ptr) == ERR_ARG                             # v == w
    assert inv(s.ptr, at(0), at(n // 2)) == ERR_ARG
    assert inv(at(5), at(0), b.ptr) == ERR_ARG and inv(at(n + 5), a.ptr, at(n)) == ERR_ARG      # s inside v, inside w
    assert inv(None, a.ptr, b.ptr) == ERR_ARG and inv(s.ptr, None, b.ptr) == ERR_ARG and inv(s.ptr, a.ptr, None) == ERR_ARG
    assert inv(s.ptr, a.ptr, b.ptr, 0) == ERR_ARG and inv(s.ptr, a.ptr, b.ptr, -1) == ERR_ARG
    untouched()
    # what is allowed beside them: read-only inputs may be one array; s right behind v
    check(to(a.ptr, a.ptr, o.ptr, p.ptr))
    assert same_bits(o.read()[0], np.float64(ALPHA) * v) and same_bits(p.read()[0], np.float64(ALPHA) * v)
    vs, fresh = Vec(np.concatenate([v, [S]])), Vec(w)
    check(inv(vs.ptr + 8 * n, vs.ptr, fresh.ptr))
    want0, want1 = ppm.scale2_inv_sqrt(S, v, w)
    assert same_bits(vs.read()[0], np.concatenate([want0, [S]])) and same_bits(fresh.read()[0], want1)


def test_a_raised_guard_skips_the_pass(lib):
    """the pair passes run behind a device-driven loop's guard as every element-wise pass does"""
    n = 513
    v, w = data(n)
    a, b, flag = Vec(v), Vec(w), Vec(np.array([1.0]))
    lib.liship_krylov_guard(flag.ptr)
    check(lib.liship_scale2_to_f64(n, ALPHA, a.ptr, b.ptr, a.ptr, b.ptr, None))
    lib.liship_krylov_guard(None)
    assert same_bits(a.read()[0], v) and same_bits(b.read()[0], w)
