"""liship_multidot_f64 (kernels/eigen.hip): K inner products over V vectors in one pass, every sum in the bits liship_dot_f64 gives that pair alone.

Each result is held to two things, with no tolerance: tests/reduction_model.py's tree (level 1 with the 16 B or the 8 B lane mapping chosen from that pair's
own two arrays, wavefront, workgroup, folds) -- or, in the reference-order mode, the T chunks of krylov_model.chunked_sum -- and the result of a separate
liship_dot_f64 call on the same two arrays.  Sizes are those of tests/reduction_cases.py (every fold stage that list reaches) plus 1, 2, 3, 2047, 2048, 2049.
Comparisons are on uint64 views (a NaN has to be a NaN); vectors carry sentinels around their n elements, the result array behind its K, and the work
buffer is poisoned before every call."""
import ctypes as C

import numpy as np
import pytest

import krylov_model as km
import lis_amd
import reduction_cases as rc
import reduction_model as rm
from lis_amd import DeviceArray as DA, check
from test_reduction_tree_gpu import SENT, Vec, canon, differing, poison, sentinels

pytestmark = pytest.mark.gpu
ERR_ARG = -1
SIZES = sorted(set(rc.SIZES) | {1, 2, 3, 2047, 2048, 2049})

ALL5 = [(i, j) for i in range(5) for j in range(i, 5)]                           # the 15 unordered pairs of 5 vectors
CG15 = [(0, 3), (1, 3), (2, 3), (1, 4), (2, 4), (2, 5), (0, 0), (1, 0), (2, 0), (1, 1), (2, 1), (2, 2), (1, 4), (3, 3), (5, 4)]   # lis_ecg's Gram block over (w x p Aw Ax Ap), and three more
CR5 = [(0, 2), (0, 1), (2, 2), (1, 2), (1, 1)]                                   # lis_ecr's alpha block over (r p Ap)
# (V, pairs): K = 1, 2, 5, 15 and V = 2 .. 6; a vector with itself; <a,b> and <b,a>; one pair named twice
CONFIGS = {
    "v2k1": (2, [(0, 1)]),
    "v2k2": (2, [(1, 0), (1, 1)]),
    "v3k5": (3, CR5),
    "v4k5": (4, [(0, 1), (2, 0), (3, 1), (3, 2), (3, 2)]),                       # lis_ecr's beta block over (Aw Ap p w), its last pair twice
    "v5k15": (5, ALL5),
    "v6k15": (6, CG15),
}


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


def data(V, n, seed):
    rng = np.random.default_rng(1000 * V + seed)
    return [rc.wide(rng, n) for _ in range(V)]


def expected(hosts, offs, pairs, T):
    out = []
    with np.errstate(all="ignore"):
        for a, b in pairs:
            terms = hosts[a] * hosts[b]
            if T > 0:
                out.append(km.chunked_sum(terms, T))
            else:
                out.append(rm.tree(terms, vector=(offs[a] == 0 and offs[b] == 0)) if len(terms) else 0.0)
    return np.array(out, np.float64)


def run(lib, work, hosts, offs, pairs, T=0):
    """one liship_multidot_f64 call -> what differs from the model and from separate liship_dot_f64 calls"""
    n, V, K = len(hosts[0]), len(hosts), len(pairs)
    vecs = [Vec(h, off) for h, off in zip(hosts, offs)]
    ptrs = (C.c_void_p * V)(*[v.ptr for v in vecs])
    cp = (C.c_int * (2 * K))(*[i for p in pairs for i in p])
    res = DA.from_host(sentinels(K + 2))
    check(lib.liship_set_reference_reductions(T))
    poison(lib, work)
    check(lib.liship_multidot_f64(n, V, ptrs, K, cp, res.ptr, work.ptr, None))
    check(lib.liship_device_synchronize())
    got = res.to_host()
    bad = []
    want = expected(hosts, offs, pairs, T)
    if differing(got[:K], want):
        bad.append(("model", differing(got[:K], want), [hex(b) for b in canon(got[:K])], [hex(b) for b in canon(want)]))
    if not (got[K:].view(np.uint64) == SENT).all():
        bad.append(("result: written past its %d doubles" % K,))
    single = DA.from_host(sentinels(2))
    alone = []
    for a, b in pairs:
        poison(lib, work)
        check(lib.liship_dot_f64(n, vecs[a].ptr, vecs[b].ptr, single.ptr, work.ptr, None))
        alone.append(single.to_host()[0])
    if differing(got[:K], alone):
        bad.append(("separate dots", differing(got[:K], alone)))
    for k, v in enumerate(vecs):
        inside, intact = v.read()
        if differing(inside, hosts[k]) or not intact:
            bad.append(("vector %d changed" % k,))
    check(lib.liship_set_reference_reductions(0))
    return bad


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_every_sum_is_the_single_dots_sum(lib, work, name):
    """aligned vectors at the lane, wavefront, block, odd-tail and fold edges"""
    V, pairs = CONFIGS[name]
    bad = {n: b for n in SIZES for b in [run(lib, work, data(V, n, n), [0] * V, pairs)] if b}
    assert bad == {}


@pytest.mark.parametrize("name", ["v2k2", "v3k5", "v6k15"])
def test_a_vector_off_alignment_moves_its_own_pairs_only(lib, work, name):
    """one vector one double past a 16 B boundary: the pairs that involve it take the 8 B lane mapping (other bits, as tests/test_reduction_model_cpu.py
    shows on this kind of data), the others keep the 16 B one; two vectors off; all of them off"""
    V, pairs = CONFIGS[name]
    bad = {}
    for n in rc.ALIGN_SIZES + [65537]:
        hosts = data(V, n, n + 7)
        layouts = [[1 if k == j else 0 for k in range(V)] for j in range(V)] + [[1, 1] + [0] * (V - 2), [1] * V]
        for offs in layouts:
            b = run(lib, work, hosts, offs, pairs)
            if b:
                bad[(n, tuple(offs))] = b
    assert bad == {}


def test_the_two_lane_mappings_differ_on_this_data():
    """(what the alignment test proves something with: at every size beyond one tile some pair of the block has other bits under the other mapping, so a pair
    sent down the wrong one would show)"""
    V, pairs = CONFIGS["v3k5"]
    for n in (2049, 4097, 65537):
        hosts = data(V, n, n + 7)
        assert any(rm.tree(hosts[a] * hosts[b], vector=True) != rm.tree(hosts[a] * hosts[b], vector=False) for a, b in pairs), n


@pytest.mark.parametrize("T", [1, 3, 8])
def test_reference_order_mode_takes_the_T_chunks(lib, work, T):
    """n < T (empty chunks), n % T != 0, more than one tile per chunk; aligned or not makes no difference there"""
    V, pairs = CONFIGS["v6k15"]
    bad = {}
    for n in (0, 1, 2, 5, 7, 8, 9, 2049, 6145):
        hosts = data(V, n, n + T)
        for offs in ([0] * V, [0, 1, 0, 0, 1, 0]):
            b = run(lib, work, hosts, offs, pairs, T)
            if b:
                bad[(n, tuple(offs))] = b
    assert bad == {}


@pytest.mark.parametrize("kind", ["signed_zeros", "inf", "nan", "denormal"])
def test_special_values(lib, work, kind):
    n = rc.SPECIAL_N
    V, pairs = CONFIGS["v3k5"]
    hosts = data(V, n, 3)
    if kind == "signed_zeros":
        hosts = [np.where(np.arange(n) % 2 == 0, -0.0, 0.0), np.full(n, -0.0), np.where(np.arange(n) % 3 == 0, -1.0, 1.0)]      # sums of -0.0 and +0.0 terms from a lane's 0.0
    elif kind == "inf":
        hosts[0][[0, 2047, n - 1]] = [np.inf, -np.inf, np.inf]          # inf - inf inside one sum, +inf in another
        hosts[2][[5, 4096]] = np.inf
    elif kind == "nan":
        hosts[1][3071 * 2] = np.nan                                      # the last lane's last pair of block 2
        hosts[2][n - 1] = np.nan                                         # the odd tail
    else:
        hosts = [h * 1e-300 for h in hosts]                             # products underflow to denormals and zeros
        hosts[0][:8] = 5e-324
    for offs in ([0, 0, 0], [0, 1, 0]):
        assert run(lib, work, hosts, offs, pairs) == []
        assert run(lib, work, hosts, offs, pairs, 3) == []


def test_arguments_out_of_range_are_refused_and_nothing_is_written(lib, work):
    hosts = data(3, 100, 1)
    vecs = [Vec(h) for h in hosts]
    ptrs = (C.c_void_p * 3)(*[v.ptr for v in vecs])
    holes = (C.c_void_p * 3)(vecs[0].ptr, None, vecs[2].ptr)
    ok = (C.c_int * 4)(0, 1, 2, 2)
    res = DA.from_host(sentinels(4))
    for n, V, vp, K, pairs in ((-1, 3, ptrs, 2, ok), (100, 0, ptrs, 2, ok), (100, 9, ptrs, 2, ok), (100, 3, ptrs, 0, ok), (100, 3, ptrs, 37, ok),
                               (100, 3, ptrs, 2, (C.c_int * 4)(0, 3, 1, 1)), (100, 3, ptrs, 2, (C.c_int * 4)(0, 1, -1, 1)), (100, 3, holes, 2, ok),
                               (100, 3, None, 2, ok), (100, 3, ptrs, 2, None)):
        assert lib.liship_multidot_f64(n, V, vp, K, pairs, res.ptr, work.ptr, None) == ERR_ARG
    assert lib.liship_multidot_f64(100, 3, ptrs, 2, ok, None, work.ptr, None) == ERR_ARG
    assert lib.liship_multidot_f64(100, 3, ptrs, 2, ok, res.ptr, None, None) == ERR_ARG
    check(lib.liship_device_synchronize())
    assert (res.to_host().view(np.uint64) == SENT).all()
