"""What tests/test_bjacobi_cpu.py (oracle against the reference library) and tests/test_bjacobi_gpu.py (liblis_amd against the oracle)
share: the matrices, their diagonal blocks, hand-built blocks for the kernels, and the reference's WD, M^-1 b and M^-H b seen through
ctypes.

Matrices: the 7-point Poisson matrix on 7 x 5 x 3 (n = 105: every block size but 1, 3, 5 and 7 leaves a partial last block) and
tests/golden/mm/testmat0.mtx (n = 100)."""
import ctypes as C
import os

import numpy as np

import ilu_cases
import orc
from lis_amd import _capi as capi

HERE = os.path.dirname(os.path.abspath(__file__))
BNS = (1, 2, 3, 4, 5, 7)
NAMED = ("p105", "testmat0")
bits, same_bits = ilu_cases.bits, ilu_cases.same_bits

_cache = {}


def system(name):
    """(ptr, idx, val) of a named matrix"""
    if name not in _cache:
        if name == "p105":
            _cache[name] = orc.poisson3d(7, 5, 3)
        elif name == "testmat0":
            _cache[name] = ilu_cases.read_mtx(os.path.join(HERE, "golden", "mm", "testmat0.mtx"))
        else:
            raise KeyError(name)
    return _cache[name]


def golden_system(case):
    """(ptr, idx, val) of a case of tests/golden/bjacobi_bits.json"""
    if case == "poisson7x5x3":
        return system("p105")
    if case == "poisson16":
        if case not in _cache:
            _cache[case] = orc.poisson3d(16, 16, 16)
        return _cache[case]
    assert case == "mm/testmat0.mtx", case
    return system("testmat0")


def rhs(n):
    """mixed signs, no zero"""
    i = np.arange(1, n + 1, dtype=np.float64)
    return np.where(i % 3 == 0, -i, i) / n


def diagonal_blocks(ptr, idx, val, bn):
    """D of the split bn x bn BSR form of a CSR matrix: nr blocks, column-major, the last one zero where it reaches beyond n"""
    n = len(ptr) - 1
    nr = (n + bn - 1) // bn
    d = np.zeros(nr * bn * bn)
    for i in range(n):
        for k in range(ptr[i], ptr[i + 1]):
            c = int(idx[k])
            if c // bn == i // bn:
                d[(i // bn) * bn * bn + i % bn + (c % bn) * bn] = val[k]
    return d


def random_blocks(nr, bn, seed):
    """nr blocks with mixed signs and magnitudes from 1e-3 to 1e3, a heavy diagonal (no pivot near zero without pivoting), and a few
    subnormal and -0.0 entries off the diagonal"""
    rng = np.random.default_rng(seed)
    bs = bn * bn
    d = rng.uniform(-1.0, 1.0, nr * bs) * 10.0 ** rng.integers(-3, 4, nr * bs)
    for b in range(nr):
        blk = d[b * bs:(b + 1) * bs]
        scale = np.abs(blk).sum()
        for i in range(bn):
            blk[i * (bn + 1)] = (scale + 1.0) * (1.0 if (b + i) % 2 else -1.0)
    if bn > 1:
        off = np.array([e for e in range(nr * bs) if (e % bs) % (bn + 1) != 0])
        pick = rng.choice(off, size=max(1, len(off) // 16), replace=False)
        d[pick[0::2]] = 4.9e-324 * rng.integers(1, 1000, len(pick[0::2]))
        d[pick[1::2]] = -0.0
    return d


def random_vector(n, seed):
    """mixed signs and magnitudes, some subnormals, some zeros of either sign"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, 1.0, n) * 10.0 ** rng.integers(-4, 5, n)
    x[rng.random(n) < 0.05] = 2.2e-310
    x[rng.random(n) < 0.05] = 0.0
    x[rng.random(n) < 0.05] = -0.0
    return x


def negative_zero_case(bn):
    """(d, x, n) of two blocks in which every product is a zero: the first of each row -0.0, the others -0.0 in block 0 and +0.0 in
    block 1.  A sum that starts with the first product gives -0.0 in block 0; one that starts at +0.0 gives +0.0 everywhere."""
    n = 2 * bn
    d = np.full(2 * bn * bn, 3.0)
    x = np.concatenate([np.full(bn, -0.0), np.full(bn, 0.0)])
    x[bn] = -0.0
    return d, x, n


# ---------------------------------------------------------------- the reference's structures (its include/lis.h: LIS_PRECON_STRUCT)
class Precon(C.Structure):
    _fields_ = [("precon_type", C.c_int), ("A", C.c_void_p), ("Ah", C.c_void_p), ("L", C.c_void_p), ("U", C.c_void_p),
                ("WD", C.POINTER(capi.MatrixDiag)), ("D", capi.PV)]


class one_thread:
    """The reference inverts the blocks in an OpenMP loop whose body (lis_array_ge) allocates through lis_malloc, and lis_malloc keeps an
    unlocked list of its allocations: with more than one thread the loop loses entries of that list and later calls of the same process
    find their objects "undefined".  A block is inverted by one thread whatever the thread count, so no number depends on it: the
    reference's lis_precon_create runs inside this block, at one thread, and everything else (conversion, split, products, psolves,
    the Krylov loops and their sums) at the thread count the library was initialised with."""
    def __init__(self, ref):
        self.dll = ref.dll

    def __enter__(self):
        self.dll.omp_get_max_threads.restype = C.c_int
        self.T = self.dll.omp_get_max_threads()
        self.dll.omp_set_num_threads(1)

    def __exit__(self, *a):
        self.dll.omp_set_num_threads(self.T)


def reference_solve(ref, A, b, options):
    """lis_solve as the reference runs it -- lis_precon_create, lis_solve_kernel, lis_precon_destroy (src/solver/lis_solver.c:367-405) -- with
    the first step at one thread (class one_thread); the result in the shape of lisdrv.solve"""
    import lisdrv
    vb, vx = lisdrv.new_vector(ref, A, b), lisdrv.new_vector(ref, A)
    S = capi.PS()
    assert ref.lis_solver_create(C.byref(S)) == 0
    assert ref.lis_solver_set_option(options.encode(), S) == 0
    S.contents.A = A
    create, kernel, destroy = ref.dll.lis_precon_create, ref.dll.lis_solve_kernel, ref.dll.lis_precon_destroy
    create.restype, create.argtypes = C.c_int, [capi.PS, C.POINTER(C.c_void_p)]
    kernel.restype, kernel.argtypes = C.c_int, [capi.PM, capi.PV, capi.PV, capi.PS, C.c_void_p]
    destroy.restype, destroy.argtypes = C.c_int, [C.c_void_p]
    pp = C.c_void_p()
    with one_thread(ref):
        err = create(S, C.byref(pp))
    if not err:
        err = kernel(A, vb, vx, S, pp)
        destroy(pp)
    it, res, st = C.c_int(), C.c_double(), C.c_int()
    ref.lis_solver_get_iter(S, C.byref(it))
    ref.lis_solver_get_residualnorm(S, C.byref(res))
    ref.lis_solver_get_status(S, C.byref(st))
    maxiter = S.contents.options[2]
    rh = np.ctypeslib.as_array(S.contents.rhistory, shape=(min(it.value, maxiter) + 1,)).copy() if S.contents.rhistory else np.zeros(0)
    out = dict(err=err, x=lisdrv.get_vector(ref, vx, A.contents.n), iter=it.value, resid=res.value, status=st.value, rhistory=rh)
    ref.lis_solver_destroy(S)
    ref.lis_vector_destroy(vb)
    ref.lis_vector_destroy(vx)
    return out


def reference_bjacobi(ref, ptr, idx, val, bn, b, storage=True):
    """{"WD", "bn", "nr", "psolve", "psolveh", "type", "split"} from the reference library: its lis_precon_create with -p bjacobi -storage bsr
    -storage_block bn on a CSR matrix, its two psolves (separate B and X, both made after the conversion so that they carry its padding).
    storage=False: no -storage option -- the reference turns to Jacobi and "WD" is its 1 / diag."""
    import lisdrv
    A = lisdrv.make_csr(ref, ptr, idx, val)
    n = A.contents.n
    S = capi.PS()
    assert ref.lis_solver_create(C.byref(S)) == 0
    opts = "-p bjacobi" + (" -storage bsr -storage_block %d" % bn if storage else "")
    assert ref.lis_solver_set_option(opts.encode(), S) == 0
    S.contents.A = A
    create = ref.dll.lis_precon_create
    create.restype, create.argtypes = C.c_int, [capi.PS, C.POINTER(C.c_void_p)]
    pp = C.c_void_p()
    with one_thread(ref):
        assert create(S, C.byref(pp)) == 0
    P = C.cast(pp, C.POINTER(Precon)).contents
    out = {"type": A.contents.matrix_type, "split": bool(A.contents.is_splited), "precon_type": P.precon_type, "option": S.contents.options[1]}
    if P.precon_type == capi_precon_type("bjacobi"):
        WD = P.WD.contents
        out.update(bn=WD.bn, nr=WD.nr, WD=np.ctypeslib.as_array(WD.value, shape=(WD.nr * WD.bn * WD.bn,)).copy())
        names = ("lis_psolve_bjacobi", "lis_psolveh_bjacobi")
    else:
        out.update(bn=1, nr=n, WD=lisdrv.get_vector(ref, P.D, n))
        names = ("lis_psolve_jacobi", "lis_psolveh_jacobi")
    S.contents.precon = pp
    for tag, name in zip(("psolve", "psolveh"), names):
        fn = getattr(ref.dll, name)
        fn.restype, fn.argtypes = C.c_int, [capi.PS, capi.PV, capi.PV]
        vb, vx = lisdrv.new_vector(ref, A, b), lisdrv.new_vector(ref, A, np.full(n, 7.0))
        assert fn(S, vb, vx) == 0
        out[tag] = lisdrv.get_vector(ref, vx, n)
        ref.lis_vector_destroy(vb)
        ref.lis_vector_destroy(vx)
    S.contents.precon = None
    destroy = ref.dll.lis_precon_destroy
    destroy.restype, destroy.argtypes = C.c_int, [C.c_void_p]
    destroy(pp)
    ref.lis_solver_destroy(S)
    ref.lis_matrix_destroy(A)
    return out


def capi_precon_type(name):
    return {"none": 0, "jacobi": 1, "ilu": 2, "ssor": 3, "bjacobi": 10}[name]
