"""What tests/golden/make_golden_bssor.py, tests/test_bssor_cpu.py (model against the reference library), tests/test_bssor_schedule_gpu.py
(kernels against the model) and tests/test_bssor_gpu.py (library against model and goldens) share: the matrices, the reference's WD and
triangular solves on a BSR matrix seen through ctypes, block sweeps built to a prescribed level schedule, and the same solves through
liblis_amd.

Triangular cases: 7-point Poisson on 7 x 5 x 3 (n = 105: block sizes 2, 4, 8 leave a partial last block) and on 6 x 5 x 4 (n = 120:
every block size divides it), block sizes 1, 2, 3, 4, 5, 8 (both sides of the "+0.0 start from bn = 4" rule), omega 1.0 and 1.3.
Whole solves: orc.poisson3d(8, 7, 6) (n = 336) in 2 x 2 and 5 x 5 blocks (5 does not divide 336), the nonsymmetric matrix of
make_golden_scale.test_matrix(n=120, seed=9) in 3 x 3 and 8 x 8, orc.fem3(4) (n = 192) in its 3 x 3 blocks."""
import ctypes as C
import os
import sys

import numpy as np

import bjacobi_cases
import bssor_oracle as oracle
import ilu_cases
import orc
import ssor_cases
from lis_amd import _capi as capi

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "bssor_bits.npz")
bits, same_bits = ilu_cases.bits, ilu_cases.same_bits

TRI_NAMES = ("p105", "p120")
TRI_BNS = (1, 2, 3, 4, 5, 8)
OMEGAS = (1.0, 1.3)
RUNS = (("poisson8x7x6", 2), ("poisson8x7x6", 5), ("nonsym120", 3), ("nonsym120", 8), ("fem3", 3))
SOLVERS = ("-i cg", "-i bicgstab", "-i gmres -restart 30", "-i bicg")
THREADS = (1, 8)
COMMON = "-p ssor -ssor_omega 1.3 -storage bsr -tol 1e-12 -maxiter 300 -print mem"

_cache = {}


def system(name):
    """(ptr, idx, val) of a named CSR matrix, built once"""
    if name not in _cache:
        if name == "p105":
            _cache[name] = orc.poisson3d(7, 5, 3)
        elif name == "p120":
            _cache[name] = orc.poisson3d(6, 5, 4)
        elif name == "poisson8x7x6":
            _cache[name] = orc.poisson3d(8, 7, 6)
        elif name == "nonsym120":
            sys.path.insert(0, os.path.join(HERE, "golden"))
            import make_golden_scale
            _cache[name] = make_golden_scale.test_matrix(n=120, seed=9)
        elif name == "fem3":
            _cache[name] = orc.fem3(4)[:3]
        else:
            raise KeyError(name)
    return _cache[name]


def rhs(n):
    return bjacobi_cases.rhs(n)


def to_bsr(ptr, idx, val, bn):
    """(bptr, bindex, value) of lis_matrix_convert_csr2bsr with bn x bn blocks, by the oracle's restatement of that conversion (a block
    row lists its block columns in the order the conversion meets them, which is what the sweeps then follow)"""
    _, bptr, bidx, bval = orc.csr2bsr(ptr, idx, val, bn, bn)
    return bptr, bidx, bval


def tri_key(name, bn, omega, what):
    return "tri|%s|bn%d|w%s|%s" % (name, bn, omega, what)


def run_key(case, solver, bn, T, what):
    return "run|%s|%s|bn%d|T%d|%s" % (case, solver, bn, T, what)


def solve_tag(name, flag, alias=False):
    return "%s%d%s" % (name, flag, "_alias" if alias else "")


# ---------------------------------------------------------------- a library with the Lis C API: split BSR matrix with WD, its solves
def wd_of(A):
    a = A.contents
    WD = C.cast(a.WD, C.POINTER(capi.MatrixDiag)).contents
    assert (WD.bn, WD.nr) == (a.bnr, a.nr)
    return np.ctypeslib.as_array(WD.value, shape=(a.nr * a.bnr * a.bnr,)).copy()


def precon_create(L, A, options, one_thread=False):
    """(err, solver, precon) of lis_precon_create on A; one_thread: at one OpenMP thread (the reference's block inversion allocates
    inside a parallel loop: bjacobi_cases.one_thread says why)"""
    S = capi.PS()
    assert L.lis_solver_create(C.byref(S)) == 0
    assert L.lis_solver_set_option(options.encode(), S) == 0
    S.contents.A = A
    create = L.dll.lis_precon_create
    create.restype, create.argtypes = C.c_int, [capi.PS, C.POINTER(C.c_void_p)]
    pp = C.c_void_p()
    if one_thread:
        with bjacobi_cases.one_thread(L):
            err = create(S, C.byref(pp))
    else:
        err = create(S, C.byref(pp))
    return err, S, pp


def precon_destroy(L, S, pp):
    destroy = L.dll.lis_precon_destroy
    destroy.restype, destroy.argtypes = C.c_int, [C.c_void_p]
    if pp:
        destroy(pp)
    L.lis_solver_destroy(S)


def prepared(L, A, omega, bn=0, one_thread=False):
    """A split, in BSR storage and with WD for omega, as lis_precon_create with -p ssor leaves it (bn > 0: -storage bsr -storage_block bn)"""
    opts = "-p ssor -ssor_omega %r" % omega + (" -storage bsr -storage_block %d" % bn if bn else "")
    err, S, pp = precon_create(L, A, opts, one_thread)
    assert err == 0, err
    precon_destroy(L, S, pp)
    a = A.contents
    assert a.matrix_type == capi.LIS_MATRIX_BSR and a.is_splited and a.WD
    return A


def library_solve(L, A, name, flag, b, alias=False):
    """lis_matrix_solve / lis_matrix_solveh on vectors made after the conversion (the reference's carry the padding of the last block)"""
    return ssor_cases.library_solve(L, A, name, flag, b, alias)


def all_library_solves(L, A, b):
    """{"wd", "solve0" ..., "solveh2_alias"}"""
    out = {"wd": wd_of(A)}
    for name, flag in oracle.SOLVES:
        for alias in (False, True):
            out[solve_tag(name, flag, alias)] = library_solve(L, A, name, flag, b, alias)
    return out


def model_solves(bsr, bn, n, omega, b):
    """the same dictionary from the model (an aliased solve is the same solve)"""
    res = oracle.all_solves(*bsr, bn, n, omega, b)
    out = {"wd": res["wd"]}
    for name, flag in oracle.SOLVES:
        out[solve_tag(name, flag)] = out[solve_tag(name, flag, True)] = res[name, flag]
    return out


_models = {}


def tri_model(name, bn, omega):
    key = (name, bn, omega)
    if key not in _models:
        ptr, idx, val = system(name)
        n = len(ptr) - 1
        _models[key] = model_solves(to_bsr(ptr, idx, val, bn), bn, n, omega, rhs(n))
    return _models[key]


def reference_triangular(ref, name, bn, omega):
    """WD and the twelve solves of the reference library on a named matrix converted by -storage bsr -storage_block bn"""
    import lisdrv
    ptr, idx, val = system(name)
    A = prepared(ref, lisdrv.make_csr(ref, ptr, idx, val), omega, bn, one_thread=True)
    out = all_library_solves(ref, A, rhs(len(ptr) - 1))
    ref.lis_matrix_destroy(A)
    return out


def reference_run(ref, case, solver, bn):
    import lisdrv
    ptr, idx, val = system(case)
    A = lisdrv.make_csr(ref, ptr, idx, val)
    b = lisdrv.matvec(ref, A, np.ones(len(ptr) - 1))
    res = bjacobi_cases.reference_solve(ref, A, b, "%s -storage_block %d %s" % (solver, bn, COMMON))
    assert res["err"] == 0 and A.contents.matrix_type == capi.LIS_MATRIX_BSR and A.contents.is_splited
    ref.lis_matrix_destroy(A)
    return res


def reference_everything(ref, T):
    """every array of the golden the reference gives at T threads: the triangular cases (which do not depend on T: the block sweeps are
    serial) and the whole solves"""
    out = {}
    for name in TRI_NAMES:
        for bn in TRI_BNS:
            for omega in OMEGAS:
                for what, v in reference_triangular(ref, name, bn, omega).items():
                    out[tri_key(name, bn, omega, what) + "|T%d" % T] = v
    for case, bn in RUNS:
        for solver in SOLVERS:
            res = reference_run(ref, case, solver, bn)
            out[run_key(case, solver, bn, T, "rhistory")] = res["rhistory"]
            out[run_key(case, solver, bn, T, "x")] = res["x"]
            out[run_key(case, solver, bn, T, "meta")] = np.array([res["iter"], res["status"]], np.int64)
    return out


def child_main(T, path):
    """in a process of its own: the reference reads its thread count once, at initialize"""
    import lisdrv
    ref = lisdrv.open_lib(orc.REF_SO, threads=T)
    np.savez(path, **reference_everything(ref, T))


def reference_in_child(T, path):
    import subprocess
    src = "import sys; sys.path[:0] = %r; import bssor_cases; bssor_cases.child_main(%d, %r)" % ([os.path.dirname(HERE), HERE], T, path)
    res = subprocess.run([sys.executable, "-c", src], capture_output=True, text=True, env=dict(os.environ, OMP_NUM_THREADS=str(T)), timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


# ---------------------------------------------------------------- block sweeps built to a prescribed schedule (liship_bsweep_f64)
LONG_ROW, SMALL_LEVEL = ssor_cases.LONG_ROW, ssor_cases.SMALL_LEVEL
CHUNK = {1: 256, 2: 256, 3: 128, 4: 128, 5: 64, 6: 32, 7: 32, 8: 32}     # kernels/bsptrsv.hip bsweep_chunk, asserted against liship_bsweep_chunk


class SweepT(C.Structure):
    _fields_ = [(k, C.c_int) for k in ("nlev", "nrows", "nnz", "ngroups")] + [(k, C.c_void_p) for k in ("lptr", "llong", "rows", "rptr", "col", "val", "groups", "h_nrows", "h_nshort")]


def block_values(rng, bn, count, special=False):
    """count blocks, small enough that sweeps of many terms stay finite; special: some entries +-0.0, denormal, 1e+-300, and a few +-inf
    (inf * 0 = NaN in the products of a term, in a long row's LDS and in the grouped sums of the transposed forms)"""
    v = rng.uniform(-1.0, 1.0, count * bn * bn) / (2.0 * bn)
    if special and len(v):
        pick = rng.random(len(v))
        v[pick < 0.03] = 0.0
        v[(pick >= 0.03) & (pick < 0.06)] = -0.0
        v[(pick >= 0.06) & (pick < 0.09)] = 4.9e-324 * 7
        v[(pick >= 0.09) & (pick < 0.11)] = -2.5e-310
        v[(pick >= 0.11) & (pick < 0.12)] = 1e-300
        v[(pick >= 0.12) & (pick < 0.125)] = 1e300
        far = np.flatnonzero(pick >= 0.999)                   # about one entry in a thousand: most of every result stays finite
        v[far] = np.where(rng.random(len(far)) < 0.5, np.inf, -np.inf)
    return v


def sweep_case(levels, bn, pad, seed, desc=False, special=False, duplicates=False):
    """A block sweep whose schedule has exactly the given levels (lists of block-row term counts, as ssor_cases.pattern takes them).
    Returns dict(n, nr, bn, gather, scatter, wd, order): gather[i] = [(j, block)] the terms block row i adds, in order -- a plain sweep's
    rows as stored; scatter[j] = [(i, block)] the same terms listed by the block row they read, which is what a transposed sweep's
    source rows store; gather is then the engine's transposed listing of scatter (sources in sweep order, ties in stored order).
    The blocks of the last block row are NOT zero where they reach beyond n: kernel and model must agree on any values there.
    desc: the sweep runs from the last block row to the first (the pattern mirrored)."""
    rng = np.random.default_rng(seed)
    rows = ssor_cases.pattern(levels, seed, duplicates=duplicates)
    nr = len(rows)
    n = nr * bn - pad
    mirror = (lambda i: nr - 1 - i) if desc else (lambda i: i)
    order = list(range(nr - 1, -1, -1)) if desc else list(range(nr))
    # scatter lists first (targets in a shuffled order), the gather listing derived from them in sweep order
    scatter = [[] for _ in range(nr)]
    for i, cols in enumerate(rows):
        scale = max(1, len(cols))
        vals = block_values(rng, bn, len(cols), special) / scale
        for q, c in enumerate(cols.tolist()):
            scatter[mirror(c)].append((mirror(i), vals[q * bn * bn:(q + 1) * bn * bn].copy()))
    for j in range(nr):
        scatter[j] = [scatter[j][p] for p in rng.permutation(len(scatter[j]))]
    gather = [[] for _ in range(nr)]
    for j in order:
        for i, blk in scatter[j]:
            gather[i].append((j, blk))
    if special:                                            # ... and for certain inside a long row, whose products pass through LDS
        for row in [r for r in gather if len(r) >= LONG_ROW][:2]:
            row[5][1][1 % (bn * bn)] = np.inf
            row[9][1][(bn * bn) - 1] = -np.inf
    wd = rng.uniform(-0.5, 0.5, nr * bn * bn)
    for i in range(nr):
        for r in range(bn):
            wd[i * bn * bn + r * (bn + 1)] += 1.5 if (i + r) % 2 else -1.5
    if special:
        wd[rng.random(len(wd)) < 0.02] = -0.0
    return dict(n=n, nr=nr, bn=bn, gather=gather, scatter=scatter, wd=wd, order=order, desc=desc)


def layout(case, groups=None):
    """the level-ordered layout of case["gather"] by the rules of include/liship.h, as host arrays: dict(nlev, lptr, llong, rows, rptr,
    col, val, groups, nrows, nshort, sizes, nlong); groups None: the engine's own grouping"""
    gather, nr, bn = case["gather"], case["nr"], case["bn"]
    terms = [[(j, 0.0) for j, _ in row] for row in gather]
    lev = ssor_cases.levels_of(terms, 1 if case["desc"] else 0)
    nlev = max(lev) + 1 if nr else 0
    short = [[] for _ in range(nlev)]
    long_ = [[] for _ in range(nlev)]
    for i in range(nr):
        (long_ if len(gather[i]) >= LONG_ROW else short)[lev[i]].append(i)
    rows, lptr, llong = [], [0], []
    for l in range(nlev):
        rows += short[l]
        llong.append(len(rows))
        rows += long_[l]
        lptr.append(len(rows))
    llong.append(len(rows))
    rptr, col, val = [0], [], []
    for i in rows:
        for j, blk in gather[i]:
            col.append(j)
            val.append(blk)
        rptr.append(len(col))
    sizes = [len(short[l]) + len(long_[l]) for l in range(nlev)]
    if groups is None:
        groups = ssor_cases.grouping(sizes)
    return dict(nlev=nlev, lptr=np.array(lptr, np.int32), llong=np.array(llong, np.int32), rows=np.array(rows, np.int32), rptr=np.array(rptr, np.int32),
                col=np.array(col, np.int32), val=(np.concatenate(val) if val else np.zeros(0)), groups=[tuple(g) for g in groups],
                nrows=np.array(sizes + [0], np.int32), nshort=np.array([len(s) for s in short] + [0], np.int32), sizes=sizes, nlong=[len(x) for x in long_])


def valid_groupings(sizes):
    """every way to cut the levels into launches: a launch is one level on its own, or a run of consecutive levels of at most
    SMALL_LEVEL rows each (a run of one such level included)"""
    out = []

    def rec(l, acc):
        if l == len(sizes):
            out.append(list(acc))
            return
        rec(l + 1, acc + [(l, l + 1, 0)])
        e = l
        while e < len(sizes) and sizes[e] <= SMALL_LEVEL:
            e += 1
            rec(e, acc + [(l, e, 1)])
    rec(0, [])
    return out


def census(lay):
    """what lis_amd_ssor_sweep_info would report for the layout: [levels, launches, own-launch levels, long rows in those, long rows in runs]"""
    own = [g[0] for g in lay["groups"] if not g[2]]
    return [lay["nlev"], len(lay["groups"]), len(own), sum(lay["nlong"][l] for l in own), sum(lay["nlong"]) - sum(lay["nlong"][l] for l in own)]


def model_sweep(case, mode, transposed, b, x0):
    """(x, work) after one sweep of the model, work in whole blocks (nr*bn doubles, the padding of the last block +0.0: the next sweep's terms
    read it unmasked): mode / transposed as liship_bsweep_f64 takes them; x0: x before the sweep (b for the
    transposed modes, where the sweep runs in place)"""
    n, bn = case["n"], case["bn"]
    with np.errstate(all="ignore"):
        if not transposed:
            x = oracle._Vec(x0, n, bn)
            oracle.sweep_plain(case["gather"], case["order"], case["wd"], n, bn, oracle._Vec(b, n, bn) if b is not None else None, x, mode == 1)
            return x.out(), None
        x, work = oracle._Vec(b, n, bn), oracle._Vec(np.zeros(n), n, bn)
        oracle.sweep_scatter(case["scatter"], case["order"], case["wd"], n, bn, x, mode == 0, work)
        return x.out(), work.v.copy()              # every block of work, +0.0 in the padding of the last one


def kernel_sweep(lib, case, lay, mode, transposed, b, x0, alias=False):
    """(x, work) after liship_bsweep_f64 on the layout; alias: b and x are the same buffer (x0 is then b)"""
    from lis_amd import DeviceArray as DA, check
    n, nr, bn = case["n"], case["nr"], case["bn"]
    keep = [DA.from_host(lay[k], np.int32) for k in ("lptr", "llong", "rows", "rptr")]
    dcol = DA.from_host(lay["col"] if len(lay["col"]) else np.zeros(1, np.int32), np.int32)
    dval = DA.from_host(lay["val"] if len(lay["val"]) else np.zeros(1), np.float64)
    groups = np.array([v for g in lay["groups"] for v in g], np.int32)
    s = SweepT()
    s.nlev, s.nrows, s.nnz, s.ngroups = lay["nlev"], nr, len(lay["col"]), len(lay["groups"])
    s.lptr, s.llong, s.rows, s.rptr = (k.ptr for k in keep)
    s.col, s.val = dcol.ptr, dval.ptr
    s.groups, s.h_nrows, s.h_nshort = groups.ctypes.data, lay["nrows"].ctypes.data, lay["nshort"].ctypes.data
    guard = 3
    dx = DA.from_host(np.concatenate((x0, np.full(guard + bn, 7.0))), np.float64)
    db = dx if alias else (DA.from_host(np.concatenate((b, np.full(guard + bn, 9.0))), np.float64) if b is not None else None)
    dwd = DA.from_host(case["wd"], np.float64)
    dwork = DA.from_host(np.full(nr * bn + guard, 5.0), np.float64)
    fn = lib.dll.liship_bsweep_f64
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(SweepT), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    check(fn(C.byref(s), n, bn, mode, transposed, db.ptr if db is not None else None, dx.ptr, dwd.ptr, dwork.ptr, None))
    x, work = dx.to_host(), dwork.to_host()
    assert np.array_equal(x[n:], np.full(guard + bn, 7.0)), "x was written at or beyond n"
    assert np.array_equal(work[nr * bn:], np.full(guard, 5.0)), "work was written beyond its blocks"
    return x[:n], work[:nr * bn]


def same(got, want):
    """every bit, a NaN matching any NaN (sign and payload are not part of the contract)"""
    return same_bits(got, want, False)
