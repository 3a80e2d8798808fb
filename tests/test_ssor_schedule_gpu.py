"""The sweep kernels of -p ssor (kernels/sptrsv.hip) and the schedule builder (lis_sweep.c) against tests/ssor_oracle.py, bit for bit,
on matrices built to a prescribed level schedule (tests/ssor_cases.py): every level size and row length at which the per-level
kernel, its tail block, its long-row workgroups and the run / own-launch switch change behaviour.

Each case proves that it reached the code it is for: the level rule and the grouping rule, restated in ssor_cases.py, give levels,
launches, own-launch levels and the long rows in them, and lis_amd_last_solve_ssor / lis_amd_ssor_schedule_info /
lis_amd_ssor_sweep_info must report the same for all four sweeps.  The oracle needs no reference library: nothing here skips.

Not asserted: sign and payload of a NaN.  Observed on an MI355X against the oracle on x86-64: NaN in the same places everywhere, but
only 28 of the 60 NaN entries of the special-value case at T = 1 (8 of 12 at T = 3) carried the same sign and payload; the test prints
the counts it sees.  Every other value, signed zeros, denormals and infinities included, is compared in every bit."""
import ctypes as C

import numpy as np
import pytest

import lis_amd
import ssor_cases
import ssor_oracle
from lis_amd import DeviceArray as DA
from ssor_cases import first_difference

pytestmark = pytest.mark.gpu
MUL, SUB, SCAT = 0, 1, 2
ERR_ARG = -1


@pytest.fixture(scope="module")
def lib():
    lib = lis_amd.load()
    assert lis_amd.gpu_available(), "no HIP device: the product path has no CPU fallback"
    assert lib.initialize([]) == 0
    lib.dll.lis_amd_set_residency(0)
    return lib


_oracle = {}


def oracle(name, key, T=1):
    if (name, key, T) not in _oracle:
        s = ssor_cases.special_system() if name == "special" else ssor_cases.system(name)
        _oracle[name, key, T] = ssor_oracle.all_solves(*s[key], ssor_cases.OMEGA, s["b"], T)
    return _oracle[name, key, T]


def reported(lib, A):
    """what the library says about the schedule it built for the last -p ssor solve on A"""
    blk, lf, lb, la = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    assert lib.dll.lis_amd_last_solve_ssor(C.byref(blk), C.byref(lf), C.byref(lb), C.byref(la)) == 1
    info = (C.c_double * 4)()
    assert lib.dll.lis_amd_ssor_schedule_info(A, info) == 0
    sweeps = []
    for w in range(4):
        si = (C.c_int * 6)()
        assert lib.dll.lis_amd_ssor_sweep_info(A, w, si) == 0
        sweeps.append(list(si))
    return {"last": (blk.value, lf.value, lb.value, la.value), "info": (int(info[2]), int(info[3])), "sweeps": sweeps}


def run_case(lib, name, T):
    s = ssor_cases.special_system() if name == "special" else ssor_cases.system(name)
    exact = name != "special"
    seen = {"nan": 0, "nan_same_bits": 0}
    for key in ("A1", "A2"):
        if key not in s:
            continue
        ptr, idx, val = s[key]
        want = oracle(name, key, T)
        assert lib.dll.lis_amd_set_reference_reductions(T if T > 1 else 0) == 0
        try:
            A = ssor_cases.library_matrix(lib, ptr, idx, val, expect_ok=exact)
            # the schedule is the one the restated rules give: the case runs the kernels it is for
            stats = [ssor_cases.sweep_stats(t, d) for t, d in ssor_cases.sweep_terms(ptr, idx, val, T)]
            rep = reported(lib, A)
            assert rep["sweeps"] == [st["info"] for st in stats], (name, key, T)
            launches = stats[0]["info"][1] + stats[1]["info"][1]
            assert rep["last"] == (T, stats[0]["info"][0], stats[1]["info"][0], launches), (name, key, T, rep["last"])
            assert rep["info"] == (launches, stats[0]["info"][0])
            print("SCHEDULE %s %s T=%d " % (name, key, T) + " ".join("%s=%s" % (w, st["info"]) for w, st in zip(("L", "U", "UT", "LT"), stats)))
            assert first_difference(ssor_cases.library_wd(A), want["wd"]) is None, (name, key, "wd")
            for solve, flag in ssor_oracle.SOLVES:
                if T > 1 and flag != ssor_oracle.SSOR:
                    continue                                        # LOWER / UPPER do not depend on T
                if exact:
                    assert np.isfinite(want[solve, flag]).all()
                for alias in (False, True):
                    got = ssor_cases.library_solve(lib, A, solve, flag, s["b"], alias)
                    d = first_difference(got, want[solve, flag], nan_payload=exact)
                    assert d is None, (name, key, T, solve, flag, "aliased" if alias else "separate") + d + where(stats, solve, flag, d[0])
                    if not exact:
                        assert np.array_equal(np.isnan(got), np.isnan(want[solve, flag]))
                        nan = np.isnan(got)
                        seen["nan"] += int(nan.sum())
                        seen["nan_same_bits"] += int((ssor_cases.bits(got)[nan] == ssor_cases.bits(want[solve, flag])[nan]).sum())
            lib.lis_matrix_destroy(A)
        finally:
            lib.dll.lis_amd_set_reference_reductions(0)
    return seen


def where(stats, solve, flag, row):
    """level, length and kernel of a row in the sweeps a solve runs, for the message of a failure"""
    sweeps = {("solve", 0): (0,), ("solve", 1): (1,), ("solve", 2): (0, 1), ("solveh", 0): (2,), ("solveh", 1): (3,), ("solveh", 2): (2, 3)}[solve, flag]
    out = []
    for w in sweeps:
        st = stats[w]
        l = st["lev"][row]
        own = any(g[0] == l and not g[2] for g in st["groups"])
        out.append("sweep %d: level %d of %d rows, %s" % (w, l, st["sizes"][l], "own launch" if own else "run"))
    return tuple(out)


CASES_T = [(name, 1) for name in ssor_cases.CASES] + [("heavy", 1)] + [(name, T) for name, c in ssor_cases.CASES.items() for T in c["T"]]


@pytest.mark.parametrize("name,T", CASES_T)
def test_solves_on_a_prescribed_schedule_are_the_oracle_bit_for_bit(lib, name, T):
    run_case(lib, name, T)


@pytest.mark.parametrize("T", [1, 3])
def test_special_values_go_through_the_sweeps_as_through_the_oracle(lib, T):
    """a zero diagonal entry (WD = +inf), inf, NaN, -0.0 and denormals in b: NaN in the same places, every other entry equal in
    every bit (signed zeros and infinities included)"""
    seen = run_case(lib, "special", T)
    assert seen["nan"] > 0
    print("NAN_BITS T=%d: %d NaN entries compared, %d with the oracle's sign and payload" % (T, seen["nan"], seen["nan_same_bits"]))


# ------------------------------------------------------------------ the kernel's contract, apart from the builder
class Sweep(C.Structure):
    _fields_ = [("nlev", C.c_int), ("nrows", C.c_int), ("nnz", C.c_int), ("ngroups", C.c_int),
                ("lptr", C.c_void_p), ("llong", C.c_void_p), ("rows", C.c_void_p), ("rptr", C.c_void_p), ("col", C.c_void_p), ("val", C.c_void_p),
                ("groups", C.POINTER(C.c_int)), ("h_nrows", C.POINTER(C.c_int)), ("h_nshort", C.POINTER(C.c_int))]


class HandSweep:
    """a liship_sweep_t laid out as include/liship.h documents it: rows by level, inside a level the short rows first"""

    def __init__(self, terms, desc):
        st = ssor_cases.sweep_stats(terms, desc)
        lev, self.sizes = st["lev"], st["sizes"]
        n, nlev = len(terms), len(st["sizes"])
        order = sorted(range(n), key=lambda i: (lev[i], len(terms[i]) >= ssor_cases.LONG_ROW, i))
        lptr = np.concatenate(([0], np.cumsum(self.sizes))).astype(np.int32)
        nshort = np.array([s - g for s, g in zip(st["sizes"], st["nlong"])], np.int32)
        rptr = np.concatenate(([0], np.cumsum([len(terms[i]) for i in order]))).astype(np.int32)
        col = np.array([c for i in order for c, _ in terms[i]], np.int32)
        val = np.array([v for i in order for _, v in terms[i]], np.float64)
        pad = np.zeros(4, np.int32)
        self.dev = [DA.from_host(np.concatenate((a, pad))) for a in (lptr, lptr[:-1] + nshort, np.array(order, np.int32), rptr, col)]
        self.dev.append(DA.from_host(np.concatenate((val, np.zeros(2)))))
        self.h_nrows, self.h_nshort = np.array(self.sizes, np.int32), nshort
        self.base = dict(nlev=nlev, nrows=n, nnz=len(col))
        self.keep = []                                               # host arrays a returned struct points into

    def grouped(self, groups):
        for l0, l1, run in groups:
            assert 0 <= l0 < l1 <= len(self.sizes) and (l1 == l0 + 1 or run)
            assert not run or max(self.sizes[l0:l1]) <= ssor_cases.SMALL_LEVEL
        assert [l for g in groups for l in range(g[0], g[1])] == list(range(len(self.sizes)))
        h_groups = np.array(groups, np.int32).reshape(-1)
        self.keep.append(h_groups)
        host = [a.ctypes.data_as(C.POINTER(C.c_int)) for a in (h_groups, self.h_nrows, self.h_nshort)]
        return Sweep(ngroups=len(groups), lptr=self.dev[0].ptr, llong=self.dev[1].ptr, rows=self.dev[2].ptr, rptr=self.dev[3].ptr,
                     col=self.dev[4].ptr, val=self.dev[5].ptr, groups=host[0], h_nrows=host[1], h_nshort=host[2], **self.base)


def groupings(sizes):
    """the builder's grouping; every level on a launch of its own; every eligible level in a run of its own; eligible levels in runs
    cut at arbitrary points"""
    rng = np.random.default_rng(5)
    own = [(l, l + 1, 0) for l in range(len(sizes))]
    single = [(l, l + 1, int(s <= ssor_cases.SMALL_LEVEL)) for l, s in enumerate(sizes)]
    cut = []
    for l0, l1, run in ssor_cases.grouping(sizes):
        while run and l1 - l0 > 1 and rng.random() < 0.7:
            mid = int(rng.integers(l0 + 1, l1))
            cut.append((l0, mid, 1))
            l0 = mid
        cut.append((l0, l1, run))
    return {"builder": ssor_cases.grouping(sizes), "all own": own, "runs of one level": single, "runs cut": cut}


@pytest.fixture(scope="module")
def sweep_fn(lib):
    fn = lib.dll.liship_sweep_f64
    fn.restype, fn.argtypes = C.c_int, [C.POINTER(Sweep), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return fn


def test_any_valid_grouping_gives_the_same_bits(lib, sweep_fn):
    """include/liship.h: any grouping of levels into runs (levels of at most 1024 rows) and own launches is valid.  The schedule of
    `alternating` (a level of one row, a small level of long rows only, large levels with long rows), MUL / SUB on A1, SCAT + MUL
    on A2, b separate from x and b == x"""
    s = ssor_cases.system("alternating")
    b = s["b"]
    n = len(b)
    hand = {key: [HandSweep(t, d) for t, d in ssor_cases.sweep_terms(*s[key])] for key in ("A1", "A2")}
    w1, w2 = oracle("alternating", "A1"), oracle("alternating", "A2")
    wd1, wd2 = DA.from_host(w1["wd"]), DA.from_host(w2["wd"])
    names = list(groupings(hand["A1"][0].sizes))
    assert len(groupings(hand["A1"][0].sizes)["runs cut"]) > len(groupings(hand["A1"][0].sizes)["builder"])
    for g in names:
        sw = {key: [h.grouped(groupings(h.sizes)[g]) for h in hand[key]] for key in ("A1", "A2")}
        for alias in (False, True):
            # MUL: forward on L of A1 = lis_matrix_solve LOWER
            db = DA.from_host(b)
            dx = db if alias else DA.from_host(np.full(n, 7.0))
            assert sweep_fn(C.byref(sw["A1"][0]), MUL, db.ptr, dx.ptr, wd1.ptr, None) == 0
            assert first_difference(dx.to_host(), w1["solve", 0]) is None, (g, alias, "MUL")
            # SUB: backward on U of A1 after it = lis_matrix_solve SSOR (b is not read)
            assert sweep_fn(C.byref(sw["A1"][1]), SUB, None, dx.ptr, wd1.ptr, None) == 0
            assert first_difference(dx.to_host(), w1["solve", 2]) is None, (g, alias, "SUB")
            # SCAT forward on U^T of A2, then MUL backward on L^T in place = lis_matrix_solveh SSOR
            db = DA.from_host(b)
            dx = db if alias else DA.from_host(np.full(n, 7.0))
            assert sweep_fn(C.byref(sw["A2"][2]), SCAT, db.ptr, dx.ptr, wd2.ptr, None) == 0
            assert sweep_fn(C.byref(sw["A2"][3]), MUL, dx.ptr, dx.ptr, wd2.ptr, None) == 0
            assert first_difference(dx.to_host(), w2["solveh", 2]) is None, (g, alias, "SCAT + MUL")
            # MUL backward on U of A1 = lis_matrix_solve UPPER; forward on U^T of A2 = lis_matrix_solveh LOWER
            for key, w, want in (("A1", 1, w1["solve", 1]), ("A2", 2, w2["solveh", 0])):
                db = DA.from_host(b)
                dx = db if alias else DA.from_host(np.full(n, 7.0))
                assert sweep_fn(C.byref(sw[key][w]), MUL, db.ptr, dx.ptr, (wd1 if key == "A1" else wd2).ptr, None) == 0
                assert first_difference(dx.to_host(), want) is None, (g, alias, key, w)


def test_sweep_refuses_what_it_cannot_serve(lib, sweep_fn):
    terms, desc = ssor_cases.sweep_terms(*ssor_cases.system("n1")["A1"])[0]
    h = HandSweep(terms, desc)
    sw = h.grouped(ssor_cases.grouping(h.sizes))
    b, x, wd = DA.from_host(np.array([2.0])), DA.from_host(np.array([7.0])), DA.from_host(np.array([0.5]))
    for mode in (MUL, SUB, SCAT):
        assert sweep_fn(None, mode, b.ptr, x.ptr, wd.ptr, None) == ERR_ARG
        assert sweep_fn(C.byref(sw), mode, b.ptr, None, wd.ptr, None) == ERR_ARG
        assert sweep_fn(C.byref(sw), mode, b.ptr, x.ptr, None, None) == ERR_ARG
    for mode in (-1, 3, 1 << 20):
        assert sweep_fn(C.byref(sw), mode, b.ptr, x.ptr, wd.ptr, None) == ERR_ARG
    assert sweep_fn(C.byref(sw), MUL, None, x.ptr, wd.ptr, None) == ERR_ARG
    assert sweep_fn(C.byref(sw), SCAT, None, x.ptr, wd.ptr, None) == ERR_ARG
    assert x.to_host()[0] == 7.0                                     # a refused call wrote nothing
    assert sweep_fn(C.byref(sw), SUB, None, x.ptr, wd.ptr, None) == 0   # SUB reads no b
    assert x.to_host()[0] == 7.0                                     # 7 - (0.0 * 0.5)
    assert sweep_fn(C.byref(sw), MUL, b.ptr, x.ptr, wd.ptr, None) == 0
    assert x.to_host()[0] == 1.0
