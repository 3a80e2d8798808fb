"""tests/reduction_model.py (the fixed reduction tree and the chunked A^T x, restated in numpy) held to what it models without a GPU:
the bits an MI355X recorded in tests/golden/reduction_bits.json, math.fsum, and the reference's lis_matvech at 1, 2, 3 and 8 OpenMP
threads; and the property of the test data that tests/test_reduction_tree_gpu.py leans on: the two level-1 layouts give different bits."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import orc
import reduction_cases as rc
import reduction_model as rm

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_SIZES = [1, 2, 63, 64, 65, 255, 1000, 2049, 4096, 65536, 65537, (1 << 20) + 3, 5_000_001]     # tests/golden/make_golden_reduction_bits.py


def bits(v):
    return [format(int(b), "016x") for b in np.atleast_1d(np.asarray(v, dtype=np.float64)).view(np.uint64)]


def test_model_gives_the_bits_the_hardware_recorded():
    """the anchor: dot, sumsq, dot2 at the 13 recorded sizes, inputs seeded as the recording script seeds them (aligned arrays)"""
    want = json.load(open(os.path.join(HERE, "golden", "reduction_bits.json")))
    bad, seen = [], 0
    for n in GOLDEN_SIZES:
        rng = np.random.default_rng(n)
        x, y = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
        got = {f"dot/{n}": bits(rm.tree(x * y)), f"sumsq/{n}": bits(rm.tree(x * x)), f"dot2/{n}": bits([rm.tree(x * y), rm.tree(x * x)])}
        for key, b in got.items():
            seen += len(b)
            if b != want[key]:
                bad.append((key, b, want[key]))
    assert seen == 52 and len(GOLDEN_SIZES) * 3 == 39           # 39 results, dot2's holding two sums each
    assert bad == []


def test_pieces_on_hand_computed_cases():
    lanes = np.arange(64, dtype=np.float64)
    assert rm.wave_sum(lanes) == 2016.0 and rm.block_sum(np.ones(256)) == 256.0
    assert [rm.grid_for(n) for n in (0, 1, 2048, 2049, 4097, 33554432, 33554435)] == [1, 1, 1, 2, 3, 16384, 16385]
    assert [rm.get_isie(k, 3, 8) for k in range(3)] == [(0, 3), (3, 6), (6, 8)] and [rm.get_isie(k, 8, 5)[1] - rm.get_isie(k, 8, 5)[0] for k in range(8)] == [1] * 5 + [0] * 3
    big, tiny = 2.0 ** 60, 1.0
    t = np.array([big, tiny, -big])                 # n = 3: the vector path adds (t0 + t1) + t2 in lane 0, the scalar path (t0 + t2) + t1 by the butterfly
    assert rm.tree(t, True) == 0.0 and rm.tree(t, False) == 1.0
    assert rm.fold(np.array([3.5])) == 3.5 and np.signbit(rm.fold(np.array([-0.0])))          # one partial is copied, sign included
    assert not np.signbit(rm.tree(np.full(5, -0.0))) and rm.tree(np.zeros(0)) == 0.0
    assert rm.root(rm.tree(np.array([3.0 * 3.0, 4.0 * 4.0]))) == 5.0


@pytest.mark.parametrize("entry", rc.ENTRIES, ids=repr)
def test_model_terms_are_the_ops(entry):
    """the term definitions: each result within the tree bound of the exactly rounded sum (math.fsum) of terms formed in plain Python
    from the op's definition in liship.h, on the wide-range data; the stored vectors equal to those expressions"""
    n = 4097
    data = rc.case_data(entry, n)
    x, y, w, d, e = (data.get(r) for r in "xywde")
    a, h, al, om, dc = rc.A, rc.SP, rc.CB, rc.CC, rc.DC
    name = entry.name
    stores = {}
    if name == "dot":
        sums = [[x[i] * y[i] for i in range(n)]]
    elif name in ("nrm2", "sumsq"):
        sums = [[x[i] * x[i] for i in range(n)]]
    elif name == "nrm1":
        sums = [[abs(x[i]) for i in range(n)]]
    elif name == "sum":
        sums = [list(x)]
    elif name == "dot2":
        sums = [[x[i] * y[i] for i in range(n)], [x[i] * x[i] for i in range(n)]]
    elif name == "count_ne":
        sums = [[float(x[i].tobytes() != np.float64(a).tobytes()) for i in range(n)]]
    elif name.startswith("cg_update"):              # x += alpha*p ; r -= alpha*q ; {sum r^2, sum r*(r*dinv)}
        xi = [w[i] + a * x[i] for i in range(n)]
        r = [d[i] - a * y[i] for i in range(n)]
        sums = [[v * v for v in r]] + ([[r[i] * (r[i] * e[i]) for i in range(n)]] if e is not None else [])
        stores = {"w": xi, "d": r}
    elif name.startswith("mgs_step"):               # w -= h*vprev ; <w, vnext> or sum w^2
        wv = [y[i] - h * x[i] for i in range(n)]
        sums = [[wv[i] * w[i] for i in range(n)]] if w is not None else [[v * v for v in wv]]
        stores = {"y": wv}
    elif name == "bicgstab_end_dev":                # x += alpha*phat + omega*s ; r = s + (-omega)*t ; {sum r^2, sum rtld*r}
        xi = [(e[i] + al * d[i]) + om * y[i] for i in range(n)]
        r = [y[i] + a * x[i] for i in range(n)]
        sums = [[v * v for v in r], [w[i] * r[i] for i in range(n)]]
        stores = {"e": xi, "y": r}
    else:                                           # y += a*x ; {sum y^2 [, sum v*y | sum y*(y*dinv) | sum y*(y*dc)]}
        yy = [y[i] + a * x[i] for i in range(n)]
        sums = [[v * v for v in yy]]
        if name.startswith("axpy_sumsq_dot"):
            sums.append([w[i] * yy[i] for i in range(n)])
        if name == "cg_residual_jacobi_dev":
            sums.append([yy[i] * (yy[i] * e[i]) for i in range(n)])
        if name == "cg_residual_jacobi_uniform_dev":
            sums.append([yy[i] * (yy[i] * dc) for i in range(n)])
        stores = {"y": yy}
    assert len(sums) == entry.nres
    for vector in (True, False):
        res, stored = rc.expected(entry, data, vector)
        for k, terms in enumerate(sums):
            exact = math.fsum(terms)
            exact = math.sqrt(exact) if entry.root else exact
            scale = math.fsum(abs(t) for t in terms)
            scale = math.sqrt(scale) if entry.root else scale
            assert abs(res[k] - exact) <= 1e-14 * math.log2(n + 1) * scale, (k, vector)
        assert set(entry.stores.values()) == set(stores)
        for role in entry.roles:
            assert np.array_equal(stored[role].view(np.uint64), np.array(stores.get(role, data[role])).view(np.uint64)), role


def test_layouts_differ_on_the_test_data():
    """at every size >= 3 the GPU test runs, for every entry, each result has other bits under the scalar-path layout than under
    the vector-path layout: a kernel that took the wrong path, or a model that ignored the path, cannot pass the alignment cases.
    (count_ne sums ones, exact in any order: its alignment cases check the count and the stores only.)"""
    for entry in rc.ENTRIES:
        for n in rc.SIZES:
            data = rc.case_data(entry, n)
            same = rc.expected(entry, data, True)[0].view(np.uint64) == rc.expected(entry, data, False)[0].view(np.uint64)
            if n >= 3 and entry.op != rm.RED_COUNT_NE:
                assert not same.any(), (entry, n)
            if n < 3 or entry.op == rm.RED_COUNT_NE:
                assert same.all(), (entry, n)       # (one or two terms: one order only)
    assert set(rc.ALIGN_SIZES) <= set(rc.SIZES) and min(rc.ALIGN_SIZES) >= 3


def test_count_ne_data_holds_every_kind_of_element():
    x = rc.case_data(rc.BY_NAME["count_ne"], 4097)["x"]
    v0 = rm.red_term(rm.RED_COUNT_NE, x, a=rc.A)[0]
    for value, differs in ((rc.A, 0.0), (-rc.A, 1.0), (0.0, 1.0), (-0.0, 1.0), (np.nextafter(rc.A, 1.0), 1.0)):
        at = x.view(np.uint64) == np.float64(value).view(np.uint64)
        assert at.any() and (v0[at] == differs).all()


@pytest.mark.parametrize("kind", rc.SPECIAL_KINDS)
def test_special_value_cases_are_what_they_say(kind):
    with np.errstate(all="ignore"):
        for name in rc.SPECIAL_ENTRIES:
            entry = rc.BY_NAME[name]
            data = rc.special_data(entry, kind)
            res, stored = rc.expected(entry, data)
            v0, v1, _, _ = rm.red_term(entry.op, a=rc.A, **data)
            if kind == "neg_zero":
                assert (res.view(np.uint64) == 0).all(), name           # +0.0
                terms = v1 if name == "axpy_sumsq_dot" else v0
                if name not in ("nrm2", "sumsq", "nrm1"):
                    assert np.signbit(terms).all() and (terms == 0.0).all(), name
            if kind == "one_inf":
                assert np.isinf(res).all(), name
            if kind == "inf_minus_inf":                 # (a sum of squares sees +inf twice)
                assert np.isnan(res[-1 if name in ("axpy_sumsq_dot",) else 0]) == (name in ("sum", "dot", "dot2", "axpy_sumsq_dot")), name
                assert np.isnan(res).any() or np.isinf(res).all(), name
            if kind in ("nan_in_tail", "nan_in_last_lane"):
                assert np.isnan(res).all(), name
                at = np.nonzero(np.isnan(v0))[0].tolist()
                assert at == ([rc.SPECIAL_N - 1] if kind == "nan_in_tail" else [rc.SPECIAL_N - 2]), name
            if kind == "subnormal_inputs" and name in ("sum", "nrm1"):
                tiny = np.abs(v0)
                assert (tiny < 2.3e-308).all() and (tiny > 0).all() and 0 < abs(res[0]) < 2.3e-308, name
            if kind == "subnormal_products" and name in ("dot", "sumsq"):
                tiny = np.abs(v0)
                assert ((tiny < 2.3e-308) & (tiny > 0)).sum() > rc.SPECIAL_N // 2 and res[0] != 0.0, name
    assert rc.SPECIAL_N & 1 and rm.grid_for(rc.SPECIAL_N) == 4 and (rc.SPECIAL_N >> 1) % 1024 == 0


def test_fold_levels():
    """the fold's three forms meet at their thresholds on wide-range partials, and each stays within the tree bound of fsum"""
    rng = np.random.default_rng(5)
    p = rc.wide(rng, 18433)
    for count in (2, 1023, 1024, 1025, 16384, 16385, 18432, 18433):
        got = rm.fold(p[:count])
        scale = math.fsum(abs(v) for v in p[:count])
        assert abs(got - math.fsum(p[:count])) <= 1e-14 * math.log2(count + 1) * scale
    lanes = np.zeros(1024)
    for r in range(16):
        lanes = lanes + p[:16384].reshape(16, 1024)[r]
    assert rm.fold(p[:16384]) == rm.block_sum(lanes)
    two = rm.level1_scalar(p[:16385])
    assert len(two) == 9 and rm.fold(p[:16385]) == rm.fold(two)


# ------------------------------------------------------------------------------------------------------------ chunked A^T x
def test_chunked_cases_are_what_they_say():
    for nsrc in rc.CHUNK_NSRC:
        for T in rc.CHUNK_T:
            rows, tptr, tidx, tval, x = rc.chunked_case(nsrc, T)
            assert rows != nsrc and len(tptr) == rows + 1 and tptr[1] == tptr[2] and tptr[-1] == tptr[-2] and len(x) == nsrc
            for c in range(rows):
                seg = tidx[tptr[c]:tptr[c + 1]]
                assert (np.diff(seg) > 0).all() and ((0 <= seg) & (seg < nsrc)).all()
            last = rm.chunk_of(nsrc - 1, T, nsrc)
            if rows > 3:
                seg = tidx[tptr[2]:tptr[3]]
                assert len(seg) and all(rm.chunk_of(j, T, nsrc) == last for j in seg)
            if rows > 4:
                prod = tval[tptr[3]:tptr[4]] * x[tidx[tptr[3]:tptr[4]]]
                assert len(prod) and (prod == 0.0).all() and np.signbit(prod).any()
            y = rm.spmv_transposed_chunked(rows, nsrc, T, tptr, tidx, tval, x)
            one = rm.spmv_transposed_chunked(rows, nsrc, 1, tptr, tidx, tval, x)
            if nsrc >= 13 and 1 < T < nsrc:                      # (T >= nsrc: one entry per chunk, the plain left-to-right sum again)
                assert not np.array_equal(y, one), (nsrc, T)          # the chunks show in the bits
            assert np.allclose(y, one, rtol=1e-9, atol=1e-300 + 1e-12 * np.abs(tval).max() * np.abs(x).max())


def model_against_matvech(ref, T):
    import lisdrv
    bad = []
    for name, (ptr, idx, val) in rc.matvech_matrices().items():
        n = len(ptr) - 1
        x = rc.wide(np.random.default_rng(n), n)
        A = lisdrv.make_csr(ref, ptr, idx, val)
        want = lisdrv.matvech(ref, A, x)
        ref.lis_matrix_destroy(A)
        tptr, tidx, tval = rm.transpose_csr(n, n, ptr, idx, val)
        got = rm.spmv_transposed_chunked(n, n, T, tptr, tidx, tval, x)
        if not np.array_equal(got.view(np.uint64), want.view(np.uint64)):
            bad.append(name)
    return bad


def child(T):
    import lisdrv
    ref = lisdrv.open_lib(orc.REF_SO, threads=T)
    print("RESULT " + json.dumps(model_against_matvech(ref, T)), flush=True)


def test_matvech_matrices_are_what_they_say():
    M = rc.matvech_matrices()
    assert [len(M[k][0]) - 1 for k in ("rand_13", "rand_5", "rand_100")] == [13, 5, 100]
    assert 13 // 8 == 1 and 5 < 8
    ptr, idx, val = M["empty_columns_40"]
    assert not np.isin([0, 7, 8, 39], idx).any() and len(idx) > 40
    for ptr, idx, val in M.values():
        n = len(ptr) - 1
        dense = np.zeros((n, n))
        for i in range(n):
            dense[i, idx[ptr[i]:ptr[i + 1]]] = val[ptr[i]:ptr[i + 1]]
        assert not np.array_equal(dense, dense.T)


@pytest.mark.skipif(not os.path.exists(orc.REF_SO), reason="oracle/_ref not built")
@pytest.mark.parametrize("T", [1, 2, 3, 8])
def test_chunked_model_is_the_reference_matvech(T):
    """in a child process: the reference reads its thread count once, at initialize"""
    res = subprocess.run([sys.executable, "-c", "import sys; sys.path[:0] = %r; import test_reduction_model_cpu as t; t.child(%d)" % ([os.path.dirname(HERE), HERE], T)],
                         capture_output=True, text=True, env=dict(os.environ, OMP_NUM_THREADS=str(T)), timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    assert json.loads([line for line in res.stdout.splitlines() if line.startswith("RESULT ")][-1][7:]) == []
