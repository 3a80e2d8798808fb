"""What tests/test_reduction_tree_gpu.py runs and tests/test_reduction_model_cpu.py vouches for: every reduction entry point of
include/liship.h with the roles of its arrays, the data of every case, and the model's expectation (tests/reduction_model.py).

Roles are those of the kernel's argument block: x, y, w, d, e are the arrays an op reads; the fused forms store ox / oy in place over
one of them (`stores`).  Data is uniform(-1, 1) * 10**integers(-8, 8): sixteen decades, so that another order of the same terms
moves bits.  case_data() picks, per entry and size, the first seed at which the vector-path and the scalar-path layouts of level 1
give different bits in every result (n >= 3): the alignment cases prove something only then, and the CPU test asserts it."""
import numpy as np

import reduction_model as rm

SIZES = [0, 1, 2, 3, 255, 256, 257, 511, 513, 2047, 2048, 2049, 2050, 4095, 4097, 6145, 65537]
ALIGN_SIZES = [3, 2049, 4097]
SPECIAL_N = 6145                  # 3072 pairs: blocks 0..2 are full, pair 3071 is the last lane's (255) last pair (u = 3) of block 2, element 6144 the odd tail
A, SP, CB, CC, DC = 0.8414709848078965, -0.3826834323650898, 1.3, -0.61, 0.2510000000000001     # a | *pa, *hprev, *palpha, *pomega, the uniform 1/diag
SCALARS = np.array([A, SP, CB, CC])       # the block of device scalars: s["pa"], s["psp"], s["pcb"], s["pcc"] point at these


class Entry:
    def __init__(self, name, op, roles, call, stores=None, root=False):
        self.name, self.op, self.roles, self.call, self.stores, self.root = name, op, roles, call, stores or {}, root
        self.nres = 2 if op in rm.TWO_RESULTS else 1

    def __repr__(self):
        return self.name


# call(L, n, p, s, r, w): L the library, p[role] device pointers, s the scalars (by value: a, c; in HBM: pa, psp, pcb, pcc), r result, w work
ENTRIES = [
    Entry("dot", rm.RED_DOT, "xy", lambda L, n, p, s, r, w: L.liship_dot_f64(n, p["x"], p["y"], r, w, None)),
    Entry("nrm2", rm.RED_SUMSQ, "x", lambda L, n, p, s, r, w: L.liship_nrm2_f64(n, p["x"], r, w, None), root=True),
    Entry("sumsq", rm.RED_SUMSQ, "x", lambda L, n, p, s, r, w: L.liship_sumsq_f64(n, p["x"], r, w, None)),
    Entry("nrm1", rm.RED_ABS, "x", lambda L, n, p, s, r, w: L.liship_nrm1_f64(n, p["x"], r, w, None)),
    Entry("sum", rm.RED_SUM, "x", lambda L, n, p, s, r, w: L.liship_sum_f64(n, p["x"], r, w, None)),
    Entry("dot2", rm.RED_DOT2, "xy", lambda L, n, p, s, r, w: L.liship_dot2_f64(n, p["x"], p["y"], r, w, None)),
    Entry("count_ne", rm.RED_COUNT_NE, "x", lambda L, n, p, s, r, w: L.liship_count_ne_f64(n, p["x"], s["a"], r, w, None)),
    Entry("cg_update", rm.RED_CG_UPDATE, "xywd",
          lambda L, n, p, s, r, w: L.liship_cg_update_f64(n, s["a"], p["x"], p["y"], p["w"], p["d"], r, w, None), {"ox": "w", "oy": "d"}),
    Entry("cg_update_jacobi", rm.RED_CG_UPDATE_JAC, "xywde",
          lambda L, n, p, s, r, w: L.liship_cg_update_jacobi_f64(n, s["a"], p["x"], p["y"], p["e"], p["w"], p["d"], r, w, None), {"ox": "w", "oy": "d"}),
    Entry("axpy_sumsq", rm.RED_AXPY_NRM2, "xy", lambda L, n, p, s, r, w: L.liship_axpy_sumsq_f64(n, s["a"], p["x"], p["y"], r, w, None), {"oy": "y"}),
    Entry("axpy_sumsq_dot", rm.RED_AXPY_NRM2_DOT, "xyw",
          lambda L, n, p, s, r, w: L.liship_axpy_sumsq_dot_f64(n, s["a"], p["x"], p["y"], p["w"], r, w, None), {"oy": "y"}),
    Entry("mgs_step_vnext", rm.RED_AXPYD_DOT, "xyw",
          lambda L, n, p, s, r, w: L.liship_mgs_step_f64(n, s["psp"], p["x"], p["y"], p["w"], r, w, None), {"oy": "y"}),
    Entry("mgs_step_null", rm.RED_AXPYD_SUMSQ, "xy",
          lambda L, n, p, s, r, w: L.liship_mgs_step_f64(n, s["psp"], p["x"], p["y"], None, r, w, None), {"oy": "y"}),
    Entry("cg_update_dev", rm.RED_CG_UPDATE, "xywd",
          lambda L, n, p, s, r, w: L.liship_cg_update_dev_f64(n, s["pa"], p["x"], p["y"], None, p["w"], p["d"], r, w, None), {"ox": "w", "oy": "d"}),
    Entry("cg_update_dev_dinv", rm.RED_CG_UPDATE_JAC, "xywde",
          lambda L, n, p, s, r, w: L.liship_cg_update_dev_f64(n, s["pa"], p["x"], p["y"], p["e"], p["w"], p["d"], r, w, None), {"ox": "w", "oy": "d"}),
    Entry("cg_residual_jacobi_dev", rm.RED_AXPY_NRM2_JAC, "xye",
          lambda L, n, p, s, r, w: L.liship_cg_residual_jacobi_dev_f64(n, s["pa"], p["x"], p["e"], p["y"], r, w, None), {"oy": "y"}),
    Entry("cg_residual_jacobi_uniform_dev", rm.RED_AXPY_NRM2_JACU, "xy",
          lambda L, n, p, s, r, w: L.liship_cg_residual_jacobi_uniform_dev_f64(n, s["pa"], p["x"], s["c"], p["y"], r, w, None), {"oy": "y"}),
    Entry("bicgstab_end_dev", rm.RED_BICGSTAB_END, "xywde",
          lambda L, n, p, s, r, w: L.liship_bicgstab_end_dev_f64(n, s["pcb"], s["pcc"], s["pa"], p["d"], p["x"], p["w"], p["e"], p["y"], r, w, None),
          {"ox": "e", "oy": "y"}),
    Entry("axpy_sumsq_dev", rm.RED_AXPY_NRM2, "xy", lambda L, n, p, s, r, w: L.liship_axpy_sumsq_dev_f64(n, s["pa"], p["x"], p["y"], r, w, None), {"oy": "y"}),
    Entry("axpy_sumsq_dot_dev", rm.RED_AXPY_NRM2_DOT, "xyw",
          lambda L, n, p, s, r, w: L.liship_axpy_sumsq_dot_dev_f64(n, s["pa"], p["x"], p["y"], p["w"], r, w, None), {"oy": "y"}),
]
BY_NAME = {e.name: e for e in ENTRIES}
SPECIAL_ENTRIES = ["dot", "nrm2", "sumsq", "nrm1", "sum", "dot2", "axpy_sumsq_dot"]      # the plain sums and one fused form
SPECIAL_KINDS = ["neg_zero", "one_inf", "inf_minus_inf", "nan_in_tail", "nan_in_last_lane", "subnormal_inputs", "subnormal_products"]


def wide(rng, n):
    return rng.uniform(-1.0, 1.0, n) * 10.0 ** rng.integers(-8, 8, n)


def expected(entry, data, vector=True):
    """-> (result[0 .. nres), {role: array the entry leaves there}) by the model"""
    v0, v1, ox, oy = rm.red_term(entry.op, a=A, sp=SP, cb=CB, cc=CC, c=DC, **data)
    res = [rm.tree(v, vector) for v in (v0, v1)[:entry.nres]]
    if entry.root:
        res[0] = rm.root(res[0])
    stored = {role: np.array(arr) for role, arr in data.items()}
    for out, val in (("ox", ox), ("oy", oy)):
        if out in entry.stores:
            stored[entry.stores[out]] = val
    return np.array(res, dtype=np.float64), stored


def _draw(entry, n, seed):
    rng = np.random.default_rng([ENTRIES.index(entry), n, seed])
    data = {role: wide(rng, n) for role in entry.roles}
    if entry.op == rm.RED_COUNT_NE:            # about a quarter of the elements ARE the value; the zero of the other sign and a neighbour are not
        data["x"] = rng.choice(np.array([A, -A, 0.0, -0.0, np.nextafter(A, 1.0)]), n) if n else data["x"]
        data["x"] = np.where(rng.integers(0, 4, n) == 0, A, data["x"])
    return data


def layouts_differ(entry, data):
    a, b = expected(entry, data, True)[0], expected(entry, data, False)[0]
    return bool(np.all(a.view(np.uint64) != b.view(np.uint64)))


def case_data(entry, n):
    """the data of (entry, n).  count_ne adds ones: exact in any order, no layout can show in its bits"""
    for seed in range(200):
        data = _draw(entry, n, seed)
        if n < 3 or entry.op == rm.RED_COUNT_NE or layouts_differ(entry, data):
            return data
    raise AssertionError("no seed separates the layouts for %s at n = %d" % (entry.name, n))


def special_data(entry, kind, n=SPECIAL_N):
    """wide-range data with the special values where they test something: in x, which every term of these entries contains"""
    rng = np.random.default_rng([ENTRIES.index(entry), n, SPECIAL_KINDS.index(kind)])
    data = {role: wide(rng, n) for role in entry.roles}
    x = data["x"]
    last_lane = 2 * ((n >> 1) - 1) + 1              # second element of the last pair: lane 255, u = 3 of the last block that has pairs
    if kind == "neg_zero":                          # terms -0.0 (+0.0 where a term is a square): every sum is +0.0
        x[:] = -0.0
        if "y" in data:
            data["y"] = -0.0 * np.ones(n) if entry.stores else np.abs(data["y"])
        if "w" in data:
            data["w"] = np.abs(data["w"])
    elif kind == "one_inf":
        x[n // 3] = np.inf
    elif kind == "inf_minus_inf":
        x[n // 3], x[n // 3 + 1500] = np.inf, -np.inf
        for role in data:                           # (the terms x*y and w*(y + a*x) keep the two signs)
            if role != "x":
                data[role][[n // 3, n // 3 + 1500]] = 1.0
    elif kind == "nan_in_tail":
        x[n - 1] = np.nan
    elif kind == "nan_in_last_lane":
        x[last_lane] = np.nan
    elif kind == "subnormal_inputs":
        x *= 1e-310 / 1e8
        x[x == 0.0] = 5e-324
    elif kind == "subnormal_products":              # |x|, |y| around 1e-155: x*x and x*y are subnormal or underflow
        for role in data:
            data[role] = rng.uniform(-1.0, 1.0, n) * 10.0 ** rng.integers(-157, -153, n)
    else:
        raise ValueError(kind)
    return data


# ------------------------------------------------------------------------------------------------------------ chunked A^T x
CHUNK_T = [1, 2, 3, 8, 64]
CHUNK_NSRC = [1, 5, 13, 100, 257]


def chunked_case(nsrc, T, extra_rows=3):
    """a transposed CSR made directly (entries of a row in ascending source row, as liship_csr_transpose_f64 leaves them) with
    rows = nsrc + extra_rows != nsrc, and x.  Row 1 and the last row are empty; the entries of row 2 all lie in the chunk of the
    last source row; row 3 holds products that are -0.0 (a -0.0 value, and a negative value times x = +0.0) and nothing else; row 4
    holds every source row."""
    rng = np.random.default_rng([nsrc, T])
    rows = nsrc + extra_rows
    x = wide(rng, nsrc)
    zero_at = rng.integers(0, nsrc)
    x[zero_at] = 0.0
    last_is, _ = rm.get_isie(rm.chunk_of(nsrc - 1, T, nsrc), T, nsrc)
    tptr, tidx, tval = [0], [], []
    for c in range(rows):
        if c == 1 or c == rows - 1:
            src = np.zeros(0, dtype=np.int64)
        elif c == 2:
            src = np.arange(last_is, nsrc)
        elif c == 3:
            src = np.unique(np.array([zero_at, nsrc - 1 - zero_at if nsrc > 1 else zero_at]))
        elif c == 4:
            src = np.arange(nsrc)
        else:
            src = np.nonzero(rng.uniform(size=nsrc) < 0.5)[0]
        val = wide(rng, len(src))
        if c == 3:
            val = np.where(src == zero_at, -np.abs(val), -0.0)
        tidx.extend(src.tolist())
        tval.extend(val.tolist())
        tptr.append(len(tidx))
    return rows, np.array(tptr, np.int32), np.array(tidx, np.int32), np.array(tval, np.float64), x


def matvech_matrices():
    """the square CSR matrices on which the chunked model is held to the reference's lis_matvech: name -> (ptr, idx, val)"""
    out = {}
    for name, n, dead in (("rand_13", 13, ()), ("rand_5", 5, ()), ("rand_100", 100, ()), ("empty_columns_40", 40, (0, 7, 8, 39))):
        rng = np.random.default_rng([n, len(dead)])
        ptr, idx, val = [0], [], []
        for i in range(n):
            cols = rng.permutation(n)[:rng.integers(0, min(n, 9) + 1)]        # unsorted within the row, some rows empty
            cols = cols[~np.isin(cols, dead)]
            idx.extend(cols.tolist())
            val.extend(wide(rng, len(cols)).tolist())
            ptr.append(len(idx))
        out[name] = (np.array(ptr, np.int32), np.array(idx, np.int32), np.array(val, np.float64))
    return out
