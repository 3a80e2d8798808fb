"""The fixed reduction tree of kernels/vector_ops.hip and the chunked A^T x of kernels/transpose.hip, restated in numpy float64 from
the kernel source and the contracts of include/liship.h.  Nothing here calls the library.

The kernels are compiled without FMA contraction, so a sum is a fixed expression of its terms: which terms a lane adds and in which
order, how the 64 lanes of a wavefront are combined (a butterfly), how the wavefronts of a workgroup are combined (serially), and how
the workgroups' partial sums are folded.  numpy's element-wise + and * are the same IEEE double operations, one rounding each; every
array statement below performs ONE such operation per lane, so the model's order is the order written here.

A lane that has nothing to add at some step skips the addition on the device; here it adds +0.0.  That is the same in every bit:
every running sum starts from +0.0, and a sum that started from +0.0 is never -0.0 (+0.0 + -0.0 = +0.0), so s + 0.0 = s.

tests/test_reduction_model_cpu.py pins this model to the bits an MI355X produced (tests/golden/reduction_bits.json);
tests/test_reduction_tree_gpu.py holds every reduction entry point to it."""
import functools

import numpy as np


def _quiet(f):
    """inf - inf and overflow are results here, as on the device: no warnings"""
    @functools.wraps(f)
    def g(*args, **kwargs):
        with np.errstate(all="ignore"):
            return f(*args, **kwargs)
    return g


BLOCK = 256                       # lanes of a level-1 / reduce_fold workgroup
WAVE = 64
U = 4                             # 16 B accesses per lane and array
PER_BLOCK = 2 * U * BLOCK         # 2048 elements (1024 pairs) per workgroup
FINAL_LANES = 1024                # reduce_final: one workgroup of 1024 lanes ...
FINAL_MAX = 1 << 14               # ... for up to 2^14 partials per result
NT_ELEMS = 32 << 20               # beyond this many elements the loads are non-temporal (the order is the same)

(RED_DOT, RED_SUMSQ, RED_ABS, RED_SUM, RED_DOT2, RED_CG_UPDATE, RED_CG_UPDATE_JAC, RED_AXPY_NRM2, RED_AXPY_NRM2_DOT, RED_AXPY_NRM2_JAC,
 RED_AXPY_NRM2_JACU, RED_COUNT_NE, RED_BICGSTAB_END, RED_AXPYD_DOT, RED_AXPYD_SUMSQ) = range(15)
TWO_RESULTS = (RED_DOT2, RED_AXPY_NRM2_DOT, RED_CG_UPDATE_JAC, RED_AXPY_NRM2_JAC, RED_AXPY_NRM2_JACU, RED_BICGSTAB_END)


# ---------------------------------------------------------------------------------------------------------------- the tree
@_quiet
def wave_sum(v):
    """v[..., 64] -> [...]: six butterfly steps, partners 32, 16, 8, 4, 2, 1 lanes away; the result is lane 0's"""
    v = np.array(v, dtype=np.float64)
    lane = np.arange(WAVE)
    for k in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ k]
    return v[..., 0]


@_quiet
def block_sum(lanes):
    """lanes[..., 64 * nw] -> [...]: the wavefronts' sums added in wavefront order, from 0.0"""
    lanes = np.asarray(lanes, dtype=np.float64)
    w = wave_sum(lanes.reshape(lanes.shape[:-1] + (lanes.shape[-1] // WAVE, WAVE)))
    t = np.zeros(lanes.shape[:-1])
    for i in range(w.shape[-1]):
        t = t + w[..., i]
    return t


def grid_for(n):
    return max(1, ((n + 1) // 2 + PER_BLOCK // 2 - 1) // (PER_BLOCK // 2))


def _padded(terms, count):
    out = np.zeros(count)
    out[:len(terms)] = terms
    return out


@_quiet
def level1_vector(terms):
    """every operand 16 B aligned.  Lane t of block b: pairs p = 1024 b + t + 256 u for u = 0..3, element 2p then 2p + 1 of each;
    lane 0 of block 0 adds the last element of an odd n after its own pairs.  -> one partial per block"""
    terms = np.asarray(terms, dtype=np.float64)
    n, grid = len(terms), grid_for(len(terms))
    a = _padded(terms[:2 * (n >> 1)], grid * PER_BLOCK).reshape(grid, U, BLOCK, 2)
    s = np.zeros((grid, BLOCK))
    for u in range(U):
        s = s + a[:, u, :, 0]
        s = s + a[:, u, :, 1]
    if n & 1:
        s[0, 0] = s[0, 0] + terms[n - 1]
    return block_sum(s)


@_quiet
def level1_scalar(terms):
    """some operand only 8 B aligned.  The same grid; lane t of block b adds the elements 2048 b + t + 256 u, u = 0..7"""
    terms = np.asarray(terms, dtype=np.float64)
    grid = grid_for(len(terms))
    a = _padded(terms, grid * PER_BLOCK).reshape(grid, 2 * U, BLOCK)
    s = np.zeros((grid, BLOCK))
    for u in range(2 * U):
        s = s + a[:, u, :]
    return block_sum(s)


@_quiet
def fold(partials):
    """`count` partials of one result -> the sum.  1: copied (finish_kernel); up to 2^14: reduce_final, lane t of 1024 adds
    partial[t], partial[t + 1024], ..., then the block sum over 16 wavefronts; more: reduce_fold in blocks of 2048 laid out as
    the scalar path of level 1, then again on the block sums"""
    p = np.asarray(partials, dtype=np.float64)
    while len(p) > 1:
        count = len(p)
        if count <= FINAL_MAX:
            a = _padded(p, -(-count // FINAL_LANES) * FINAL_LANES).reshape(-1, FINAL_LANES)
            s = np.zeros(FINAL_LANES)
            for r in range(a.shape[0]):
                s = s + a[r]
            return np.float64(block_sum(s))
        p = level1_scalar(p)                  # (its grid, ceil(ceil(count / 2) / 1024), is reduce_fold's ceil(count / 2048))
    return np.float64(p[0])


def tree(terms, vector=True):
    """the sum of `terms` as the library's default mode forms it (before any root)"""
    return fold(level1_vector(terms) if vector else level1_scalar(terms))


def root(s):
    """nrm2: sqrt applied once, to the final sum (a single-block reduction applies it in level 1: to the same number)"""
    with np.errstate(invalid="ignore"):
        return np.sqrt(np.float64(s))


# ---------------------------------------------------------------------------------------------------------------- the terms
def red_term(op, x, y=None, w=None, d=None, e=None, a=0.0, sp=0.0, cb=0.0, cc=0.0, c=0.0):
    """Per element: the term(s) v0, v1 the op adds to its sum(s), and what the fused forms store (ox, oy); None where the op has
    none.  Every product and every sum is rounded once.  a: the coefficient (by value or read from HBM), sp: the device scalar of
    the Gram-Schmidt step (negated here), cb, cc: alpha and omega of RED_BICGSTAB_END, c: the uniform 1/diag."""
    a, sp, cb, cc, c = (np.float64(v) for v in (a, sp, cb, cc, c))
    v1 = ox = oy = None
    with np.errstate(all="ignore"):
        if op == RED_DOT:
            v0 = x * y
        elif op == RED_SUMSQ:
            v0 = x * x
        elif op == RED_ABS:
            v0 = np.abs(x)
        elif op == RED_SUM:
            v0 = np.array(x, dtype=np.float64)
        elif op == RED_DOT2:
            v0, v1 = x * y, x * x
        elif op in (RED_CG_UPDATE, RED_CG_UPDATE_JAC):            # x: p, y: q, w: the iterate, d: the residual, e: 1/diag
            ox = w + a * x
            oy = d + (-a) * y
            v0 = oy * oy
            if op == RED_CG_UPDATE_JAC:
                z = oy * e
                v1 = oy * z
        elif op == RED_COUNT_NE:
            v0 = (np.asarray(x, dtype=np.float64).view(np.uint64) != a.view(np.uint64)).astype(np.float64)
        elif op in (RED_AXPY_NRM2, RED_AXPY_NRM2_DOT, RED_AXPY_NRM2_JAC, RED_AXPY_NRM2_JACU):
            oy = y + a * x
            v0 = oy * oy
            if op == RED_AXPY_NRM2_DOT:
                v1 = w * oy
            if op == RED_AXPY_NRM2_JAC:
                z = oy * e
                v1 = oy * z
            if op == RED_AXPY_NRM2_JACU:
                z = oy * c
                v1 = oy * z
        elif op == RED_BICGSTAB_END:                              # x: t, y: s (becomes r), w: rtld, d: phat, e: the iterate
            t1 = e + cb * d
            ox = t1 + cc * y
            oy = y + a * x
            v0 = oy * oy
            v1 = w * oy
        elif op in (RED_AXPYD_DOT, RED_AXPYD_SUMSQ):
            oy = y + (-sp) * x
            v0 = oy * w if op == RED_AXPYD_DOT else oy * oy
        else:
            raise ValueError(op)
    return v0, v1, ox, oy


# ---------------------------------------------------------------------------------------------------------------- chunked A^T x
def get_isie(k, T, n):
    """LIS_GET_ISIE(k, T, n): the rows of chunk k of T (the static schedule of `omp for`)"""
    if k < n % T:
        ie = n // T + 1
        is_ = ie * k
    else:
        ie = n // T
        is_ = ie * k + n % T
    return is_, is_ + ie


def chunk_of(j, T, n):
    for k in range(T):
        is_, ie = get_isie(k, T, n)
        if is_ <= j < ie:
            return k
    raise ValueError((j, T, n))


def spmv_transposed_chunked(rows, nsrc, T, tptr, tidx, tval, x):
    """y[c] of liship_spmv_csr_transposed_chunked_f64: the entries of transposed row c in stored order, grouped by the chunk of
    their source row; each group summed left to right from 0.0; the groups added in chunk order from 0.0 (a chunk without entries
    adds +0.0)"""
    y = np.zeros(rows)
    owner = np.array([chunk_of(j, T, nsrc) for j in range(nsrc)], dtype=np.int64)
    with np.errstate(all="ignore"):
        for c in range(rows):
            parts = [np.float64(0.0)] * T
            for k in range(int(tptr[c]), int(tptr[c + 1])):
                j = int(tidx[k])
                parts[owner[j]] = parts[owner[j]] + np.float64(tval[k]) * np.float64(x[j])
            total = np.float64(0.0)
            for part in parts:
                total = total + part
            y[c] = total
    return y


def transpose_csr(n, ncols, ptr, idx, val):
    """A^T with the entries of every transposed row in the order lis_matvech_csr meets them (ascending position in A's arrays)"""
    cols = [[] for _ in range(ncols)]
    for i in range(n):
        for k in range(int(ptr[i]), int(ptr[i + 1])):
            cols[int(idx[k])].append((i, val[k]))
    tptr = np.zeros(ncols + 1, dtype=np.int32)
    tptr[1:] = np.cumsum([len(c) for c in cols])
    tidx = np.array([i for c in cols for i, _ in c], dtype=np.int32)
    tval = np.array([v for c in cols for _, v in c], dtype=np.float64)
    return tptr, tidx, tval
