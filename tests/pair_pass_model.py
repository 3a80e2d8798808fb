"""A numpy model of the two pair passes (liship_scale2_inv_sqrt_f64, liship_scale2_to_f64; kernels/vector_ops.hip) in the lane mapping of
kernels/vector_pass.hpp, numpy only.

A workgroup of 256 lanes owns a tile of 2048 elements.  In the 16 B walk (every array 16 B aligned) lane t of block b takes the element pairs
p = 1024 b + t + 256 u, u = 0..3, element 2p before 2p + 1, and lane 0 of block 0 takes the last element of an odd n after its own pairs; in the 8 B walk lane t
of block b takes the elements 2048 b + t + 256 u, u = 0..7.  Each result is one rounded product alpha * x; for the inverse-square-root form the factor is
1.0 / sqrt(s), formed once (every lane forms the same double) -- two roundings, then one per element."""
import numpy as np

BLOCK = 256
U = 4
PAIRS_PER_BLOCK = BLOCK * U


def grid(n):
    return ((n + 1) // 2 + PAIRS_PER_BLOCK - 1) // PAIRS_PER_BLOCK


def lane_elements(n, vec):
    """-> list of (block, lane, [elements in the order the lane meets them]) for the lanes that meet any"""
    out = []
    for b in range(grid(n)):
        for t in range(BLOCK):
            mine = []
            if vec:
                for u in range(U):
                    p = b * PAIRS_PER_BLOCK + t + u * BLOCK
                    if p < n // 2:
                        mine += [2 * p, 2 * p + 1]
                if n % 2 and b == 0 and t == 0:
                    mine.append(n - 1)
            else:
                for u in range(2 * U):
                    i = b * 2 * PAIRS_PER_BLOCK + t + u * BLOCK
                    if i < n:
                        mine.append(i)
            if mine:
                out.append((b, t, mine))
    return out


def inv_sqrt(s):
    """the factor of the inverse-square-root form: sqrt rounded, then the reciprocal rounded; no fabs (s < 0: NaN; s = 0: inf; s = inf: 0)"""
    with np.errstate(all="ignore"):
        return np.float64(1.0) / np.sqrt(np.float64(s))


def scale2_to(alpha, in0, in1, vec=True):
    """out0 = alpha * in0, out1 = alpha * in1, element by element as the lanes meet them; entries no lane meets stay NaN-marked (there must be none)"""
    n = len(in0)
    assert len(in1) == n
    alpha = np.float64(alpha)
    out0, out1 = np.full(n, np.nan), np.full(n, np.nan)
    met = np.zeros(n, np.int64)
    with np.errstate(all="ignore"):
        for _, _, mine in lane_elements(n, vec):
            idx = np.array(mine)
            out0[idx] = alpha * in0[idx]
            out1[idx] = alpha * in1[idx]
            met[idx] += 1
    assert np.all(met == 1), "every element belongs to exactly one lane"
    return out0, out1


def scale2_inv_sqrt(s, v, w, vec=True):
    return scale2_to(inv_sqrt(s), v, w, vec)
