"""Inputs of the quad-precision tests, shared by tests/golden/make_golden_quad.py (which runs the reference on them), tests/test_quad_cpu.py and
tests/test_quad_gpu.py: double-double vectors with magnitudes in 1e-8 .. 1e8, mixed signs and non-zero low parts, dots and rows that cancel to about 1e-20
of their terms, a matrix whose rows have the lengths at which the row sum changes its path, and the two matrices of the whole solves.
No NaN, inf or subnormal, nothing beyond 1e+-100."""
import numpy as np

import orc
import quad_model as qm

DOT_SIZES = [0, 1, 2, 3, 7, 8, 9, 64, 65, 1023, 1024, 1025]
THREADS = [1, 2, 4, 8]
ROW_LENGTHS = [0, 1, 2, 3, 4, 5, 63, 64, 65, 129, 2, 2, 0, 7]      # the cancelling row is row 10; row 11 shares its columns
VEC_N = 37                                                         # vector operations: odd, so every T has an odd last element somewhere
SOLVERS = ["cg", "bicg", "cgs", "bicgstab"]
PRECONS = ["none", "jacobi"]
TOL = 1e-25


def dd_vector(n, seed, lo_exp=-8, hi_exp=8):
    """normalised pairs: |hi| = 10^U(lo_exp, hi_exp), random sign, lo a random fraction of half an ulp of hi"""
    rng = np.random.default_rng(seed)
    hi = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(lo_exp, hi_exp, n)
    lo = hi * rng.uniform(-1.0, 1.0, n) * 2.0 ** -54
    lo[lo == 0.0] = hi[lo == 0.0] * 2.0 ** -60
    return qm.fast_two_sum(hi, lo)


def scalar_pairs(count=300, seed=11):
    a, b = dd_vector(count, seed), dd_vector(count, seed + 1)
    return a, b


def dot_vectors(n):
    """x, y of length n; from n >= 8 the first pairs of terms cancel to ~1e-20 of their size (x[2k+1] = -x[2k] but for 1e-4 of its low part)"""
    x, y = dd_vector(n, 100 + n), dd_vector(n, 200 + n)
    if n >= 8:
        xh, xl, yh, yl = x[0].copy(), x[1].copy(), y[0].copy(), y[1].copy()
        for k in range(0, n - 1, 2):
            xh[k + 1], xl[k + 1] = -xh[k], -xl[k] * (1.0 - 2.0 ** -13)
            yh[k + 1], yl[k + 1] = yh[k], yl[k]
        x, y = (xh, xl), (yh, yl)
    return x, y


def rows_matrix(seed=5):
    """CSR with rows of ROW_LENGTHS entries over 140 columns (column 139 is empty), values in 1e-8 .. 1e8 of mixed sign; row 10 = (a, a) on columns (c0, c1) and
    x[c1] = -x[c0] but for a fraction of its low part: the row cancels to ~1e-20 of its terms"""
    rng = np.random.default_rng(seed)
    ncols = 140
    ptr = np.zeros(len(ROW_LENGTHS) + 1, np.int32)
    ptr[1:] = np.cumsum(ROW_LENGTHS)
    idx = np.empty(int(ptr[-1]), np.int32)
    for r, k in enumerate(ROW_LENGTHS):
        idx[ptr[r]:ptr[r + 1]] = rng.choice(ncols - 1, k, replace=False)
    val = rng.choice([-1.0, 1.0], len(idx)) * 10.0 ** rng.uniform(-8, 8, len(idx))
    c0, c1 = 17, 90
    idx[ptr[10]:ptr[11]] = (c0, c1)
    idx[ptr[11]:ptr[12]] = (c1, c0)
    val[ptr[10] + 1] = val[ptr[10]]
    xh, xl = dd_vector(ncols, 77)
    xh[c1], xl[c1] = -xh[c0], -xl[c0] * (1.0 - 2.0 ** -13)
    return ptr, idx, val, (xh, xl), ncols


def transposed_input(seed=6):
    """x of length rows for A^T x of rows_matrix()"""
    return dd_vector(len(ROW_LENGTHS), seed, -3, 3)


def solve_matrices():
    """the symmetric fixture (1-D Poisson, 200 rows) and an unsymmetric one (tridiagonal convection-diffusion with a varying, dominant diagonal, 240 rows).
    The case list runs all four solvers on both, CG included, and every recorded solve has to converge: the off-diagonals differ by 2 %, an asymmetry
    small enough that the reference's CG still reaches 1e-25 on it"""
    out = {"poisson1d": orc.poisson1d(200)}
    n = 240
    rng = np.random.default_rng(42)
    ptr = np.zeros(n + 1, np.int32)
    idx, val = [], []
    for i in range(n):
        if i > 0:
            idx.append(i - 1); val.append(-1.0 - 0.01)
        idx.append(i); val.append(2.5 + rng.uniform(0.0, 1.0))
        if i < n - 1:
            idx.append(i + 1); val.append(-1.0 + 0.01)
        ptr[i + 1] = len(idx)
    out["convdiff"] = (ptr, np.array(idx, np.int32), np.array(val))
    return out


def solve_rhs(name, ptr, idx, val):
    n = len(ptr) - 1
    rng = np.random.default_rng(len(name))
    xs = rng.uniform(-1.0, 1.0, n)
    return orc.spmv_csr(ptr, idx, val, xs)


def solve_x0(n):
    return np.random.default_rng(9).uniform(-0.5, 0.5, n)


def solve_options(solver, precon, zeros):
    return f"-i {solver} -p {precon} -f quad -tol {TOL} -maxiter 600 -print mem -initx_zeros {'true' if zeros else 'false'}"


def solve_key(mat, solver, precon, zeros, T):
    return f"solve/{mat}/{solver}/{precon}/{'zeros' if zeros else 'x0'}/T{T}"


def solve_threads(solver):
    return [1] if solver == "bicg" else THREADS
