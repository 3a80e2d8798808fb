"""numpy restatement of the double-double arithmetic of -f quad (lis_amd/csrc/kernels/dd.hpp) and of the sums the quad kernels form
(lis_amd/csrc/kernels/quad.hip): every function works element-wise on float64 arrays, a dd value is a pair (hi, lo).

The operation order is that of the reference's SSE2 forms (include/lis_precision.h: USE_SSE2, USE_FAST_QUAD_ADD, USE_FMA2_SSE2); two-prod's error
term is Dekker's sum over the halves split with 134217729.0, which is exact and so equals the fma the kernels use wherever nothing overflows or
underflows.  tests/test_quad_cpu.py holds all of this to the reference's bits (tests/golden/quad_bits.npz)."""
import numpy as np

SPLITTER = 134217729.0


def two_sum(a, b):
    s = a + b
    v = s - a
    return s, (a - (s - v)) + (b - v)


def fast_two_sum(a, b):
    s = a + b
    return s, b - (s - a)


def two_diff(a, b):
    s = a - b
    v = s - a
    return s, (a - (s - v)) - (b + v)


def split(a):
    t = SPLITTER * a
    hi = t - (t - a)
    return hi, a - hi


def two_prod(a, b):
    p = a * b
    ah, al = split(a)
    bh, bl = split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def mul(b, c):
    """the scalar form (LIS_QUAD_MUL_SSE2): lis_quad_mul, the odd last element of a thread's chunk"""
    p, e = two_prod(b[0], c[0])
    e = e + c[0] * b[1]
    e = e + b[0] * c[1]
    return fast_two_sum(p, e)


def mul2(b, c):
    """the packed form (LIS_QUAD_MUL2_SSE2): the elements taken in pairs; mul2(b, c) == mul(c, b)"""
    p, e = two_prod(b[0], c[0])
    e = e + b[0] * c[1]
    e = e + c[0] * b[1]
    return fast_two_sum(p, e)


def muld(b, c):
    p, e = two_prod(b[0], c)
    e = e + b[1] * c
    return fast_two_sum(p, e)


def add(b, c):
    s, e = two_sum(b[0], c[0])
    e = e + b[1]
    e = e + c[1]
    return fast_two_sum(s, e)


def minus(a):
    return -a[0], -a[1]


def fma(a, b, c):
    return add(a, mul(b, c))


def fma2(a, b, c):
    return add(a, mul2(b, c))


def fmad(a, b, c):
    return add(a, muld(b, c))


def div(b, c):
    q1 = b[0] / c[0]
    r = muld(c, q1)
    d, e = two_diff(b[0], r[0])
    e = e - r[1]
    e = e + b[1]
    q2 = (d + e) / c[0]
    return fast_two_sum(q1, q2)


# ------------------------------------------------------------------ vector operations
def chunks(n, T):
    """LIS_GET_ISIE(t, T, n) for t = 0 .. T-1 (include/lis.h:1067-1078); T <= 1: one chunk"""
    T = max(T, 1)
    q, r = divmod(n, T)
    out = []
    for t in range(T):
        is_ = (q + 1) * t if t < r else q * t + r
        out.append((is_, is_ + (q + 1 if t < r else q)))
    return out


def tail_mask(n, T):
    """True where an element is the odd last one of its chunk: it takes the scalar form"""
    m = np.zeros(n, bool)
    for is_, ie in chunks(n, T):
        if (ie - is_) & 1:
            m[ie - 1] = True
    return m


def _fma_by_place(a, b, c, T):
    n = len(a[0])
    m = tail_mask(n, T)
    s = fma(a, b, c)
    p = fma2(a, b, c)
    return np.where(m, s[0], p[0]), np.where(m, s[1], p[1])


def _bc(alpha, n):
    return np.full(n, alpha[0]), np.full(n, alpha[1])


def axpy(alpha, x, y, T=0):
    """y + alpha*x"""
    return _fma_by_place(y, _bc(alpha, len(x[0])), x, T)


def xpay(x, alpha, y, T=0):
    """x + alpha*y"""
    return _fma_by_place(x, _bc(alpha, len(x[0])), y, T)


def axpyz(alpha, x, y, T=0):
    """z = y + alpha*x"""
    return axpy(alpha, x, y, T)


# ------------------------------------------------------------------ sums
def _s(v, i):
    return v[0][i], v[1][i]


def dot_ref(x, y, T):
    """lis_vector_dotex_mmm(x, y) at T threads: per chunk two accumulators over the pairs, their sum, the odd last element; chunk sums in order from (0, 0)"""
    n = len(x[0])
    z = np.float64(0.0)
    terms = mul2(y, x)
    total = (z, z)
    for is_, ie in chunks(n, T):
        a0, a1 = (z, z), (z, z)
        pe = is_ + ((ie - is_) & ~1)
        for i in range(is_, pe, 2):
            a0 = add(a0, _s(terms, i))
            a1 = add(a1, _s(terms, i + 1))
        s = add(a0, a1)
        if pe < ie:
            s = fma(s, _s(y, pe), _s(x, pe))
        total = add(total, s)
    return total


def dot_tree_grid(n):
    return min(max((n + 2047) // 2048, 1), 1024)


def _tree(v):
    """v: (..., 256) lanes -> one value per leading index: 64 lanes fold by lane l + off for off = 32 .. 1, then the 4 wavefronts in order"""
    hi = v[0].reshape(v[0].shape[:-1] + (4, 64)).copy()
    lo = v[1].reshape(hi.shape).copy()
    off = 32
    while off >= 1:
        h, l = add((hi[..., :off], lo[..., :off]), (hi[..., off:2 * off], lo[..., off:2 * off]))
        hi[..., :off], lo[..., :off] = h, l
        off //= 2
    t = (hi[..., 0, 0], lo[..., 0, 0])
    for w in range(1, 4):
        t = add(t, (hi[..., w, 0], lo[..., w, 0]))
    return t


def _lane_chains(lanes, n, term):
    """lane g of `lanes` chains term(i) for i = g, g + lanes, ... from (0, 0)"""
    hi, lo = np.zeros(lanes), np.zeros(lanes)
    for base in range(0, n, lanes):
        cnt = min(lanes, n - base)
        th, tl = term(base, base + cnt)
        h, l = add((hi[:cnt], lo[:cnt]), (th, tl))
        hi[:cnt], lo[:cnt] = h, l
    return hi, lo


def dot_tree(x, y):
    """liship_dot_dd_f64 in the default mode"""
    n = len(x[0])
    G = dot_tree_grid(n)
    terms = mul2(y, x)
    acc = _lane_chains(G * 256, n, lambda a, b: (terms[0][a:b], terms[1][a:b]))
    part = _tree((acc[0].reshape(G, 256), acc[1].reshape(G, 256)))
    part = (np.atleast_1d(part[0]), np.atleast_1d(part[1]))
    acc2 = _lane_chains(256, G, lambda a, b: (part[0][a:b], part[1][a:b]))
    t = _tree(acc2)
    return np.float64(t[0]), np.float64(t[1])


def spmv_csr(ptr, idx, val, x):
    """lis_matvec_csr_mp2: per row accumulators 0 / 1 over the entry pairs from (0, 0), y = acc0 + acc1, then an odd last entry"""
    n = len(ptr) - 1
    yh, yl = np.zeros(n), np.zeros(n)
    z = np.float64(0.0)
    t = muld((x[0][idx], x[1][idx]), val) if len(idx) else (np.zeros(0), np.zeros(0))
    for r in range(n):
        s, e = int(ptr[r]), int(ptr[r + 1])
        a0, a1 = (z, z), (z, z)
        pe = s + ((e - s) & ~1)
        for j in range(s, pe, 2):
            a0 = add(a0, _s(t, j))
            a1 = add(a1, _s(t, j + 1))
        y = add(a0, a1)
        if pe < e:
            y = add(y, _s(t, pe))
        yh[r], yl[r] = y
    return yh, yl


def spmv_csr_t(ptr, idx, val, x, ncols):
    """lis_matvech_csr_mp2 at one thread: y[j] = (0, 0) + the chain from (0, 0) over the rows i ascending that hold column j"""
    n = len(ptr) - 1
    wh, wl = np.zeros(ncols), np.zeros(ncols)
    for i in range(n):
        for k in range(int(ptr[i]), int(ptr[i + 1])):
            j = int(idx[k])
            wh[j], wl[j] = fmad((wh[j], wl[j]), (x[0][i], x[1][i]), val[k])
    return add((np.zeros(ncols), np.zeros(ncols)), (wh, wl))
