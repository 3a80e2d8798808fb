// ilu.hip -- ILU(k) on the GPU (-p ilu, lis_ilu.c): the numerical factorisation along the forward levels, the block triangular sweeps
// and the block gather.  ONE factorisation serves CSR and BSR storage: a place of the pattern holds a bn x bn block of doubles,
// column-major (entry (r, c) at r + c*bn), bn = 1, 2, 3 a template parameter, a block in registers while it is worked on; the point
// form on CSR storage is bn = 1 (the same chain of roundings, bit for bit).  Factorisation and sweeps are "rows" policies
// of the level walker (level_schedule.hpp), a block row where sptrsv.hip has a row.  ref lis_precon_iluk.c:638-762 (point),
// :1714-1819 and :2006-2037 (block), the OpenMP branches.
//
// Factorisation of block row i: L, D, U of the row start at 0 and take A's kept blocks (of a block column stored twice the later
// one wins; the pattern holds no column outside the row's T-block, so those find no place).  For every pivot j of L(i), ascending:
//   buf = L_ij * Dinv_j, stored over L_ij                                  (lis_array_matmat, LIS_INS_VALUE)
//   for every block (c, U_jc) of U(j) with c in row i's pattern: target -= buf * U_jc      (LIS_SUB_VALUE; target in L, D or U)
// then 1.0 on the diagonal of the padding when i is the last block row and bn does not divide n, and D_i inverted in place by
// lis_array_ge (block_ops.hpp).  An entry of a product is a[r]*b[0] + a[r+bn]*b[1] (+ a[r+2bn]*b[2]) summed left to right FROM THE
// FIRST PRODUCT; SUB forms that sum, then subtracts it once (lis_array.c:726-789).  -ffp-contract=off rounds every product alone.
// At bn = 1 that is l = L[i][j] * d[j], target = target - l * u, d[i] = 1 / D: the point form.
// A target takes one update per pivot, so within one pivot the updates are independent.  A short block row is one thread's; a long
// one (>= LISHIP_SWEEP_LONG_ROW block terms) a workgroup's: the pivots in order behind barriers, the updates of one pivot spread
// over the threads, a whole block each; one thread when `serial` (a block column stored twice: one pivot may update a target twice).
//
// Where block column c lies in block row i: the L part of a row is ascending, the U part has an ascending copy of its columns with
// the places (uskey / uspos; uspos NULL: U's rows are ascending as they are): a binary search in the row's own keys, which stay in
// the CU's L1 / L2 while the row is worked on.  Of equal keys the last one answers (the reference's jw[] keeps the later place of a
// column stored twice).
//
// Sweeps (layout of lis_sweep.c, a place holding bn*bn doubles), bn = 2, 3 -- at bn = 1 they are sptrsv.hip's: x_i = b_i; per term
// in stored order
//   x_i[r] = x_i[r] - ((a[r]*xj[0] + a[r+bn]*xj[1]) + a[r+2bn]*xj[2])      (lis_array_matvec, LIS_SUB_VALUE)
// and, with a diagonal (the backward sweep on U), x_i = Dinv_i x_i by the same sums (LIS_INS_VALUE).  Entries of x at or beyond n
// (the padding of the last block) read as +0.0 -- their products are formed, the sign of a zero sum depends on them -- and are never
// written.  A long block row: the per-term sums of a chunk in parallel into LDS, then bn lanes, one per r, subtract them in term
// order.  A block row reads its own b_i before it writes x_i and no other row's b: b may be x.
#include "level_schedule.hpp"
#include "block_ops.hpp"

namespace {

// ------------------------------------------------------------------ block arithmetic in the reference's order
template <int BN>
__device__ __forceinline__ void load_block(double *r, const double *p)
{
#pragma unroll
    for (int e = 0; e < BN * BN; e++) r[e] = p[e];
}
template <int BN>
__device__ __forceinline__ void store_block(double *p, const double *r)
{
#pragma unroll
    for (int e = 0; e < BN * BN; e++) p[e] = r[e];
}
template <int BN>
__device__ __forceinline__ void zero_block(double *p)
{
#pragma unroll
    for (int e = 0; e < BN * BN; e++) p[e] = 0.0;
}

// entry (r, c) of a * b, summed left to right from the first product
template <int BN>
__device__ __forceinline__ double prod_entry(const double *a, const double *b, int r, int c)
{
    double s = a[r] * b[c * BN];
#pragma unroll
    for (int l = 1; l < BN; l++) { const double p = a[r + l * BN] * b[l + c * BN]; s = s + p; }
    return s;
}
// c = a * b (INS) or c -= a * b (SUB)
template <int BN, bool SUB>
__device__ __forceinline__ void matmat(const double *a, const double *b, double *c)
{
#pragma unroll
    for (int j = 0; j < BN; j++)
#pragma unroll
        for (int r = 0; r < BN; r++) {
            const double s = prod_entry<BN>(a, b, r, j);
            c[r + j * BN] = SUB ? c[r + j * BN] - s : s;
        }
}
// row r of a * x, summed left to right from the first product
template <int BN>
__device__ __forceinline__ double matvec_row(const double *a, const double *x, int r)
{
    double s = a[r] * x[0];
#pragma unroll
    for (int l = 1; l < BN; l++) { const double p = a[r + l * BN] * x[l]; s = s + p; }
    return s;
}

// ------------------------------------------------------------------ factorisation
struct Fac {
    int n, nr, serial;
    const int *aptr, *aindex;
    const double *avalue;
    const int *lptr, *lcol, *uptr, *ucol, *uskey, *uspos;
    double *lval, *uval, *d;
    const int *slptr, *sllong, *srows;  // the schedule: levels, first long row of each, block rows in level order
};

// the last index in [lo, hi) whose key is c, or -1
__device__ __forceinline__ int find_last(const int *key, int lo, int hi, int c)
{
    int a = lo, b = hi;
    while (a < b) {
        const int m = (a + b) >> 1;
        if (key[m] <= c) a = m + 1; else b = m;
    }
    return (a > lo && key[a - 1] == c) ? a - 1 : -1;
}

struct Row { int i, l0, l1, u0, u1; };

__device__ __forceinline__ Row row_of(const Fac &f, int i)
{
    return Row{i, f.lptr[i], f.lptr[i + 1], f.uptr[i], f.uptr[i + 1]};
}

// where block row r keeps block column c: in L, as the pivot, in U -- or nowhere
template <int BN>
__device__ __forceinline__ double *place(const Fac &f, const Row &r, int c)
{
    constexpr size_t BS = BN * BN;
    if (c == r.i) return f.d + (size_t)r.i * BS;
    if (c < r.i) {
        const int p = find_last(f.lcol, r.l0, r.l1, c);
        return p < 0 ? nullptr : f.lval + (size_t)p * BS;
    }
    const int p = find_last(f.uskey, r.u0, r.u1, c);
    return p < 0 ? nullptr : f.uval + (size_t)(f.uspos ? f.uspos[p] : p) * BS;
}

template <int BN>
__device__ __forceinline__ void copy_from_a(const Fac &f, const Row &r, int k)
{
    const int c = f.aindex[k];
    if (c < 0 || c >= f.nr) return;
    double *t = place<BN>(f, r, c);
    if (!t) return;
    double a[BN * BN];
    load_block<BN>(a, f.avalue + (size_t)k * (BN * BN));
    store_block<BN>(t, a);
}

// target -= l * U_jc for term k of U(j)
template <int BN>
__device__ __forceinline__ void update(const Fac &f, const Row &r, const double *l, int k)
{
    double *t = place<BN>(f, r, f.ucol[k]);
    if (!t) return;
    double u[BN * BN], c[BN * BN];
    load_block<BN>(u, f.uval + (size_t)k * (BN * BN));
    load_block<BN>(c, t);
    matmat<BN, true>(l, u, c);
    store_block<BN>(t, c);
}

// L_ij = L_ij * Dinv_jrow, stored; l holds it (jrow = lcol[j])
template <int BN>
__device__ __forceinline__ void scale_pivot(const Fac &f, int j, int jrow, double *l)
{
    double a[BN * BN], dj[BN * BN];
    load_block<BN>(a, f.lval + (size_t)j * (BN * BN));
    load_block<BN>(dj, f.d + (size_t)jrow * (BN * BN));
    matmat<BN, false>(a, dj, l);
    store_block<BN>(f.lval + (size_t)j * (BN * BN), l);
}

// the padding's 1.0, then D_i inverted in place
template <int BN>
__device__ __forceinline__ void finish_diagonal(const Fac &f, int i)
{
    double a[BN * BN], lu[BN * BN];
    double *blk = f.d + (size_t)i * (BN * BN);
    load_block<BN>(a, blk);
    pad_last_block<BN>(f.n, f.nr, i, a);
    invert_block(BN, RegRef{a}, RegRef{lu});
    store_block<BN>(blk, a);
}

// one block row, one thread, everything in order
template <int BN>
__device__ void row_by_thread(const Fac &f, int i)
{
    constexpr size_t BS = BN * BN;
    const Row r = row_of(f, i);
    for (int k = r.l0; k < r.l1; k++) zero_block<BN>(f.lval + (size_t)k * BS);
    for (int k = r.u0; k < r.u1; k++) zero_block<BN>(f.uval + (size_t)k * BS);
    zero_block<BN>(f.d + (size_t)i * BS);
    const int a1 = f.aptr[i + 1];
    for (int k = f.aptr[i]; k < a1; k++) copy_from_a<BN>(f, r, k);
    for (int j = r.l0; j < r.l1; j++) {
        double l[BN * BN];
        const int jrow = f.lcol[j];
        scale_pivot<BN>(f, j, jrow, l);
        const int k1 = f.uptr[jrow + 1];
        for (int k = f.uptr[jrow]; k < k1; k++) update<BN>(f, r, l, k);
    }
    finish_diagonal<BN>(f, i);
}

// one block row, the whole workgroup (every thread calls it: the trip counts are uniform)
template <int BN, int BLK>
__device__ void row_by_workgroup(const Fac &f, int i)
{
    constexpr size_t BS = BN * BN;
    const int t = (int)threadIdx.x;
    if (f.serial) {
        if (t == 0) row_by_thread<BN>(f, i);
        return;
    }
    const Row r = row_of(f, i);
    for (int k = r.l0 + t; k < r.l1; k += BLK) zero_block<BN>(f.lval + (size_t)k * BS);
    for (int k = r.u0 + t; k < r.u1; k += BLK) zero_block<BN>(f.uval + (size_t)k * BS);
    if (t == 0) zero_block<BN>(f.d + (size_t)i * BS);
    __syncthreads();
    const int a1 = f.aptr[i + 1];
    for (int k = f.aptr[i] + t; k < a1; k += BLK) copy_from_a<BN>(f, r, k);      // no block column twice: no two threads share a place
    __syncthreads();
    for (int j = r.l0; j < r.l1; j++) {                                         // pivots in order
        double l[BN * BN];
        const int jrow = f.lcol[j];
        if (t == 0) scale_pivot<BN>(f, j, jrow, l);
        __syncthreads();
        load_block<BN>(l, f.lval + (size_t)j * BS);
        const int k1 = f.uptr[jrow + 1];
        for (int k = f.uptr[jrow] + t; k < k1; k += BLK) update<BN>(f, r, l, k);
        __syncthreads();
    }
    if (t == 0) finish_diagonal<BN>(f, i);
}

// the block rows of the factorisation (level_schedule.hpp); no LDS.  In a run every long row ends on a barrier of its own.
template <int BN>
struct FacRows {
    Fac f;
    __device__ __forceinline__ const int *level_ptr() const { return f.slptr; }
    __device__ __forceinline__ const int *level_long() const { return f.sllong; }
    __device__ __forceinline__ void short_row(int r) const { row_by_thread<BN>(f, f.srows[r]); }
    template <int BLK, bool IN_RUN>
    __device__ __forceinline__ void long_row(int r) const { row_by_workgroup<BN, BLK>(f, f.srows[r]); if (IN_RUN) __syncthreads(); }
};

// ------------------------------------------------------------------ sweeps
struct BSweep {
    int n;
    const int *lptr, *llong, *rows, *rptr, *col;
    const double *val, *b, *dinv;       // dinv NULL: no diagonal
    double *x;
};

// block j of v with +0.0 from n on
template <int BN>
__device__ __forceinline__ void load_x(double *r, const double *v, int j, int n)
{
#pragma unroll
    for (int e = 0; e < BN; e++) { const int at = j * BN + e; r[e] = at < n ? v[at] : 0.0; }
}

template <int BN, bool WITH_D>
struct BSweepRows {
    BSweep s;
    __device__ __forceinline__ const int *level_ptr() const { return s.lptr; }
    __device__ __forceinline__ const int *level_long() const { return s.llong; }

    // the sums of term k, one per scalar row of the block
    __device__ __forceinline__ void term(int k, double *sum) const
    {
        double a[BN * BN], xj[BN];
        load_block<BN>(a, s.val + (size_t)k * (BN * BN));
        load_x<BN>(xj, s.x, s.col[k], s.n);
#pragma unroll
        for (int r = 0; r < BN; r++) sum[r] = matvec_row<BN>(a, xj, r);
    }

    // x_i = Dinv_i x_i (xi: the block after its terms, +0.0 in the padding), rows below n written
    __device__ __forceinline__ void finish(int i, const double *xi) const
    {
        double w[BN];
        if (WITH_D) {
            double d[BN * BN];
            load_block<BN>(d, s.dinv + (size_t)i * (BN * BN));
#pragma unroll
            for (int r = 0; r < BN; r++) w[r] = matvec_row<BN>(d, xi, r);
        } else {
#pragma unroll
            for (int r = 0; r < BN; r++) w[r] = xi[r];
        }
#pragma unroll
        for (int r = 0; r < BN; r++) if (i * BN + r < s.n) s.x[i * BN + r] = w[r];
    }

    // one short block row, one lane, in order
    __device__ __forceinline__ void short_row(int r) const
    {
        const int i = s.rows[r];
        double xi[BN], sum[BN];
        load_x<BN>(xi, s.b, i, s.n);
        const int k1 = s.rptr[r + 1];
        for (int k = s.rptr[r]; k < k1; k++) {
            term(k, sum);
#pragma unroll
            for (int e = 0; e < BN; e++) xi[e] = xi[e] - sum[e];
        }
#pragma unroll
        for (int e = 0; e < BN; e++) if (i * BN + e >= s.n) xi[e] = 0.0;
        finish(i, xi);
    }

    // one long block row, the whole workgroup: the sums of BLK terms at once into LDS (sum r of term u at part[r*BLK + u]), then lane r
    // < BN subtracts row r's in term order.  The trip count is uniform, and the row ends on a barrier: the next one may reuse the LDS.
    template <int BLK, bool IN_RUN>
    __device__ __forceinline__ void long_row(int r) const
    {
        __shared__ double part[BN * BLK];
        __shared__ double xs[BN];
        const int t = (int)threadIdx.x;
        const int i = s.rows[r];
        const int k0 = s.rptr[r], k1 = s.rptr[r + 1];
        double acc = 0.0;
        if (t < BN) { const int at = i * BN + t; acc = at < s.n ? s.b[at] : 0.0; }
        for (int kb = k0; kb < k1; kb += BLK) {
            const int k = kb + t;
            if (k < k1) {
                double sum[BN];
                term(k, sum);
#pragma unroll
                for (int e = 0; e < BN; e++) part[e * BLK + t] = sum[e];
            }
            __syncthreads();
            if (t < BN) {
                const int cnt = min(BLK, k1 - kb);
                for (int u = 0; u < cnt; u++) acc = acc - part[t * BLK + u];
            }
            __syncthreads();
        }
        if (t < BN) xs[t] = (i * BN + t < s.n) ? acc : 0.0;
        __syncthreads();
        if (t == 0) {
            double xi[BN];
#pragma unroll
            for (int e = 0; e < BN; e++) xi[e] = xs[e];
            finish(i, xi);
        }
        __syncthreads();
    }
};

template <int BN>
int run_sweep(const liship_sweep_t *sw, int n, const double *dinv, const double *b, double *x, hipStream_t st)
{
    const BSweep s{n, sw->lptr, sw->llong, sw->rows, sw->rptr, sw->col, sw->val, b, dinv, x};
    return dinv ? walk_levels(sw, BSweepRows<BN, true>{s}, st) : walk_levels(sw, BSweepRows<BN, false>{s}, st);
}

// every launch of the factorisation; the pointers were checked by the entry points
int run_factor(const Fac &f, int bn, const liship_sweep_t *sw, hipStream_t st)
{
    switch (bn) {
    case 1:  return walk_levels(sw, FacRows<1>{f}, st);
    case 2:  return walk_levels(sw, FacRows<2>{f}, st);
    default: return walk_levels(sw, FacRows<3>{f}, st);
    }
}

constexpr int GATHER_THREADS = 256;

// dst block p = src block perm[p], a thread per double
__global__ __launch_bounds__(GATHER_THREADS) void block_gather_kernel(long long count, int bs, const int *__restrict__ perm,
                                                                      const double *__restrict__ src, double *__restrict__ dst)
{
    const long long g = (long long)blockIdx.x * GATHER_THREADS + threadIdx.x;
    if (g >= count) return;
    const long long p = g / bs;
    const int e = (int)(g - p * bs);
    dst[g] = src[(long long)perm[p] * bs + e];
}

}  // namespace

// the point form: block rows of one row, blocks of one double
extern "C" int liship_ilu_factor_f64(const liship_ilu_t *p, const liship_sweep_t *sw, void *stream)
{
    if (!p || !sw || p->n < 0 || sw->nrows != p->n) return LISHIP_ERR_ARG;
    if (p->n == 0) return 0;
    if (!p->aptr || !p->lptr || !p->uptr || !p->d || !sw->lptr || !sw->llong || !sw->rows) return LISHIP_ERR_ARG;
    const Fac f{p->n, p->n, p->serial, p->aptr, p->aindex, p->avalue, p->lptr, p->lcol, p->uptr, p->ucol, p->uskey, p->uspos,
                p->lval, p->uval, p->d, sw->lptr, sw->llong, sw->rows};
    return run_factor(f, 1, sw, as_stream(stream));
}

extern "C" int liship_bilu_factor_f64(const liship_bilu_t *p, const liship_sweep_t *sw, void *stream)
{
    if (!p || !sw || p->n < 0 || p->nr < 0 || p->bn < 1 || p->bn > 3 || sw->nrows != p->nr) return LISHIP_ERR_ARG;
    if ((long long)p->nr != ((long long)p->n + p->bn - 1) / p->bn) return LISHIP_ERR_ARG;
    if (p->nr == 0) return 0;
    if (!p->aptr || !p->lptr || !p->uptr || !p->d || !sw->lptr || !sw->llong || !sw->rows) return LISHIP_ERR_ARG;
    const Fac f{p->n, p->nr, p->serial, p->aptr, p->aindex, p->avalue, p->lptr, p->lcol, p->uptr, p->ucol, p->uskey, p->uspos,
                p->lval, p->uval, p->d, sw->lptr, sw->llong, sw->rows};
    return run_factor(f, p->bn, sw, as_stream(stream));
}

extern "C" int liship_bilu_sweep_f64(const liship_sweep_t *sw, int n, int bn, const double *dinv, const double *b, double *x, void *stream)
{
    if (!sw || n < 0 || bn < 1 || bn > 3 || (long long)sw->nrows != ((long long)n + bn - 1) / bn) return LISHIP_ERR_ARG;
    if (n == 0) return 0;
    if (!b || !x) return LISHIP_ERR_ARG;
    if (bn == 1)                         // a block of one double: the point sweeps (sptrsv.hip), the same roundings in the same order
        return dinv ? liship_sweep_f64(sw, LISHIP_SWEEP_MUL, b, x, dinv, stream) : liship_sweep_plain_f64(sw, b, x, stream);
    hipStream_t st = as_stream(stream);
    return bn == 2 ? run_sweep<2>(sw, n, dinv, b, x, st) : run_sweep<3>(sw, n, dinv, b, x, st);
}

extern "C" int liship_block_gather_f64(int nblocks, int bs, const int *perm, const double *src, double *dst, void *stream)
{
    if (nblocks < 0 || bs < 1) return LISHIP_ERR_ARG;
    if (nblocks == 0) return 0;
    if (!perm || !src || !dst) return LISHIP_ERR_ARG;
    const long long count = (long long)nblocks * bs;
    const long long grid = (count + GATHER_THREADS - 1) / GATHER_THREADS;
    if (grid > 0x7fffffffLL) return LISHIP_ERR_ARG;
    hipLaunchKernelGGL(block_gather_kernel, dim3((unsigned)grid), dim3(GATHER_THREADS), 0, as_stream(stream), count, bs, perm, src, dst);
    LAUNCH_CHECK();
    return 0;
}
