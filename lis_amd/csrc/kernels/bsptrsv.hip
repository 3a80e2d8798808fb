// bsptrsv.hip -- level-scheduled BLOCK triangular sweeps for -p ssor on BSR storage (lis_ssor.c): lis_matrix_solve_bsr and
// lis_matrix_solveh_bsr (ref src/matrix/lis_matrix_bsr.c:1397-2090, serial in the reference at any thread count) on the layouts of
// lis_sweep.c, a place of val holding one bn x bn block, column-major (entry (r, c) at r + c*bn), bn = 2 .. 8 a template parameter.
// At bn = 1 the entry point runs the point sweeps of sptrsv.hip: the same chain of roundings.
//
// Every scalar row is ONE ordered chain, a rounded product and a rounded add or subtract per step (-ffp-contract=off):
//   plain      MUL  t = b_i;   per term k in stored order, c = 0 .. bn-1 ascending:  t[r] = t[r] - a_k(r,c) * x_j[c];   x_i = WD_i t
//              SUB  t = +0.0;  t[r] = t[r] + a_k(r,c) * x_j[c] likewise;                                                  x_i = x_i - WD_i t
//   transposed MUL  t = b_i;   per term k (a row of the transposed listing: source rows in scatter order):
//                              t[c] = t[c] - (sum over r of a_k(r,c) * x_j[r]);                        x_i = WD_i^T t
//              SCAT t = b_i;   t[c] = t[c] - (sum over r of a_k(r,c) * work_j[r]);                     x_i = t, work_i = WD_i^T t
// where (WD_i t)[r] = sum over c of WD_i(r,c) * t[c] and (WD_i^T t)[c] = sum over r of WD_i(r,c) * t[r].  Every such sum -- the
// grouped sums of the transposed terms included -- runs left to right and starts with its first product for bn <= 3 and at +0.0 from
// bn = 4 on (the reference's `default:` branches): the two differ in the sign of a zero.  The plain terms are individual
// subtractions, NOT the grouped sum of the block ILU sweep (ilu.hip).
// SCAT is the first sweep of SSOR-h, whose scatter hands on WD_j^T x_j without storing it into x: a row's finish keeps it in `work`
// (bn doubles per block row; the padding of the last block holds +0.0, what x reads there), which later terms read instead of forming
// it again.
//
// b and x read as +0.0 at and beyond n (the padding of the last block when bn does not divide n) and x is never written there; the
// transposed finishes take the padding of t as +0.0 too, which is what a scatter that reads x there sees.  A block row reads its own
// b_i before it writes x_i and no other row's b: b may be x.
//
// A short block row is one lane's: t in registers at compile-time indices, the block streamed column by column (bn doubles at a
// time, never a whole block: 8 x 8 doubles would not fit the 128 registers of the run kernel's 1024-thread workgroup).  A long one
// (LISHIP_SWEEP_LONG_ROW terms or more) is a workgroup's: the products (plain: bn*bn per term, transposed: the bn grouped sums) of a
// chunk of terms in parallel into LDS, then lane r < bn applies its row's in (term, c) order.  The chunk depends on bn alone
// (bsweep_chunk: 16 KB of LDS at most, so bn = 8 takes 32 terms where one size for all would need 128 KB).
#include "level_schedule.hpp"

namespace {

// terms of a long block row whose products are in LDS at once: the largest power of two <= 256 that keeps them within 16 KB
constexpr int bsweep_chunk(int bn)
{
    int c = 256;
    while (c * bn * bn * 8 > 16384) c /= 2;
    return c;
}
static_assert(bsweep_chunk(2) == 256 && bsweep_chunk(3) == 128 && bsweep_chunk(4) == 128 && bsweep_chunk(5) == 64, "chunks");
static_assert(bsweep_chunk(6) == 32 && bsweep_chunk(7) == 32 && bsweep_chunk(8) == 32, "chunks");

struct BSsor {
    int n;
    const int *lptr, *llong, *rows, *rptr, *col;
    const double *val, *b, *wd;
    double *x, *work;
};

// v[at], +0.0 at and beyond n
__device__ __forceinline__ double read_padded(const double *v, int at, int n) { return at < n ? v[at] : 0.0; }

// acc + p, or p alone where the reference's sum starts with its first product (bn <= 3)
template <int BN>
__device__ __forceinline__ double sum_step(double acc, double p, bool first)
{
    return (BN <= 3 && first) ? p : acc + p;
}

// Between two columns of a large block: the sums so far are formed here, and no load of the next column is issued before.  Fully
// unrolled, the compiler would otherwise issue the 64 loads of an 8 x 8 block first and do the arithmetic last, which spills out of
// the 128 registers a lane of the run kernel's 1024-thread workgroup has.  (An empty statement: it only pins the order.)
template <int BN>
__device__ __forceinline__ void column_fence(double *t)
{
    if (BN >= 6) {
#pragma unroll
        for (int e = 0; e < BN; e++) asm volatile("" : "+v"(t[e]) : : "memory");
    }
}

template <int BN, int MODE, bool TR>
struct BSsorRows {
    static constexpr int BS = BN * BN;
    static constexpr int CHUNK = bsweep_chunk(BN);
    BSsor s;
    __device__ __forceinline__ const int *level_ptr() const { return s.lptr; }
    __device__ __forceinline__ const int *level_long() const { return s.llong; }

    // what a term reads of block row j: x, or the first SSOR-h sweep's work vector (whole blocks: no padding to mask)
    __device__ __forceinline__ double source(int j, int e) const
    {
        if (TR && MODE == LISHIP_SWEEP_SCAT) return s.work[j * BN + e];
        return read_padded(s.x, j * BN + e, s.n);
    }

    // column c of term k applied to t (plain), or its grouped sum (transposed)
    __device__ __forceinline__ void plain_term(int k, double *t) const
    {
        const double *a = s.val + (size_t)k * BS;
        const int j = s.col[k];
#pragma unroll
        for (int c = 0; c < BN; c++) {
            const double xc = source(j, c);
#pragma unroll
            for (int r = 0; r < BN; r++) {
                const double p = a[r + c * BN] * xc;
                t[r] = MODE == LISHIP_SWEEP_SUB ? t[r] + p : t[r] - p;
            }
            column_fence<BN>(t);
        }
    }
    __device__ __forceinline__ double grouped_sum(const double *a, const double *tv, int c) const
    {
        double sum = 0.0;
#pragma unroll
        for (int r = 0; r < BN; r++) sum = sum_step<BN>(sum, a[r + c * BN] * tv[r], r == 0);
        return sum;
    }
    __device__ __forceinline__ void transposed_term(int k, double *t) const
    {
        const double *a = s.val + (size_t)k * BS;
        const int j = s.col[k];
        double tv[BN];
#pragma unroll
        for (int r = 0; r < BN; r++) tv[r] = source(j, r);
#pragma unroll
        for (int c = 0; c < BN; c++) { t[c] = t[c] - grouped_sum(a, tv, c); column_fence<BN>(t); }
    }

    // entry e of WD_i t (plain) or WD_i^T t (transposed); t read through T (registers or LDS)
    template <class T>
    __device__ __forceinline__ double wd_entry(const double *w, const T &t, int e) const
    {
        double sum = 0.0;
#pragma unroll
        for (int q = 0; q < BN; q++) sum = sum_step<BN>(sum, (TR ? w[q + e * BN] : w[e + q * BN]) * t[q], q == 0);
        return sum;
    }

    // one short block row, one lane, in order
    __device__ __forceinline__ void short_row(int r) const
    {
        const int i = s.rows[r];
        double t[BN];
#pragma unroll
        for (int e = 0; e < BN; e++) t[e] = (!TR && MODE == LISHIP_SWEEP_SUB) ? 0.0 : read_padded(s.b, i * BN + e, s.n);
        const int k1 = s.rptr[r + 1];
#pragma unroll 1
        for (int k = s.rptr[r]; k < k1; k++) {
            if (TR) transposed_term(k, t); else plain_term(k, t);
        }
        if (TR) {
#pragma unroll
            for (int e = 0; e < BN; e++) if (i * BN + e >= s.n) t[e] = 0.0;
        }
        const double *w = s.wd + (size_t)i * BS;
        double out[BN];
#pragma unroll
        for (int e = 0; e < BN; e++) { out[e] = wd_entry(w, t, e); column_fence<BN>(out); }
#pragma unroll
        for (int e = 0; e < BN; e++) {
            const int at = i * BN + e;
            if (TR && MODE == LISHIP_SWEEP_SCAT) {
                s.work[at] = at < s.n ? out[e] : 0.0;
                if (at < s.n) s.x[at] = t[e];
            } else if (at < s.n) {
                s.x[at] = (!TR && MODE == LISHIP_SWEEP_SUB) ? s.x[at] - out[e] : out[e];
            }
        }
    }

    // one long block row, the whole workgroup.  Plain: work item (term u, column c) puts the BN products of that column at
    // part[(u*BN + c)*BN + r]; transposed: its grouped sum at part[u*BN + c].  Then lane e < BN applies its scalar row's in (term, c)
    // order.  The trip counts are uniform, and the row ends on a barrier: the next one may reuse the LDS.
    template <int BLK, bool IN_RUN>
    __device__ __forceinline__ void long_row(int r) const
    {
        __shared__ double part[CHUNK * (TR ? BN : BS)];
        __shared__ double ts[BN];
        const int lane = (int)threadIdx.x;
        const int i = s.rows[r];
        const int k0 = s.rptr[r], k1 = s.rptr[r + 1];
        double acc = 0.0;
        if (lane < BN && !(!TR && MODE == LISHIP_SWEEP_SUB)) acc = read_padded(s.b, i * BN + lane, s.n);
        for (int kb = k0; kb < k1; kb += CHUNK) {
            const int cnt = min(CHUNK, k1 - kb);
            for (int it = lane; it < cnt * BN; it += BLK) {
                const int u = it / BN, c = it - u * BN;
                const double *a = s.val + (size_t)(kb + u) * BS;
                const int j = s.col[kb + u];
                if (TR) {
                    double tv[BN];
#pragma unroll
                    for (int q = 0; q < BN; q++) tv[q] = source(j, q);
                    double sum = 0.0;
#pragma unroll
                    for (int q = 0; q < BN; q++) sum = sum_step<BN>(sum, a[q + c * BN] * tv[q], q == 0);
                    part[it] = sum;
                } else {
                    const double xc = source(j, c);
#pragma unroll
                    for (int q = 0; q < BN; q++) part[it * BN + q] = a[q + c * BN] * xc;
                }
            }
            __syncthreads();
            if (lane < BN) {
                if (TR) {
                    for (int u = 0; u < cnt; u++) acc = acc - part[u * BN + lane];
                } else {
                    for (int q = 0; q < cnt * BN; q++) {
                        const double p = part[q * BN + lane];
                        acc = MODE == LISHIP_SWEEP_SUB ? acc + p : acc - p;
                    }
                }
            }
            __syncthreads();
        }
        if (lane < BN) ts[lane] = (TR && i * BN + lane >= s.n) ? 0.0 : acc;
        __syncthreads();
        if (lane < BN) {
            const int at = i * BN + lane;
            const double out = wd_entry(s.wd + (size_t)i * BS, ts, lane);
            if (TR && MODE == LISHIP_SWEEP_SCAT) {
                s.work[at] = at < s.n ? out : 0.0;
                if (at < s.n) s.x[at] = ts[lane];
            } else if (at < s.n) {
                s.x[at] = (!TR && MODE == LISHIP_SWEEP_SUB) ? s.x[at] - out : out;
            }
        }
        __syncthreads();
    }
};

template <int BN>
int run_bsweep(const liship_sweep_t *sw, const BSsor &s, int mode, int transposed, hipStream_t st)
{
    if (!transposed) return mode == LISHIP_SWEEP_MUL ? walk_levels(sw, BSsorRows<BN, LISHIP_SWEEP_MUL, false>{s}, st)
                                                     : walk_levels(sw, BSsorRows<BN, LISHIP_SWEEP_SUB, false>{s}, st);
    return mode == LISHIP_SWEEP_MUL ? walk_levels(sw, BSsorRows<BN, LISHIP_SWEEP_MUL, true>{s}, st)
                                    : walk_levels(sw, BSsorRows<BN, LISHIP_SWEEP_SCAT, true>{s}, st);
}

}  // namespace

extern "C" int liship_bsweep_chunk(int bn)
{
    return bn >= 2 && bn <= 8 ? bsweep_chunk(bn) : bn == 1 ? LEVEL_BLOCK : 0;
}

extern "C" int liship_bsweep_f64(const liship_sweep_t *sw, int n, int bn, int mode, int transposed, const double *b, double *x,
                                 const double *wd, double *work, void *stream)
{
    if (!sw || n < 0 || bn < 1 || bn > 8 || (long long)sw->nrows != ((long long)n + bn - 1) / bn) return LISHIP_ERR_ARG;
    if (transposed ? (mode != LISHIP_SWEEP_MUL && mode != LISHIP_SWEEP_SCAT) : (mode != LISHIP_SWEEP_MUL && mode != LISHIP_SWEEP_SUB)) return LISHIP_ERR_ARG;
    if (n == 0) return 0;
    const int needs_b = !(mode == LISHIP_SWEEP_SUB && !transposed);
    if (!x || !wd || (needs_b && !b)) return LISHIP_ERR_ARG;
    if (bn == 1)                         // a block of one double: the point sweeps (sptrsv.hip), the same roundings in the same order
        return liship_sweep_f64(sw, mode, b, x, wd, stream);
    if (transposed && mode == LISHIP_SWEEP_SCAT && !work) return LISHIP_ERR_ARG;
    if (!sw->lptr || !sw->llong || !sw->rows || !sw->rptr || (sw->nnz > 0 && (!sw->col || !sw->val))) return LISHIP_ERR_ARG;
    const BSsor s{n, sw->lptr, sw->llong, sw->rows, sw->rptr, sw->col, sw->val, b, wd, x, work};
    hipStream_t st = as_stream(stream);
    switch (bn) {
#define BS_CASE(K) case K: return run_bsweep<K>(sw, s, mode, transposed, st);
    BS_CASE(2) BS_CASE(3) BS_CASE(4) BS_CASE(5) BS_CASE(6) BS_CASE(7)
#undef BS_CASE
    default: return run_bsweep<8>(sw, s, mode, transposed, st);
    }
}
