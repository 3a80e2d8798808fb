// quad.hip -- double-double ("quad", -f quad) kernels: a vector is two arrays (hi, lo) as in the reference (LIS_VECTOR value / value_lo),
// the matrix stays 8 B values + 4 B indices.  The arithmetic is dd.hpp's, i.e. the reference's SSE2 forms; what each kernel restates:
//   axpy / xpay / axpyz   lis_vector_axpyex_mmm / xpayex_mmm / axpyzex_mmmm (src/precision/lis_precision_vec.c:82-261): per thread chunk
//                         LIS_GET_ISIE(t, T, n) the elements go in pairs through the packed FMA2 form, an odd last element of the chunk through the scalar
//                         FMA form -- the two round differently (dd.hpp: mul / mul2), so an element's form follows from its place in its chunk
//   muld                  lis_psolve_jacobi's quad branch (src/precon/lis_precon_jacobi.c:126-145): x = b * d, d double
//   dot                   lis_vector_dotex_mmm (:265-383): per chunk two accumulators over the pairs, their sum, then an odd last element; the
//                         chunk sums added in thread order from (0, 0).  T = 0 (the default): per-lane chains and a fixed tree of sloppy adds
//   spmv_csr              lis_matvec_csr_mp2 (src/precision/lis_precision_matvec.c:225-249): per row two accumulators from (0, 0) over the entry pairs,
//                         y = acc0 + acc1, then an odd last entry by one FMAD.  Independent of T
//   spmv_csr_t            lis_matvech_csr_mp2 at one thread (:598-640): per output the chain from (0, 0) over the rows that hold the column, ascending,
//                         then one add onto (0, 0); walks the transposed CSR copy, whose rows list exactly that order.  The reference at T > 1 has no
//                         defined bits here (its remainder loop drops the thread's slab offset), so this is the form at every T
#include "common.hpp"
#include "dd.hpp"
#include "liship.h"

namespace {

constexpr int BLOCK = 256;
constexpr int NW = BLOCK / WAVE;

// ------------------------------------------------------------------------------ element-wise passes
// is element i the odd last element of its chunk LIS_GET_ISIE(k, T, n) (include/lis.h:1067-1078)?  T <= 1: one chunk
__device__ __forceinline__ bool chunk_tail(long long i, long long n, int T)
{
    if (T <= 1) return (n & 1) && i == n - 1;
    const long long q = n / T, r = n % T, border = r * (q + 1);
    if (i < border) { const long long len = q + 1; return (len & 1) && (i % len) == len - 1; }
    return (q & 1) && ((i - border) % q) == q - 1;         // q >= 1: an element behind the border exists only then
}

enum { DD_AXPY, DD_XPAY, DD_AXPYZ };

// z = y + a*x (AXPY: z is y; AXPYZ) or y = x + a*y (XPAY).  Every lane reads its element before it writes it: the outputs may be the inputs
template <int OP>
__global__ __launch_bounds__(BLOCK)
void ew_dd_kernel(long long n, int T, dd_t a, const double *xhi, const double *xlo, const double *yhi, const double *ylo, double *zhi, double *zlo)
{
    const long long stride = (long long)gridDim.x * BLOCK;
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride) {
        const dd_t x = dd_make(xhi[i], xlo[i]), y = dd_make(yhi[i], ylo[i]);
        const bool tail = chunk_tail(i, n, T);
        dd_t z;
        if (OP == DD_XPAY) z = tail ? dd_fma(x, a, y) : dd_fma2(x, a, y);
        else               z = tail ? dd_fma(y, a, x) : dd_fma2(y, a, x);
        zhi[i] = z.hi; zlo[i] = z.lo;
    }
}

__global__ __launch_bounds__(BLOCK)
void muld_dd_kernel(long long n, const double *bhi, const double *blo, const double *__restrict__ d, double *xhi, double *xlo)
{
    const long long stride = (long long)gridDim.x * BLOCK;
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride) {
        const dd_t x = dd_muld(dd_make(bhi[i], blo[i]), d[i]);
        xhi[i] = x.hi; xlo[i] = x.lo;
    }
}

__global__ __launch_bounds__(BLOCK)
void widen_dd_kernel(long long n, const double *__restrict__ v, double *__restrict__ hi, double *__restrict__ lo)
{
    const long long stride = (long long)gridDim.x * BLOCK;
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride) { hi[i] = v[i]; lo[i] = 0.0; }
}

inline int ew_grid(long long n)
{
    long long g = (n + BLOCK - 1) / BLOCK;
    if (g < 1) g = 1;
    if (g > 8192) g = 8192;
    return (int)g;
}

// ------------------------------------------------------------------------------ dot
// the tree: lane l of 64 takes lane l + off for off = 32 .. 1 (only lanes below off hold a meaningful sum afterwards), the workgroup's 4
// wavefronts are added in order by lane 0.  tests/quad_model.py restates it
__device__ __forceinline__ dd_t wave_tree_dd(dd_t v)
{
#pragma unroll
    for (int off = WAVE / 2; off >= 1; off >>= 1) {
        const dd_t o = dd_make(__shfl_down(v.hi, off, WAVE), __shfl_down(v.lo, off, WAVE));
        v = dd_add(v, o);
    }
    return v;
}
__device__ __forceinline__ dd_t block_tree_dd(dd_t v, dd_t *scratch)
{
    v = wave_tree_dd(v);
    if ((threadIdx.x & (WAVE - 1)) == 0) scratch[threadIdx.x / WAVE] = v;
    __syncthreads();
    dd_t t = dd_make(0.0, 0.0);
    if (threadIdx.x == 0) {
        t = scratch[0];
#pragma unroll
        for (int w = 1; w < NW; w++) t = dd_add(t, scratch[w]);
    }
    __syncthreads();
    return t;
}

// level 1: lane g of G*256 chains its elements g, g + G*256, ... from (0, 0); one partial (hi, lo) per workgroup
__global__ __launch_bounds__(BLOCK)
void dot_dd_level1(long long n, const double *__restrict__ xhi, const double *__restrict__ xlo, const double *__restrict__ yhi, const double *__restrict__ ylo,
                   double *__restrict__ partial)
{
    __shared__ dd_t scratch[NW];
    const long long stride = (long long)gridDim.x * BLOCK;
    dd_t acc = dd_make(0.0, 0.0);
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride)
        acc = dd_fma2(acc, dd_make(yhi[i], ylo[i]), dd_make(xhi[i], xlo[i]));
    const dd_t t = block_tree_dd(acc, scratch);
    if (threadIdx.x == 0) { partial[2 * blockIdx.x] = t.hi; partial[2 * blockIdx.x + 1] = t.lo; }
}
// level 2: one workgroup, lane l chains the partials l, l + 256, ..., then the same tree
__global__ __launch_bounds__(BLOCK)
void dot_dd_level2(int count, const double *__restrict__ partial, double *__restrict__ result)
{
    __shared__ dd_t scratch[NW];
    dd_t acc = dd_make(0.0, 0.0);
    for (int i = threadIdx.x; i < count; i += BLOCK) acc = dd_add(acc, dd_make(partial[2 * i], partial[2 * i + 1]));
    const dd_t t = block_tree_dd(acc, scratch);
    if (threadIdx.x == 0) { result[0] = t.hi; result[1] = t.lo; }
}

// the reference's order: workgroup c is thread c of T.  Its 256 lanes form the terms of a tile of the chunk (the pairs through mul2), lane 0 chains the
// terms at even places of the chunk onto accumulator 0, lane 64 those at odd places onto accumulator 1; then acc0 + acc1 and the odd last element
constexpr int DOT_TILE = 1024;        // even: a tile border never splits a pair
__global__ __launch_bounds__(BLOCK)
void dot_dd_ref_kernel(long long n, int T, const double *__restrict__ xhi, const double *__restrict__ xlo, const double *__restrict__ yhi, const double *__restrict__ ylo,
                       double *__restrict__ partial)
{
    __shared__ double thi[DOT_TILE], tlo[DOT_TILE];
    __shared__ dd_t acc1_s;
    const int c = blockIdx.x;
    const long long q = n / T, r = n % T;
    const long long is = c < r ? (q + 1) * c : q * c + r, ie = is + (c < r ? q + 1 : q);
    const long long pairs_end = is + ((ie - is) & ~1LL);
    dd_t acc = dd_make(0.0, 0.0);                       // lane 0: accumulator 0; lane 64: accumulator 1
    for (long long base = is; base < pairs_end; base += DOT_TILE) {
        const int cnt = (int)(pairs_end - base < DOT_TILE ? pairs_end - base : DOT_TILE);
        for (int j = threadIdx.x; j < cnt; j += BLOCK) {
            const long long i = base + j;
            const dd_t t = dd_mul2(dd_make(yhi[i], ylo[i]), dd_make(xhi[i], xlo[i]));
            thi[j] = t.hi; tlo[j] = t.lo;
        }
        __syncthreads();
        if (threadIdx.x == 0)    for (int j = 0; j < cnt; j += 2) acc = dd_add(acc, dd_make(thi[j], tlo[j]));
        if (threadIdx.x == WAVE) for (int j = 1; j < cnt; j += 2) acc = dd_add(acc, dd_make(thi[j], tlo[j]));
        __syncthreads();
    }
    if (threadIdx.x == WAVE) acc1_s = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        dd_t s = dd_add(acc, acc1_s);
        if (pairs_end < ie) s = dd_fma(s, dd_make(yhi[pairs_end], ylo[pairs_end]), dd_make(xhi[pairs_end], xlo[pairs_end]));
        partial[2 * c] = s.hi; partial[2 * c + 1] = s.lo;
    }
}
__global__ void dot_dd_ref_final(int T, const double *__restrict__ partial, double *__restrict__ result)
{
    if (threadIdx.x != 0) return;
    dd_t s = dd_make(0.0, 0.0);
    for (int c = 0; c < T; c++) s = dd_add(s, dd_make(partial[2 * c], partial[2 * c + 1]));
    result[0] = s.hi; result[1] = s.lo;
}

// ------------------------------------------------------------------------------ products
// y = A x.  A workgroup owns 256 consecutive rows, one per lane.  The rows' slice [k0, k1) of value[] / index[] goes through LDS in stages of STAGE
// entries by coalesced loads (a 7-point block of 256 rows is 1792 entries: one stage); a lane then walks the part of its row that lies in the stage.
// Entry j of a row goes to accumulator (j - row start) & 1; an odd last entry is added after acc0 + acc1.  No shuffle tree: a row's order is the
// reference's whatever its length, a row longer than a stage simply spans several.
constexpr int SPMV_ROWS = BLOCK;
constexpr int STAGE = 2048;
__global__ __launch_bounds__(BLOCK)
void spmv_csr_dd_kernel(int n, const int *__restrict__ ptr, const int *__restrict__ idx, const double *__restrict__ val,
                        const double *__restrict__ xhi, const double *__restrict__ xlo, double *__restrict__ yhi, double *__restrict__ ylo)
{
    __shared__ double valL[STAGE];
    __shared__ int idxL[STAGE];
    const int r0 = blockIdx.x * SPMV_ROWS, r1 = min(r0 + SPMV_ROWS, n);
    const int k0 = ptr[r0], k1 = ptr[r1];
    const int r = r0 + (int)threadIdx.x;
    int s = 0, e = 0;
    if (r < r1) { s = ptr[r]; e = ptr[r + 1]; }
    const int pairs_end = s + ((e - s) & ~1);           // entries [s, pairs_end) go in pairs, entry pairs_end (if < e) is the odd one
    dd_t acc0 = dd_make(0.0, 0.0), acc1 = dd_make(0.0, 0.0), y = dd_make(0.0, 0.0);
    for (int c0 = k0; c0 < k1; c0 += STAGE) {
        const int c1 = min(c0 + STAGE, k1);
        for (int k = c0 + (int)threadIdx.x; k < c1; k += BLOCK) { valL[k - c0] = load_stream(val + k); idxL[k - c0] = load_stream(idx + k); }
        __syncthreads();
        const int jb = max(s, c0), je = min(e, c1);
        for (int j = jb; j < je; j++) {
            const int col = idxL[j - c0];
            const dd_t t = dd_muld(dd_make(xhi[col], xlo[col]), valL[j - c0]);
            if (j >= pairs_end) y = dd_add(dd_add(acc0, acc1), t);        // the odd last entry: after acc0 + acc1
            else if ((j - s) & 1) acc1 = dd_add(acc1, t);
            else acc0 = dd_add(acc0, t);
        }
        __syncthreads();
    }
    if (r < r1) {
        if (pairs_end == e) y = dd_add(acc0, acc1);
        store_stream(yhi + r, y.hi); store_stream(ylo + r, y.lo);
    }
}

// y = A^T x on the transposed CSR copy: one lane per output, the chain in the row's order, then the add onto (0, 0)
__global__ __launch_bounds__(BLOCK)
void spmv_csr_t_dd_kernel(int rows, const int *__restrict__ ptr, const int *__restrict__ idx, const double *__restrict__ val,
                          const double *__restrict__ xhi, const double *__restrict__ xlo, double *__restrict__ yhi, double *__restrict__ ylo)
{
    const int r = blockIdx.x * BLOCK + (int)threadIdx.x;
    if (r >= rows) return;
    dd_t acc = dd_make(0.0, 0.0);
    for (int k = ptr[r]; k < ptr[r + 1]; k++) {
        const int col = idx[k];
        acc = dd_fmad(acc, dd_make(xhi[col], xlo[col]), val[k]);
    }
    const dd_t y = dd_add(dd_make(0.0, 0.0), acc);
    yhi[r] = y.hi; ylo[r] = y.lo;
}

template <int OP>
int run_ew_dd(int n, double ahi, double alo, const double *xhi, const double *xlo, const double *yhi, const double *ylo, double *zhi, double *zlo, void *stream)
{
    if (n < 0) return LISHIP_ERR_ARG;
    if (n == 0) return 0;
    if (!xhi || !xlo || !yhi || !ylo || !zhi || !zlo) return LISHIP_ERR_ARG;
    ew_dd_kernel<OP><<<ew_grid(n), BLOCK, 0, as_stream(stream)>>>(n, liship_internal_ref_chunks(), dd_make(ahi, alo), xhi, xlo, yhi, ylo, zhi, zlo);
    LAUNCH_CHECK();
    return 0;
}

} // namespace

extern "C" int liship_axpy_dd_f64(int n, double ahi, double alo, const double *xhi, const double *xlo, double *yhi, double *ylo, void *stream)
{ return run_ew_dd<DD_AXPY>(n, ahi, alo, xhi, xlo, yhi, ylo, yhi, ylo, stream); }
extern "C" int liship_xpay_dd_f64(int n, const double *xhi, const double *xlo, double ahi, double alo, double *yhi, double *ylo, void *stream)
{ return run_ew_dd<DD_XPAY>(n, ahi, alo, xhi, xlo, yhi, ylo, yhi, ylo, stream); }
extern "C" int liship_axpyz_dd_f64(int n, double ahi, double alo, const double *xhi, const double *xlo, const double *yhi, const double *ylo,
                                   double *zhi, double *zlo, void *stream)
{ return run_ew_dd<DD_AXPYZ>(n, ahi, alo, xhi, xlo, yhi, ylo, zhi, zlo, stream); }

extern "C" int liship_muld_dd_f64(int n, const double *bhi, const double *blo, const double *d, double *xhi, double *xlo, void *stream)
{
    if (n < 0) return LISHIP_ERR_ARG;
    if (n == 0) return 0;
    if (!bhi || !blo || !d || !xhi || !xlo) return LISHIP_ERR_ARG;
    muld_dd_kernel<<<ew_grid(n), BLOCK, 0, as_stream(stream)>>>(n, bhi, blo, d, xhi, xlo);
    LAUNCH_CHECK();
    return 0;
}

extern "C" int liship_widen_dd_f64(int n, const double *v, double *hi, double *lo, void *stream)
{
    if (n < 0) return LISHIP_ERR_ARG;
    if (n == 0) return 0;
    if (!v || !hi || !lo) return LISHIP_ERR_ARG;
    widen_dd_kernel<<<ew_grid(n), BLOCK, 0, as_stream(stream)>>>(n, v, hi, lo);
    LAUNCH_CHECK();
    return 0;
}

// workgroups of the tree's first level: one per 2048 elements, 1024 at the most (tests/quad_model.py: dot_tree_grid)
extern "C" int liship_dot_dd_grid(int n)
{
    long long g = ((long long)n + 2047) / 2048;
    if (g < 1) g = 1;
    if (g > 1024) g = 1024;
    return (int)g;
}

extern "C" size_t liship_dot_dd_work_bytes(void) { return sizeof(double) * 2 * 1024; }

// result[0 .. 2) = <x, y> as (hi, lo).  work: liship_dot_dd_work_bytes() of HBM, or T pairs in the reference-order mode (T <= 1024)
extern "C" int liship_dot_dd_f64(int n, const double *xhi, const double *xlo, const double *yhi, const double *ylo, double *result, void *work, void *stream)
{
    if (n < 0 || !result || !work) return LISHIP_ERR_ARG;
    if (n > 0 && (!xhi || !xlo || !yhi || !ylo)) return LISHIP_ERR_ARG;
    double *partial = static_cast<double *>(work);
    hipStream_t st = as_stream(stream);
    const int T = liship_internal_ref_chunks();
    if (T > 0) {
        if (T > 1024) return LISHIP_ERR_ARG;
        dot_dd_ref_kernel<<<T, BLOCK, 0, st>>>(n, T, xhi, xlo, yhi, ylo, partial);
        LAUNCH_CHECK();
        dot_dd_ref_final<<<1, WAVE, 0, st>>>(T, partial, result);
        LAUNCH_CHECK();
        return 0;
    }
    const int grid = liship_dot_dd_grid(n);
    dot_dd_level1<<<grid, BLOCK, 0, st>>>(n, xhi, xlo, yhi, ylo, partial);
    LAUNCH_CHECK();
    dot_dd_level2<<<1, BLOCK, 0, st>>>(grid, partial, result);
    LAUNCH_CHECK();
    return 0;
}

extern "C" int liship_spmv_csr_dd_rows_per_block(void) { return SPMV_ROWS; }
extern "C" int liship_spmv_csr_dd_stage(void) { return STAGE; }

extern "C" int liship_spmv_csr_dd_f64(int n, const int *ptr, const int *index, const double *value, const double *xhi, const double *xlo,
                                      double *yhi, double *ylo, void *stream)
{
    if (n < 0) return LISHIP_ERR_ARG;
    if (n == 0) return 0;
    if (!ptr || !index || !value || !xhi || !xlo || !yhi || !ylo) return LISHIP_ERR_ARG;
    spmv_csr_dd_kernel<<<(n + SPMV_ROWS - 1) / SPMV_ROWS, BLOCK, 0, as_stream(stream)>>>(n, ptr, index, value, xhi, xlo, yhi, ylo);
    LAUNCH_CHECK();
    return 0;
}

extern "C" int liship_spmv_csr_t_dd_f64(int rows, const int *tptr, const int *tindex, const double *tvalue, const double *xhi, const double *xlo,
                                        double *yhi, double *ylo, void *stream)
{
    if (rows < 0) return LISHIP_ERR_ARG;
    if (rows == 0) return 0;
    if (!tptr || !tindex || !tvalue || !xhi || !xlo || !yhi || !ylo) return LISHIP_ERR_ARG;
    spmv_csr_t_dd_kernel<<<(rows + BLOCK - 1) / BLOCK, BLOCK, 0, as_stream(stream)>>>(rows, tptr, tindex, tvalue, xhi, xlo, yhi, ylo);
    LAUNCH_CHECK();
    return 0;
}

// dd.hpp as the host compiler built it, for tests: op 0 add, 1 mul (scalar form), 2 mul2 (packed form), 3 muld (b.hi is the double), 4 div,
// 5 two-prod with the fma, 6 two-prod by Dekker's split (both of a.hi, b.hi); out[0 .. 2)
extern "C" int liship_dd_scalar(int op, double ahi, double alo, double bhi, double blo, double *out)
{
    const dd_t a = dd_make(ahi, alo), b = dd_make(bhi, blo);
    dd_t r;
    switch (op) {
    case 0: r = dd_add(a, b); break;
    case 1: r = dd_mul(a, b); break;
    case 2: r = dd_mul2(a, b); break;
    case 3: r = dd_muld(a, bhi); break;
    case 4: r = dd_div(a, b); break;
    case 5: r = dd_two_prod(ahi, bhi); break;
    case 6: r = dd_two_prod_dekker(ahi, bhi); break;
    default: return LISHIP_ERR_ARG;
    }
    out[0] = r.hi; out[1] = r.lo;
    return 0;
}
