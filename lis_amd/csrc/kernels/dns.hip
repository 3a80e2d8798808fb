// dns.hip -- y = A x and y = A^T x for dense (LIS_MATRIX_DNS) storage: value[j*n + i], column-major, n rows, np columns.
//
// The reference (src/matvec/lis_matvec_dns.c):
//   lis_matvec_dns   :50-85   y[i] = 0, then y[i] += value[j*n+i] * x[j] for j = 0 .. np-1, zeros multiplied too.  One chain per row, from +0.0; the
//                             OpenMP build splits the ROWS, so the bits are the same at every thread count.
//   lis_matvech_dns  :87-130  (OpenMP branch) thread k sums value[j*n+i] * x[i] over its rows LIS_GET_ISIE(k, T, n) from 0.0, then
//                             y[j] = ((0.0 + t_0) + t_1) + ...  -- T row chunks per column, the chunk sums added in chunk order.
// Both are pure streams of 8 n np bytes, and only the ADDS of one output are ordered.  A lane per output alone gives n / 64 wavefronts (128 at n = 8192 for
// 256 CUs), far too few loads in flight.  So a workgroup owns a strip of 32 outputs, ALL its 256 lanes load and multiply a slab of 64 terms per output
// (coalesced along i, which is the contiguous direction for both products) into LDS, and one lane per output folds the slab in order while the other
// wavefronts are already loading the next one (two LDS buffers, one barrier per slab; the slab after next is in flight in registers).
//   forward      lane (r, g): row i0 + r, columns g, g + 8, ... of the slab; prod[col][row], 32 doubles per column: writes and the fold are conflict-free
//   transposed   lane (l, w): row i0 + l of the slab, columns w, w + 4, ... of the strip; prod[col][row] with a stride of 65 doubles, so that the fold
//                -- lane c walks column c -- reads 32 different bank pairs (130 c mod 64 = 2 c)
// Every product is rounded before it is added (-ffp-contract=off); the fold is a plain left-to-right chain.
#include "common.hpp"
#include "liship.h"

namespace {

constexpr int THREADS = 256;
constexpr int ROWS = 32;                      // forward: rows of y per workgroup
constexpr int SLAB = 64;                      //          columns per slab
constexpr int GROUPS = THREADS / ROWS;        //          column groups of the workgroup (8)
constexpr int CPT = SLAB / GROUPS;            //          columns per lane and slab (8)
constexpr int TCOLS = 32;                     // transposed: columns of A (entries of y) per workgroup
constexpr int TSLAB = 64;                     //             rows per slab (one wavefront wide)
constexpr int TWAVES = THREADS / TSLAB;       //             wavefronts (4)
constexpr int TCPT = TCOLS / TWAVES;          //             columns per lane and slab (8)
constexpr int TPAD = TSLAB + 1;               //             LDS stride of a column

__global__ __launch_bounds__(THREADS)
void spmv_dns_kernel(int n, int np, const double *__restrict__ value, const double *__restrict__ x, double *__restrict__ y)
{
    __shared__ double prod[2][SLAB][ROWS];
    const int r = (int)threadIdx.x % ROWS, g = (int)threadIdx.x / ROWS;
    const long long i = (long long)blockIdx.x * ROWS + r;
    const bool row_ok = i < n;
    const int nslabs = (np + SLAB - 1) / SLAB;
    const double *col0 = value + (row_ok ? (size_t)i : 0);
    double v[CPT], w[CPT] = {};
#pragma unroll
    for (int q = 0; q < CPT; q++) {
        const int j = g + q * GROUPS;
        v[q] = (row_ok && j < np) ? load_stream(col0 + (size_t)j * (size_t)n) : 0.0;
    }
    double acc = 0.0;
    for (int s = 0; s < nslabs; s++) {
        const int j0 = s * SLAB, b = s & 1;
        if (s + 1 < nslabs) {
#pragma unroll
            for (int q = 0; q < CPT; q++) {
                const long long j = (long long)j0 + SLAB + g + q * GROUPS;
                w[q] = (row_ok && j < np) ? load_stream(col0 + (size_t)j * (size_t)n) : 0.0;
            }
        }
#pragma unroll
        for (int q = 0; q < CPT; q++) {
            const long long j = (long long)j0 + g + q * GROUPS;
            const double xj = j < np ? x[j] : 0.0;
            prod[b][g + q * GROUPS][r] = v[q] * xj;
        }
        __syncthreads();
        if (g == 0) {                                  // one lane per row: the slab's terms in column order
            const int cnt = np - j0 < SLAB ? np - j0 : SLAB;
            if (cnt == SLAB) {
#pragma unroll 16
                for (int jj = 0; jj < SLAB; jj++) acc += prod[b][jj][r];
            } else for (int jj = 0; jj < cnt; jj++) acc += prod[b][jj][r];
        }
#pragma unroll
        for (int q = 0; q < CPT; q++) v[q] = w[q];
    }
    if (g == 0 && row_ok) y[i] = acc;
}

// chunk k of T over n rows: LIS_GET_ISIE (include/lis.h of the reference, :1067-1078)
__device__ __forceinline__ void chunk_rows(int k, int T, int n, long long *is, long long *ie)
{
    const int q = n / T, rem = n % T;
    if (k < rem) { *is = (long long)k * (q + 1); *ie = *is + q + 1; }
    else { *is = (long long)k * q + rem; *ie = *is + q; }
}

__global__ __launch_bounds__(THREADS)
void spmv_dns_t_kernel(int n, int np, int T, const double *__restrict__ value, const double *__restrict__ x, double *__restrict__ y)
{
    __shared__ double prod[2][TCOLS][TPAD];
    const int lane = (int)threadIdx.x % TSLAB, wv = (int)threadIdx.x / TSLAB;
    const long long j0 = (long long)blockIdx.x * TCOLS;
    const bool folds = (int)threadIdx.x < TCOLS;
    double total = 0.0;
    int b = 0;
    for (int k = 0; k < T; k++) {
        long long is, ie;
        chunk_rows(k, T, n, &is, &ie);
        double part = 0.0, v[TCPT] = {}, w[TCPT] = {}, xv = 0.0, xw = 0.0;
        if (is < ie) {
            const long long i = is + lane;
            const bool ok = i < ie;
            xv = ok ? x[i] : 0.0;
#pragma unroll
            for (int q = 0; q < TCPT; q++) {
                const long long j = j0 + wv + q * TWAVES;
                v[q] = (ok && j < np) ? load_stream(value + (size_t)j * (size_t)n + (size_t)i) : 0.0;
            }
        }
        for (long long i0 = is; i0 < ie; i0 += TSLAB) {
            if (i0 + TSLAB < ie) {
                const long long i = i0 + TSLAB + lane;
                const bool ok = i < ie;
                xw = ok ? x[i] : 0.0;
#pragma unroll
                for (int q = 0; q < TCPT; q++) {
                    const long long j = j0 + wv + q * TWAVES;
                    w[q] = (ok && j < np) ? load_stream(value + (size_t)j * (size_t)n + (size_t)i) : 0.0;
                }
            }
#pragma unroll
            for (int q = 0; q < TCPT; q++) prod[b][wv + q * TWAVES][lane] = v[q] * xv;
            __syncthreads();
            if (folds) {                               // one lane per column: the slab's terms in row order
                const int cnt = ie - i0 < TSLAB ? (int)(ie - i0) : TSLAB;
                if (cnt == TSLAB) {
#pragma unroll 16
                    for (int ii = 0; ii < TSLAB; ii++) part += prod[b][threadIdx.x][ii];
                } else for (int ii = 0; ii < cnt; ii++) part += prod[b][threadIdx.x][ii];
            }
            b ^= 1;
#pragma unroll
            for (int q = 0; q < TCPT; q++) v[q] = w[q];
            xv = xw;
        }
        total += part;                                 // (a chunk without rows adds +0.0, as the reference's zeroed w does)
    }
    if (folds && j0 + threadIdx.x < np) y[j0 + threadIdx.x] = total;
}

} // namespace

// {rows of y per workgroup, columns per slab} of the forward kernel, {entries of y per workgroup, rows per slab} of the transposed one
extern "C" int liship_dns_tile_info(int info[4])
{
    if (!info) return LISHIP_ERR_ARG;
    info[0] = ROWS; info[1] = SLAB; info[2] = TCOLS; info[3] = TSLAB;
    return 0;
}

extern "C" int liship_spmv_dns_f64(int n, int np, const double *value, const double *x, double *y, void *stream)
{
    if (n < 0 || np < 0) return LISHIP_ERR_ARG;
    if (n == 0) return 0;
    spmv_dns_kernel<<<(unsigned)(((long long)n + ROWS - 1) / ROWS), THREADS, 0, as_stream(stream)>>>(n, np, value, x, y);
    LAUNCH_CHECK();
    return 0;
}

extern "C" int liship_spmv_dns_t_f64(int n, int np, int T, const double *value, const double *x, double *y, void *stream)
{
    if (n < 0 || np < 0 || T < 1) return LISHIP_ERR_ARG;
    if (np == 0) return 0;
    spmv_dns_t_kernel<<<(unsigned)(((long long)np + TCOLS - 1) / TCOLS), THREADS, 0, as_stream(stream)>>>(n, np, T, value, x, y);
    LAUNCH_CHECK();
    return 0;
}
