// vbr.hip -- y = A x for variable-block (LIS_MATRIX_VBR) storage, on the matrix's own six arrays.
//
// The reference (src/matvec/lis_matvec_vbr.c:117-142): y = 0, then for block row bi, for its blocks bc = bptr[bi] .. bptr[bi+1] in stored order, for the
// block's columns j = col[bj] .. col[bj+1] (bj = bindex[bc]), for its rows i = row[bi] .. row[bi+1]:  y[i] += value[k++] * x[j], k from ptr[bc].  The OpenMP
// build splits the BLOCK ROWS, so row i's sum is the same chain at every thread count: from +0.0, blocks in stored order, a block's columns ascending,
// every product rounded before it is added (-ffp-contract=off), explicit zeros multiplied too.
//
// One lane per row.  brow[i] (made once per matrix by liship_vbr_block_rows) names the row's block row; the lanes of one block row then read the SAME
// bptr / bindex / ptr / col entries (one address per wavefront instruction: a broadcast out of L1) and the same x[j], and CONSECUTIVE addresses of value[]
// (ptr[bc] + (j - col[bj]) * bnr + ii: blocks are column-major), so a block row of 64 rows and more streams value[] in whole 512 B lines like the dense
// kernel's forward access, and a matrix of 1 x 1 blocks runs as a lane-per-row CSR product does.  The loads of UNROLL columns are issued before the first of
// their adds; the adds stay one chain.  No LDS, no cross-lane step: a row never waits for another, and rows of short block rows pack into wavefronts as they
// come.  What this shape does not do: split a long row (one block of n x n runs n / 64 wavefronts, each a chain of n terms) -- dns.hip's slab form does,
// and a dense matrix belongs in DNS storage.
//
// liship_vbr_check runs before the first product of a matrix: no product is launched on arrays that could send a lane out of bounds.
#include "common.hpp"
#include "liship.h"

namespace {

constexpr int THREADS = 256;                  // rows of y per workgroup
constexpr int UNROLL = 4;                     // columns of a block whose value loads are in flight before the first add

__global__ __launch_bounds__(THREADS)
void spmv_vbr_kernel(int n, const int *__restrict__ row, const int *__restrict__ col, const int *__restrict__ ptr, const int *__restrict__ bptr,
                     const int *__restrict__ bindex, const int *__restrict__ brow, const double *__restrict__ value, const double *__restrict__ x,
                     double *__restrict__ y)
{
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    const int bi = brow[i];
    const int r0 = row[bi];
    const size_t bnr = (size_t)(row[bi + 1] - r0);
    const int ii = (int)i - r0;
    double t = 0.0;
    const int bend = bptr[bi + 1];
    for (int bc = bptr[bi]; bc < bend; bc++) {
        const int bj = bindex[bc];
        int j = col[bj];
        const int jend = col[bj + 1];
        const double *v = value + (size_t)ptr[bc] + (size_t)ii;
        for (; j + UNROLL <= jend; j += UNROLL, v += UNROLL * bnr) {
            double a[UNROLL], b[UNROLL];
#pragma unroll
            for (int q = 0; q < UNROLL; q++) { a[q] = load_stream(v + q * bnr); b[q] = x[j + q]; }
#pragma unroll
            for (int q = 0; q < UNROLL; q++) t += a[q] * b[q];
        }
        for (; j < jend; j++, v += bnr) t += load_stream(v) * x[j];
    }
    store_stream(y + i, t);
}

// brow[i] = the block row of row i: one lane per block row writes its rows.  Only after liship_vbr_check: row[] ascends from 0 to n.
__global__ __launch_bounds__(THREADS)
void vbr_block_rows_kernel(int n, int nr, const int *__restrict__ row, int *__restrict__ brow)
{
    const long long bi = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (bi >= nr) return;
    int lo = row[bi], hi = row[bi + 1];
    if (lo < 0) lo = 0;
    if (hi > n) hi = n;
    for (int i = lo; i < hi; i++) brow[i] = (int)bi;
}

// Bits of *flags (LISHIP_VBR_BAD_*): every lane guards its own reads, so the kernel itself stays inside the arrays whatever they hold.
__global__ __launch_bounds__(THREADS)
void vbr_check_kernel(int n, int np, int nnz, int nr, int nc, int bnnz, const int *__restrict__ row, const int *__restrict__ col,
                      const int *__restrict__ ptr, const int *__restrict__ bptr, const int *__restrict__ bindex, int *flags)
{
    const long long k = (long long)blockIdx.x * THREADS + threadIdx.x;
    int bad = 0;
    if (k < nr) {
        if (row[k + 1] <= row[k]) bad |= LISHIP_VBR_BAD_ROW;
        if (k == 0 && row[0] != 0) bad |= LISHIP_VBR_BAD_ROW;
        if (k == nr - 1 && row[nr] != n) bad |= LISHIP_VBR_BAD_ROW;
        const int b0 = bptr[k], b1 = bptr[k + 1];
        if (b1 < b0) bad |= LISHIP_VBR_BAD_BPTR;
        if (k == 0 && b0 != 0) bad |= LISHIP_VBR_BAD_BPTR;
        if (k == nr - 1 && b1 != bnnz) bad |= LISHIP_VBR_BAD_BPTR;
        // the sizes of this block row's blocks, where bptr lets the lane reach them
        if (b0 >= 0 && b1 <= bnnz) {
            const long long bnr = (long long)row[k + 1] - row[k];
            for (int bc = b0; bc < b1; bc++) {
                const int bj = bindex[bc];
                if (bj < 0 || bj >= nc) continue;                              // (reported by the lane of bc below)
                if ((long long)ptr[bc + 1] - ptr[bc] != bnr * ((long long)col[bj + 1] - col[bj])) bad |= LISHIP_VBR_BAD_SIZE;
            }
        }
    }
    if (k < nc) {
        if (col[k + 1] <= col[k]) bad |= LISHIP_VBR_BAD_COL;
        if (k == 0 && col[0] != 0) bad |= LISHIP_VBR_BAD_COL;
        if (k == nc - 1 && col[nc] != np) bad |= LISHIP_VBR_BAD_COL;
    }
    if (k < bnnz) {
        if (ptr[k + 1] < ptr[k]) bad |= LISHIP_VBR_BAD_PTR;
        if (k == 0 && ptr[0] < 0) bad |= LISHIP_VBR_BAD_PTR;
        if (k == bnnz - 1 && ptr[bnnz] > nnz) bad |= LISHIP_VBR_BAD_PTR;
        if (bindex[k] < 0 || bindex[k] >= nc) bad |= LISHIP_VBR_BAD_BINDEX;
    }
    if (bad) atomicOr(flags, bad);
}

// lis_matrix_shift_diagonal on the copy's value[]: one lane per block row runs the reference's search for the diagonal block (src/matrix/lis_matrix_vbr.c:969-989:
// i >= bjj*bnc && i < (bjj+1)*bnc, right on uniform blocks only) and shifts the entries it finds -- the host routine's walk (lisi_vbr_diagonal_walk), entry for entry
__global__ __launch_bounds__(THREADS)
void vbr_shift_kernel(int n, int nr, const int *__restrict__ row, const int *__restrict__ col, const int *__restrict__ ptr, const int *__restrict__ bptr,
                      const int *__restrict__ bindex, double *__restrict__ value, double sigma)
{
    const long long bi = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (bi >= nr) return;
    int k = 0, i = row[bi];
    const int bnr = row[bi + 1] - row[bi];
    for (int bc = bptr[bi]; bc < bptr[bi + 1]; bc++) {
        const int bjj = bindex[bc], bnc = col[bjj + 1] - col[bjj];
        if (i >= (long long)bjj * bnc && i < ((long long)bjj + 1) * bnc)
            for (int j = i % bnc; j < bnc && k < bnr && i < n; j++) {
                value[(size_t)ptr[bc] + (size_t)j * (size_t)bnr + (size_t)k] -= sigma;
                i++; k++;
            }
        if (k == bnr) break;
    }
}

// lis_matrix_scale on the copy's value[]: one lane per row, one rounding per factor -- value*d[i] (Jacobi), value*d[i]*d[j] in that order (symmetric), as
// lis_matrix_scale_vbr / _scale_symm_vbr write them (:1055-1069, :1097-1111)
__global__ __launch_bounds__(THREADS)
void vbr_scale_kernel(int n, const int *__restrict__ row, const int *__restrict__ col, const int *__restrict__ ptr, const int *__restrict__ bptr,
                      const int *__restrict__ bindex, const int *__restrict__ brow, double *__restrict__ value, const double *__restrict__ d, int symm)
{
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    const int bi = brow[i];
    const int r0 = row[bi];
    const size_t bnr = (size_t)(row[bi + 1] - r0);
    const double di = d[i];
    for (int bc = bptr[bi]; bc < bptr[bi + 1]; bc++) {
        const int bj = bindex[bc];
        double *v = value + (size_t)ptr[bc] + (size_t)((int)i - r0);
        for (int j = col[bj]; j < col[bj + 1]; j++, v += bnr) *v = symm ? *v * di * d[j] : *v * di;
    }
}

inline unsigned grid_for(long long count) { return (unsigned)((count + THREADS - 1) / THREADS); }

} // namespace

// {rows of y per workgroup, columns of a block loaded ahead of their adds}
extern "C" int liship_vbr_tile_info(int info[2])
{
    if (!info) return LISHIP_ERR_ARG;
    info[0] = THREADS; info[1] = UNROLL;
    return 0;
}

// *flags_host = 0 when the six arrays describe a VBR matrix of n rows, np columns and nnz stored values, else the LISHIP_VBR_BAD_* bits.  Synchronizes the stream.
extern "C" int liship_vbr_check(int n, int np, int nnz, int nr, int nc, int bnnz, const int *row, const int *col, const int *ptr, const int *bptr,
                                const int *bindex, int *flags_host, void *stream)
{
    if (!flags_host) return LISHIP_ERR_ARG;
    *flags_host = 0;
    if (n < 0 || np < 0 || nnz < 0 || bnnz < 0) return LISHIP_ERR_ARG;
    if (nr < 1 || nr > n || nc < 1 || nc > np) { *flags_host = (nr < 1 || nr > n ? LISHIP_VBR_BAD_ROW : 0) | (nc < 1 || nc > np ? LISHIP_VBR_BAD_COL : 0); return 0; }
    int *flags = nullptr;
    HIP_TRY(hipMalloc(&flags, sizeof(int)));
    hipError_t e = hipMemsetAsync(flags, 0, sizeof(int), as_stream(stream));
    if (e == hipSuccess) {
        long long lanes = nr > nc ? nr : nc;
        if (bnnz > lanes) lanes = bnnz;
        vbr_check_kernel<<<grid_for(lanes), THREADS, 0, as_stream(stream)>>>(n, np, nnz, nr, nc, bnnz, row, col, ptr, bptr, bindex, flags);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(flags_host, flags, sizeof(int), hipMemcpyDeviceToHost, as_stream(stream));
    if (e == hipSuccess) e = hipStreamSynchronize(as_stream(stream));
    (void)hipFree(flags);
    return e == hipSuccess ? 0 : (int)e;
}

// brow: n ints.  row[] must have passed liship_vbr_check.
extern "C" int liship_vbr_block_rows(int n, int nr, const int *row, int *brow, void *stream)
{
    if (n < 0 || nr < 0) return LISHIP_ERR_ARG;
    if (n == 0 || nr == 0) return 0;
    vbr_block_rows_kernel<<<grid_for(nr), THREADS, 0, as_stream(stream)>>>(n, nr, row, brow);
    LAUNCH_CHECK();
    return 0;
}

extern "C" int liship_spmv_vbr_f64(int n, const int *row, const int *col, const int *ptr, const int *bptr, const int *bindex, const int *brow,
                                   const double *value, const double *x, double *y, void *stream)
{
    if (n < 0) return LISHIP_ERR_ARG;
    if (n == 0) return 0;
    spmv_vbr_kernel<<<grid_for(n), THREADS, 0, as_stream(stream)>>>(n, row, col, ptr, bptr, bindex, brow, value, x, y);
    LAUNCH_CHECK();
    return 0;
}

// value[] of a checked VBR copy edited in place: A <- A - sigma I by the reference's search, and the two scalings by d[] (n doubles; np = n)
extern "C" int liship_vbr_shift_diagonal_f64(int n, int nr, const int *row, const int *col, const int *ptr, const int *bptr, const int *bindex, double *value,
                                             double sigma, void *stream)
{
    if (n < 0 || nr < 0) return LISHIP_ERR_ARG;
    if (n == 0 || nr == 0) return 0;
    vbr_shift_kernel<<<grid_for(nr), THREADS, 0, as_stream(stream)>>>(n, nr, row, col, ptr, bptr, bindex, value, sigma);
    LAUNCH_CHECK();
    return 0;
}

extern "C" int liship_vbr_scale_f64(int n, const int *row, const int *col, const int *ptr, const int *bptr, const int *bindex, const int *brow, double *value,
                                    const double *d, int symm, void *stream)
{
    if (n < 0) return LISHIP_ERR_ARG;
    if (n == 0) return 0;
    vbr_scale_kernel<<<grid_for(n), THREADS, 0, as_stream(stream)>>>(n, row, col, ptr, bptr, bindex, brow, value, d, symm);
    LAUNCH_CHECK();
    return 0;
}
