// bdiag.hip -- the block diagonal of a BSR matrix as a preconditioner (-p bjacobi, lis_bjacobi.c): nr blocks of bn x bn doubles,
// block b at d[b*bn*bn ..], column-major (entry (i, j) at i + j*bn), the layout of LIS_MATRIX_DIAG.
//
// bdiag_inverse_kernel: every block replaced by its inverse, one lane per block.  It restates lis_array_ge (ref
// src/array/lis_array.c:907-956) operation for operation: LU without pivoting on a copy `lu` (the pivot's reciprocal kept on the
// diagonal, t = lu[i+k*n] * lu[k+k*n], lu[i+j*n] -= t * lu[k+j*n]), then per column k the forward substitution from (i == k) with
// j ascending and the backward substitution with i descending, j ascending from i + 1, ending t * lu[i+i*n] -- both IN PLACE in the
// block, which is read and overwritten in the reference's order.  Every product and every subtraction is rounded on its own
// (-ffp-contract=off); a zero pivot gives 1 / 0 = inf and goes on as it does there.  Before that the last block of a matrix whose
// n is no multiple of bn gets 1.0 on the diagonal of its padding (ref lis_matrix_diag.c:787-794).
//   bn = 1: 1.0 / d.  bn = 2 .. 8: compile-time sizes, block and lu in registers.  Larger bn: the block stays in HBM and lu lives in
//   a work array of bn*bn doubles per block, entry e of block b at work[e*nr + b] (consecutive lanes, consecutive addresses).
// One lane reads bn*bn consecutive doubles: the wavefront uses every byte of the lines it touches, through L2 -- the inverse runs
// once per lis_precon_create, not per iteration.
//
// bdiag_matvec_kernel<TRANSPOSED>: y = D x (ref lis_matrix_diag_matvec, lis_matrix_diag.c:810-895) or y = D^T x block by block
// (lis_matrix_diag_matvech -> lis_array_matvech, lis_array.c:532-569), one lane per row, summed left to right over j.  The sum
// starts with the first product where the reference writes the row as one expression (plain: bn <= 4, transposed: bn <= 3) and at
// +0.0 where it runs a loop from t = 0.0: the two differ in the sign of a zero.  Entries of x at or beyond n (the padding of the last
// block) are +0.0, rows at or beyond n are not written.  Plain form: term j of lane i reads d[b*bs + i + j*bn], consecutive lanes
// consecutive addresses.  Transposed form: d[b*bs + i*bn + j], stride bn between lanes -- the bn terms of the 64 lanes cover
// whole lines, each line fetched once from HBM and served from L1 / L2 for the other terms.
#include "block_ops.hpp"
#include "liship.h"

namespace {

constexpr int BD_THREADS = 256;
constexpr int BD_MAX_FIXED = 8;       // block sizes with a compile-time instantiation of the inverse

struct StridedRef {
    double *p; size_t stride;
    __device__ __forceinline__ double &operator()(int e) const { return p[(size_t)e * stride]; }
};

__device__ __forceinline__ void pad_last_block(int n, int nr, int bn, int b, double *blk)
{
    const int k = n % bn;
    if (k != 0 && b == nr - 1)
        for (int i = bn - 1; i >= k; i--) blk[i * (bn + 1)] = 1.0;
}

template <int BN>
__global__ __launch_bounds__(BD_THREADS) void bdiag_inverse_kernel(int n, int nr, double *d)
{
    const int b = blockIdx.x * BD_THREADS + threadIdx.x;
    if (b >= nr) return;
    double *blk = d + (size_t)b * (BN * BN);
    if (BN == 1) { blk[0] = 1.0 / blk[0]; return; }
    double a[BN * BN], lu[BN * BN];
#pragma unroll
    for (int e = 0; e < BN * BN; e++) a[e] = blk[e];
    pad_last_block<BN>(n, nr, b, a);
    invert_block(BN, RegRef{a}, RegRef{lu});
#pragma unroll
    for (int e = 0; e < BN * BN; e++) blk[e] = a[e];
}

__global__ __launch_bounds__(BD_THREADS) void bdiag_inverse_generic_kernel(int n, int nr, int bn, double *d, double *work)
{
    const int b = blockIdx.x * BD_THREADS + threadIdx.x;
    if (b >= nr) return;
    double *blk = d + (size_t)b * bn * bn;
    pad_last_block(n, nr, bn, b, blk);
    invert_block(bn, RegRef{blk}, StridedRef{work + b, (size_t)nr});
}

// BN > 0: the block size at compile time; BN == 0: any block size from the argument (the loop form of the reference, from +0.0)
template <int BN, bool TRANSPOSED>
__global__ __launch_bounds__(BD_THREADS) void bdiag_matvec_kernel(int n, int bn_arg, const double *__restrict__ d, const double *__restrict__ x, double *__restrict__ y)
{
    const int bn = BN > 0 ? BN : bn_arg;
    const int r = blockIdx.x * BD_THREADS + threadIdx.x;
    if (r >= n) return;
    const int b = r / bn, i = r - b * bn;
    const double *blk = d + (size_t)b * bn * bn;
    const int x0 = b * bn;
    const bool from_zero = BN == 0 || BN > (TRANSPOSED ? 3 : 4);
    double t = 0.0;
#pragma unroll
    for (int j = 0; j < bn; j++) {
        const double xv = x0 + j < n ? x[x0 + j] : 0.0;
        const double p = (TRANSPOSED ? blk[i * bn + j] : blk[i + j * bn]) * xv;
        t = (j == 0 && !from_zero) ? p : t + p;
    }
    y[r] = t;
}

template <bool TRANSPOSED>
int launch_matvec(int n, int bn, const double *d, const double *x, double *y, hipStream_t s)
{
    const dim3 grid((unsigned)((n + BD_THREADS - 1) / BD_THREADS)), block(BD_THREADS);
    switch (bn) {
#define BD_CASE(K) case K: hipLaunchKernelGGL((bdiag_matvec_kernel<K, TRANSPOSED>), grid, block, 0, s, n, bn, d, x, y); break;
    BD_CASE(1) BD_CASE(2) BD_CASE(3) BD_CASE(4) BD_CASE(5) BD_CASE(6) BD_CASE(7) BD_CASE(8)
#undef BD_CASE
    default: hipLaunchKernelGGL((bdiag_matvec_kernel<0, TRANSPOSED>), grid, block, 0, s, n, bn, d, x, y); break;
    }
    LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" int liship_bdiag_inverse_f64(int n, int nr, int bn, double *d, double *work, void *stream)
{
    if (n < 0 || nr < 0 || bn < 1 || (long long)nr != ((long long)n + bn - 1) / bn) return LISHIP_ERR_ARG;
    if (nr == 0) return 0;
    if (!d || (bn > BD_MAX_FIXED && !work)) return LISHIP_ERR_ARG;
    const dim3 grid((unsigned)((nr + BD_THREADS - 1) / BD_THREADS)), block(BD_THREADS);
    hipStream_t s = as_stream(stream);
    switch (bn) {
#define BD_CASE(K) case K: hipLaunchKernelGGL(bdiag_inverse_kernel<K>, grid, block, 0, s, n, nr, d); break;
    BD_CASE(1) BD_CASE(2) BD_CASE(3) BD_CASE(4) BD_CASE(5) BD_CASE(6) BD_CASE(7) BD_CASE(8)
#undef BD_CASE
    default: hipLaunchKernelGGL(bdiag_inverse_generic_kernel, grid, block, 0, s, n, nr, bn, d, work); break;
    }
    LAUNCH_CHECK();
    return 0;
}

extern "C" int liship_bdiag_matvec_f64(int n, int nr, int bn, int transposed, const double *d, const double *x, double *y, void *stream)
{
    if (n < 0 || nr < 0 || bn < 1 || (long long)nr != ((long long)n + bn - 1) / bn) return LISHIP_ERR_ARG;
    if (n == 0) return 0;
    if (!d || !x || !y || x == y) return LISHIP_ERR_ARG;
    return transposed ? launch_matvec<true>(n, bn, d, x, y, as_stream(stream)) : launch_matvec<false>(n, bn, d, x, y, as_stream(stream));
}
