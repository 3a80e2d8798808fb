// spgeam.hip -- A <- A - sigma B on two CSR matrices that live in HBM (lis_matrix_shift_matrix, host/lis_shift.c), for gfx950 (f64).
//
// The reference forms the difference through two dense n x n copies (src/matrix/lis_matrix_ops.c:833-856: csr -> dns, lis_matrix_axpy_dns,
// dns -> csr).  What that leaves in A, restated by tests/shift_model.py: every row holds the union of the two rows' columns in ascending
// order, every entry is (-sigma) * b + a -- an absent term counts as 0.0, the product and the sum are rounded once each
// (-ffp-contract=off) -- and an entry that comes out exactly 0.0 is dropped.  Here that is work per row on the sparse arrays:
//
//   liship_csr_shift_matrix_try_f64    ONE launch.  A row whose result keeps A's own layout -- its columns already ascending, every
//                                      surviving entry of B's row on a column A's row stores, no result exactly zero -- is updated where
//                                      it lies and marked done.  Any other row is left untouched, counted in *flag, and its result's
//                                      length is written to count[].  *flag == 0 after the launch: the shift is complete (the common
//                                      case of a stiffness and a mass matrix on one pattern).  Two rows that list the same columns in the
//                                      same order are taken entry against entry, without a search; a row of B inside A's is looked up
//                                      in A's by bisection.
//   liship_csr_shift_matrix_scan       the new row starts from count[] (the scan of convert.hip), the new nnz to the host
//   liship_csr_shift_matrix_fill_f64   the new index / value arrays: a row marked done is copied (it holds its result already), any
//                                      other row is merged
//
// One lane per row, as liship_csr_shift_diagonal_f64: rows are independent, a pencil's rows are short (7 to 81 entries for the stencils and
// element matrices the eigensolvers meet), and the lanes of a wavefront walk neighbouring rows, so the cache lines one step of the walk
// touches are the lines the next steps touch (the value and index streams cross HBM once).  Nothing is staged, so no row is too long for a
// stage: a row of any length takes the same walk.  Two rows that both list their columns in ascending order are merged by two cursors; when
// one of them does not, the walk picks the smallest column beyond the last one emitted by a scan over both rows -- quadratic in the rows'
// length, for the rare unsorted row, and ascending by construction.
//
// Bounds: the kernels read ptr[0 .. n] of both matrices and index / value inside [ptr[r], ptr[r + 1]); a column is only ever compared,
// never used as an address.  The fill writes row r at nptr[r] + k with k below the count the try kernel formed for the same row from the
// same arrays (a done row: its own length).
#include <limits.h>
#include "common.hpp"
#include "liship.h"

// convert.hip
int liship_internal_exclusive_scan(int m, const int *count, int *out, long long *scratch, void *stream);

namespace {

constexpr int BLOCK = LISHIP_SHIFT_MATRIX_ROWS;      // rows per workgroup
inline int grid_for(long long n) { return (int)((n + BLOCK - 1) / BLOCK); }

__device__ __forceinline__ bool ascending(const int *__restrict__ idx, int s, int e)
{
    bool up = true;
    for (int k = s + 1; k < e; k++) up &= idx[k] > idx[k - 1];
    return up;
}

// position of column c in the ascending row idx[s .. e), -1 when the row does not store it
__device__ __forceinline__ int find_column(const int *__restrict__ idx, int s, int e, int c)
{
    while (s < e) {
        const int m = s + ((e - s) >> 1);
        const int v = idx[m];
        if (v == c) return m;
        if (v < c) s = m + 1; else e = m;
    }
    return -1;
}

// the result row of A's row [a0, a1) and B's row [b0, b1): its length; with EMIT its entries to oidx / oval
template <bool EMIT>
__device__ __forceinline__ int merge_row(const int *__restrict__ aidx, const double *__restrict__ aval, int a0, int a1,
                                         const int *__restrict__ bidx, const double *__restrict__ bval, int b0, int b1,
                                         double msigma, int *__restrict__ oidx, double *__restrict__ oval)
{
    int kept = 0;
    if (ascending(aidx, a0, a1) && ascending(bidx, b0, b1)) {
        int i = a0, j = b0;
        while (i < a1 || j < b1) {
            const int ca = i < a1 ? aidx[i] : INT_MAX, cb = j < b1 ? bidx[j] : INT_MAX;
            const int c = ca < cb ? ca : cb;
            const double a = ca == c ? aval[i++] : 0.0, b = cb == c ? bval[j++] : 0.0;
            const double t = msigma * b;
            const double r = t + a;
            if (r != 0.0) {
                if (EMIT) { oidx[kept] = c; oval[kept] = r; }
                kept++;
            }
        }
        return kept;
    }
    for (int last = -1;;) {                          // the smallest column beyond `last` in either row, then the entry of each row that stores it
        int c = INT_MAX;
        for (int k = a0; k < a1; k++) { const int v = aidx[k]; if (v > last && v < c) c = v; }
        for (int k = b0; k < b1; k++) { const int v = bidx[k]; if (v > last && v < c) c = v; }
        if (c == INT_MAX) break;
        double a = 0.0, b = 0.0;
        for (int k = a0; k < a1; k++) if (aidx[k] == c) { a = aval[k]; break; }
        for (int k = b0; k < b1; k++) if (bidx[k] == c) { b = bval[k]; break; }
        const double t = msigma * b;
        const double r = t + a;
        if (r != 0.0) {
            if (EMIT) { oidx[kept] = c; oval[kept] = r; }
            kept++;
        }
        last = c;
    }
    return kept;
}

__global__ __launch_bounds__(BLOCK)
void shift_matrix_try(int n, const int *aptr, const int *aidx, double *aval, const int *bptr, const int *bidx, const double *bval, double msigma,
                      int *__restrict__ count, int *__restrict__ done, int *__restrict__ flag)
{                                                    // (B may be A itself -- A - sigma A --: no restrict on the matrices' arrays)
    const long long r = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (r >= n) return;
    const int a0 = aptr[r], a1 = aptr[r + 1], b0 = bptr[r], b1 = bptr[r + 1];
    // the two rows list the same columns in the same ascending order (a stiffness and a mass matrix on one pattern): entry k meets entry k, no search, and the
    // loads of a step depend on nothing but k
    if (a1 - a0 == b1 - b0) {
        bool same = true;
        int prev = -1;
        for (int k = 0; k < a1 - a0; k++) {
            const int c = aidx[a0 + k];
            const double t = msigma * bval[b0 + k];
            const double r1 = t + aval[a0 + k];
            same &= (c == bidx[b0 + k]) & (c > prev) & (r1 != 0.0);
            prev = c;
        }
        if (same) {
            for (int k = 0; k < a1 - a0; k++) { const double t = msigma * bval[b0 + k]; aval[a0 + k] = t + aval[a0 + k]; }
            count[r] = a1 - a0;
            done[r] = 1;
            return;
        }
    }
    // in place all the same?  A's row ascending; zeros: stored zeros of A that no entry of B lifts (they would be dropped)
    bool ok = true;
    int zeros = 0, prev = -1;
    for (int k = a0; k < a1; k++) {
        const int c = aidx[k];
        ok &= c > prev;
        prev = c;
        zeros += aval[k] == 0.0;
    }
    if (ok) {
        for (int k = b0; k < b1; k++) {
            const double t = msigma * bval[k];
            const int at = find_column(aidx, a0, a1, bidx[k]);
            if (at < 0) { const double r0 = t + 0.0; ok &= !(r0 != 0.0); }         // a column A's row lacks: fine only when its entry is dropped
            else { const double a = aval[at]; const double r1 = t + a; ok &= r1 != 0.0; zeros -= a == 0.0; }
        }
        ok &= zeros == 0;
    }
    if (ok) {
        for (int k = b0; k < b1; k++) {
            const int at = find_column(aidx, a0, a1, bidx[k]);
            if (at >= 0) { const double t = msigma * bval[k]; aval[at] = t + aval[at]; }
        }
        count[r] = a1 - a0;
        done[r] = 1;
        return;
    }
    count[r] = merge_row<false>(aidx, aval, a0, a1, bidx, bval, b0, b1, msigma, nullptr, nullptr);
    done[r] = 0;
    atomicAdd(flag, 1);
}

__global__ __launch_bounds__(BLOCK)
void shift_matrix_fill(int n, const int *__restrict__ aptr, const int *__restrict__ aidx, const double *__restrict__ aval,
                       const int *__restrict__ bptr, const int *__restrict__ bidx, const double *__restrict__ bval, double msigma,
                       const int *__restrict__ done, const int *__restrict__ nptr, int *__restrict__ nidx, double *__restrict__ nval)
{
    const long long r = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (r >= n) return;
    const int a0 = aptr[r], a1 = aptr[r + 1], o = nptr[r];
    if (done[r]) {
        for (int k = a0; k < a1; k++) { nidx[o + k - a0] = aidx[k]; nval[o + k - a0] = aval[k]; }
        return;
    }
    (void)merge_row<true>(aidx, aval, a0, a1, bidx, bval, bptr[r], bptr[r + 1], msigma, nidx + o, nval + o);
}

} // namespace

extern "C" int liship_csr_shift_matrix_try_f64(int n, const int *aptr, const int *aindex, double *avalue, const int *bptr, const int *bindex,
                                               const double *bvalue, double sigma, int *count, int *done, int *flag, void *stream)
{
    if (n < 0 || !flag || (n > 0 && (!aptr || !bptr || !count || !done))) return LISHIP_ERR_ARG;   // (index / value may be NULL when no row has an entry: never read then)
    hipStream_t st = as_stream(stream);
    HIP_TRY(hipMemsetAsync(flag, 0, sizeof(int), st));
    if (n == 0) return 0;
    shift_matrix_try<<<grid_for(n), BLOCK, 0, st>>>(n, aptr, aindex, avalue, bptr, bindex, bvalue, -sigma, count, done, flag);
    LAUNCH_CHECK();
    return 0;
}

extern "C" int liship_csr_shift_matrix_scan(int n, const int *count, int *nptr, long long *scratch, int *nnz, void *stream)
{
    if (n < 0 || !nptr || !nnz || (n > 0 && (!count || !scratch))) return LISHIP_ERR_ARG;
    hipStream_t st = as_stream(stream);
    const int rc = liship_internal_exclusive_scan(n, count, nptr, scratch, stream);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(nnz, nptr + n, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

extern "C" int liship_csr_shift_matrix_fill_f64(int n, const int *aptr, const int *aindex, const double *avalue, const int *bptr, const int *bindex,
                                                const double *bvalue, double sigma, const int *done, const int *nptr, int *nindex, double *nvalue, void *stream)
{
    if (n < 0 || (n > 0 && (!aptr || !bptr || !done || !nptr))) return LISHIP_ERR_ARG;
    if (n == 0) return 0;
    shift_matrix_fill<<<grid_for(n), BLOCK, 0, as_stream(stream)>>>(n, aptr, aindex, avalue, bptr, bindex, bvalue, -sigma, done, nptr, nindex, nvalue);
    LAUNCH_CHECK();
    return 0;
}
