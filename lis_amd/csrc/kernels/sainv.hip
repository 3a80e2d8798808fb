// sainv.hip -- preconditioners applied as products: SAINV (M^-1 = Z D^-1 W^T) and I+S (M^-1 = I - alpha S).
//
// Every application is a row sum over a packed CSR {ptr, index, value}: out[r] = epilogue(sum_k value[k] * x[index[k]]), the sum
// formed from +0.0 in STORED order by one lane -- the order of the reference's lis_matvech_ilu (lis_matrix_ilu.c:302-311) for the
// gather side, and, over the transposed form whose rows list their terms by source row, the order of the scatter loops of
// lis_matvec_ilu (:418-436) and lis_psolveh_is (lis_precon_is.c:505-524) at one thread.  With T > 1 (reference-order mode) the
// source rows fall into the T chunks of LIS_GET_ISIE; a chunk's terms are summed from +0.0 and the chunk sums are added in chunk
// order from +0.0, which is what the OpenMP build's per-thread buffers give.  A chunk without terms adds +0.0 to a sum that is
// never -0.0 (it started from +0.0): skipped.
//
// One workgroup owns BLOCK consecutive rows, whose entries are one contiguous run of the arrays.  The run is walked in tiles of
// STAGE entries: all lanes form the products of a tile with coalesced loads of value / index and park them in LDS, then every lane
// adds the part of ITS row that lies in the tile, left to right.  Tiles ascend and a row's entries ascend, so the order is the stored
// one whatever the row's length: a row of one entry and a row of 100 000 (the full inverse factor at drop 0) take the same path.
// The epilogues (the scale by d, x - alpha t, x - sum) run in the same kernel; no product is contracted into an add (-ffp-contract=off).
#include "common.hpp"
#include "liship.h"

namespace {

constexpr int BLOCK = 256;
constexpr int STAGE = 2048;            // products per tile: 16 KB of LDS, + 8 KB of source rows in the chunked form

enum { EPI_SCALE, EPI_PLAIN, EPI_IS, EPI_ISH };

template <int EPI, bool CHUNKED>
__global__ __launch_bounds__(BLOCK)
void rows_in_order(int n, const int *__restrict__ ptr, const int *__restrict__ idx, const double *__restrict__ val,
                   const double *__restrict__ x, const double *__restrict__ d, double alpha, int nsrc, int T,
                   double *__restrict__ y, const double *skip)
{
    __shared__ double prod[STAGE];
    __shared__ int src[CHUNKED ? STAGE : 1];
    if (skip && skip[0] != 0.0) return;
    const int tid = (int)threadIdx.x;
    const int r0 = (int)blockIdx.x * BLOCK, r = r0 + tid;
    const int rend = min(n, r0 + BLOCK);
    const int kb = ptr[r0], ke = ptr[rend];                    // the workgroup's run of entries (uniform)
    const int b = r < n ? ptr[r] : ke, e = r < n ? ptr[r + 1] : ke;
    const int q = CHUNKED ? nsrc / T : 0, rem = CHUNKED ? nsrc % T : 0;
    const long long big = (long long)rem * (q + 1);            // source rows below `big` lie in chunks of q + 1 rows
    double total = 0.0, part = 0.0;
    int chunk = 0;
    for (int t0 = kb; t0 < ke; t0 += STAGE) {
        const int t1 = min(ke, t0 + STAGE);
        for (int k = t0 + tid; k < t1; k += BLOCK) {
            const int j = idx[k];
            prod[k - t0] = val[k] * x[j];
            if (CHUNKED) src[k - t0] = j;
        }
        __syncthreads();
        const int lo = max(b, t0), hi = min(e, t1);
        for (int k = lo; k < hi; k++) {
            if (CHUNKED) {
                const int j = src[k - t0];
                const int kc = j < big ? j / (q + 1) : rem + (int)((j - big) / q);
                if (kc != chunk) { total += part; part = 0.0; chunk = kc; }
            }
            part += prod[k - t0];
        }
        __syncthreads();
    }
    if (r >= n) return;
    if (CHUNKED) { total += part; part = total; }
    if (EPI == EPI_SCALE) y[r] = part * d[r];
    else if (EPI == EPI_PLAIN) y[r] = part;
    else if (EPI == EPI_IS) y[r] = x[r] - alpha * part;
    else y[r] = x[r] - part;
}

// the first min(keep, length) entries of every row of U, packed at tptr; tavalue: alpha * value, the factor lis_psolveh_is forms first
__global__ __launch_bounds__(BLOCK)
void truncate_rows(int n, int keep, const int *__restrict__ uptr, const int *__restrict__ uidx, const double *__restrict__ uval,
                   const int *__restrict__ tptr, double alpha, int *__restrict__ tidx, double *__restrict__ tval, double *__restrict__ taval)
{
    const int r = blockIdx.x * BLOCK + threadIdx.x;
    if (r >= n) return;
    const int from = uptr[r], to = tptr[r];
    const int len = min(keep, uptr[r + 1] - from);
    for (int k = 0; k < len; k++) {
        const double v = uval[from + k];
        tidx[to + k] = uidx[from + k];
        tval[to + k] = v;
        taval[to + k] = alpha * v;
    }
}

template <int EPI>
int launch(int n, const int *ptr, const int *idx, const double *val, const double *x, const double *d, double alpha,
           int nsrc, int T, double *y, void *stream)
{
    if (n < 0 || nsrc < 0 || !ptr || !x || !y) return LISHIP_ERR_ARG;
    if (n == 0) return 0;
    const int grid = (n + BLOCK - 1) / BLOCK;
    if (T > 1) rows_in_order<EPI, true><<<grid, BLOCK, 0, as_stream(stream)>>>(n, ptr, idx, val, x, d, alpha, nsrc, T, y, liship_internal_guard());
    else rows_in_order<EPI, false><<<grid, BLOCK, 0, as_stream(stream)>>>(n, ptr, idx, val, x, d, alpha, nsrc, 1, y, liship_internal_guard());
    LAUNCH_CHECK();
    return 0;
}

} // namespace

// t[r] = (sum of row r of {ptr, idx, val} times b, stored order, from +0.0) * d[r]
extern "C" int liship_sainv_gather_scale_f64(int n, const int *ptr, const int *idx, const double *val, const double *d,
                                             const double *b, double *t, void *stream)
{
    if (!d) return LISHIP_ERR_ARG;
    return launch<EPI_SCALE>(n, ptr, idx, val, b, d, 0.0, n, 1, t, stream);
}

// x[c] = the terms of row c of the transposed form {tptr, tidx, tval} (by source row) times t, in T chunks of the nsrc source rows (T <= 1: one chain)
extern "C" int liship_sainv_rows_f64(int n, int nsrc, int T, const int *tptr, const int *tidx, const double *tval,
                                     const double *t, double *x, void *stream)
{
    return launch<EPI_PLAIN>(n, tptr, tidx, tval, t, nullptr, 0.0, nsrc, T, x, stream);
}

// y[r] = x[r] - alpha * (sum of row r of the truncated U times x); y must not be x
extern "C" int liship_is_psolve_f64(int n, const int *ptr, const int *idx, const double *val, double alpha,
                                    const double *x, double *y, void *stream)
{
    if (x == y) return LISHIP_ERR_ARG;
    return launch<EPI_IS>(n, ptr, idx, val, x, nullptr, alpha, n, 1, y, stream);
}

// y[c] = x[c] - (the terms (alpha u) x[source row] of column c, by source row, in T chunks); tval holds alpha * u; y must not be x
extern "C" int liship_is_psolveh_f64(int n, int nsrc, int T, const int *tptr, const int *tidx, const double *tval,
                                     const double *x, double *y, void *stream)
{
    if (x == y) return LISHIP_ERR_ARG;
    return launch<EPI_ISH>(n, tptr, tidx, tval, x, nullptr, 0.0, nsrc, T, y, stream);
}

// rows of U cut to their first `keep` entries at the row starts tptr (the prefix sums of min(keep, length)): index, value and alpha * value
extern "C" int liship_is_truncate_f64(int n, int keep, const int *uptr, const int *uidx, const double *uval, const int *tptr,
                                      double alpha, int *tidx, double *tval, double *taval, void *stream)
{
    if (n < 0 || keep < 0 || !uptr || !tptr) return LISHIP_ERR_ARG;
    if (n == 0) return 0;
    truncate_rows<<<(n + BLOCK - 1) / BLOCK, BLOCK, 0, as_stream(stream)>>>(n, keep, uptr, uidx, uval, tptr, alpha, tidx, tval, taval);
    LAUNCH_CHECK();
    return 0;
}
