// sptrsv.hip -- level-scheduled sparse triangular sweeps for the SSOR and ILU(k) preconditioners (lis_ssor.c, lis_ilu.c).
//
// A sweep is a list of levels; the rows of one level do not depend on each other, every row depends only on rows of earlier
// levels.  The schedule (lis_ssor.c) stores the rows of each level and their terms contiguously in level order: rows[] the
// row ids, rptr[] the term offsets of the level-ordered rows, col[] / val[] the terms in the order the reference adds them.
// Inside a level the rows shorter than LISHIP_SWEEP_LONG_ROW come first, the long ones last (lptr[l] .. llong[l] .. lptr[l + 1]).
//
// Every row is ONE strictly ordered chain of additions with the reference's roundings (lis_matrix_csr.c:1572-1627 and
// :1804-1855), no tree anywhere; the Makefile's -ffp-contract=off keeps every product rounded on its own:
//   MUL   acc = b[i];  acc -= v * x[j] ...;           x[i] = acc * wd[i]     forward SSOR, LOWER / UPPER, the second psolveh sweep
//   SUB   acc = 0.0;   acc += v * x[j] ...;           x[i] -= acc * wd[i]    backward SSOR
//   SCAT  acc = b[i];  acc -= v * (x[j] * wd[j]) ...; x[i] = acc             first psolveh sweep (the transposed scatter of t = x[j] * wd[j])
//   PLAIN acc = b[i];  acc -= v * x[j] ...;           x[i] = acc             ILU: forward on L, backward on L^T (no diagonal, wd unread)
// A row reads its own b[i] before it writes x[i], and no other row's b: b and x may be the same vector.
//
// Dependencies between levels are kernel boundaries on the stream, or __syncthreads() inside the single-workgroup kernel
// that runs a run of small levels (all of it on one CU, whose vector L1 the workgroup's waves share: no data crosses a CU).
// No workgroup ever waits on a flag another workgroup writes.
#include "common.hpp"
#include "liship.h"

namespace {

constexpr int LEVEL_BLOCK = 256;        // one level per launch: a thread per short row, a workgroup per long row
constexpr int RUN_BLOCK = 1024;         // a run of small levels: one workgroup

struct Sweep {
    const int *lptr, *llong, *rows, *rptr, *col;
    const double *val, *b, *wd;
    double *x;
};

template <int MODE>
__device__ __forceinline__ double row_start(const Sweep &s, int i)
{
    if (MODE == LISHIP_SWEEP_SUB) return 0.0;
    return s.b[i];
}

template <int MODE>
__device__ __forceinline__ double term(const Sweep &s, int k)
{
    const int j = s.col[k];
    if (MODE == LISHIP_SWEEP_SCAT) { const double t = s.x[j] * s.wd[j]; return s.val[k] * t; }
    return s.val[k] * s.x[j];
}

template <int MODE>
__device__ __forceinline__ double combine(double acc, double p)
{
    if (MODE == LISHIP_SWEEP_SUB) return acc + p;
    return acc - p;
}

template <int MODE>
__device__ __forceinline__ void row_finish(const Sweep &s, int i, double acc)
{
    if (MODE == LISHIP_SWEEP_MUL) s.x[i] = acc * s.wd[i];
    else if (MODE == LISHIP_SWEEP_SUB) { const double t = acc * s.wd[i]; s.x[i] = s.x[i] - t; }
    else s.x[i] = acc;
}

// one short row, one lane, in order
template <int MODE>
__device__ __forceinline__ void short_row(const Sweep &s, int r)
{
    const int i = s.rows[r];
    double acc = row_start<MODE>(s, i);
    const int k1 = s.rptr[r + 1];
    for (int k = s.rptr[r]; k < k1; k++) acc = combine<MODE>(acc, term<MODE>(s, k));
    row_finish<MODE>(s, i, acc);
}

// one long row, the whole workgroup: the products of BS terms at once into LDS (loads wide), then thread 0 adds them in order.
// Every thread of the workgroup calls it: the trip count is uniform.
template <int MODE, int BS>
__device__ __forceinline__ void long_row(const Sweep &s, int r, double *prod)
{
    const int i = s.rows[r];
    const int k0 = s.rptr[r], k1 = s.rptr[r + 1];
    double acc = 0.0;
    if (threadIdx.x == 0) acc = row_start<MODE>(s, i);
    for (int kb = k0; kb < k1; kb += BS) {
        const int k = kb + (int)threadIdx.x;
        if (k < k1) prod[threadIdx.x] = term<MODE>(s, k);
        __syncthreads();
        if (threadIdx.x == 0) {
            const int cnt = min(BS, k1 - kb);
            for (int u = 0; u < cnt; u++) acc = combine<MODE>(acc, prod[u]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) row_finish<MODE>(s, i, acc);
}

// one level: blocks [0, nshort_blocks) take a short row per thread, each further block one long row
template <int MODE>
__global__ __launch_bounds__(LEVEL_BLOCK) void sweep_level(Sweep s, int level, int nshort_blocks)
{
    __shared__ double prod[LEVEL_BLOCK];
    const int r0 = s.lptr[level], rl = s.llong[level];
    if ((int)blockIdx.x < nshort_blocks) {
        const int r = r0 + (int)blockIdx.x * LEVEL_BLOCK + (int)threadIdx.x;
        if (r < rl) short_row<MODE>(s, r);
    } else {
        long_row<MODE, LEVEL_BLOCK>(s, rl + (int)blockIdx.x - nshort_blocks, prod);
    }
}

// levels [l0, l1) in one workgroup, a barrier between consecutive levels
template <int MODE>
__global__ __launch_bounds__(RUN_BLOCK) void sweep_run(Sweep s, int l0, int l1)
{
    __shared__ double prod[RUN_BLOCK];
    for (int l = l0; l < l1; l++) {
        const int r0 = s.lptr[l], rl = s.llong[l], r1 = s.lptr[l + 1];
        for (int r = r0 + (int)threadIdx.x; r < rl; r += RUN_BLOCK) short_row<MODE>(s, r);
        for (int r = rl; r < r1; r++) long_row<MODE, RUN_BLOCK>(s, r, prod);
        __syncthreads();
    }
}

template <int MODE>
int run_sweep(const liship_sweep_t *sw, const double *b, double *x, const double *wd, hipStream_t st)
{
    const Sweep s{sw->lptr, sw->llong, sw->rows, sw->rptr, sw->col, sw->val, b, wd, x};
    for (int g = 0; g < sw->ngroups; g++) {
        const int l0 = sw->groups[3 * g], l1 = sw->groups[3 * g + 1], run = sw->groups[3 * g + 2];
        if (run) {
            sweep_run<MODE><<<1, RUN_BLOCK, 0, st>>>(s, l0, l1);
        } else {
            const int nshort = sw->h_nshort[l0];
            const int nsb = (nshort + LEVEL_BLOCK - 1) / LEVEL_BLOCK;
            const int grid = nsb + (sw->h_nrows[l0] - nshort);
            sweep_level<MODE><<<grid, LEVEL_BLOCK, 0, st>>>(s, l0, nsb);
        }
        LAUNCH_CHECK();
    }
    return 0;
}

}  // namespace

extern "C" int liship_sweep_plain_f64(const liship_sweep_t *sw, const double *b, double *x, void *stream)
{
    if (!sw || !x || !b) return LISHIP_ERR_ARG;
    return run_sweep<LISHIP_SWEEP_PLAIN>(sw, b, x, nullptr, as_stream(stream));
}

extern "C" int liship_sweep_f64(const liship_sweep_t *sw, int mode, const double *b, double *x, const double *wd, void *stream)
{
    if (!sw || !x || !wd || mode < LISHIP_SWEEP_MUL || mode > LISHIP_SWEEP_SCAT || (mode != LISHIP_SWEEP_SUB && !b)) return LISHIP_ERR_ARG;
    hipStream_t st = as_stream(stream);
    switch (mode) {
    case LISHIP_SWEEP_MUL: return run_sweep<LISHIP_SWEEP_MUL>(sw, b, x, wd, st);
    case LISHIP_SWEEP_SUB: return run_sweep<LISHIP_SWEEP_SUB>(sw, b, x, wd, st);
    default:               return run_sweep<LISHIP_SWEEP_SCAT>(sw, b, x, wd, st);
    }
}
