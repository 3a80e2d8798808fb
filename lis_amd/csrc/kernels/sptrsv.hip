// sptrsv.hip -- level-scheduled sparse triangular sweeps for the SSOR and ILU(k) preconditioners (lis_ssor.c, lis_ilu.c).
//
// The schedule (lis_sweep.c; walked by level_schedule.hpp) stores the rows of each level and their terms contiguously in level
// order: rows[] the row ids, rptr[] the term offsets of the level-ordered rows, col[] / val[] the terms in the order the reference
// adds them.  Inside a level the rows shorter than LISHIP_SWEEP_LONG_ROW come first, the long ones last.
//
// Every row is ONE strictly ordered chain of additions with the reference's roundings (lis_matrix_csr.c:1572-1627 and
// :1804-1855), no tree anywhere; the Makefile's -ffp-contract=off keeps every product rounded on its own:
//   MUL   acc = b[i];  acc -= v * x[j] ...;           x[i] = acc * wd[i]     forward SSOR, LOWER / UPPER, the second psolveh sweep
//   SUB   acc = 0.0;   acc += v * x[j] ...;           x[i] -= acc * wd[i]    backward SSOR
//   SCAT  acc = b[i];  acc -= v * (x[j] * wd[j]) ...; x[i] = acc             first psolveh sweep (the transposed scatter of t = x[j] * wd[j])
//   PLAIN acc = b[i];  acc -= v * x[j] ...;           x[i] = acc             ILU: forward on L, backward on L^T (no diagonal, wd unread)
// A row reads its own b[i] before it writes x[i], and no other row's b: b and x may be the same vector.
#include "level_schedule.hpp"

namespace {

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

// the rows of a sweep in mode MODE (level_schedule.hpp)
template <int MODE>
struct SweepRows {
    Sweep s;
    __device__ __forceinline__ const int *level_ptr() const { return s.lptr; }
    __device__ __forceinline__ const int *level_long() const { return s.llong; }

    // one short row, one lane, in order
    __device__ __forceinline__ void short_row(int r) const
    {
        const int i = s.rows[r];
        double acc = row_start<MODE>(s, i);
        const int k1 = s.rptr[r + 1];
        for (int k = s.rptr[r]; k < k1; k++) acc = combine<MODE>(acc, term<MODE>(s, k));
        row_finish<MODE>(s, i, acc);
    }

    // one long row, the whole workgroup: the products of BS terms at once into LDS (loads wide), then thread 0 adds them in order.
    // The trip count is uniform, and the row ends on a barrier: the next one may reuse prod[].
    template <int BS, bool IN_RUN>
    __device__ __forceinline__ void long_row(int r) const
    {
        __shared__ double prod[BS];
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
};

template <int MODE>
int run_sweep(const liship_sweep_t *sw, const double *b, double *x, const double *wd, hipStream_t st)
{
    return walk_levels(sw, SweepRows<MODE>{{sw->lptr, sw->llong, sw->rows, sw->rptr, sw->col, sw->val, b, wd, x}}, st);
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
