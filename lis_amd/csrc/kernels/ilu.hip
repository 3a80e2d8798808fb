// ilu.hip -- the numerical factorisation of ILU(k) along the forward levels (lis_ilu.c builds pattern and schedule).
//
// Row i of the factor depends on the rows its L pattern names, all of earlier levels: the rows of one level are independent.
// Like the sweeps (sptrsv.hip): a level of more than LISHIP_SWEEP_SMALL_LEVEL rows is one launch, a run of smaller levels one
// single-workgroup launch with __syncthreads() between levels; no workgroup ever waits on a flag another workgroup writes.
//
// One row: L, D, U of the row start at 0 and take A's kept entries; then for every pivot j of L(i), ascending,
//   l = L[i][j] * d[j] (d holds 1 / pivot), stored; for every term (c, u) of U(j) with c in row i's pattern: target = target - l * u
// -- the product rounded, then the subtraction (-ffp-contract=off) --; finally d[i] = 1 / D.  A target takes one update per
// pivot, so within one pivot the updates are independent: a long row's workgroup spreads them over its threads and keeps the
// pivots in order with a barrier; a short row's thread runs the whole row in order.  Every value is the reference's chain of
// roundings (lis_precon_iluk.c:638-762, the OpenMP branch).
//
// Where column c lies in row i: the L part of the row is ascending, the U part has an ascending copy with the places
// (uskey / uspos); a binary search in the row's own keys, which stay in the CU's L1 / L2 while the row is worked on.  Of equal keys
// the last one answers (the reference's jw[] keeps the later place of a column stored twice).  When a row of A stores a column
// twice a pivot may hit one target twice: `serial` hands such matrices' long rows to one thread.
#include "common.hpp"
#include "liship.h"

namespace {

constexpr int LEVEL_BLOCK = 256;        // one level per launch: a thread per short row, a workgroup per long row
constexpr int RUN_BLOCK = 1024;         // a run of small levels: one workgroup

struct Fac {
    int n, serial;
    const int *aptr, *aindex;
    const double *avalue;
    const int *lptr, *lcol, *uptr, *ucol, *uskey, *uspos;
    double *lval, *uval, *d;
    const int *slptr, *sllong, *srows;  // the schedule: levels, first long row of each, rows in level order
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

// where row r keeps column c: in L, as the pivot, in U -- or nowhere
__device__ __forceinline__ double *place(const Fac &f, const Row &r, int c)
{
    if (c == r.i) return f.d + r.i;
    if (c < r.i) {
        const int p = find_last(f.lcol, r.l0, r.l1, c);
        return p < 0 ? nullptr : f.lval + p;
    }
    const int p = find_last(f.uskey, r.u0, r.u1, c);
    if (p < 0) return nullptr;
    return f.uval + (f.uspos ? f.uspos[p] : p);
}

__device__ __forceinline__ void update(const Fac &f, const Row &r, double l, int k)
{
    double *t = place(f, r, f.ucol[k]);
    if (t) { const double p = l * f.uval[k]; *t = *t - p; }
}

// one row, one thread, everything in order
__device__ void row_by_thread(const Fac &f, int i)
{
    const Row r = row_of(f, i);
    for (int k = r.l0; k < r.l1; k++) f.lval[k] = 0.0;
    for (int k = r.u0; k < r.u1; k++) f.uval[k] = 0.0;
    f.d[i] = 0.0;
    const int a1 = f.aptr[i + 1];
    for (int k = f.aptr[i]; k < a1; k++) {
        const int c = f.aindex[k];
        if (c < 0 || c >= f.n) continue;
        double *t = place(f, r, c);
        if (t) *t = f.avalue[k];
    }
    for (int j = r.l0; j < r.l1; j++) {
        const int jrow = f.lcol[j];
        const double l = f.lval[j] * f.d[jrow];
        f.lval[j] = l;
        const int k1 = f.uptr[jrow + 1];
        for (int k = f.uptr[jrow]; k < k1; k++) update(f, r, l, k);
    }
    f.d[i] = 1.0 / f.d[i];
}

// one row, the whole workgroup (every thread calls it: the trip counts are uniform)
template <int BS>
__device__ void row_by_workgroup(const Fac &f, int i)
{
    const int t = (int)threadIdx.x;
    if (f.serial) {
        if (t == 0) row_by_thread(f, i);
        return;
    }
    const Row r = row_of(f, i);
    for (int k = r.l0 + t; k < r.l1; k += BS) f.lval[k] = 0.0;
    for (int k = r.u0 + t; k < r.u1; k += BS) f.uval[k] = 0.0;
    if (t == 0) f.d[i] = 0.0;
    __syncthreads();
    const int a1 = f.aptr[i + 1];
    for (int k = f.aptr[i] + t; k < a1; k += BS) {          // no column twice: no two threads share a place
        const int c = f.aindex[k];
        if (c < 0 || c >= f.n) continue;
        double *p = place(f, r, c);
        if (p) *p = f.avalue[k];
    }
    __syncthreads();
    for (int j = r.l0; j < r.l1; j++) {                     // pivots in order
        const int jrow = f.lcol[j];
        if (t == 0) f.lval[j] = f.lval[j] * f.d[jrow];
        __syncthreads();
        const double l = f.lval[j];
        const int k1 = f.uptr[jrow + 1];
        for (int k = f.uptr[jrow] + t; k < k1; k += BS) update(f, r, l, k);
        __syncthreads();
    }
    if (t == 0) f.d[i] = 1.0 / f.d[i];
}

// one level: blocks [0, nshort_blocks) take a short row per thread, each further block one long row
__global__ __launch_bounds__(LEVEL_BLOCK) void factor_level(Fac f, int level, int nshort_blocks)
{
    const int r0 = f.slptr[level], rl = f.sllong[level];
    if ((int)blockIdx.x < nshort_blocks) {
        const int r = r0 + (int)blockIdx.x * LEVEL_BLOCK + (int)threadIdx.x;
        if (r < rl) row_by_thread(f, f.srows[r]);
    } else {
        row_by_workgroup<LEVEL_BLOCK>(f, f.srows[rl + (int)blockIdx.x - nshort_blocks]);
    }
}

// levels [l0, l1) in one workgroup, a barrier between consecutive levels
__global__ __launch_bounds__(RUN_BLOCK) void factor_run(Fac f, int l0, int l1)
{
    for (int l = l0; l < l1; l++) {
        const int r0 = f.slptr[l], rl = f.sllong[l], r1 = f.slptr[l + 1];
        for (int r = r0 + (int)threadIdx.x; r < rl; r += RUN_BLOCK) row_by_thread(f, f.srows[r]);
        for (int r = rl; r < r1; r++) { row_by_workgroup<RUN_BLOCK>(f, f.srows[r]); __syncthreads(); }
        __syncthreads();
    }
}

}  // namespace

extern "C" int liship_ilu_factor_f64(const liship_ilu_t *p, const liship_sweep_t *sw, void *stream)
{
    if (!p || !sw || p->n < 0 || sw->nrows != p->n) return LISHIP_ERR_ARG;
    if (p->n == 0) return 0;
    if (!p->aptr || !p->lptr || !p->uptr || !p->d || !sw->lptr || !sw->llong || !sw->rows) return LISHIP_ERR_ARG;
    hipStream_t st = as_stream(stream);
    const Fac f{p->n, p->serial, p->aptr, p->aindex, p->avalue, p->lptr, p->lcol, p->uptr, p->ucol, p->uskey, p->uspos,
                p->lval, p->uval, p->d, sw->lptr, sw->llong, sw->rows};
    for (int g = 0; g < sw->ngroups; g++) {
        const int l0 = sw->groups[3 * g], l1 = sw->groups[3 * g + 1], run = sw->groups[3 * g + 2];
        if (run) {
            factor_run<<<1, RUN_BLOCK, 0, st>>>(f, l0, l1);
        } else {
            const int nshort = sw->h_nshort[l0];
            const int nsb = (nshort + LEVEL_BLOCK - 1) / LEVEL_BLOCK;
            const int grid = nsb + (sw->h_nrows[l0] - nshort);
            factor_level<<<grid, LEVEL_BLOCK, 0, st>>>(f, l0, nsb);
        }
        LAUNCH_CHECK();
    }
    return 0;
}
