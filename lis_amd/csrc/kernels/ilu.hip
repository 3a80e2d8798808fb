// ilu.hip -- the numerical factorisation of ILU(k) along the forward levels (lis_ilu.c builds the pattern, lis_sweep.c the schedule).
//
// Row i of the factor depends on the rows its L pattern names, all of earlier levels: the rows of one level are independent.
// The levels are walked like those of the sweeps (level_schedule.hpp): a level of more than LISHIP_SWEEP_SMALL_LEVEL rows is one
// launch, a run of smaller levels one single-workgroup launch.
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
#include "level_schedule.hpp"
#include "ilu_pattern.hpp"

namespace {

struct Fac {
    int n, serial;
    const int *aptr, *aindex;
    const double *avalue;
    const int *lptr, *lcol, *uptr, *ucol, *uskey, *uspos;
    double *lval, *uval, *d;
    const int *slptr, *sllong, *srows;  // the schedule: levels, first long row of each, rows in level order
};

// where row r keeps column c: in L, as the pivot, in U -- or nowhere
__device__ __forceinline__ double *place(const Fac &f, const Row &r, int c)
{
    if (c == r.i) return f.d + r.i;
    bool lower;
    const int p = place_index(f, r, c, &lower);
    return p < 0 ? nullptr : (lower ? f.lval : f.uval) + p;
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

// the rows of the factorisation (level_schedule.hpp); no LDS.  In a run every long row ends on a barrier of its own.
struct FacRows {
    Fac f;
    __device__ __forceinline__ const int *level_ptr() const { return f.slptr; }
    __device__ __forceinline__ const int *level_long() const { return f.sllong; }
    __device__ __forceinline__ void short_row(int r) const { row_by_thread(f, f.srows[r]); }
    template <int BS, bool IN_RUN>
    __device__ __forceinline__ void long_row(int r) const { row_by_workgroup<BS>(f, f.srows[r]); if (IN_RUN) __syncthreads(); }
};

}  // namespace

extern "C" int liship_ilu_factor_f64(const liship_ilu_t *p, const liship_sweep_t *sw, void *stream)
{
    if (!p || !sw || p->n < 0 || sw->nrows != p->n) return LISHIP_ERR_ARG;
    if (p->n == 0) return 0;
    if (!p->aptr || !p->lptr || !p->uptr || !p->d || !sw->lptr || !sw->llong || !sw->rows) return LISHIP_ERR_ARG;
    const FacRows rows{{p->n, p->serial, p->aptr, p->aindex, p->avalue, p->lptr, p->lcol, p->uptr, p->ucol, p->uskey, p->uspos,
                        p->lval, p->uval, p->d, sw->lptr, sw->llong, sw->rows}};
    return walk_levels(sw, rows, as_stream(stream));
}
