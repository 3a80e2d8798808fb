// coo.hip -- the row form of a COO matrix, built in HBM from its triplets.
//
// lis_matvec_coo is serial in every build of the reference (src/matvec/lis_matvec_coo.c:75-87): y = 0, then y[row[k]] += value[k] * x[col[k]] for
// ascending k.  Row i's sum is therefore the chain, from +0.0, of its triplets in stored order -- what the CSR kernels form of a row that lists
// exactly those entries in that order.  So a COO matrix lives in HBM as CSR rows (the whole plan serves it: index codes, value records, renumbering):
//   row[] non-decreasing   the triplets are grouped already: ptr[] is read off the row starts, and col[] / value[] ARE index[] / value[] where they
//                          lie -- no second copy of the entries
//   otherwise              a stable grouping by row (liship_group_by_key_f64, transpose.hip: count, scan, scatter positions, order, gather)
// Setup-time code: runs once per matrix, not on the hot path.
#include "common.hpp"
#include "liship.h"

// ptr: n + 1 ints (the caller's).  *index / *value: col / val themselves (in place), or fresh arrays the caller releases with liship_free.
// LISHIP_ERR_ARG: a row outside [0, n), with nothing built.  Synchronizes the stream.
extern "C" int liship_coo_rows_f64(int n, int nnz, const int *row, const int *col, const double *val,
                                   int *ptr, int **index, double **value, void *stream)
{
    if (n < 0 || nnz < 0 || !index || !value || !ptr) return LISHIP_ERR_ARG;
    *index = nullptr; *value = nullptr;
    int flags = 0;
    int rc = liship_key_facts(n, nnz, row, &flags, stream);
    if (rc) return rc;
    if (flags & 2) return LISHIP_ERR_ARG;
    if (!(flags & 1)) {                              // grouped already (nnz == 0 included): in place
        rc = liship_sorted_key_starts(n, nnz, row, ptr, stream);
        if (rc) return rc;
        *index = const_cast<int *>(col); *value = const_cast<double *>(val);
        return (int)hipStreamSynchronize(as_stream(stream));
    }
    int *gidx = nullptr; double *gval = nullptr;
    hipError_t e = hipMalloc(&gidx, sizeof(int) * ((size_t)nnz + 4));             // (+16 B: the slack every index / value array of a CSR copy has)
    if (e == hipSuccess) e = hipMalloc(&gval, sizeof(double) * ((size_t)nnz + 2));
    if (e == hipSuccess) rc = liship_group_by_key_f64(n, nnz, row, col, val, ptr, gidx, gval, stream); else rc = (int)e;
    if (rc) { (void)hipFree(gidx); (void)hipFree(gval); return rc; }
    *index = gidx; *value = gval;
    return 0;
}
