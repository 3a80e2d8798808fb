/*
 * lis_upload.c -- the HBM copy of a matrix, built from its host arrays (lisd_mat_ready / mat_upload), and the decisions that the
 * conversion in HBM (lis_convert_hbm.c) shares with it: the plan, the constant-coefficient row form, the ELL column codes, the plane.
 *
 * Data layout in HBM (all f64 / i32):
 *   CSR       ptr[n+1], index[nnz], value[nnz] + the merge-path row split (liship_csr_plan_t)
 *   CSC       kept as the column-ordered transpose, i.e. CSR whose rows list their entries by ascending
 *             column: the reference's serial CSC loop (src/matvec/lis_matvec_csc.c:128-144) adds the
 *             terms of output row i in exactly that order
 *   ELL/DIA   column-major [maxnzr|nnd][n];  JAD  perm/ptr/index/value (one chunk);  BSR  bptr/bindex/value
 *   COO       kept as CSR rows that list a row's triplets in ascending k -- the order in which the reference's serial walk
 *             (src/matvec/lis_matvec_coo.c:75-87) adds them to y[row[k]] --, built IN HBM from the uploaded row / col / value (kernels/coo.hip):
 *             row[] non-decreasing: ptr[] from the row starts, col[] and value[] serve as index[] and value[] where they lie (d->row keeps the
 *             uploaded row[]); otherwise a stable grouping by row, after which the uploaded triplets are released
 *   DNS       value[np][n] column-major as the host holds it; the native kernel pair of kernels/dns.hip
 *   VBR       row / col / ptr / bptr / bindex / value as the host holds them, checked in HBM before anything is launched on them (liship_vbr_check), plus the
 *             block row of every row, made there (liship_vbr_block_rows); the native kernel of kernels/vbr.hip
 */
#include <stdio.h>
#include "lis_internal.h"

/* what only the COO, DNS and VBR arms call is referenced weakly: tests/c/upload_cases.c links this file against stubs of the calls the six older formats make, and the
 * library always holds the real ones */
extern LIS_INT lisi_one_rank_only(LIS_INT type) __attribute__((weak));
extern int liship_coo_rows_f64(int n, int nnz, const int *row, const int *col, const double *value, int *ptr, int **index, double **out_value, void *stream) __attribute__((weak));
extern int liship_vbr_check(int n, int np, int nnz, int nr, int nc, int bnnz, const int *row, const int *col, const int *ptr, const int *bptr, const int *bindex,
                            int *flags_host, void *stream) __attribute__((weak));
extern int liship_vbr_block_rows(int n, int nr, const int *row, int *brow, void *stream) __attribute__((weak));

/* a fresh HBM array holding src[0 .. count), queued on the library's stream; the array is the caller's from the allocation on, whatever the copy answers */
LIS_INT lisd_upload_i(int **dst, const int *src, size_t count)
{
	HIPCHK(lisd_malloc((void **)dst, (count + 4) * sizeof(int)));          /* +4: 16 B slack for vector loads */
	if (count) HIPCHK(liship_memcpy_h2d(*dst, src, count * sizeof(int), lisg.stream));
	return LIS_SUCCESS;
}
LIS_INT lisd_upload_d(double **dst, const double *src, size_t count)
{
	HIPCHK(lisd_malloc((void **)dst, (count + 2) * sizeof(double)));
	if (count && src) HIPCHK(liship_memcpy_h2d(*dst, src, count * sizeof(double), lisg.stream));
	return LIS_SUCCESS;
}

/* the three arrays of CSR rows laid out on the host: up, waited for, and the host arrays freed whatever happened */
static LIS_INT upload_csr_arrays(size_t rows, size_t nnz, int *hptr, int *hidx, double *hval, int **dptr, int **didx, double **dval)
{
	LIS_INT err = lisd_upload_i(dptr, hptr, rows + 1);
	if (!err) err = lisd_upload_i(didx, hidx, nnz);
	if (!err) err = lisd_upload_d(dval, hval, nnz);
	if (!err) { int rc = liship_stream_synchronize(lisg.stream); if (rc) err = lisi_hip_error(__FILE__, __func__, __LINE__, rc); }
	free(hptr); free(hidx); free(hval);
	return err;
}

/* XCD strips of the native ELL / DIA kernels (liship_spmv_formats_set_plane): the plane of the grid is the largest offset most rows reach -- for DIA read off its
 * offsets (the largest positive one: a diagonal serves every row it fits), for ELL found by two passes over index[] in HBM.  Used only where x does not fit the
 * 256 MB Infinity Cache (measured: 512^3 ELL 0.671 -> 0.733 of the roofline with the counters' traffic at 1.01 x the algorithmic bytes instead of 1.26 x, DIA 0.687 ->
 * 0.709; at 256^3, where x + y sit in that cache, the strips COST ELL 7 %: profiles/r06_formats_512.txt). */
void lisd_fmt_find_plane(lisd_mat *d, const int *host_dia_offsets)
{
	d->xs_rows = 0;
	if (d->type == LIS_MATRIX_DIA && host_dia_offsets) {
		int best = 0;
		for (int k = 0; k < d->nnd; k++) if (host_dia_offsets[k] > best && host_dia_offsets[k] < d->n) best = host_dia_offsets[k];
		d->xs_rows = best;
	} else if (d->type == LIS_MATRIX_ELL && d->index) {
		int plane = 0;
		if (liship_ell_scan_band(d->n, d->maxnzr, d->index, &plane, lisg.stream) == 0) d->xs_rows = plane;
	}
}

/* the one-byte column codes of a native ELL copy (d->n, d->maxnzr, d->index): an optimisation -- out of memory leaves the 4 B indices to serve, any other code is an error */
LIS_INT lisd_ell_index_codes(lisd_mat *d)
{
	if (lisg.no_index_codes) return LIS_SUCCESS;
	int nd = 0;
	const int rc = liship_ell_encode_indices(d->n, d->maxnzr, d->index, &d->ell_codes, &d->ell_dict, &nd, lisg.stream);
	if (rc) { (void)liship_free(d->ell_codes); (void)liship_free(d->ell_dict); d->ell_codes = NULL; d->ell_dict = NULL; }
	if (rc && rc != 2 /* hipErrorOutOfMemory */) HIPCHK(rc);
	return LIS_SUCCESS;
}

/* the permutation the last reordered plan found (liship_csr_plan_reorder), tried first by the next plan of the same size: a program that edits A->value between solves
 * rebuilds the HBM copy and its plan each time, and the walk (1.4 s on the Queen-class matrix) is most of that.  One entry; a hint is only ever a hint. */
static struct { int *perm; int n; long long nnz; } renum_cache;
void lisd_renum_cache_drop(void) { free(renum_cache.perm); renum_cache.perm = NULL; renum_cache.n = 0; renum_cache.nnz = 0; }

/* the renumbered form of a plan (liship_csr_plan_reorder: never an error when the matrix does not qualify; out of memory leaves the plan as it was) */
static LIS_INT plan_try_reorder(liship_csr_plan_t plan, int n, const int *dptr, const int *dindex, const double *dvalue)
{
	long long pnnz = 0;
	(void)liship_csr_plan_info(plan, NULL, &pnnz, NULL);
	const int *hint = (renum_cache.perm && renum_cache.n == n && renum_cache.nnz == pnnz) ? renum_cache.perm : NULL;      /* the last walk, when the sizes match (a matrix whose values were edited; any other matrix drops it for a walk of its own) */
	int rc = liship_csr_plan_reorder_with(plan, dptr, dindex, dvalue, 0, hint, lisg.stream);
	if (rc && rc != 2) HIPCHK(rc);
	if (!rc && liship_csr_plan_reordered(plan) > 0 && !hint) {
		int *keep = (int *)malloc(sizeof(int) * (size_t)n);
		if (keep && liship_csr_plan_reorder_permutation(plan, keep) == 0) {
			free(renum_cache.perm);
			renum_cache.perm = keep; renum_cache.n = n; renum_cache.nnz = pnnz;
		} else free(keep);
	}
	return LIS_SUCCESS;
}
/* LAZY renumbering (round 6): called by lis_solve before it looks for a renumbered form.  A CSR copy on one rank whose plan has served lisg.reorder_after products
 * in the caller's numbering gets the attempt once; what the attempt costs (the numbering found on the device -- kernels/csr_order.hpp --, P A P^T and its plan built in HBM: +0.17 s and +3.5 GB on the
 * Queen-class matrix; rounds 4-5 walked the graph on the host: 1.6 s) is paid by a program that has shown it iterates long enough to earn it back (0.06-0.1 ms per
 * iteration there: ~3000 iterations), never by the first solves. */
LIS_INT lisd_mat_lazy_reorder(LIS_MATRIX A)
{
	lisd_mat *d = MDEV(A);
	if (lisg.no_reorder || lisg.reorder_after <= 0 || !d->ready || d->reorder_tried) return LIS_SUCCESS;
	{	/* when: the ski-rental point -- build once the products served have cost about what the form costs.  Lists that exist but are long (the Queen class: the form
		 * saves 5-15 % of an iteration) wait for reorder_after products; a plan whose lists FAILED (no locality at all: 30-40 % of the roofline, the form doubles the
		 * rate; building it costs ~200 of those products whatever the size) waits for a sixteenth of that (256 by default) */
		long long wait = lisg.reorder_after;
		if (d->type == LIS_MATRIX_CSR && d->plan && liship_csr_plan_lists_failed(d->plan)) wait = wait / 16 > 0 ? wait / 16 : 1;
		if (d->served < wait) return LIS_SUCCESS;
	}
	/* (several ranks: each renumbers its own rows and owned columns -- the plan knows its ghost columns --; a matrix served as CSR from another layout with ghost columns stays as it is) */
	if (d->type != LIS_MATRIX_CSR || !d->plan || !d->value || d->split_jad || d->solve_holds || A->is_scaled || A->is_splited || d->n != A->n ||
	    (A->np != A->n && A->matrix_type != LIS_MATRIX_CSR)) return LIS_SUCCESS;
	d->reorder_tried = 1;
	return plan_try_reorder(d->plan, d->n, d->ptr, d->index, d->value);
}
LIS_INT lis_amd_set_reorder_after(long long products) { lisg.reorder_after = products < 0 ? 0 : products; return LIS_SUCCESS; }
long long lis_amd_matrix_products_served(LIS_MATRIX A) { return MDEV(A)->served; }

/* the row split of a CSR-ordered HBM matrix and, where its columns allow it, the one-byte column codes
 * (liship.h "index coding"; LIS_AMD_NO_INDEX_CODES=1 keeps the 4 B indices for A/B measurements) */
static LIS_INT csr_plan_impl(liship_csr_plan_t *plan, int n, int ncols, const int *dptr, const int *dindex, const double *dvalue, int reorder)
{
	int rc = liship_csr_plan_create(plan, n, dptr, lisg.stream);
	if (rc && lis_amd_trim_count() > 0) rc = liship_csr_plan_create(plan, n, dptr, lisg.stream);   /* the plan allocates in the kernel layer */
	HIPCHK(rc);
	if (ncols > n) HIPCHK(liship_csr_plan_set_ghost_columns(*plan, ncols));
	if (!lisg.no_index_codes) {
		/* the codes are an optimisation: a matrix that cannot have them (out of memory included) keeps its 4 B indices */
		rc = liship_csr_plan_encode_indices(*plan, dptr, dindex, lisg.stream);
		if (rc && lis_amd_trim_count() > 0) rc = liship_csr_plan_encode_indices(*plan, dptr, dindex, lisg.stream);
		if (rc && rc != 2 /* hipErrorOutOfMemory */) HIPCHK(rc);
		if (!rc && !lisg.no_row_patterns && liship_csr_plan_coded(*plan)) {       /* whole rows that repeat: one byte per row */
			rc = liship_csr_plan_encode_row_patterns(*plan, dptr, lisg.stream);
			if (rc && rc != 2) HIPCHK(rc);
			if (!rc && !lisg.no_value_records && dvalue) {        /* ... and carry the same values: nothing left to stream */
				rc = liship_csr_plan_encode_row_values(*plan, dptr, dvalue, lisg.stream);
				if (rc && rc != 2) HIPCHK(rc);
			}
		}
	}
	if (!lisg.no_local_columns && !liship_csr_plan_coded(*plan)) {      /* block-local columns where they pay: long rows, and (round 6) short rows whose row blocks share their columns */
		/* LIS_AMD_NO_INDEX_CODES=1 asks for the reference's own arrays in the product of a short-row matrix (the contract form): no lists for short rows then either */
		HIPCHK(liship_spmv_csr_set_local_short_rows((lisg.no_index_codes || lisg.no_local_short_rows) ? 0 : 1));
		rc = liship_csr_plan_localize_columns(*plan, dptr, dindex, lisg.stream);
		if (rc && lis_amd_trim_count() > 0) rc = liship_csr_plan_localize_columns(*plan, dptr, dindex, lisg.stream);
		if (rc && rc != 2) HIPCHK(rc);
		/* lists that stay long say the numbering has no locality: rows and columns renumbered inside the plan (one rank: its row ranges follow the original order).
		 * At plan time only when asked (LIS_AMD_REORDER_AFTER=0); by default the plan first serves lisg.reorder_after products in the caller's numbering
		 * (lisd_mat_lazy_reorder): building the form costs ~3000 iterations of what it saves per iteration on the Queen-class matrix, and the solves
		 * people time first take 40-50 */
		if (!rc && reorder && !lisg.no_reorder && (lisg.nprocs == 1 || ncols >= n) && dvalue && lisg.reorder_after == 0) LISCHK(plan_try_reorder(*plan, n, dptr, dindex, dvalue));
	}
	/* a plan that streams index[] / codes (no row patterns): the plane of a structured grid from the band of the matrix, for the XCD strips */
	rc = liship_csr_plan_scan_band(*plan, dptr, dindex, lisg.stream);
	if (rc && rc != 2) HIPCHK(rc);
	return LIS_SUCCESS;
}
LIS_INT lisd_csr_plan(liship_csr_plan_t *plan, int n, const int *dptr, const int *dindex, const double *dvalue) { return csr_plan_impl(plan, n, 0, dptr, dindex, dvalue, 1); }
/* ... of a rank's local rows: columns [n, ncols) are its ghost columns (the renumbered form keeps them apart: liship_csr_plan_set_ghost_columns) */
LIS_INT lisd_csr_plan_cols(liship_csr_plan_t *plan, int n, int ncols, const int *dptr, const int *dindex, const double *dvalue) { return csr_plan_impl(plan, n, ncols, dptr, dindex, dvalue, 1); }
/* ... of a matrix no solve iterates on (a transposed copy, a scaled copy, the halves of a split JAD matrix): no renumbered form (products would not use it) */
LIS_INT lisd_csr_plan_plain(liship_csr_plan_t *plan, int n, const int *dptr, const int *dindex, const double *dvalue) { return csr_plan_impl(plan, n, 0, dptr, dindex, dvalue, 0); }

/* the longest run [b,e) of clear flags among ghost[0 .. count); ghost[count] is the caller's room for the sentinel */
static void longest_clear_run(unsigned char *ghost, int count, int *b, int *e)
{
	int run_b = 0;
	ghost[count] = 1;
	*b = 0; *e = 0;
	for (int r = 0; r <= count; r++)
		if (ghost[r]) {
			if (r - run_b > *e - *b) { *b = run_b; *e = r; }
			run_b = r + 1;
		}
}

/* the longest run of rows that reference no ghost column (columns >= n): those rows run while the halo is in flight, the boundary
 * rows after it.  Read from the host layout of whatever format A has (CSR / CSC / ELL / DIA / JAD; BSR: block rows; split matrices: none). */
static void find_inner_rows(LIS_MATRIX A, int *b, int *e)
{
	const int n = A->n;
	int count = n;
	*b = 0; *e = 0;
	if (A->np == n) { *e = A->matrix_type == LIS_MATRIX_BSR ? A->nr : n; return; }       /* no ghost columns at all (BSR counts block rows) */
	if (A->is_splited || n <= 0) return;
	unsigned char *ghost = (unsigned char *)calloc((size_t)n + 1, 1);
	if (!ghost) return;                                               /* (no overlap then: exchange first) */
	switch (A->matrix_type) {
	case LIS_MATRIX_CSR:
		if (!A->ptr) { free(ghost); return; }
		for (int r = 0; r < n; r++)
			for (int k = A->ptr[r]; k < A->ptr[r + 1]; k++) if (A->index[k] >= n) { ghost[r] = 1; break; }
		break;
	case LIS_MATRIX_CSC:
		for (int c = n; c < A->np; c++)
			for (int k = A->ptr[c]; k < A->ptr[c + 1]; k++) ghost[A->index[k]] = 1;
		break;
	case LIS_MATRIX_ELL:
		for (int j = 0; j < A->maxnzr; j++)
			for (int r = 0; r < n; r++) if (A->index[(size_t)j * n + r] >= n) ghost[r] = 1;
		break;
	case LIS_MATRIX_DIA:                                              /* a diagonal reaches the ghosts in the rows where n <= r + offset < np (explicit zeros are read too) */
		for (int dgl = 0; dgl < A->nnd; dgl++) {
			const long long o = A->index[dgl];
			long long lo = (long long)n - o, hi = (long long)A->np - o;
			if (lo < 0) lo = 0;
			if (hi > n) hi = n;
			for (long long r = lo; r < hi; r++) ghost[r] = 1;
		}
		break;
	case LIS_MATRIX_JAD:
		for (int j = 0; j < A->maxnzr; j++)
			for (int sl = 0; sl < A->ptr[j + 1] - A->ptr[j]; sl++) if (A->index[A->ptr[j] + sl] >= n) ghost[A->row[sl]] = 1;
		break;
	case LIS_MATRIX_BSR: {                                            /* in BLOCK rows: ghost columns start on a fresh block column (lis_matrix_bsr.c:425-428) */
		if (!A->bptr) { free(ghost); return; }
		const int first_ghost = (n + A->bnc - 1) / A->bnc;
		for (int br = 0; br < A->nr; br++)
			for (int k = A->bptr[br]; k < A->bptr[br + 1]; k++) if (A->bindex[k] >= first_ghost) { ghost[br] = 1; break; }
		count = A->nr;
		break;
	}
	default:
		free(ghost);
		return;
	}
	longest_clear_run(ghost, count, b, e);
	free(ghost);
}

static LIS_INT upload_csc_as_csr(LIS_MATRIX A, lisd_mat *d)
{
	const int n = A->n, np = A->np, nnz = A->nnz;
	int *tptr = (int *)calloc((size_t)n + 2, sizeof(int));
	int *tidx = (int *)malloc(sizeof(int) * (size_t)(nnz > 0 ? nnz : 1));
	double *tval = (double *)malloc(sizeof(double) * (size_t)(nnz > 0 ? nnz : 1));
	if (!tptr || !tidx || !tval) { free(tptr); free(tidx); free(tval); return LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "csc transpose\n"); }
	for (int k = 0; k < nnz; k++) tptr[A->index[k] + 1]++;
	for (int r = 0; r < n; r++) tptr[r + 1] += tptr[r];
	int *fill = (int *)malloc(sizeof(int) * (size_t)(n > 0 ? n : 1));
	memcpy(fill, tptr, sizeof(int) * (size_t)n);
	for (int c = 0; c < np; c++)                    /* columns ascending: the reference's summation order */
		for (int k = A->ptr[c]; k < A->ptr[c + 1]; k++) {
			const int dst = fill[A->index[k]]++;
			tidx[dst] = c; tval[dst] = A->value[k];
		}
	free(fill);
	return upload_csr_arrays((size_t)n, (size_t)nnz, tptr, tidx, tval, &d->ptr, &d->index, &d->value);
}

/* A JAD matrix is laid out in HBM row by row, in the ORIGINAL row order: row perm[s] gets the s-th entry of every
 * jagged diagonal that is long enough, diagonal by diagonal -- the order in which lis_matvec_jad adds them to
 * y[perm[s]] starting from 0 (lis_matvec_jad.c:57-75), so the CSR kernel forms the same sums bit for bit.  The
 * jagged layout is what a vector CPU wants; on MI355X it costs a permuted y and maxnzr separate streams per lane
 * (68 % of the roofline, spmv_jad_kernel, kept for the kernel-level API), the row layout runs at the CSR rate. */
static LIS_INT upload_jad_as_csr(LIS_MATRIX A, lisd_mat *d)
{
	const int n = A->n, nnz = A->nnz, maxnzr = A->maxnzr;
	int *cptr = (int *)calloc((size_t)n + 2, sizeof(int));
	int *cidx = (int *)malloc(sizeof(int) * (size_t)(nnz > 0 ? nnz : 1));
	double *cval = (double *)malloc(sizeof(double) * (size_t)(nnz > 0 ? nnz : 1));
	int *fill = (int *)malloc(sizeof(int) * (size_t)(n > 0 ? n : 1));
	if (!cptr || !cidx || !cval || !fill) { free(cptr); free(cidx); free(cval); free(fill); return LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "jad re-layout\n"); }
	for (int j = 0; j < maxnzr; j++) {
		const int len = A->ptr[j + 1] - A->ptr[j];
		for (int s = 0; s < len; s++) cptr[A->row[s] + 1]++;
	}
	for (int r = 0; r < n; r++) cptr[r + 1] += cptr[r];
	memcpy(fill, cptr, sizeof(int) * (size_t)n);
	for (int j = 0; j < maxnzr; j++) {                /* diagonals ascending: each row receives its entries in summation order */
		const int b = A->ptr[j], len = A->ptr[j + 1] - b;
		for (int s = 0; s < len; s++) {
			const int dst = fill[A->row[s]]++;
			cidx[dst] = A->index[b + s]; cval[dst] = A->value[b + s];
		}
	}
	free(fill);
	return upload_csr_arrays((size_t)n, (size_t)nnz, cptr, cidx, cval, &d->ptr, &d->index, &d->value);
}

/* ------------------------------------------------------------------ the constant-coefficient row form
 * ELL and DIA matrices with constant coefficients.  Both formats add the terms of a row in a fixed order from 0 -- ELL its maxnzr
 * slots, padding included (value 0, index i: lis_matvec_ell.c:113-128), DIA its diagonals in ascending order over the rows where
 * i + offset stays inside the matrix, explicit zeros included (lis_matvec_dia.c:148-172) -- so a CSR layout that lists exactly
 * those terms, zeros and all, in that order, gives the CSR kernel the same sums bit for bit (0 * x[i] is kept: it is NaN when x[i]
 * is not finite, as in the reference).  The layout pays when the plan then finds value records (liship.h): a constant-coefficient
 * stencil in ELL or DIA streams 100 or 72 B per row, its row form one byte per row.  A cheap screen (few distinct values among the
 * first entries) keeps every other matrix away from the attempt; when the plan finds no value records the row form is dropped and
 * the native arrays serve as before.  *taken says which.  The upload lays the rows out on the host, the conversion in HBM by kernels;
 * whether to try (lisd_row_form_wanted) and whether to keep (lisd_row_form_adopt) is decided here for both. */
int lisd_few_distinct_values(const double *v, size_t count)
{
	unsigned long long seen[8];
	int ns = 0;
	const size_t lim = count < 65536 ? count : 65536;
	for (size_t k = 0; k < lim; k++) {
		unsigned long long b;
		memcpy(&b, v + k, 8);
		int j = 0;
		while (j < ns && seen[j] != b) j++;
		if (j == ns) { if (ns == 8) return 0; seen[ns++] = b; }
	}
	return 1;
}

/* rows of `width` terms: value records hold up to 32 entries per row, and every switch the row form rests on is on */
int lisd_row_form_wanted(long long width, int n)
{
	return !lisg.no_row_form && !lisg.no_value_records && !lisg.no_row_patterns && !lisg.no_index_codes && n > 0 && width >= 1 && width <= 32 && (long long)n * width < 0x7fffffffLL;
}

/* takes the three HBM arrays of a row form: planned, and kept in d (type CSR, nnz) when the plan finds value records -- *taken = 1 --, else freed with their plan.
 * An optimisation: out of memory on the way is not an error */
LIS_INT lisd_row_form_adopt(lisd_mat *d, int n, int *rptr, int *ridx, double *rval, LIS_INT nnz, int *taken)
{
	liship_csr_plan_t plan = NULL;
	const LIS_INT err = lisd_csr_plan(&plan, n, rptr, ridx, rval);
	*taken = 0;
	if (!err && plan && liship_csr_plan_value_records(plan)) {
		d->ptr = rptr; d->index = ridx; d->value = rval; d->plan = plan;
		d->type = LIS_MATRIX_CSR; d->nnz = nnz; *taken = 1;
		return LIS_SUCCESS;
	}
	if (plan) (void)liship_csr_plan_destroy(plan);          /* not this matrix: the native layout */
	(void)liship_free(rptr); (void)liship_free(ridx); (void)liship_free(rval);
	return err == LIS_ERR_OUT_OF_MEMORY ? LIS_SUCCESS : err;
}

static LIS_INT try_row_form(LIS_MATRIX A, lisd_mat *d, int *taken)
{
	*taken = 0;
	const int n = A->n;
	const int width = A->matrix_type == LIS_MATRIX_ELL ? A->maxnzr : A->nnd;
	if (!lisd_row_form_wanted(width, n) || !lisd_few_distinct_values(A->value, (size_t)n * (size_t)width)) return LIS_SUCCESS;
	int *cptr = (int *)malloc(sizeof(int) * ((size_t)n + 1));
	if (!cptr) return LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "row form\n");
	const int T = lisi_host_threads();
	const long long ncols = A->np;
	if (A->matrix_type == LIS_MATRIX_ELL) {
		for (int i = 0; i <= n; i++) cptr[i] = i * width;
	} else {
		cptr[0] = 0;
		for (int i = 0; i < n; i++) {                 /* the diagonals that reach row i: 0 <= i + offset < np (lis_matvec_dia.c:154-160) */
			int c = 0;
			for (int k = 0; k < width; k++) { const long long j = (long long)i + A->index[k]; c += (j >= 0 && j < ncols); }
			cptr[i + 1] = cptr[i] + c;
		}
	}
	const size_t nnz = (size_t)cptr[n];
	int *cidx = (int *)malloc(sizeof(int) * (nnz ? nnz : 1));
	double *cval = (double *)malloc(sizeof(double) * (nnz ? nnz : 1));
	if (!cidx || !cval) { free(cptr); free(cidx); free(cval); return LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "row form\n"); }
	if (A->matrix_type == LIS_MATRIX_ELL) {
#pragma omp parallel for num_threads(T) schedule(static)
		for (int i = 0; i < n; i++)
			for (int j = 0; j < width; j++) { cidx[(size_t)i * width + j] = A->index[(size_t)j * n + i]; cval[(size_t)i * width + j] = A->value[(size_t)j * n + i]; }
	} else {
#pragma omp parallel for num_threads(T) schedule(static)
		for (int i = 0; i < n; i++) {
			int at = cptr[i];
			for (int k = 0; k < width; k++) {
				const long long j = (long long)i + A->index[k];
				if (j >= 0 && j < ncols) { cidx[at] = (int)j; cval[at] = A->value[(size_t)k * n + i]; at++; }
			}
		}
	}
	int *rptr = NULL, *ridx = NULL; double *rval = NULL;
	const LIS_INT err = upload_csr_arrays((size_t)n, nnz, cptr, cidx, cval, &rptr, &ridx, &rval);
	if (!err) return lisd_row_form_adopt(d, n, rptr, ridx, rval, (LIS_INT)nnz, taken);
	(void)liship_free(rptr); (void)liship_free(ridx); (void)liship_free(rval);
	return err == LIS_ERR_OUT_OF_MEMORY ? LIS_SUCCESS : err;
}

/* BSR matrices with constant coefficients (the 2 x 2 blocking of a stencil streams its explicit zeros: 0.38 ms at 256^3 where every other format takes 0.05): as for
 * ELL / DIA above, CSR rows that list the format's terms in the format's order -- lis_matvec_bsr adds to a scalar row its blocks in order, a block's columns in order,
 * zeros included (lis_matvec_bsr.c:123-148, :293-343) -- are built IN HBM from the native arrays (liship_bsr_to_rows) and kept when the plan finds value records on them.
 * Only without padding (n a multiple of bnr, the columns a multiple of bnc: the padded x entries would otherwise be columns of the row form) and in single-rank jobs.
 * *taken = 1: d->ptr / index / value / plan hold the row form, d->type is CSR; the native arrays stay with the caller. */
/* (the facts about the matrix come as arguments: the in-HBM conversion calls this before the target's header is filled in) */
LIS_INT lisd_try_bsr_row_form(int n, int np, int bnr, int bnc, int splited, lisd_mat *d, const int *dbptr, const int *dbindex, const double *dbvalue, LIS_INT bnnz, int values_few, int *taken)
{
	*taken = 0;
	if (lisg.nprocs > 1 || n <= 0 || bnnz <= 0 || !values_few || n % bnr != 0 || np % bnc != 0 || np != n || splited) return LIS_SUCCESS;
	const long long slots = (long long)bnnz * bnr * bnc, width = slots / n;
	if (slots >= 0x7fffffffLL || !lisd_row_form_wanted(width > 0 ? width : 1, n)) return LIS_SUCCESS;
	int *rptr = NULL, *ridx = NULL, rc; double *rval = NULL;
	LIS_INT err = LIS_SUCCESS;
	if (lisd_malloc((void **)&rptr, sizeof(int) * ((size_t)n + 5)) || lisd_malloc((void **)&ridx, sizeof(int) * ((size_t)slots + 4)) ||
	    lisd_malloc((void **)&rval, sizeof(double) * ((size_t)slots + 2))) err = LIS_ERR_OUT_OF_MEMORY;
	else if ((rc = liship_bsr_to_rows(n, bnr, bnc, dbptr, dbindex, dbvalue, rptr, ridx, rval, lisg.stream)) != 0) err = lisi_hip_error(__FILE__, __func__, __LINE__, rc);
	if (err) {
		(void)liship_free(rptr); (void)liship_free(ridx); (void)liship_free(rval);
		return err == LIS_ERR_OUT_OF_MEMORY ? LIS_SUCCESS : err;          /* an optimisation: out of memory on the way is not an error */
	}
	LISCHK(lisd_row_form_adopt(d, n, rptr, ridx, rval, (LIS_INT)slots, taken));
	if (*taken && bnr == bnc && bnr <= 4 && liship_csr_plan_value_records(d->plan) == 2)       /* a lane per block row (optional; the plan decides) */
		(void)liship_csr_plan_encode_block_rows(d->plan, bnr, d->ptr, lisg.stream);
	return LIS_SUCCESS;
}

/* ------------------------------------------------------------------ split matrices
 * A split matrix (lis_split.c) lives in HBM as CSR rows that list the terms of a row in the order the reference's is_splited
 * branch adds them -- D x first -- and the kernels start the sum at -0.0, which makes the first product the initial value
 * (t0 = D[i]*x[i]; t0 += ...: lis_matvec_csr.c:70-87) bit for bit, signed zeros included.  JAD is not one chain:
 * (D x + sum over L) + sum over U with both partial sums started at 0 (lis_matvec_jad.c:60-140) -- two products, then two
 * element-wise passes (lisd_spmv). */
static LIS_INT upload_rows(LIS_INT rows, LIS_INT *ptr, LIS_INT *idx, LIS_SCALAR *val, int **dptr, int **didx, double **dval, liship_csr_plan_t *plan, int from_zero, int half)
{
	LISCHK(upload_csr_arrays((size_t)rows, (size_t)ptr[rows], ptr, idx, val, dptr, didx, dval));
	LISCHK(half ? lisd_csr_plan_plain(plan, rows, *dptr, *didx, *dval) : lisd_csr_plan(plan, rows, *dptr, *didx, *dval));
	if (!from_zero) HIPCHK(liship_csr_plan_set_first_term_initialises(*plan, 1));
	return LIS_SUCCESS;
}

static LIS_INT upload_split(LIS_MATRIX A, lisd_mat *d)
{
	LIS_INT *ptr, *idx; LIS_SCALAR *val;
	if (A->matrix_type == LIS_MATRIX_JAD) {
		LISCHK(lisi_split_jad_part(A, 0, &ptr, &idx, &val));
		LISCHK(upload_rows(A->n, ptr, idx, val, &d->ptr, &d->index, &d->value, &d->plan, 1, 1));
		LISCHK(lisi_split_jad_part(A, 1, &ptr, &idx, &val));
		LISCHK(upload_rows(A->n, ptr, idx, val, &d->u_ptr, &d->u_index, &d->u_value, &d->u_plan, 1, 1));
		LISCHK(lisd_upload_d(&d->dsplit, A->D->value, (size_t)A->n));
		HIPCHK(lisd_malloc((void **)&d->jw, ((size_t)A->n + 16) * sizeof(double)));
		d->type = LIS_MATRIX_CSR;
		d->split_jad = 1;
		return LIS_SUCCESS;
	}
	LIS_INT rows; int from_zero;
	LISCHK(lisi_split_rows(A, &rows, &ptr, &idx, &val, &from_zero));
	d->nnz = ptr[rows];
	LISCHK(upload_rows(rows, ptr, idx, val, &d->ptr, &d->index, &d->value, &d->plan, from_zero, 0));
	d->type = LIS_MATRIX_CSR;
	d->n = rows;                          /* BSR: nr*bnr rows, the padding rows included (the vectors carry the pad) */
	return LIS_SUCCESS;
}

/* ------------------------------------------------------------------ host writes to adopted arrays
 * The reference adopts the caller's arrays (lis_matrix_csr.c:98-103) and reads them live on every product
 * (lis_matvec_csr.c:97-109); here the product runs on an HBM copy built once.  Arrays that came from lis_matrix_malloc_<fmt> -- or that the library made itself:
 * element-wise assembly, conversions in HBM -- live on pages of the library's (lis_pages.c): under lazy coherence they are read-only while the HBM copy lives,
 * the first host write faults, opens them and sets host_written, and the next use rebuilds the copy (arrays, plan, transposed operator).  Arrays the caller
 * malloc'ed cannot be watched: lis_amd_matrix_host_modified(A) is the contract for those, and LIS_AMD_MATRIX_CHECK=1 the debugging aid -- every use of A then
 * re-hashes its host arrays and rebuilds the copy (with one line on stderr) when they changed. */
static unsigned long long hash_words(const void *p, size_t bytes)
{
	const unsigned long long *w = (const unsigned long long *)p;
	const size_t nw = bytes / 8;
	unsigned long long h = 0x9E3779B97F4A7C15ull ^ bytes;
	#pragma omp parallel for reduction(^:h) schedule(static) num_threads(lisi_host_threads())
	for (long long c = 0; c < (long long)((nw + 4095) / 4096); c++) {
		const size_t lo = (size_t)c * 4096, hi = lo + 4096 < nw ? lo + 4096 : nw;
		unsigned long long a = 0x243F6A8885A308D3ull + (unsigned long long)c, b = 0x13198A2E03707344ull;
		for (size_t i = lo; i + 1 < hi; i += 2) { a = (a ^ w[i]) * 0x9E3779B97F4A7C15ull; b = (b ^ w[i + 1]) * 0xC2B2AE3D27D4EB4Full; }
		if ((hi - lo) & 1) a = (a ^ w[hi - 1]) * 0x9E3779B97F4A7C15ull;
		h ^= (a ^ (b >> 29) ^ (a << 17)) * 0xD6E8FEB86659FD93ull;
	}
	const unsigned char *t = (const unsigned char *)p + nw * 8;
	for (size_t i = 0; i < bytes % 8; i++) h = (h ^ t[i]) * 0x100000001B3ull;
	return h;
}

static int host_arrays(LIS_MATRIX A, const void *arr[6], size_t bytes[6])
{
	const size_t n = (size_t)A->n;
	int k = 0;
#define ARR(p, b) do { if (p) { arr[k] = (p); bytes[k] = (b); k++; } } while (0)
	if (A->is_splited) return 0;                       /* (the split parts L, U, D are the library's own work arrays: not watched) */
	switch (A->matrix_type) {
	case LIS_MATRIX_CSR: ARR(A->ptr, 4 * (n + 1)); ARR(A->index, 4 * (size_t)A->nnz); ARR(A->value, 8 * (size_t)A->nnz); break;
	case LIS_MATRIX_CSC: ARR(A->ptr, 4 * ((size_t)A->np + 1)); ARR(A->index, 4 * (size_t)A->nnz); ARR(A->value, 8 * (size_t)A->nnz); break;
	case LIS_MATRIX_ELL: ARR(A->index, 4 * n * (size_t)A->maxnzr); ARR(A->value, 8 * n * (size_t)A->maxnzr); break;
	case LIS_MATRIX_DIA: ARR(A->index, 4 * (size_t)A->nnd); ARR(A->value, 8 * n * (size_t)A->nnd); break;
	case LIS_MATRIX_JAD: ARR(A->row, 4 * n); ARR(A->ptr, 4 * ((size_t)A->maxnzr + 1)); ARR(A->index, 4 * (size_t)A->nnz); ARR(A->value, 8 * (size_t)A->nnz); break;
	case LIS_MATRIX_BSR: ARR(A->bptr, 4 * ((size_t)A->nr + 1)); ARR(A->bindex, 4 * (size_t)A->bnnz); ARR(A->value, 8 * (size_t)A->bnnz * (size_t)A->bnr * (size_t)A->bnc); break;
	case LIS_MATRIX_COO: ARR(A->row, 4 * (size_t)A->nnz); ARR(A->col, 4 * (size_t)A->nnz); ARR(A->value, 8 * (size_t)A->nnz); break;
	case LIS_MATRIX_DNS: ARR(A->value, 8 * n * (size_t)A->np); break;
	case LIS_MATRIX_VBR:
		ARR(A->row, 4 * ((size_t)A->nr + 1)); ARR(A->col, 4 * ((size_t)A->nc + 1)); ARR(A->ptr, 4 * ((size_t)A->bnnz + 1));
		ARR(A->bptr, 4 * ((size_t)A->nr + 1)); ARR(A->bindex, 4 * (size_t)A->bnnz); ARR(A->value, 8 * (size_t)A->nnz); break;
	default: break;
	}
#undef ARR
	return k;
}

static unsigned long long host_arrays_hash(LIS_MATRIX A)
{
	const void *arr[6]; size_t bytes[6];
	const int k = host_arrays(A, arr, bytes);
	unsigned long long h = 0;
	for (int i = 0; i < k; i++) h = (h * 0x9E3779B97F4A7C15ull) ^ hash_words(arr[i], bytes[i]);
	return h;
}

/* COO: the triplets go up as they are and the row form is made of them in HBM (liship_coo_rows_f64): no host pass over the entries.  In place (rows grouped
 * already): d->index / d->value ARE the uploaded col / value, d->row keeps the uploaded row[] until the copy goes, and the transposed copy is the transposition of
 * these rows (d->coo_in_order, lis_matvech.c); grouped: the uploaded triplets are released, d->row stays NULL, the transposed copy groups the triplets by column */
static LIS_INT upload_coo_as_csr(LIS_MATRIX A, lisd_mat *d)
{
	const int n = A->n, nnz = A->nnz;
	int *drow = NULL, *dcol = NULL, *gidx = NULL; double *dval = NULL, *gval = NULL;
	LIS_INT err = lisd_upload_i(&drow, A->row, (size_t)nnz);
	if (!err) err = lisd_upload_i(&dcol, A->col, (size_t)nnz);
	if (!err) err = lisd_upload_d(&dval, A->value, (size_t)nnz);
	if (!err) { const int rc = lisd_malloc((void **)&d->ptr, sizeof(int) * ((size_t)n + 5)); if (rc) err = lisi_hip_error(__FILE__, __func__, __LINE__, rc); }
	if (!err) {
		const int rc = liship_coo_rows_f64(n, nnz, drow, dcol, dval, d->ptr, &gidx, &gval, lisg.stream);
		if (rc == LISHIP_ERR_ARG) err = LISI_ERR(LIS_ERR_ILL_ARG, "COO matrix: a row index lies outside [0, %D)\n", (LIS_INT)n);
		else if (rc) err = lisi_hip_error(__FILE__, __func__, __LINE__, rc);
	}
	if (err) { (void)liship_free(drow); (void)liship_free(dcol); (void)liship_free(dval); return err; }
	d->index = gidx; d->value = gval;
	if (gidx == dcol) { d->row = drow; d->coo_in_order = 1; }
	else { (void)liship_free(drow); (void)liship_free(dcol); (void)liship_free(dval); }
	return LIS_SUCCESS;
}

/* VBR: the six arrays go up as they are.  One kernel then checks them -- the product's lanes take addresses from every one of them -- and a violation is
 * LIS_ERR_ILL_ARG naming the array, with nothing launched on the arrays; then the block row of every row is made from the checked row[] */
static LIS_INT upload_vbr(LIS_MATRIX A, lisd_mat *d)
{
	static const struct { int bit; const char *what; } bad[] = {
		{LISHIP_VBR_BAD_ROW, "row[] must ascend strictly from 0 to n"}, {LISHIP_VBR_BAD_COL, "col[] must ascend strictly from 0 to np"},
		{LISHIP_VBR_BAD_BPTR, "bptr[] must ascend from 0 to bnnz"}, {LISHIP_VBR_BAD_PTR, "ptr[] must ascend inside [0, nnz]"},
		{LISHIP_VBR_BAD_BINDEX, "bindex[] holds a block column outside [0, nc)"}, {LISHIP_VBR_BAD_SIZE, "ptr[bc+1] - ptr[bc] is not the size of block bc"},
	};
	int flags = 0;
	if (A->nnz < 0 || A->bnnz < 0 || A->nr < 1 || A->nc < 1) return LISI_ERR(LIS_ERR_ILL_ARG, "VBR matrix: nnz = %D, bnnz = %D, nr = %D, nc = %D\n", A->nnz, A->bnnz, A->nr, A->nc);
	d->nr = A->nr; d->nc = A->nc;
	LISCHK(lisd_upload_i(&d->row, A->row, (size_t)A->nr + 1));
	LISCHK(lisd_upload_i(&d->col, A->col, (size_t)A->nc + 1));
	LISCHK(lisd_upload_i(&d->ptr, A->ptr, (size_t)A->bnnz + 1));
	LISCHK(lisd_upload_i(&d->bptr, A->bptr, (size_t)A->nr + 1));
	LISCHK(lisd_upload_i(&d->bindex, A->bindex, (size_t)A->bnnz));
	LISCHK(lisd_upload_d(&d->value, A->value, (size_t)A->nnz));
	HIPCHK(liship_vbr_check(A->n, A->np, A->nnz, A->nr, A->nc, A->bnnz, d->row, d->col, d->ptr, d->bptr, d->bindex, &flags, lisg.stream));
	for (size_t k = 0; k < sizeof(bad) / sizeof(bad[0]); k++)
		if (flags & bad[k].bit) return LISI_ERR(LIS_ERR_ILL_ARG, "VBR matrix: %s (n = %D, np = %D, nr = %D, nc = %D, bnnz = %D, nnz = %D)\n", bad[k].what, A->n, A->np, A->nr, A->nc, A->bnnz, A->nnz);
	HIPCHK(lisd_malloc((void **)&d->brow, sizeof(int) * ((size_t)A->n + 4)));
	HIPCHK(liship_vbr_block_rows(A->n, A->nr, d->row, d->brow, lisg.stream));
	return LIS_SUCCESS;
}

static LIS_INT mat_upload(LIS_MATRIX A);
LIS_INT lisd_mat_ready(LIS_MATRIX A)
{
	lisd_mat *d = MDEV(A);
	if (d->ready && d->solve_holds) return LIS_SUCCESS;       /* a solve in the plan's numbering has P A P^T's arrays in d->ptr / index / value (lis_solver.c): the copy stays as it is until the solve hands it back */
	if (d->ready && !d->device_only) {
		if (d->host_written) lisd_mat_free(A);             /* a host write to one of its arrays was seen (page fault): the copy is stale */
		else if (lisg.matrix_check && d->checked && lisp_lazy_arrays(A) == 0 && host_arrays_hash(A) != d->host_hash) {
			fprintf(stderr, "liblis_amd: LIS_AMD_MATRIX_CHECK: the host arrays of matrix %p changed since its HBM copy was built and lis_amd_matrix_host_modified() was "
			                "not called: rebuilding the copy\n", (void *)A);
			lisd_mat_free(A);
		}
	}
	if (d->ready) return LIS_SUCCESS;
	const LIS_INT err = mat_upload(A);
	if (err) { lisd_mat_free(A); return err; }      /* a half-made HBM copy (arrays up, plan failed ...) must not be uploaded over by the next call */
	{	/* the arrays the copy was built from: watched from here on where they live on the library's pages */
		const void *arr[6]; size_t bytes[6];
		const int k = host_arrays(A, arr, bytes);
		for (int i = 0; i < k; i++) (void)lisp_adopt(A, (void *)arr[i]);
		(void)lisp_matrix_protect(A);
		if (lisg.matrix_check) { d->host_hash = host_arrays_hash(A); d->checked = 1; }
	}
	return LIS_SUCCESS;
}

static LIS_INT mat_upload(LIS_MATRIX A)
{
	lisd_mat *d = MDEV(A);
	LISCHK(lisd_init());
	if (A->status < LIS_MATRIX_CSR) return LISI_ERR(LIS_ERR_ILL_ARG, "matrix A is not assembled\n");
	LISCHK(lisp_fill_matrix(A));
	d->host_written = 0;
	d->n = A->n; d->np = A->np; d->nnz = A->nnz;
	d->type = A->matrix_type;
	const size_t n = (size_t)A->n;
	if (A->is_splited && !(A->matrix_type == LIS_MATRIX_BSR && A->bnr != A->bnc)) LISCHK(upload_split(A, d));      /* (with ghost columns: exchange first, no overlap) */
	else switch (A->matrix_type) {
	case LIS_MATRIX_CSR:
		LISCHK(lisd_upload_i(&d->ptr, A->ptr, n + 1));
		LISCHK(lisd_upload_i(&d->index, A->index, (size_t)A->nnz));
		LISCHK(lisd_upload_d(&d->value, A->value, (size_t)A->nnz));
		LISCHK(lisd_csr_plan_cols(&d->plan, A->n, A->np, d->ptr, d->index, d->value));
		break;
	case LIS_MATRIX_CSC:
	case LIS_MATRIX_JAD:
		LISCHK(A->matrix_type == LIS_MATRIX_CSC ? upload_csc_as_csr(A, d) : upload_jad_as_csr(A, d));
		d->type = LIS_MATRIX_CSR;
		LISCHK(lisd_csr_plan(&d->plan, A->n, d->ptr, d->index, d->value));
		break;
	case LIS_MATRIX_ELL:
		d->maxnzr = A->maxnzr;
		{ int taken = 0; LISCHK(try_row_form(A, d, &taken)); if (taken) break; }
		LISCHK(lisd_upload_i(&d->index, A->index, n * (size_t)A->maxnzr));
		LISCHK(lisd_upload_d(&d->value, A->value, n * (size_t)A->maxnzr));
		LISCHK(lisd_ell_index_codes(d));
		lisd_fmt_find_plane(d, NULL);
		break;
	case LIS_MATRIX_DIA:
		d->nnd = A->nnd;
		{ int taken = 0; LISCHK(try_row_form(A, d, &taken)); if (taken) break; }
		LISCHK(lisd_upload_i(&d->index, A->index, (size_t)A->nnd));
		LISCHK(lisd_upload_d(&d->value, A->value, n * (size_t)A->nnd));
		lisd_fmt_find_plane(d, A->index);
		break;
	case LIS_MATRIX_BSR:
		d->nr = A->nr; d->nc = A->nc; d->bnr = A->bnr; d->bnc = A->bnc;
		LISCHK(lisd_upload_i(&d->bptr, A->bptr, (size_t)A->nr + 1));
		LISCHK(lisd_upload_i(&d->bindex, A->bindex, (size_t)A->bnnz));
		LISCHK(lisd_upload_d(&d->value, A->value, (size_t)A->bnnz * (size_t)A->bnr * (size_t)A->bnc));
		{	/* constant coefficients: the row form (value records) instead of the native blocks, which d->value holds until the row form is taken */
			int taken = 0;
			double *native = d->value;
			LISCHK(lisd_try_bsr_row_form(A->n, A->np, A->bnr, A->bnc, A->is_splited, d, d->bptr, d->bindex, native, A->bnnz, lisd_few_distinct_values(A->value, (size_t)A->bnnz * (size_t)A->bnr * (size_t)A->bnc), &taken));
			if (taken) { (void)liship_free(native); (void)liship_free(d->bptr); (void)liship_free(d->bindex); d->bptr = NULL; d->bindex = NULL; }
		}
		break;
	case LIS_MATRIX_COO:
		if (!lisi_one_rank_only || !liship_coo_rows_f64) return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "COO storage: this build holds no row-form builder\n");
		LISCHK(lisi_one_rank_only(A->matrix_type));
		LISCHK(upload_coo_as_csr(A, d));
		d->type = LIS_MATRIX_CSR;
		LISCHK(lisd_csr_plan(&d->plan, A->n, d->ptr, d->index, d->value));
		break;
	case LIS_MATRIX_DNS:
		if (lisi_one_rank_only) LISCHK(lisi_one_rank_only(A->matrix_type));
		LISCHK(lisd_upload_d(&d->value, A->value, n * (size_t)A->np));
		break;
	case LIS_MATRIX_VBR:
		if (!lisi_one_rank_only || !liship_vbr_check || !liship_vbr_block_rows) return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "VBR storage: this build holds no checking kernel\n");
		LISCHK(lisi_one_rank_only(A->matrix_type));
		LISCHK(upload_vbr(A, d));
		break;
	default:
		return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "storage format %D is not served by liblis_amd\n", A->matrix_type);
	}
	HIPCHK(liship_stream_synchronize(lisg.stream));
	find_inner_rows(A, &d->inner_begin, &d->inner_end);
	d->ready = 1;
	return LIS_SUCCESS;
}

void lisd_mat_free(LIS_MATRIX A)
{
	lisd_mat *d = MDEV(A);
	(void)lisp_fill_matrix(A);         /* host arrays still held in HBM only (a matrix converted there) come home before the copy goes */
	if (d->plan) (void)liship_csr_plan_destroy(d->plan);
	if (d->u_plan) (void)liship_csr_plan_destroy(d->u_plan);
	(void)liship_free(d->u_ptr); (void)liship_free(d->u_index); (void)liship_free(d->u_value); (void)liship_free(d->dsplit); (void)liship_free(d->jw);
	if (d->t_plan) (void)liship_csr_plan_destroy(d->t_plan);
	if (d->rt_plan) (void)liship_csr_plan_destroy(d->rt_plan);
	(void)liship_free(d->rt_ptr); (void)liship_free(d->rt_index); (void)liship_free(d->rt_value);
	(void)liship_free(d->t_ptr); (void)liship_free(d->t_index); (void)liship_free(d->t_value); (void)liship_free(d->wr); (void)liship_free(d->t_diag);
	(void)liship_free(d->ell_codes); (void)liship_free(d->ell_dict);
	(void)liship_free(d->ptr); (void)liship_free(d->index); (void)liship_free(d->row);
	(void)liship_free(d->col); (void)liship_free(d->brow); (void)liship_free(d->t_borders);
	(void)liship_free(d->bptr); (void)liship_free(d->bindex); (void)liship_free(d->value);
	(void)liship_free(d->export_index); (void)liship_free(d->ws); free(d->export_run);
	(void)liship_free(d->sx); (void)liship_free(d->sy);
	lisi_precon_release(d, NULL, NULL);   /* what the preconditioners cached on this copy */
	memset(d, 0, sizeof(*d));
	lisp_matrix_release(A, 0);         /* no copy left that a host write could leave stale: the watched arrays are plain memory again */
}

/* ------------------------------------------------------------------ values edited in place (lis_matrix_shift_diagonal, lis_shift.c; lis_matrix_scale of VBR, lis_scale.c)
 * A kernel changed d->value of a CSR (or VBR) copy where it lies: everything derived from the old values goes -- the plan with its value records and its renumbered
 * form, the transposed copies in both numberings, what the preconditioners cached on the copy -- and the plan is made again from the HBM arrays, by the
 * call that made it at upload time (mat_upload / upload_split / lis_amd_matrix_set_csr_device).  The transposed copy and the caches come back on their
 * next use.  No matrix array crosses the bus. */
LIS_INT lisd_mat_values_changed(LIS_MATRIX A)
{
	lisd_mat *d = MDEV(A);
	if (d->plan) { (void)liship_csr_plan_destroy(d->plan); d->plan = NULL; }
	if (d->t_plan) { (void)liship_csr_plan_destroy(d->t_plan); d->t_plan = NULL; }
	(void)liship_free(d->t_ptr); (void)liship_free(d->t_index); (void)liship_free(d->t_value); (void)liship_free(d->t_diag);
	d->t_ptr = NULL; d->t_index = NULL; d->t_value = NULL; d->t_diag = NULL; d->t_ready = 0; d->t_nnz = 0;
	if (d->rt_plan) { (void)liship_csr_plan_destroy(d->rt_plan); d->rt_plan = NULL; }
	(void)liship_free(d->rt_ptr); (void)liship_free(d->rt_index); (void)liship_free(d->rt_value);
	d->rt_ptr = NULL; d->rt_index = NULL; d->rt_value = NULL; d->rt_ready = 0; d->rt_nnz = 0;
	lisi_precon_release(d, NULL, NULL);
	d->reorder_tried = 0; d->served = 0;
	if (d->type == LIS_MATRIX_VBR) {             /* (no plan: the VBR kernel reads value[] itself; the chunk borders of A^T x depend on row[] alone) */
		HIPCHK(liship_stream_synchronize(lisg.stream));
		return LIS_SUCCESS;
	}
	if (A->is_splited) {
		LISCHK(lisd_csr_plan(&d->plan, d->n, d->ptr, d->index, d->value));
		HIPCHK(liship_csr_plan_set_first_term_initialises(d->plan, 1));      /* (CSR chain rows: upload_rows, from_zero = 0) */
	} else LISCHK(lisd_csr_plan_cols(&d->plan, A->n, d->device_only ? d->np : A->np, d->ptr, d->index, d->value));
	HIPCHK(liship_stream_synchronize(lisg.stream));
	return LIS_SUCCESS;
}

/* ... and the same edit made by the library on the watched host arrays: they open for it without the write being taken for the program's (host_written
 * stays as it is, the copy is kept), then close again; LIS_AMD_MATRIX_CHECK's hash is taken anew */
void lisd_mat_host_edit_begin(LIS_MATRIX A) { lisp_matrix_release(A, 0); }
void lisd_mat_host_edit_end(LIS_MATRIX A)
{
	lisd_mat *d = MDEV(A);
	(void)lisp_matrix_protect(A);
	if (lisg.matrix_check && d->checked) d->host_hash = host_arrays_hash(A);
}

/* ------------------------------------------------------------------ what the copy looks like (tests, drivers) */
LIS_INT lis_amd_matrix_upload(LIS_MATRIX A) { return lisd_mat_ready(A); }
/* a fact of the plan of A's copy, 0 where there is no copy or no plan */
#define PLAN_FACT(A, fact) ((lisd_mat_ready(A) == LIS_SUCCESS && MDEV(A)->plan) ? fact(MDEV(A)->plan) : 0)
LIS_INT lis_amd_matrix_index_codes(LIS_MATRIX A)     { return PLAN_FACT(A, liship_csr_plan_coded); }
LIS_INT lis_amd_matrix_row_patterns(LIS_MATRIX A)    { return PLAN_FACT(A, liship_csr_plan_row_patterns); }
LIS_INT lis_amd_matrix_pattern_records(LIS_MATRIX A) { return PLAN_FACT(A, liship_csr_plan_pattern_records); }
LIS_INT lis_amd_matrix_value_records(LIS_MATRIX A)   { return PLAN_FACT(A, liship_csr_plan_value_records); }
LIS_INT lis_amd_matrix_dominant_pattern(LIS_MATRIX A){ return PLAN_FACT(A, liship_csr_plan_dominant_pattern); }
LIS_INT lis_amd_matrix_wide_dominant(LIS_MATRIX A)   { return PLAN_FACT(A, liship_csr_plan_wide_dominant); }
LIS_INT lis_amd_matrix_strip_rows(LIS_MATRIX A)      { return PLAN_FACT(A, liship_csr_plan_strip_rows); }
LIS_INT lis_amd_matrix_block_rows(LIS_MATRIX A)      { return PLAN_FACT(A, liship_csr_plan_block_rows); }
long long lis_amd_matrix_reordered(LIS_MATRIX A)     { return PLAN_FACT(A, liship_csr_plan_reordered); }
LIS_INT lis_amd_matrix_local_columns(LIS_MATRIX A)   { const long long listed = PLAN_FACT(A, liship_csr_plan_localized); return listed > 0x7fffffffLL ? 0x7fffffff : (LIS_INT)listed; }
LIS_INT lis_amd_matrix_marching(LIS_MATRIX A)
{
	if (lisd_mat_ready(A) != LIS_SUCCESS) return 0;
	if (!(MDEV(A)->type == LIS_MATRIX_CSR && MDEV(A)->plan)) return 0;
	if (liship_csr_plan_block2_march(MDEV(A)->plan)) return 4;
	if (liship_csr_plan_box27(MDEV(A)->plan)) return 3;
	return liship_csr_plan_marching(MDEV(A)->plan);
}
LIS_INT lis_amd_matrix_device_type(LIS_MATRIX A) { return lisd_mat_ready(A) == LIS_SUCCESS ? MDEV(A)->type : 0; }
void *lis_amd_matrix_csr_plan(LIS_MATRIX A) { return (lisd_mat_ready(A) == LIS_SUCCESS && MDEV(A)->type == LIS_MATRIX_CSR) ? (void *)MDEV(A)->plan : NULL; }
LIS_INT lis_amd_set_matrix_check(LIS_INT on) { lisg.matrix_check = on ? 1 : 0; return LIS_SUCCESS; }
LIS_INT lis_amd_matrix_host_written(LIS_MATRIX A) { return MDEV(A)->host_written; }
/* tests of the write watch without a GPU: the arrays of an assembled matrix are adopted and write-protected exactly as lisd_mat_ready does after an upload */
LIS_INT lis_amd_matrix_page_test_watch(LIS_MATRIX A)
{
	const void *arr[6]; size_t bytes[6];
	const int k = host_arrays(A, arr, bytes);
	MDEV(A)->host_written = 0;
	for (int i = 0; i < k; i++) (void)lisp_adopt(A, (void *)arr[i]);
	return lisp_matrix_protect(A);
}
LIS_INT lis_amd_matrix_host_modified(LIS_MATRIX A)
{
	if (MDEV(A)->device_only) return LISI_ERR(LIS_ERR_ILL_ARG, "matrix lives in HBM only\n");
	lisd_mat_free(A);
	return LIS_SUCCESS;
}
