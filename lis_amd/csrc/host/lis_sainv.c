/*
 * lis_sainv.c -- the SAINV preconditioner (ref src/precon/lis_precon_sainv.c), M^-1 = Z D^-1 W^T: built on the host, applied in HBM.
 *
 * Build (host, ref :122-378, the `#if 1` branch): a right-looking A-biorthogonalisation.  Step i takes the FINAL rows W_i and Z_i, forms
 * l = A Z_i (through the CSC copy of A, rows jj > i only) and u = W_i^T A, the pivot t = u . Z_i with d[i] = 1 / t (a zero pivot gives 1 / 0,
 * as in the reference), and subtracts (l_j d_i) W_i from W_j and (u_j d_i) Z_i from Z_j for the later rows j the step met, in the order it met them;
 * a term whose |t| * (1 / ||A[i,:]||inf) is not above the drop tolerance is dropped, a kept term on a new column is APPENDED to its row.  The
 * pattern depends on the values and every step needs the finished rows before it: nothing to schedule ahead of time, and no device scheduler
 * that waits on other workgroups, so the factor is made here.  The reference clears two dense n-vectors per step (memset at :226 and :248,
 * O(n^2) over the build); here l is cleared at the columns listed in il (it is written nowhere else) and u at a list of the columns W_i^T A
 * met: the same values in every bit at O(work).
 * A in another storage format: the loop runs on a CSR copy converted as the reference does (:72-83); A itself is untouched.
 *
 * The factor lives on the HBM copy of A (lisd_mat.sainv): W, Z as packed rows {ptr, index, value} in the reference's stored order (unit
 * diagonal first), d, a work vector, and the transposed row forms of Z and -- for M^-H, on first use -- of W, made in HBM by the
 * transposition lis_matvech uses (kernels/transpose.hip: a row's terms by source row).  It is dropped with the copy (host edits, page-watch
 * writes, conversions, lisd_mat_values_changed) and made again by the next begin.  precon->L / U / D / temp stay NULL.
 *   psolve : t = (W-rows . b) .* d  [lis_matvech_ilu + the scale loop, :763-770];  x = rows of Z^T . t  [lis_matvec_ilu's scatter, :771]
 *   psolveh: the same with W and Z swapped (:831-839)
 * Two launches (kernels/sainv.hip), no third pass; b may be x.  The scatter side sums in T chunks of source rows in the reference-order
 * mode (lis_amd_set_reference_reductions(T): the reference's per-thread buffers), in one chain otherwise.
 * Refused, each before A is touched: several ranks, -scale, -adds true, a split A, a matrix that lives in HBM only, the Jacobi solver.
 */
#include <stdio.h>
#include "lis_krylov.h"

typedef struct {
	int n, wnnz, znnz;
	double tol;
	int *wp, *wi, *zp, *zi; double *wv, *zv, *d;        /* HBM: the packed rows of W and Z, d */
	int *ztp, *zti, *wtp, *wti; double *ztv, *wtv;      /* HBM: the transposed row forms (W's on first M^-H) */
	double *t;                                          /* HBM: n doubles between the two launches */
	double build_s;
} lisd_sainv;

void lisd_sainv_free(void *p)
{
	lisd_sainv *s = (lisd_sainv *)p;
	if (!s) return;
	(void)liship_free(s->wp); (void)liship_free(s->wi); (void)liship_free(s->wv);
	(void)liship_free(s->zp); (void)liship_free(s->zi); (void)liship_free(s->zv); (void)liship_free(s->d);
	(void)liship_free(s->ztp); (void)liship_free(s->zti); (void)liship_free(s->ztv);
	(void)liship_free(s->wtp); (void)liship_free(s->wti); (void)liship_free(s->wtv);
	(void)liship_free(s->t);
	free(s);
}

/* ------------------------------------------------------------------ the build (host) */
#define ROW_CAP0 4                                     /* entries a row holds in the slab before it gets a block of its own */
typedef struct { int *idx; double *val; int nnz, cap; } srow;
typedef struct { srow *row; int *slab_i; double *slab_v; int n; } srows;

static void srows_free(srows *m)
{
	if (m->row) for (int i = 0; i < m->n; i++) if (m->row[i].cap > ROW_CAP0) free(m->row[i].val);
	free(m->row); free(m->slab_i); free(m->slab_v);
	memset(m, 0, sizeof(*m));
}

static int srows_init(srows *m, int n)
{	/* W = Z = I */
	const size_t rows = (size_t)(n > 0 ? n : 1);
	m->n = n;
	m->row = (srow *)malloc(sizeof(srow) * rows);
	m->slab_i = (int *)malloc(sizeof(int) * rows * ROW_CAP0);
	m->slab_v = (double *)malloc(sizeof(double) * rows * ROW_CAP0);
	if (!m->row || !m->slab_i || !m->slab_v) { free(m->row); m->row = NULL; srows_free(m); return 1; }
	for (int i = 0; i < n; i++) {
		srow *r = &m->row[i];
		r->idx = m->slab_i + (size_t)i * ROW_CAP0; r->val = m->slab_v + (size_t)i * ROW_CAP0;
		r->idx[0] = i; r->val[0] = 1.0; r->nnz = 1; r->cap = ROW_CAP0;
	}
	return 0;
}

static int srow_append(srow *r, int col, double v)
{
	if (r->nnz == r->cap) {                              /* one block: cap doubles, then cap ints */
		const int cap = r->cap * 2;
		double *val = (double *)malloc((sizeof(double) + sizeof(int)) * (size_t)cap);
		if (!val) return 1;
		int *idx = (int *)(val + cap);
		memcpy(val, r->val, sizeof(double) * (size_t)r->nnz); memcpy(idx, r->idx, sizeof(int) * (size_t)r->nnz);
		if (r->cap > ROW_CAP0) free(r->val);
		r->val = val; r->idx = idx; r->cap = cap;
	}
	r->idx[r->nnz] = col; r->val[r->nnz] = v; r->nnz++;
	return 0;
}

/* row j -= drop(dd * row i): ref :278-319 (W) and :323-364 (Z); ww: zero on entry and on return */
static int srow_update(srow *rj, const srow *ri, double dd, double nrm, double tol, int *ww)
{
	for (int k = 0; k < rj->nnz; k++) ww[rj->idx[k]] = k + 1;
	for (int ik = 0; ik < ri->nnz; ik++) {
		const int jk = ww[ri->idx[ik]];
		const double t = dd * ri->val[ik];
		if (!(fabs(t) * nrm > tol)) continue;
		if (jk != 0) rj->val[jk - 1] -= t;
		else if (srow_append(rj, ri->idx[ik], -t)) { for (int k = 0; k < rj->nnz; k++) ww[rj->idx[k]] = 0; return 1; }
	}
	for (int k = 0; k < rj->nnz; k++) ww[rj->idx[k]] = 0;
	return 0;
}

static LIS_INT srows_pack(const srows *m, int **ptr_out, int **idx_out, double **val_out)
{
	const int n = m->n;
	long long nnz = 0;
	for (int i = 0; i < n; i++) nnz += m->row[i].nnz;
	if (nnz >= 0x7fffffffLL) return LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "the SAINV factor does not fit (%D rows)\n", (LIS_INT)n);
	int *ptr = (int *)malloc(sizeof(int) * ((size_t)n + 1)), *idx = (int *)malloc(sizeof(int) * (size_t)(nnz + 1));
	double *val = (double *)malloc(sizeof(double) * (size_t)(nnz + 1));
	if (!ptr || !idx || !val) { free(ptr); free(idx); free(val); return LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "malloc size = %D\n", (LIS_INT)nnz); }
	ptr[0] = 0;
	for (int i = 0; i < n; i++) {
		const srow *r = &m->row[i];
		memcpy(idx + ptr[i], r->idx, sizeof(int) * (size_t)r->nnz); memcpy(val + ptr[i], r->val, sizeof(double) * (size_t)r->nnz);
		ptr[i + 1] = ptr[i] + r->nnz;
	}
	*ptr_out = ptr; *idx_out = idx; *val_out = val;
	return LIS_SUCCESS;
}

/* W, Z (packed, caller frees) and d of the n x n CSR matrix (ptr, index, value) at drop tolerance tol */
static LIS_INT build_factor(int n, const int *ptr, const int *index, const double *value, double tol,
                            int **wp, int **wi, double **wv, int **zp, int **zi, double **zv, double **d_out)
{
	LIS_INT err = LIS_SUCCESS;
	const size_t rows = (size_t)(n > 0 ? n : 1), nnz = (size_t)(n > 0 ? ptr[n] : 0);
	srows W = {0}, Z = {0};
	/* the CSC copy: a column's entries by row, ties by place in the row (lis_matrix_convert_csr2csc) */
	int *cp = (int *)calloc(rows + 1, sizeof(int)), *ci = (int *)malloc(sizeof(int) * (nnz + 1)), *fill = (int *)malloc(sizeof(int) * rows);
	double *cv = (double *)malloc(sizeof(double) * (nnz + 1));
	double *l = (double *)calloc(rows, sizeof(double)), *u = (double *)calloc(rows, sizeof(double)), *d = (double *)malloc(sizeof(double) * rows);
	int *il = (int *)malloc(sizeof(int) * rows), *iu = (int *)malloc(sizeof(int) * rows), *tu = (int *)malloc(sizeof(int) * rows);
	int *ww = (int *)calloc(rows, sizeof(int));
	unsigned char *met = (unsigned char *)calloc(rows, 1);
	if (!cp || !ci || !fill || !cv || !l || !u || !d || !il || !iu || !tu || !ww || !met || srows_init(&W, n) || srows_init(&Z, n)) {
		err = LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "malloc size = %D\n", (LIS_INT)n); goto out;
	}
	for (size_t k = 0; k < nnz; k++) if (index[k] >= 0 && index[k] < n) cp[index[k] + 1]++;
	for (int c = 0; c < n; c++) cp[c + 1] += cp[c];
	memcpy(fill, cp, sizeof(int) * (size_t)n);
	for (int i = 0; i < n; i++)
		for (int k = ptr[i]; k < ptr[i + 1]; k++) {
			const int c = index[k];
			if (c < 0 || c >= n) continue;
			ci[fill[c]] = i; cv[fill[c]++] = value[k];
		}
	for (int i = 0; i < n; i++) {
		const srow *wi_ = &W.row[i], *zi_ = &Z.row[i];
		double nrm = 0.0;                                /* 1 / nrm_inf(A[i,:]) */
		for (int j = ptr[i]; j < ptr[i + 1]; j++) { const double a = fabs(value[j]); nrm = nrm >= a ? nrm : a; }
		nrm = 1.0 / nrm;
		int cl = 0, cu = 0, ct = 0;
		for (int k = 0; k < zi_->nnz; k++) {             /* l = A Z_i, the rows after i */
			const int ii = zi_->idx[k];
			for (int j = cp[ii]; j < cp[ii + 1]; j++) {
				const int jj = ci[j];
				if (jj > i) {
					l[jj] += cv[j] * zi_->val[k];
					if (ww[jj] == 0) { ww[jj] = 1; il[cl++] = jj; }
				}
			}
		}
		for (int k = 0; k < cl; k++) ww[il[k]] = 0;
		for (int k = 0; k < wi_->nnz; k++) {             /* u = W_i^T A */
			const int ii = wi_->idx[k];
			for (int j = ptr[ii]; j < ptr[ii + 1]; j++) {
				const int jj = index[j];
				if (jj < 0 || jj >= n) continue;
				u[jj] += value[j] * wi_->val[k];
				if (!met[jj]) { met[jj] = 1; tu[ct++] = jj; }
				if (jj > i && ww[jj] == 0) { ww[jj] = 1; iu[cu++] = jj; }
			}
		}
		for (int k = 0; k < cu; k++) ww[iu[k]] = 0;
		double t = 0.0;                                  /* the pivot u . Z_i */
		for (int k = 0; k < zi_->nnz; k++) t += u[zi_->idx[k]] * zi_->val[k];
		d[i] = 1.0 / t;
		for (int jj = 0; jj < cl && !err; jj++) {
			const int j = il[jj];
			if (srow_update(&W.row[j], wi_, l[j] * d[i], nrm, tol, ww)) err = LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "row %D of W\n", (LIS_INT)j);
		}
		for (int jj = 0; jj < cu && !err; jj++) {
			const int j = iu[jj];
			if (srow_update(&Z.row[j], zi_, u[j] * d[i], nrm, tol, ww)) err = LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "row %D of Z\n", (LIS_INT)j);
		}
		if (err) goto out;
		for (int k = 0; k < cl; k++) l[il[k]] = 0.0;     /* what the reference's memsets clear, at the places written */
		for (int k = 0; k < ct; k++) { u[tu[k]] = 0.0; met[tu[k]] = 0; }
	}
	if ((err = srows_pack(&W, wp, wi, wv))) goto out;
	if ((err = srows_pack(&Z, zp, zi, zv))) { free(*wp); free(*wi); free(*wv); *wp = *wi = NULL; *wv = NULL; goto out; }
	*d_out = d; d = NULL;
out:
	srows_free(&W); srows_free(&Z);
	free(cp); free(ci); free(fill); free(cv); free(l); free(u); free(d); free(il); free(iu); free(tu); free(ww); free(met);
	return err;
}

/* fresh HBM arrays holding the transposed row form of the packed rows {dptr, didx, dval} (n x n): a row's terms by source row, ties by place */
LIS_INT lisd_rows_transposed(int n, int nnz, const int *dptr, const int *didx, const double *dval, int **tptr, int **tidx, double **tval)
{
	int *work = NULL;
	*tptr = NULL; *tidx = NULL; *tval = NULL;
	int rc = lisd_malloc((void **)tptr, sizeof(int) * ((size_t)n + 1) + 16);
	if (!rc) rc = lisd_malloc((void **)tidx, sizeof(int) * (size_t)nnz + 16);
	if (!rc) rc = lisd_malloc((void **)tval, sizeof(double) * (size_t)nnz + 16);
	if (!rc) rc = lisd_malloc((void **)&work, sizeof(int) * ((size_t)n + (size_t)nnz) + 16);
	if (!rc) rc = liship_csr_transpose_f64(n, n, nnz, dptr, didx, dval, *tptr, *tidx, *tval, work, lisg.stream);
	if (!rc) rc = liship_stream_synchronize(lisg.stream);
	(void)liship_free(work);
	if (rc) { (void)liship_free(*tptr); (void)liship_free(*tidx); (void)liship_free(*tval); *tptr = NULL; *tidx = NULL; *tval = NULL; }
	HIPCHK(rc);
	return LIS_SUCCESS;
}

/* the factor of A at tol: host build from A's CSR form (its own arrays, or a converted copy), one upload, Z's transposed form */
static LIS_INT factor_build(LIS_MATRIX A, double tol, lisd_sainv **out)
{
	LIS_MATRIX B = NULL;
	const int *ptr, *index; const double *value;
	int *wp = NULL, *wi = NULL, *zp = NULL, *zi = NULL; double *wv = NULL, *zv = NULL, *dd = NULL;
	LIS_INT err;
	const int n = A->n;
	const double t0 = lis_wtime();
	lisd_sainv *s = (lisd_sainv *)calloc(1, sizeof(lisd_sainv));
	if (!s) return LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "malloc size = %D\n", (LIS_INT)sizeof(lisd_sainv));
	int *cp = NULL, *ci = NULL; double *cv = NULL;
	if (A->matrix_type == LIS_MATRIX_CSR) {
		if ((err = lisp_fill_matrix(A))) goto out;
		ptr = A->ptr; index = A->index; value = A->value;
	} else if (A->matrix_type == LIS_MATRIX_COO) {
		/* COO: lis_matrix_convert would sort A's own arrays in place (lis_convert.c) and drop the HBM copy this factor is about to be cached on.  The rows are
		 * read off by a STABLE grouping of the triplets instead, A untouched: for a matrix that -storage coo made of CSR rows these ARE those rows, entry for
		 * entry, which is what the reference builds its factor from (it creates the preconditioner before it converts: lis_solver.c:384, :749) */
		if ((err = lisp_fill_matrix(A))) goto out;
		const LIS_INT nnz = A->nnz;
		cp = (int *)calloc((size_t)n + 2, sizeof(int));
		ci = (int *)malloc(sizeof(int) * (size_t)(nnz > 0 ? nnz : 1));
		cv = (double *)malloc(sizeof(double) * (size_t)(nnz > 0 ? nnz : 1));
		if (!cp || !ci || !cv) { err = LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "malloc size = %D\n", nnz); goto out; }
		for (LIS_INT k = 0; k < nnz; k++) {
			if (A->row[k] < 0 || A->row[k] >= n) { err = LISI_ERR(LIS_ERR_ILL_ARG, "COO matrix: a row index lies outside [0, %D)\n", (LIS_INT)n); goto out; }
			cp[A->row[k] + 2]++;
		}
		for (int r = 0; r < n; r++) cp[r + 2] += cp[r + 1];            /* cp[r + 1]: where row r's next entry goes; after the fill: where row r ends */
		for (LIS_INT k = 0; k < nnz; k++) { const int at = cp[A->row[k] + 1]++; ci[at] = A->col[k]; cv[at] = A->value[k]; }
		ptr = cp; index = ci; value = cv;
	} else {
		if ((err = lis_matrix_duplicate(A, &B)) || (err = lis_matrix_set_type(B, LIS_MATRIX_CSR)) || (err = lis_matrix_convert(A, B))) goto out;
		ptr = B->ptr; index = B->index; value = B->value;
	}
	if (!ptr || (ptr[n] > 0 && (!index || !value))) { err = LISI_ERR(LIS_ERR_ILL_ARG, "matrix A has no CSR arrays on the host\n"); goto out; }
	if ((err = build_factor(n, ptr, index, value, tol, &wp, &wi, &wv, &zp, &zi, &zv, &dd))) goto out;
	s->n = n; s->tol = tol; s->wnnz = wp[n]; s->znnz = zp[n];
	if ((err = lisd_upload_i(&s->wp, wp, (size_t)n + 1)) || (err = lisd_upload_i(&s->wi, wi, (size_t)s->wnnz)) || (err = lisd_upload_d(&s->wv, wv, (size_t)s->wnnz)) ||
	    (err = lisd_upload_i(&s->zp, zp, (size_t)n + 1)) || (err = lisd_upload_i(&s->zi, zi, (size_t)s->znnz)) || (err = lisd_upload_d(&s->zv, zv, (size_t)s->znnz)) ||
	    (err = lisd_upload_d(&s->d, dd, (size_t)n)) || (err = lisd_upload_d(&s->t, NULL, (size_t)n))) goto out;
	{	int rc = liship_stream_synchronize(lisg.stream);              /* (the host arrays are free to go) */
		if (rc) { err = lisi_hip_error(__FILE__, __func__, __LINE__, rc); goto out; } }
	if ((err = lisd_rows_transposed(n, s->znnz, s->zp, s->zi, s->zv, &s->ztp, &s->zti, &s->ztv))) goto out;
	s->build_s = lis_wtime() - t0;
	lisg.sainv_builds++;
out:
	if (B) lis_matrix_destroy(B);
	free(cp); free(ci); free(cv);
	free(wp); free(wi); free(wv); free(zp); free(zi); free(zv); free(dd);
	if (err) { lisd_sainv_free(s); return err; }
	*out = s;
	return LIS_SUCCESS;
}

/* what every entry needs of A: assembled, one of the served formats, not split, host arrays, one rank */
static LIS_INT check_served(LIS_MATRIX A)
{
	LISCHK(lisi_matrix_check(A, LISI_CHECK_ASSEMBLED));
	if (lisg.nprocs > 1) return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-p sainv is served on one rank only: the biorthogonalisation walks all rows in order (A is untouched)\n");
	if (!lisi_format_served(A->matrix_type)) return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-p sainv: storage format %D is not served by liblis_amd (A is untouched)\n", A->matrix_type);
	if (A->is_splited) return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-p sainv on a split matrix (an earlier -p ssor, -p is or -p bjacobi solve splits A) is not served: lis_matrix_merge(A) first (A is untouched)\n");
	if (MDEV(A)->device_only) return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-p sainv on a matrix that lives in HBM only is not served: the factor is built from the host arrays (A is untouched)\n");
	return LIS_SUCCESS;
}

/* the factor on the HBM copy of A, built on first use and when the tolerance changed */
static LIS_INT get_factor(LIS_MATRIX A, double tol, lisd_sainv **out)
{
	LISCHK(lisd_mat_ready(A));
	lisd_mat *d = MDEV(A);
	lisd_sainv *s = (lisd_sainv *)d->sainv;
	if (s && (s->tol != tol || s->n != A->n)) { lisd_sainv_free(s); d->sainv = s = NULL; }
	if (!s) {
		LISCHK(factor_build(A, tol, &s));
		d = MDEV(A);
		if (!d->ready) { lisd_sainv_free(s); return LISI_ERR(LIS_ERR_ILL_ARG, "the HBM copy of A went away during the SAINV build\n"); }
		d->sainv = s;
	}
	*out = s;
	return LIS_SUCCESS;
}

static LIS_INT apply_on(lisd_sainv *s, int transposed, const double *b, double *x)
{
	const int T = lisg.ref_reductions > 1 ? lisg.ref_reductions : 1;
	if (!transposed) {
		HIPCHK(liship_sainv_gather_scale_f64(s->n, s->wp, s->wi, s->wv, s->d, b, s->t, lisg.stream));
		HIPCHK(liship_sainv_rows_f64(s->n, s->n, T, s->ztp, s->zti, s->ztv, s->t, x, lisg.stream));
	} else {
		if (!s->wtp) LISCHK(lisd_rows_transposed(s->n, s->wnnz, s->wp, s->wi, s->wv, &s->wtp, &s->wti, &s->wtv));
		HIPCHK(liship_sainv_gather_scale_f64(s->n, s->zp, s->zi, s->zv, s->d, b, s->t, lisg.stream));
		HIPCHK(liship_sainv_rows_f64(s->n, s->n, T, s->wtp, s->wti, s->wtv, s->t, x, lisg.stream));
	}
	return LIS_SUCCESS;
}

/* ------------------------------------------------------------------ create */
LIS_INT lisi_sainv_create(LIS_SOLVER solver, LIS_PRECON precon)
{
	LIS_MATRIX A = solver->A;
	LISCHK(lisi_matrix_check(A, LISI_CHECK_ASSEMBLED));
	/* refusals first, none of which needs a device: A is left as it was */
	if (solver->options[LIS_OPTIONS_SCALE] != LIS_SCALE_NONE) return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-p sainv together with -scale is not served (A is untouched)\n");
	if (solver->options[LIS_OPTIONS_ADDS]) return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-p sainv with -adds true is not served (A is untouched)\n");
	if (solver->options[LIS_OPTIONS_SOLVER] == LIS_SOLVER_JACOBI)
		return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "the Jacobi solver with -p sainv (system rescaling) is not served (A is untouched)\n");
	LISCHK(check_served(A));
	LISCHK(lisd_init());
	lisd_sainv *s;
	LISCHK(get_factor(A, (double)solver->params[LIS_PARAMS_DROP - LIS_OPTIONS_LEN], &s));
	precon->A = A;
	return LIS_SUCCESS;
}

/* ------------------------------------------------------------------ the solve's side (the SAINV row of lisi_precon_kinds) */
LIS_INT lisd_sainv_begin(LIS_MATRIX A, LIS_SOLVER solver, lisi_precon_state *st)
{
	lisd_sainv *s;
	st->A = A; st->n = A->n; st->param = (double)solver->params[LIS_PARAMS_DROP - LIS_OPTIONS_LEN];
	st->T = lisg.ref_reductions > 1 ? lisg.ref_reductions : 1;
	LISCHK(check_served(A));
	LISCHK(get_factor(A, st->param, &s));          /* (built now if the HBM copy was rebuilt since lis_precon_create: a -storage conversion, a host edit) */
	lisg.last_sainv = 1; lisg.last_sainv_wnnz = s->wnnz; lisg.last_sainv_znnz = s->znnz; lisg.last_sainv_blocks = st->T;
	return LIS_SUCCESS;
}

LIS_INT lisd_sainv_apply(const lisi_precon_state *st, int transposed, const double *b, double *x)
{	/* x = M^-1 b, or M^-H b (b may be x): what begin left on the HBM copy, made again on a copy that a product rebuilt in mid-solve */
	lisd_sainv *s = (lisd_sainv *)MDEV(st->A)->sainv;
	if (!s || s->tol != st->param) LISCHK(get_factor(st->A, st->param, &s));
	return apply_on(s, transposed, b, x);
}

/* ------------------------------------------------------------------ introspection and tools (include/lis_amd.h) */
LIS_INT lis_amd_last_solve_sainv(LIS_INT *nnz_w, LIS_INT *nnz_z, LIS_INT *blocks)
{
	if (nnz_w) *nnz_w = lisg.last_sainv ? lisg.last_sainv_wnnz : 0;
	if (nnz_z) *nnz_z = lisg.last_sainv ? lisg.last_sainv_znnz : 0;
	if (blocks) *blocks = lisg.last_sainv ? lisg.last_sainv_blocks : 0;
	return lisg.last_sainv;
}

static LIS_INT tool_factor(LIS_MATRIX A, LIS_REAL tol, lisd_sainv **s)
{
	LISCHK(check_served(A));
	LISCHK(lisd_init());
	return get_factor(A, (double)tol, s);
}

LIS_INT lis_amd_sainv_factor(LIS_MATRIX A, LIS_REAL tol, LIS_INT sizes[3])
{
	lisd_sainv *s;
	LISCHK(tool_factor(A, tol, &s));
	if (sizes) { sizes[0] = s->n; sizes[1] = s->wnnz; sizes[2] = s->znnz; }
	return LIS_SUCCESS;
}

LIS_INT lis_amd_sainv_copy(LIS_MATRIX A, LIS_REAL tol, LIS_INT *wptr, LIS_INT *windex, LIS_SCALAR *wvalue,
                           LIS_INT *zptr, LIS_INT *zindex, LIS_SCALAR *zvalue, LIS_SCALAR *d)
{
	lisd_sainv *s;
	LISCHK(tool_factor(A, tol, &s));
	const size_t n = (size_t)s->n;
	HIPCHK(liship_stream_synchronize(lisg.stream));
	if (wptr) LISCHK(lisd_staged_d2h(wptr, s->wp, sizeof(int) * (n + 1)));
	if (zptr) LISCHK(lisd_staged_d2h(zptr, s->zp, sizeof(int) * (n + 1)));
	if (windex && s->wnnz) LISCHK(lisd_staged_d2h(windex, s->wi, sizeof(int) * (size_t)s->wnnz));
	if (zindex && s->znnz) LISCHK(lisd_staged_d2h(zindex, s->zi, sizeof(int) * (size_t)s->znnz));
	if (wvalue && s->wnnz) LISCHK(lisd_staged_d2h(wvalue, s->wv, sizeof(double) * (size_t)s->wnnz));
	if (zvalue && s->znnz) LISCHK(lisd_staged_d2h(zvalue, s->zv, sizeof(double) * (size_t)s->znnz));
	if (d && n) LISCHK(lisd_staged_d2h(d, s->d, sizeof(double) * n));
	return LIS_SUCCESS;
}

LIS_INT lis_amd_sainv_psolve(LIS_MATRIX A, LIS_REAL tol, LIS_VECTOR B, LIS_VECTOR X, LIS_INT transposed)
{
	lisd_sainv *s;
	LISCHK(tool_factor(A, tol, &s));
	if (B->n != A->n || X->n != A->n) return LISI_ERR(LIS_ERR_ILL_ARG, "sizes of A, B and X do not match\n");
	double *db, *dx;
	LISCHK(lisd_vec_in(B, &db));
	if (X == B) dx = db;
	else LISCHK(lisd_vec_out(X, &dx));
	const LIS_INT err = apply_on(s, transposed != 0, db, dx);
	const LIS_INT done = lisd_vec_done(X);
	return err ? err : done;
}

typedef struct { lisd_sainv *s; const double *b; double *x; } timed_args;
static LIS_INT psolve_once(void *ctx) { const timed_args *t = (const timed_args *)ctx; return apply_on(t->s, 0, t->b, t->x); }

LIS_INT lis_amd_sainv_times(LIS_MATRIX A, LIS_REAL tol, LIS_VECTOR B, LIS_VECTOR X, LIS_INT reps, double *build_s, double *psolve_ms)
{
	lisd_sainv *s;
	LISCHK(tool_factor(A, tol, &s));
	if (B->n != A->n || X->n != A->n || X == B) return LISI_ERR(LIS_ERR_ILL_ARG, "sizes of A, B and X do not match, or X is B\n");
	if (build_s) *build_s = s->build_s;
	double *db, *dx;
	LISCHK(lisd_vec_in(B, &db));
	LISCHK(lisd_vec_out(X, &dx));
	timed_args args = {s, db, dx};
	const LIS_INT err = lisi_sweep_times(reps, psolve_once, &args, psolve_ms);
	const LIS_INT done = lisd_vec_done(X);
	return err ? err : done;
}

LIS_INT lis_amd_sainv_info(LIS_MATRIX A, LIS_REAL tol, double info[6])
{	/* {host seconds of the build, nnz(W), nnz(Z), bytes one psolve streams, launches per psolve, host builds of SAINV factors since lis_initialize} */
	lisd_sainv *s;
	LISCHK(tool_factor(A, tol, &s));
	const double n = (double)s->n;
	info[0] = s->build_s;
	info[1] = (double)s->wnnz;
	info[2] = (double)s->znnz;
	/* W's rows (12 B a term, 4 B a row start), b, d and t written; Z^T's rows, t read and x written */
	info[3] = 12.0 * ((double)s->wnnz + (double)s->znnz) + 2.0 * 4.0 * (n + 1.0) + 5.0 * 8.0 * n;
	info[4] = 2.0;
	info[5] = (double)lisg.sainv_builds;
	return LIS_SUCCESS;
}
