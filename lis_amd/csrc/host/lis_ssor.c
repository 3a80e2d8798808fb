/*
 * lis_ssor.c -- the SSOR preconditioner (ref src/precon/lis_precon_ssor.c) on level-scheduled sweeps (kernels/sptrsv.hip).
 *
 * create (ref :57-95): -storage conversion of the caller's A, lis_matrix_split(A) -- A STAYS split, every later lis_matvec adds
 * D, L, U in that order --, and WD = 1 / (omega D) built only while A->use_wd != LIS_SOLVER_SOR: a second solve on the same A with
 * another -ssor_omega keeps the first omega's WD, as in the reference.
 * psolve  = lis_matrix_solve(A, B, X, LIS_MATRIX_SSOR)   (lis_matrix_csr.c:1572-1627, the OpenMP branch)
 * psolveh = lis_matrix_solveh(A, B, X, LIS_MATRIX_SSOR)  (lis_matrix_csr.c:1804-1855)
 * The reference runs T row blocks (LIS_GET_ISIE) of T threads, each sweeping its own block and skipping the terms that reach out
 * of it: block-Jacobi SSOR with T blocks.  Here T = 1 (true SSOR, independent of any core count) unless the reference-order mode
 * asks for T (lis_amd_set_reference_reductions(T)), which reproduces the reference at T threads.
 *
 * Schedule: per sweep, the level of a row is 1 + the largest level of the rows its kept terms read; rows of a level and their terms
 * are stored contiguously in level order (the reference's in-row order kept).  The transposed sweeps of psolveh hold, for row jj of
 * U^T, its terms by source row ascending, of L^T by source row descending (ties by position in the source row): a row-wise sum in
 * that order is the reference's scatter sum bit for bit.  Built on the host (O(nnz), from the split parts), cached on the HBM copy
 * of A (lisd_mat.ssor) and dropped with it (lisd_mat_free: host edits, page-watch writes, conversions).
 */
#include <stdio.h>
#include "lis_krylov.h"


typedef lisi_sweep_t sweep_t;              /* lis_internal.h: shared with lis_ilu.c */

typedef struct {
	int T;                                     /* 0: slot unused */
	sweep_t sw[SW_COUNT];
} sched_t;

typedef struct {
	sched_t s[2];                              /* the block counts in use: T = 1 (LOWER / UPPER, the default) and the parity mode's T */
	int next;
	double *wd;                                /* HBM copy of A->WD */
	int wd_n;
	double build_s;                            /* host seconds spent building schedules */
} lisd_ssor;

void lisi_sweep_free(lisi_sweep_t *s)
{
	(void)liship_free(s->lptr); (void)liship_free(s->llong); (void)liship_free(s->rows); (void)liship_free(s->rptr);
	(void)liship_free(s->col); (void)liship_free(s->val);
	free(s->groups); free(s->nrows); free(s->nshort);
	memset(s, 0, sizeof(*s));
}

void lisd_ssor_free(void *p)
{
	lisd_ssor *ss = (lisd_ssor *)p;
	if (!ss) return;
	for (int t = 0; t < 2; t++) for (int w = 0; w < SW_COUNT; w++) lisi_sweep_free(&ss->s[t].sw[w]);
	(void)liship_free(ss->wd);
	free(ss);
}

/* block of row i among T blocks of LIS_GET_ISIE (ref include/lis.h:1067): the first n % T blocks hold n / T + 1 rows */
int *lisi_block_of(int n, int T)
{
	int *b = (int *)malloc(sizeof(int) * (size_t)(n > 0 ? n : 1));
	if (!b) return NULL;
	const int q = n / T, rem = n % T;
	for (int i = 0; i < n; i++) b[i] = (i < rem * (q + 1)) ? i / (q + 1) : rem + (i - rem * (q + 1)) / q;
	return b;
}

static LIS_INT up_i(int **dst, const int *src, size_t count)
{
	HIPCHK(lisd_malloc((void **)dst, (count + 4) * sizeof(int)));
	if (count) HIPCHK(liship_memcpy_h2d(*dst, src, count * sizeof(int), lisg.stream));
	return LIS_SUCCESS;
}
static LIS_INT up_d(double **dst, const double *src, size_t count)
{
	HIPCHK(lisd_malloc((void **)dst, (count + 2) * sizeof(double)));
	if (count && src) HIPCHK(liship_memcpy_h2d(*dst, src, count * sizeof(double), lisg.stream));
	return LIS_SUCCESS;
}

/* levels + level-ordered layout of n rows whose terms (tp, tc, tv) read only rows before them (desc = 0) or after them (desc = 1).
 * tv NULL: no values (a schedule only, or values that arrive later on the device); weight: what decides whether row i is a long
 * row instead of its term count; src_out: for every place of the layout the term (index into tc) that lies there (caller frees) */
LIS_INT lisi_sweep_build(lisi_sweep_t *s, int n, const int *tp, const int *tc, const double *tv, int desc, const int *weight, int **src_out)
{
	LIS_INT err = LIS_SUCCESS;
	const int nnz = tp[n];
	int *lev = (int *)malloc(sizeof(int) * (size_t)(n + 1));
	int *rows = (int *)malloc(sizeof(int) * (size_t)(n + 1)), *rptr = (int *)malloc(sizeof(int) * (size_t)(n + 1));
	int *col = (int *)malloc(sizeof(int) * (size_t)(nnz + 1));
	double *val = tv ? (double *)malloc(sizeof(double) * (size_t)(nnz + 1)) : NULL;
	int *src = src_out ? (int *)malloc(sizeof(int) * (size_t)(nnz + 1)) : NULL;
	int *lptr = NULL, *llong = NULL, *fill_s = NULL, *fill_l = NULL;
#define ROW_WEIGHT(i) (weight ? weight[(i)] : tp[(i) + 1] - tp[(i)])
	if (!lev || !rows || !rptr || !col || (tv && !val) || (src_out && !src)) { err = LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "malloc size = %D\n", (LIS_INT)nnz); goto out; }
	int nlev = 0;
	for (int q = 0; q < n; q++) {
		const int i = desc ? n - 1 - q : q;
		int l = 0;
		for (int k = tp[i]; k < tp[i + 1]; k++) { const int lj = lev[tc[k]] + 1; if (lj > l) l = lj; }
		lev[i] = l;
		if (l + 1 > nlev) nlev = l + 1;
	}
	s->nrows = (int *)calloc((size_t)nlev + 1, sizeof(int)); s->nshort = (int *)calloc((size_t)nlev + 1, sizeof(int));
	lptr = (int *)calloc((size_t)nlev + 1, sizeof(int)); llong = (int *)calloc((size_t)nlev + 1, sizeof(int));
	fill_s = (int *)calloc((size_t)nlev + 1, sizeof(int)); fill_l = (int *)calloc((size_t)nlev + 1, sizeof(int));
	s->groups = (int *)malloc(sizeof(int) * 3 * ((size_t)nlev + 1));
	if (!s->nrows || !s->nshort || !lptr || !llong || !fill_s || !fill_l || !s->groups) { err = LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "malloc size = %D\n", (LIS_INT)nlev); goto out; }
	for (int i = 0; i < n; i++) { s->nrows[lev[i]]++; if (ROW_WEIGHT(i) < LISHIP_SWEEP_LONG_ROW) s->nshort[lev[i]]++; }
	for (int l = 0; l < nlev; l++) { lptr[l + 1] = lptr[l] + s->nrows[l]; llong[l] = lptr[l] + s->nshort[l]; fill_s[l] = lptr[l]; fill_l[l] = llong[l]; }
	for (int i = 0; i < n; i++) {             /* rows by level; inside a level short rows first, each part by ascending row */
		const int l = lev[i];
		if (ROW_WEIGHT(i) < LISHIP_SWEEP_LONG_ROW) rows[fill_s[l]++] = i; else rows[fill_l[l]++] = i;
	}
	rptr[0] = 0;
	for (int r = 0; r < n; r++) {
		const int i = rows[r];
		int at = rptr[r];
		for (int k = tp[i]; k < tp[i + 1]; k++, at++) { col[at] = tc[k]; if (val) val[at] = tv[k]; if (src) src[at] = k; }
		rptr[r + 1] = at;
	}
	/* launches: runs of small levels in one workgroup, every large level on its own */
	int ng = 0;
	for (int l = 0; l < nlev; ) {
		if (s->nrows[l] <= LISHIP_SWEEP_SMALL_LEVEL) {
			int e = l;
			while (e < nlev && s->nrows[e] <= LISHIP_SWEEP_SMALL_LEVEL) e++;
			s->groups[3 * ng] = l; s->groups[3 * ng + 1] = e; s->groups[3 * ng + 2] = 1; ng++;
			l = e;
		} else {
			s->groups[3 * ng] = l; s->groups[3 * ng + 1] = l + 1; s->groups[3 * ng + 2] = 0; ng++;
			l++;
		}
	}
	if ((err = up_i(&s->lptr, lptr, (size_t)nlev + 1)) || (err = up_i(&s->llong, llong, (size_t)nlev + 1)) || (err = up_i(&s->rows, rows, (size_t)n)) ||
	    (err = up_i(&s->rptr, rptr, (size_t)n + 1)) || (err = up_i(&s->col, col, (size_t)nnz)) || ((tv || src_out) && (err = up_d(&s->val, val, (size_t)nnz)))) goto out;      /* (values that arrive later: room only) */
	{	int rc = liship_stream_synchronize(lisg.stream);          /* (the host arrays go below) */
		if (rc) { err = lisi_hip_error(__FILE__, __func__, __LINE__, rc); goto out; } }
	s->k.nlev = nlev; s->k.nrows = n; s->k.nnz = nnz; s->k.ngroups = ng;
	s->k.lptr = s->lptr; s->k.llong = s->llong; s->k.rows = s->rows; s->k.rptr = s->rptr; s->k.col = s->col; s->k.val = s->val;
	s->k.groups = s->groups; s->k.h_nrows = s->nrows; s->k.h_nshort = s->nshort;
	s->bytes = 4.0 * n + 4.0 * (n + 1) + 12.0 * nnz + 24.0 * n;
	s->built = 1;
	if (src_out) { *src_out = src; src = NULL; }
out:
#undef ROW_WEIGHT
	free(lev); free(rows); free(rptr); free(col); free(val); free(src); free(lptr); free(llong); free(fill_s); free(fill_l);
	if (err) lisi_sweep_free(s);
	return err;
}

/* the terms of one sweep under T blocks: those whose row and column lie in the same block (T = 1: all of them) */
static LIS_INT sweep_make(LIS_MATRIX A, int which, int T, sweep_t *s)
{
	const int n = A->n;
	LIS_MATRIX_CORE P = (which == SW_L || which == SW_LT) ? A->L : A->U;
	int *blk = lisi_block_of(n, T);
	int *tp = (int *)calloc((size_t)n + 2, sizeof(int));
	const int pn = P->ptr[n];
	int *tc = (int *)malloc(sizeof(int) * (size_t)(pn + 1));
	double *tv = (double *)malloc(sizeof(double) * (size_t)(pn + 1));
	LIS_INT err = LIS_SUCCESS;
	if (!blk || !tp || !tc || !tv) { err = LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "malloc size = %D\n", (LIS_INT)pn); goto out; }
#define KEEP(i, c) ((c) >= 0 && (c) < n && blk[(i)] == blk[(c)])
	if (which == SW_L || which == SW_U) {          /* the rows themselves, stored order */
		int at = 0;
		for (int i = 0; i < n; i++) {
			for (int k = P->ptr[i]; k < P->ptr[i + 1]; k++) if (KEEP(i, P->index[k])) { tc[at] = P->index[k]; tv[at] = P->value[k]; at++; }
			tp[i + 1] = at;
		}
	} else {                                      /* transposed: U^T by source row ascending, L^T by source row descending */
		for (int i = 0; i < n; i++)
			for (int k = P->ptr[i]; k < P->ptr[i + 1]; k++) if (KEEP(i, P->index[k])) tp[P->index[k] + 1]++;
		for (int i = 0; i < n; i++) tp[i + 1] += tp[i];
		int *fill = (int *)malloc(sizeof(int) * (size_t)(n + 1));
		if (!fill) { err = LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "malloc size = %D\n", (LIS_INT)n); goto out; }
		memcpy(fill, tp, sizeof(int) * (size_t)n);
		for (int q = 0; q < n; q++) {
			const int i = which == SW_UT ? q : n - 1 - q;
			for (int k = P->ptr[i]; k < P->ptr[i + 1]; k++) {
				const int c = P->index[k];
				if (KEEP(i, c)) { const int at = fill[c]++; tc[at] = i; tv[at] = P->value[k]; }
			}
		}
		free(fill);
	}
#undef KEEP
	err = lisi_sweep_build(s, n, tp, tc, tv, which == SW_U || which == SW_LT, NULL, NULL);
out:
	free(blk); free(tp); free(tc); free(tv);
	return err;
}

/* A: an assembled, split CSR matrix with WD, one rank */
static LIS_INT check_split(LIS_MATRIX A)
{
	LISCHK(lisi_matrix_check(A, LISI_CHECK_ASSEMBLED));
	if (A->matrix_type != LIS_MATRIX_CSR) return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "triangular solves are served for CSR storage only\n");
	if (!A->is_splited || !A->L || !A->U || !A->D || !A->WD || !A->WD->value) return LISI_ERR(LIS_ERR_ILL_ARG, "matrix A is not split or has no WD (lis_precon_create with -p ssor prepares it)\n");
	if (lisg.nprocs > 1) return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "triangular solves are served on one rank only\n");
	return LIS_SUCCESS;
}

/* the sweep `which` of the schedule for T blocks, built on first use; the HBM copy of A must be ready (its lifetime is the cache's) */
static LIS_INT get_sweep(LIS_MATRIX A, int T, int which, const liship_sweep_t **out)
{
	lisd_mat *d = MDEV(A);
	if (!d->ssor) { d->ssor = calloc(1, sizeof(lisd_ssor)); if (!d->ssor) return LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "malloc size = %D\n", (LIS_INT)sizeof(lisd_ssor)); }
	lisd_ssor *ss = (lisd_ssor *)d->ssor;
	sched_t *sc = NULL;
	for (int t = 0; t < 2; t++) if (ss->s[t].T == T) sc = &ss->s[t];
	if (!sc) {
		sc = &ss->s[ss->next];
		ss->next ^= 1;
		for (int w = 0; w < SW_COUNT; w++) lisi_sweep_free(&sc->sw[w]);
		sc->T = T;
	}
	sweep_t *s = &sc->sw[which];
	if (!s->built) {
		const double t0 = lis_wtime();
		LISCHK(sweep_make(A, which, T, s));
		ss->build_s += lis_wtime() - t0;
	}
	*out = &s->k;
	return LIS_SUCCESS;
}

static LIS_INT upload_wd(LIS_MATRIX A, const double **out)
{
	lisd_ssor *ss = (lisd_ssor *)MDEV(A)->ssor;
	if (ss->wd && ss->wd_n != A->n) { (void)liship_free(ss->wd); ss->wd = NULL; }
	if (!ss->wd) { HIPCHK(lisd_malloc((void **)&ss->wd, ((size_t)A->n + 2) * sizeof(double))); ss->wd_n = A->n; }
	if (A->n) HIPCHK(liship_memcpy_h2d(ss->wd, A->WD->value, sizeof(double) * (size_t)A->n, lisg.stream));
	*out = ss->wd;
	return LIS_SUCCESS;
}

static int blocks(void) { return lisg.ref_reductions > 0 ? lisg.ref_reductions : 1; }

/* ------------------------------------------------------------------ create */
LIS_INT lisi_ssor_create(LIS_SOLVER solver, LIS_PRECON precon)
{
	LIS_MATRIX A = solver->A;
	const LIS_INT storage = solver->options[LIS_OPTIONS_STORAGE];
	const double w = solver->params[LIS_PARAMS_SSOR_OMEGA - LIS_OPTIONS_LEN];
	LISCHK(lisi_matrix_check(A, LISI_CHECK_ASSEMBLED));
	/* refusals first: A is left as it was */
	if ((storage ? storage : A->matrix_type) != LIS_MATRIX_CSR)
		return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-p ssor is served for CSR storage only (A is untouched)\n");
	if (lisg.nprocs > 1) return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-p ssor is served on one rank only (A is untouched)\n");
	if (solver->options[LIS_OPTIONS_SCALE] != LIS_SCALE_NONE) return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-p ssor together with -scale is not served (A is untouched)\n");
	if (solver->options[LIS_OPTIONS_ADDS]) return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-p ssor with -adds true is not served (A is untouched)\n");
	if (A->matrix_type != LIS_MATRIX_CSR) LISCHK(lisi_matrix_retype(A, LIS_MATRIX_CSR, 0));      /* lis_matrix_convert_self */
	LISCHK(lis_matrix_split(A));
	if (A->use_wd != LIS_SOLVER_SOR) {           /* WD = D, scaled by omega, inverted (lis_matrix_diag_scale / _inverse) */
		if (!A->WD) {
			LIS_MATRIX_DIAG WD = (LIS_MATRIX_DIAG)calloc(1, sizeof(struct LIS_MATRIX_DIAG_STRUCT));
			if (WD) WD->value = (LIS_SCALAR *)calloc((size_t)(A->np > 0 ? A->np : 1), sizeof(LIS_SCALAR));
			if (!WD || !WD->value) { if (WD) free(WD); return LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "malloc size = %D\n", A->np); }
			WD->status = LIS_MATRIX_NULL; WD->is_destroy = LIS_TRUE; WD->bn = 1;
			WD->n = A->n; WD->nr = A->n; WD->gn = A->gn; WD->np = A->np;
			WD->comm = A->comm; WD->my_rank = A->my_rank; WD->nprocs = A->nprocs; WD->is = A->is; WD->ie = A->ie; WD->origin = A->origin;
			A->WD = WD;
		}
		for (LIS_INT i = 0; i < A->n; i++) { const double t = w * A->D->value[i]; A->WD->value[i] = 1.0 / t; }
		A->use_wd = LIS_SOLVER_SOR;
	}
	precon->A = A;
	return LIS_SUCCESS;
}

void lisi_ssor_wd_free(LIS_MATRIX A)
{
	if (A->WD) { free(A->WD->value); free(A->WD); A->WD = NULL; }
}

/* ------------------------------------------------------------------ the solve's side (lis_krylov.h d_psolve / d_psolveh) */
LIS_INT lisd_ssor_begin(LIS_MATRIX A, int *T)
{
	const liship_sweep_t *f, *b;
	const double *wd;
	*T = blocks();
	LISCHK(get_sweep(A, *T, SW_L, &f));
	LISCHK(get_sweep(A, *T, SW_U, &b));
	LISCHK(upload_wd(A, &wd));
	lisg.last_ssor = 1; lisg.last_ssor_blocks = *T;
	lisg.last_ssor_levels_fwd = f->nlev; lisg.last_ssor_levels_bwd = b->nlev;
	lisg.last_ssor_launches = f->ngroups + b->ngroups;
	return LIS_SUCCESS;
}

LIS_INT lisd_ssor_psolve(LIS_MATRIX A, int T, const double *b, double *x)
{
	const liship_sweep_t *f, *u;
	LISCHK(get_sweep(A, T, SW_L, &f));
	LISCHK(get_sweep(A, T, SW_U, &u));
	const double *wd = ((lisd_ssor *)MDEV(A)->ssor)->wd;
	HIPCHK(liship_sweep_f64(f, LISHIP_SWEEP_MUL, b, x, wd, lisg.stream));
	HIPCHK(liship_sweep_f64(u, LISHIP_SWEEP_SUB, NULL, x, wd, lisg.stream));
	return LIS_SUCCESS;
}

LIS_INT lisd_ssor_psolveh(LIS_MATRIX A, int T, const double *b, double *x)
{
	const liship_sweep_t *ut, *lt;
	LISCHK(get_sweep(A, T, SW_UT, &ut));
	LISCHK(get_sweep(A, T, SW_LT, &lt));
	const double *wd = ((lisd_ssor *)MDEV(A)->ssor)->wd;
	if (b != x) HIPCHK(liship_memcpy_d2d(x, b, sizeof(double) * (size_t)A->n, lisg.stream));
	HIPCHK(liship_sweep_f64(ut, LISHIP_SWEEP_SCAT, x, x, wd, lisg.stream));
	HIPCHK(liship_sweep_f64(lt, LISHIP_SWEEP_MUL, x, x, wd, lisg.stream));
	return LIS_SUCCESS;
}

/* ------------------------------------------------------------------ lis_matrix_solve / lis_matrix_solveh (ref lis_matrix_ops.c, CSR only)
 * LOWER / UPPER are sequential in the reference at any thread count (T = 1 here); SSOR takes the blocks of the solves. */
static LIS_INT solve_common(LIS_MATRIX A, LIS_VECTOR B, LIS_VECTOR X, LIS_INT flag, int herm)
{
	LISCHK(check_split(A));
	if (flag != LIS_MATRIX_LOWER && flag != LIS_MATRIX_UPPER && flag != LIS_MATRIX_SSOR) return LISI_ERR(LIS_ERR_ILL_ARG, "flag %D is not LOWER, UPPER or SSOR\n", flag);
	if (B->n != A->n || X->n != A->n) return LISI_ERR(LIS_ERR_ILL_ARG, "sizes of A, B and X do not match\n");
	LISCHK(lisd_mat_ready(A));
	const int T = flag == LIS_MATRIX_SSOR ? blocks() : 1;
	const liship_sweep_t *s1, *s2 = NULL;
	const double *wd;
	if (!herm) {
		LISCHK(get_sweep(A, T, flag == LIS_MATRIX_UPPER ? SW_U : SW_L, &s1));
		if (flag == LIS_MATRIX_SSOR) LISCHK(get_sweep(A, T, SW_U, &s2));
	} else {
		LISCHK(get_sweep(A, T, flag == LIS_MATRIX_UPPER ? SW_LT : SW_UT, &s1));
		if (flag == LIS_MATRIX_SSOR) LISCHK(get_sweep(A, T, SW_LT, &s2));
	}
	LISCHK(upload_wd(A, &wd));
	double *db, *dx;
	LISCHK(lisd_vec_in(B, &db));
	if (X == B) dx = db;
	else LISCHK(lisd_vec_out(X, &dx));
	if (!herm) {
		HIPCHK(liship_sweep_f64(s1, LISHIP_SWEEP_MUL, db, dx, wd, lisg.stream));
		if (s2) HIPCHK(liship_sweep_f64(s2, LISHIP_SWEEP_SUB, NULL, dx, wd, lisg.stream));
	} else {                                      /* X = B first (lis_matrix_solveh_csr :1774), then the scatter sweeps in place */
		if (dx != db) HIPCHK(liship_memcpy_d2d(dx, db, sizeof(double) * (size_t)A->n, lisg.stream));
		if (s2) {
			HIPCHK(liship_sweep_f64(s1, LISHIP_SWEEP_SCAT, dx, dx, wd, lisg.stream));
			HIPCHK(liship_sweep_f64(s2, LISHIP_SWEEP_MUL, dx, dx, wd, lisg.stream));
		} else HIPCHK(liship_sweep_f64(s1, LISHIP_SWEEP_MUL, dx, dx, wd, lisg.stream));
	}
	return lisd_vec_done(X);
}

LIS_INT lis_matrix_solve(LIS_MATRIX A, LIS_VECTOR B, LIS_VECTOR X, LIS_INT flag) { return solve_common(A, B, X, flag, 0); }
LIS_INT lis_matrix_solveh(LIS_MATRIX A, LIS_VECTOR B, LIS_VECTOR X, LIS_INT flag) { return solve_common(A, B, X, flag, 1); }

/* ------------------------------------------------------------------ introspection (include/lis_amd.h) */
LIS_INT lis_amd_last_solve_ssor(LIS_INT *blocks_out, LIS_INT *levels_fwd, LIS_INT *levels_bwd, LIS_INT *launches_per_psolve)
{
	if (blocks_out) *blocks_out = lisg.last_ssor ? lisg.last_ssor_blocks : 0;
	if (levels_fwd) *levels_fwd = lisg.last_ssor ? lisg.last_ssor_levels_fwd : 0;
	if (levels_bwd) *levels_bwd = lisg.last_ssor ? lisg.last_ssor_levels_bwd : 0;
	if (launches_per_psolve) *launches_per_psolve = lisg.last_ssor ? lisg.last_ssor_launches : 0;
	return lisg.last_ssor;
}

LIS_INT lis_amd_ssor_schedule_info(LIS_MATRIX A, double info[4])
{	/* {seconds spent building schedules for A, bytes per psolve, launches per psolve, levels of the forward sweep} at the solves' T */
	LISCHK(check_split(A));
	LISCHK(lisd_mat_ready(A));
	const liship_sweep_t *f, *b;
	const int T = blocks();
	LISCHK(get_sweep(A, T, SW_L, &f));
	LISCHK(get_sweep(A, T, SW_U, &b));
	lisd_ssor *ss = (lisd_ssor *)MDEV(A)->ssor;
	sched_t *sc = ss->s[0].T == T ? &ss->s[0] : &ss->s[1];
	info[0] = ss->build_s;
	info[1] = sc->sw[SW_L].bytes + sc->sw[SW_U].bytes;
	info[2] = (double)(f->ngroups + b->ngroups);
	info[3] = (double)f->nlev;
	return LIS_SUCCESS;
}

LIS_INT lis_amd_ssor_sweep_info(LIS_MATRIX A, LIS_INT sweep, LIS_INT info[6])
{	/* one of the four sweeps (0 forward on L, 1 backward on U, 2 forward on U^T, 3 backward on L^T) at the solves' T, read-only:
	 * {levels, launches, levels on a launch of their own, long rows in those levels, long rows in runs, terms} */
	LISCHK(check_split(A));
	if (sweep < 0 || sweep >= SW_COUNT || !info) return LISI_ERR(LIS_ERR_ILL_ARG, "sweep %D is not 0 .. 3, or info is NULL\n", sweep);
	LISCHK(lisd_mat_ready(A));
	const liship_sweep_t *s;
	LISCHK(get_sweep(A, blocks(), (int)sweep, &s));
	LIS_INT own = 0, long_own = 0, long_run = 0;
	for (int g = 0; g < s->ngroups; g++)
		for (int l = s->groups[3 * g]; l < s->groups[3 * g + 1]; l++) {
			const int nlong = s->h_nrows[l] - s->h_nshort[l];
			if (s->groups[3 * g + 2]) long_run += nlong;
			else { own++; long_own += nlong; }
		}
	info[0] = s->nlev; info[1] = s->ngroups; info[2] = own; info[3] = long_own; info[4] = long_run; info[5] = s->nnz;
	return LIS_SUCCESS;
}

LIS_INT lis_amd_ssor_psolve_times(LIS_MATRIX A, LIS_VECTOR B, LIS_VECTOR X, LIS_INT reps, double *ms)
{	/* reps psolves X = M^-1 B on the library's stream, each timed by device events (ms[k]) */
	LISCHK(check_split(A));
	LISCHK(lisd_mat_ready(A));
	const double *wd;
	int T = blocks();
	LISCHK(lisd_ssor_begin(A, &T));
	LISCHK(upload_wd(A, &wd));
	double *db, *dx;
	LISCHK(lisd_vec_in(B, &db));
	LISCHK(lisd_vec_out(X, &dx));
	void *timer = NULL;
	HIPCHK(liship_timer_create(&timer));
	LIS_INT err = LIS_SUCCESS;
	for (LIS_INT k = 0; k < reps && !err; k++) {
		float e = 0.0f;
		int rc = liship_timer_start(timer, lisg.stream);
		if (!rc) err = lisd_ssor_psolve(A, T, db, dx);
		if (!rc && !err) rc = liship_timer_stop(timer, lisg.stream);
		if (!rc && !err) rc = liship_stream_synchronize(lisg.stream);
		if (!rc && !err) rc = liship_timer_elapsed_ms(timer, &e);
		if (rc) err = lisi_hip_error(__FILE__, __func__, __LINE__, rc);
		ms[k] = e;
	}
	(void)liship_timer_destroy(timer);
	if (err) return err;
	return lisd_vec_done(X);
}
