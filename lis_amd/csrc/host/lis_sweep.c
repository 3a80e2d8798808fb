/*
 * lis_sweep.c -- the host side of the level-scheduled sweeps, shared by SSOR (lis_ssor.c) and ILU(k) (lis_ilu.c); the device side is
 * kernels/level_schedule.hpp.  A client lists the terms of a sweep (lisi_sweep_terms) and lays them out by level (lisi_sweep_build).
 *
 * Schedule: the level of a row is 1 + the largest level of the rows its terms read; rows of a level and their terms are stored
 * contiguously in level order, the in-row order of the listing kept.  The transposed listings hold, for row jj of U^T, its terms
 * by source row ascending, of L^T by source row descending (ties by position in the source row): a row-wise sum in that order is
 * the reference's scatter sum bit for bit.
 */
#include <stdio.h>
#include "lis_krylov.h"

int lisi_sweep_blocks(void) { return lisg.ref_reductions > 0 ? lisg.ref_reductions : 1; }

/* block of row i among T blocks of LIS_GET_ISIE (ref include/lis.h:1067): the first n % T blocks hold n / T + 1 rows */
int *lisi_block_of(int n, int T)
{
	int *b = (int *)malloc(sizeof(int) * (size_t)(n > 0 ? n : 1));
	if (!b) return NULL;
	const int q = n / T, rem = n % T;
	for (int i = 0; i < n; i++) b[i] = (i < rem * (q + 1)) ? i / (q + 1) : rem + (i - rem * (q + 1)) / q;
	return b;
}

/* the terms of one sweep over the row-wise pattern (ptr, idx), listed row by row: tp[n + 1] offsets, tc the row each term reads,
 * tid its index in idx (caller frees all three).  LISI_TERMS_ROWS: the rows as stored; _T_ASC / _T_DESC: the transposed pattern,
 * the terms of a row by source row ascending / descending, ties by position in the source row.  blk not NULL: only the terms
 * whose column is a row and lies in its row's block */
LIS_INT lisi_sweep_terms(int n, const int *ptr, const int *idx, const int *blk, int order, int **tp_out, int **tc_out, int **tid_out)
{
	const int nnz = ptr[n];
	int *tp = (int *)calloc((size_t)n + 2, sizeof(int)), *fill = (int *)malloc(sizeof(int) * (size_t)(n + 1));
	int *tc = (int *)malloc(sizeof(int) * (size_t)(nnz + 1)), *tid = (int *)malloc(sizeof(int) * (size_t)(nnz + 1));
	if (!tp || !fill || !tc || !tid) { free(tp); free(fill); free(tc); free(tid); return LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "malloc size = %D\n", (LIS_INT)nnz); }
#define KEEP(i, c) (!blk || ((c) >= 0 && (c) < n && blk[(i)] == blk[(c)]))
#define LISTED_ROW(i, c) (order == LISI_TERMS_ROWS ? (i) : (c))
	for (int i = 0; i < n; i++)
		for (int k = ptr[i]; k < ptr[i + 1]; k++) if (KEEP(i, idx[k])) tp[LISTED_ROW(i, idx[k]) + 1]++;
	for (int i = 0; i < n; i++) tp[i + 1] += tp[i];
	memcpy(fill, tp, sizeof(int) * (size_t)n);
	for (int q = 0; q < n; q++) {
		const int i = order == LISI_TERMS_T_DESC ? n - 1 - q : q;
		for (int k = ptr[i]; k < ptr[i + 1]; k++) {
			const int c = idx[k];
			if (KEEP(i, c)) { const int at = fill[LISTED_ROW(i, c)]++; tc[at] = order == LISI_TERMS_ROWS ? c : i; tid[at] = k; }
		}
	}
#undef LISTED_ROW
#undef KEEP
	free(fill);
	*tp_out = tp; *tc_out = tc; *tid_out = tid;
	return LIS_SUCCESS;
}

void lisi_sweep_free(lisi_sweep_t *s)
{
	(void)liship_free(s->lptr); (void)liship_free(s->llong); (void)liship_free(s->rows); (void)liship_free(s->rptr);
	(void)liship_free(s->col); (void)liship_free(s->val);
	free(s->groups); free(s->nrows); free(s->nshort);
	memset(s, 0, sizeof(*s));
}

/* levels + level-ordered layout of n rows whose terms (tp, tc, tv) read only rows before them (desc = 0) or after them (desc = 1).
 * tv NULL: no values (a schedule only, or values that arrive later on the device); weight: what decides whether row i is a long
 * row instead of its term count; src_out: for every place of the layout the term (index into tc) that lies there (caller frees) */
LIS_INT lisi_sweep_build(lisi_sweep_t *s, int n, const int *tp, const int *tc, const double *tv, int desc, const int *weight, int **src_out)
{
	return lisi_sweep_build_places(s, n, tp, tc, tv, desc, weight, src_out, 1);
}

/* the same with `place` doubles of room per term in val (block layouts: bn*bn; values given by tv only for place == 1) */
LIS_INT lisi_sweep_build_places(lisi_sweep_t *s, int n, const int *tp, const int *tc, const double *tv, int desc, const int *weight, int **src_out, int place)
{
	if (place < 1 || (tv && place != 1)) return LISI_ERR(LIS_ERR_ILL_ARG, "a sweep layout takes its values at build time only with one double per term\n");
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
	if ((err = lisd_upload_i(&s->lptr, lptr, (size_t)nlev + 1)) || (err = lisd_upload_i(&s->llong, llong, (size_t)nlev + 1)) || (err = lisd_upload_i(&s->rows, rows, (size_t)n)) ||
	    (err = lisd_upload_i(&s->rptr, rptr, (size_t)n + 1)) || (err = lisd_upload_i(&s->col, col, (size_t)nnz)) || ((tv || src_out) && (err = lisd_upload_d(&s->val, val, (size_t)nnz * (size_t)place)))) goto out;      /* (values that arrive later: room only) */
	{	int rc = liship_stream_synchronize(lisg.stream);          /* (the host arrays go below) */
		if (rc) { err = lisi_hip_error(__FILE__, __func__, __LINE__, rc); goto out; } }
	s->k.nlev = nlev; s->k.nrows = n; s->k.nnz = nnz; s->k.ngroups = ng;
	s->k.lptr = s->lptr; s->k.llong = s->llong; s->k.rows = s->rows; s->k.rptr = s->rptr; s->k.col = s->col; s->k.val = s->val;
	s->k.groups = s->groups; s->k.h_nrows = s->nrows; s->k.h_nshort = s->nshort;
	s->built = 1;
	if (src_out) { *src_out = src; src = NULL; }
out:
#undef ROW_WEIGHT
	free(lev); free(rows); free(rptr); free(col); free(val); free(src); free(lptr); free(llong); free(fill_s); free(fill_l);
	if (err) lisi_sweep_free(s);
	return err;
}

/* bytes one application moves: the level-ordered streams (row id and offset per row, column and value per term) + the vectors,
 * vec_bytes_per_row = 24 with a diagonal (b, x, wd), 16 plain (b, x) */
double lisi_sweep_bytes(int n, int nnz, double vec_bytes_per_row)
{
	return lisi_sweep_bytes_places(n, nnz, 1, vec_bytes_per_row);
}
/* ... with `place` doubles per term (a block layout: n block rows, vec_bytes_per_row per block row) */
double lisi_sweep_bytes_places(int n, int nnz, int place, double vec_bytes_per_row)
{
	return 4.0 * n + 4.0 * (n + 1) + (4.0 + 8.0 * place) * nnz + vec_bytes_per_row * n;
}

/* the launches of a schedule: {levels, launches, levels on a launch of their own, long rows in those levels, long rows in runs} */
void lisi_sweep_census(const liship_sweep_t *s, LIS_INT census[5])
{
	LIS_INT own = 0, long_own = 0, long_run = 0;
	for (int g = 0; g < s->ngroups; g++)
		for (int l = s->groups[3 * g]; l < s->groups[3 * g + 1]; l++) {
			const int nlong = s->h_nrows[l] - s->h_nshort[l];
			if (s->groups[3 * g + 2]) long_run += nlong;
			else { own++; long_own += nlong; }
		}
	census[0] = s->nlev; census[1] = s->ngroups; census[2] = own; census[3] = long_own; census[4] = long_run;
}

/* reps calls of apply(ctx) on the library's stream, each timed by device events: ms[k] (ms NULL: timed, not kept) */
LIS_INT lisi_sweep_times(LIS_INT reps, LIS_INT (*apply)(void *ctx), void *ctx, double *ms)
{
	void *timer = NULL;
	HIPCHK(liship_timer_create(&timer));
	LIS_INT err = LIS_SUCCESS;
	for (LIS_INT k = 0; k < reps && !err; k++) {
		float e = 0.0f;
		int rc = liship_timer_start(timer, lisg.stream);
		if (!rc) err = apply(ctx);
		if (!rc && !err) rc = liship_timer_stop(timer, lisg.stream);
		if (!rc && !err) rc = liship_stream_synchronize(lisg.stream);
		if (!rc && !err) rc = liship_timer_elapsed_ms(timer, &e);
		if (rc) err = lisi_hip_error(__FILE__, __func__, __LINE__, rc);
		if (ms) ms[k] = e;
	}
	(void)liship_timer_destroy(timer);
	return err;
}
