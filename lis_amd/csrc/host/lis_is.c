/*
 * lis_is.c -- the I+S preconditioner (ref src/precon/lis_precon_is.c), the -is_level != 0 form: M^-1 = I - alpha S, S the first m + 1 stored
 * entries of every row of the strict upper part of A (m: -is_m, alpha: -is_alpha).
 *
 * create (ref :69-99): A in CSR storage is split and STAYS split, as after -p ssor: every later lis_matvec adds D, L, U in that order.
 * The solve (lis_solver.c scale_system, ref lis_solver.c:613-636) then multiplies A's parts and b by 1 / diag -- I + S is made for a unit diagonal --
 * and leaves them so, as -scale jacobi does; that drops the HBM copy, and begin cuts the rows again from the scaled U.
 *   psolve  (ref :449-458)  t = the first min(m + 1, length) entries of row i of A->U times x, from +0.0 in stored order; y[i] = x[i] - alpha t
 *   psolveh (ref :505-524)  the terms (alpha u) x[i] -- alpha u formed first -- added per output column in source-row order from +0.0, in the T
 *                           chunks of source rows of the reference-order mode; y = x - sum
 * The rows are truncated once per (alpha, m) in HBM (kernels/sainv.hip liship_is_truncate_f64, the row starts being the prefix sums of
 * min(m + 1, length) over A->U->ptr) into a row form and, with alpha u as values, its transposed form (kernels/transpose.hip); both live
 * on the HBM copy of A (lisd_mat.is) and are dropped with it.  Each application is one launch, the epilogue inside; y must not be x.
 * Refused, each before A is touched: -is_level 0 (that form builds a product matrix P and replaces the system), A not in CSR storage (the
 * reference converts A in place there), several ranks, -scale, -adds true, a matrix that lives in HBM only, the Jacobi solver.
 */
#include <stdio.h>
#include <limits.h>
#include "lis_krylov.h"

typedef struct {
	int n, m, nnz;
	double alpha;
	int *p, *i, *tp, *ti; double *v, *tv;            /* HBM: the truncated rows (values u) and their transposed form (values alpha u) */
} lisd_is;

void lisd_is_free(void *q)
{
	lisd_is *s = (lisd_is *)q;
	if (!s) return;
	(void)liship_free(s->p); (void)liship_free(s->i); (void)liship_free(s->v);
	(void)liship_free(s->tp); (void)liship_free(s->ti); (void)liship_free(s->tv);
	free(s);
}

static LIS_INT check_split(LIS_MATRIX A)
{
	LISCHK(lisi_matrix_check(A, LISI_CHECK_ASSEMBLED));
	if (lisg.nprocs > 1) return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-p is is served on one rank only (A is untouched)\n");
	if (A->matrix_type != LIS_MATRIX_CSR) return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-p is is served for CSR storage only: the reference converts A in place there (A is untouched)\n");
	if (!A->is_splited || !A->U || !A->U->ptr) return LISI_ERR(LIS_ERR_ILL_ARG, "matrix A is not split (lis_precon_create with -p is prepares it)\n");
	return LIS_SUCCESS;
}

static LIS_INT build(LIS_MATRIX A, double alpha, int m, lisd_is **out)
{
	const int n = A->n, keep = m < 0 ? 0 : (m >= INT_MAX - 1 ? INT_MAX : m + 1);
	const LIS_MATRIX_CORE U = A->U;
	int *tptr = (int *)malloc(sizeof(int) * ((size_t)n + 1));
	int *up = NULL, *ui = NULL; double *uv = NULL, *av = NULL;
	lisd_is *s = (lisd_is *)calloc(1, sizeof(lisd_is));
	LIS_INT err = LIS_SUCCESS;
	if (!tptr || !s) { free(tptr); free(s); return LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "malloc size = %D\n", (LIS_INT)n); }
	tptr[0] = 0;
	for (int r = 0; r < n; r++) { const int len = U->ptr[r + 1] - U->ptr[r]; tptr[r + 1] = tptr[r] + (len < keep ? len : keep); }
	s->n = n; s->m = m; s->alpha = alpha; s->nnz = tptr[n];
	const size_t unnz = (size_t)U->ptr[n];
	if ((err = lisd_upload_i(&up, U->ptr, (size_t)n + 1)) || (err = lisd_upload_i(&ui, U->index, unnz)) || (err = lisd_upload_d(&uv, U->value, unnz)) ||
	    (err = lisd_upload_i(&s->p, tptr, (size_t)n + 1)) || (err = lisd_upload_d(&s->v, NULL, (size_t)s->nnz)) || (err = lisd_upload_d(&av, NULL, (size_t)s->nnz))) goto out;
	{	int rc = lisd_malloc((void **)&s->i, ((size_t)s->nnz + 4) * sizeof(int));
		if (!rc) rc = liship_is_truncate_f64(n, keep, up, ui, uv, s->p, alpha, s->i, s->v, av, lisg.stream);
		if (!rc) rc = liship_stream_synchronize(lisg.stream);
		if (rc) { err = lisi_hip_error(__FILE__, __func__, __LINE__, rc); goto out; } }
	err = lisd_rows_transposed(n, s->nnz, s->p, s->i, av, &s->tp, &s->ti, &s->tv);
out:
	(void)liship_free(up); (void)liship_free(ui); (void)liship_free(uv); (void)liship_free(av);
	free(tptr);
	if (err) { lisd_is_free(s); return err; }
	*out = s;
	return LIS_SUCCESS;
}

static LIS_INT get_rows(LIS_MATRIX A, double alpha, int m, lisd_is **out)
{
	LISCHK(check_split(A));
	LISCHK(lisd_mat_ready(A));
	lisd_mat *d = MDEV(A);
	lisd_is *s = (lisd_is *)d->is;
	if (s && (s->alpha != alpha || s->m != m || s->n != A->n)) { lisd_is_free(s); d->is = s = NULL; }
	if (!s) { LISCHK(build(A, alpha, m, &s)); d->is = s; }
	*out = s;
	return LIS_SUCCESS;
}

static LIS_INT apply_on(const lisd_is *s, int transposed, const double *x, double *y)
{
	if (!transposed) HIPCHK(liship_is_psolve_f64(s->n, s->p, s->i, s->v, s->alpha, x, y, lisg.stream));
	else HIPCHK(liship_is_psolveh_f64(s->n, s->n, lisg.ref_reductions > 1 ? lisg.ref_reductions : 1, s->tp, s->ti, s->tv, x, y, lisg.stream));
	return LIS_SUCCESS;
}

/* ------------------------------------------------------------------ create */
LIS_INT lisi_is_create(LIS_SOLVER solver, LIS_PRECON precon)
{
	LIS_MATRIX A = solver->A;
	const LIS_INT storage = solver->options[LIS_OPTIONS_STORAGE];
	LISCHK(lisi_matrix_check(A, LISI_CHECK_ASSEMBLED));
	/* refusals first, none of which needs a device: A is left as it was */
	if (solver->options[LIS_OPTIONS_ISLEVEL] == 0)
		return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-p is with -is_level 0 is not served: that form builds a product matrix and replaces the system (A is untouched)\n");
	if (lisg.nprocs > 1) return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-p is is served on one rank only (A is untouched)\n");
	if (A->matrix_type != LIS_MATRIX_CSR || (storage && storage != LIS_MATRIX_CSR))
		return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-p is is served for CSR storage only: the reference converts A in place there (A is untouched)\n");
	if (solver->options[LIS_OPTIONS_SCALE] != LIS_SCALE_NONE) return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-p is together with -scale is not served (A is untouched)\n");
	if (solver->options[LIS_OPTIONS_ADDS]) return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-p is with -adds true is not served (A is untouched)\n");
	if (MDEV(A)->device_only) return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-p is on a matrix that lives in HBM only is not served: its split needs the host arrays (A is untouched)\n");
	if (solver->options[LIS_OPTIONS_SOLVER] == LIS_SOLVER_JACOBI)
		return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "the Jacobi solver with -p is is not served (A is untouched)\n");
	LISCHK(lisd_init());
	LISCHK(lis_matrix_split(A));
	lisd_is *s;
	LISCHK(get_rows(A, (double)solver->params[LIS_PARAMS_ALPHA - LIS_OPTIONS_LEN], (int)solver->options[LIS_OPTIONS_M], &s));
	precon->A = A;
	return LIS_SUCCESS;
}

/* ------------------------------------------------------------------ the solve's side (the I+S row of lisi_precon_kinds) */
LIS_INT lisd_is_begin(LIS_MATRIX A, LIS_SOLVER solver, lisi_precon_state *st)
{
	lisd_is *s;
	st->A = A; st->n = A->n; st->param = (double)solver->params[LIS_PARAMS_ALPHA - LIS_OPTIONS_LEN]; st->m = (int)solver->options[LIS_OPTIONS_M];
	LISCHK(get_rows(A, st->param, st->m, &s));     /* (made now if the HBM copy was rebuilt since lis_precon_create) */
	lisg.last_is = 1; lisg.last_is_m = st->m;
	return LIS_SUCCESS;
}

LIS_INT lisd_is_apply(const lisi_precon_state *st, int transposed, const double *b, double *x)
{	/* x = M^-1 b, or M^-H b (b must NOT be x) */
	lisd_is *s = (lisd_is *)MDEV(st->A)->is;
	if (!s || s->alpha != st->param || s->m != st->m) LISCHK(get_rows(st->A, st->param, st->m, &s));
	return apply_on(s, transposed, b, x);
}

/* ------------------------------------------------------------------ introspection and tools (include/lis_amd.h) */
LIS_INT lis_amd_last_solve_is(LIS_INT *m)
{
	if (m) *m = lisg.last_is ? lisg.last_is_m : 0;
	return lisg.last_is;
}

LIS_INT lis_amd_is_psolve(LIS_MATRIX A, LIS_SCALAR alpha, LIS_INT m, LIS_VECTOR X, LIS_VECTOR Y, LIS_INT transposed)
{
	lisd_is *s;
	LISCHK(check_split(A));
	LISCHK(lisd_init());
	LISCHK(get_rows(A, (double)alpha, (int)m, &s));
	if (X->n != A->n || Y->n != A->n || X == Y) return LISI_ERR(LIS_ERR_ILL_ARG, "sizes of A, X and Y do not match, or Y is X\n");
	double *dx, *dy;
	LISCHK(lisd_vec_in(X, &dx));
	LISCHK(lisd_vec_out(Y, &dy));
	const LIS_INT err = apply_on(s, transposed != 0, dx, dy);
	const LIS_INT done = lisd_vec_done(Y);
	return err ? err : done;
}
