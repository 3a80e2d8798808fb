/*
 * lis_bjacobi.c -- the block Jacobi preconditioner (ref src/precon/lis_precon_jacobi.c:220-293) inverted and applied in HBM (kernels/bdiag.hip).
 *
 * create (ref :221-251): -storage conversion of the caller's A (lis_matrix_convert_self, lis_matrix_ops.c:326-368: only when -storage
 * names another type than A has; a BSR matrix keeps its blocks whatever -storage_block says).  A that is no BSR matrix after that:
 * the solver's option and the preconditioner become Jacobi, and lis_precon_create goes on with the Jacobi row's create.  A BSR matrix:
 * lis_matrix_split(A) -- A STAYS split, every later lis_matvec adds D, L, U in that order --, WD = D with 1.0 on the diagonal of the
 * last block's padding when bn does not divide n (lis_matrix_diag.c:787-794), every block inverted by lis_array_ge's statement.
 *   psolve  = lis_matrix_diag_matvec(WD, B, X)    (lis_matrix_diag.c:810-895)
 *   psolveh = lis_matrix_diag_matvech(WD, B, X)   (:899-978)
 * Nothing here depends on a thread count: the reference gives each block to one thread.
 *
 * The inverse lives in HBM, cached on the HBM copy of A (lisd_mat.bjacobi) and dropped with it (lisd_mat_free: host edits, page-watch
 * writes, conversions); it is made from A->D->value, the values a split matrix multiplies by.  precon->WD gets a copy on the host.
 * Refused, each before A is touched: several ranks, -scale, -adds true, VBR, non-square blocks, a matrix that lives in HBM only, the
 * Jacobi solver.
 */
#include <stdio.h>
#include "lis_krylov.h"

typedef struct {
	int n, nr, bn;
	double *inv;                               /* HBM: nr blocks of bn x bn, column-major, inverted */
} lisd_bjacobi;

void lisd_bjacobi_free(void *p)
{
	lisd_bjacobi *bj = (lisd_bjacobi *)p;
	if (!bj) return;
	(void)liship_free(bj->inv);
	free(bj);
}

/* A: an assembled, split BSR matrix with square blocks, one rank */
static LIS_INT check_block(LIS_MATRIX A)
{
	LISCHK(lisi_matrix_check(A, LISI_CHECK_ASSEMBLED));
	if (A->matrix_type != LIS_MATRIX_BSR || A->bnr != A->bnc) return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "block Jacobi is served for BSR storage with square blocks only\n");
	if (!A->is_splited || !A->D || !A->D->value) return LISI_ERR(LIS_ERR_ILL_ARG, "matrix A is not split (lis_precon_create with -p bjacobi prepares it)\n");
	if (lisg.nprocs > 1) return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "block Jacobi is served on one rank only\n");
	return LIS_SUCCESS;
}

/* the inverted block diagonal of A on its HBM copy, made on first use */
static LIS_INT get_inverse(LIS_MATRIX A, lisd_bjacobi **out)
{
	LISCHK(check_block(A));
	LISCHK(lisd_mat_ready(A));
	lisd_mat *d = MDEV(A);
	if (!d->bjacobi) {
		const int bn = A->bnr, nr = A->nr;
		const size_t count = (size_t)nr * bn * bn;
		double *work = NULL;
		lisd_bjacobi *bj = (lisd_bjacobi *)calloc(1, sizeof(lisd_bjacobi));
		if (!bj) return LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "malloc size = %D\n", (LIS_INT)sizeof(lisd_bjacobi));
		bj->n = A->n; bj->nr = nr; bj->bn = bn;
		LIS_INT err = lisd_upload_d(&bj->inv, A->D->value, count);
		int rc = 0;
		if (!err && bn > 8) rc = lisd_malloc((void **)&work, count * sizeof(double));          /* (the generic kernel's LU copies: bn*bn doubles per block) */
		if (!err && !rc) rc = liship_bdiag_inverse_f64(A->n, nr, bn, bj->inv, work, lisg.stream);
		if (!err && !rc) rc = liship_stream_synchronize(lisg.stream);                      /* (A->D->value and work are free to go) */
		(void)liship_free(work);
		if (!err && rc) err = lisi_hip_error(__FILE__, __func__, __LINE__, rc);
		if (err) { lisd_bjacobi_free(bj); return err; }
		d->bjacobi = bj;
	}
	*out = (lisd_bjacobi *)d->bjacobi;
	return LIS_SUCCESS;
}

static LIS_INT apply(const lisd_bjacobi *bj, int transposed, const double *b, double *x)
{
	HIPCHK(liship_bdiag_matvec_f64(bj->n, bj->nr, bj->bn, transposed, bj->inv, b, x, lisg.stream));
	return LIS_SUCCESS;
}

/* ------------------------------------------------------------------ create */
static void wd_free(LIS_MATRIX_DIAG WD)
{
	if (WD) { free(WD->value); free(WD); }
}

void lisi_bjacobi_wd_free(LIS_PRECON precon)
{
	if (precon->WD && precon->WD->is_destroy) wd_free(precon->WD);
	precon->WD = NULL;
}

/* What lis_matrix_convert_self (ref lis_matrix_ops.c:326-368) makes of A under -storage / -storage_block, shared by the preconditioners
 * that work on blocks (-p bjacobi, -p ssor): the type, and for BSR the blocks A has, or the ones the conversion makes -- -storage_block b
 * gives b x b, none the sizes of lis_matrix_set_blocksize; a BSR matrix keeps its blocks whatever -storage_block says.  Nothing is touched. */
LIS_INT lisi_storage_result(LIS_MATRIX A, LIS_INT storage, LIS_INT block, LIS_INT *bnr, LIS_INT *bnc)
{
	const LIS_INT result = storage ? storage : A->matrix_type;
	*bnr = *bnc = 1;
	if (result == LIS_MATRIX_BSR) {
		const int converts = A->matrix_type != LIS_MATRIX_BSR;
		if (converts && block > 0) *bnr = *bnc = block;
		else { *bnr = converts ? A->conv_bnr : A->bnr; *bnc = converts ? A->conv_bnc : A->bnc; }
	}
	return result;
}

/* ... and the conversion itself, only when -storage names another type than A has */
LIS_INT lisi_convert_self(LIS_MATRIX A, LIS_INT result, LIS_INT block)
{
	if (result != A->matrix_type) LISCHK(lisi_matrix_retype(A, result, result == LIS_MATRIX_BSR ? block : 0));
	return LIS_SUCCESS;
}

LIS_INT lisi_bjacobi_create(LIS_SOLVER solver, LIS_PRECON precon)
{
	LIS_MATRIX A = solver->A;
	const LIS_INT storage = solver->options[LIS_OPTIONS_STORAGE], block = solver->options[LIS_OPTIONS_STORAGE_BLOCK];
	PPRIV(precon)->from_bjacobi = 1;             /* (stays set when the type below becomes Jacobi: the fallback's mark) */
	LISCHK(lisi_matrix_check(A, LISI_CHECK_ASSEMBLED));
	LISCHK(lisd_init());                         /* no device: the no-device code, before anything that could succeed */
	LIS_INT bnr, bnc;
	const LIS_INT result = lisi_storage_result(A, storage, block, &bnr, &bnc);       /* what A is after lis_matrix_convert_self */
	/* refusals first: A is left as it was */
	if (lisg.nprocs > 1) return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-p bjacobi is served on one rank only (A is untouched)\n");
	if (solver->options[LIS_OPTIONS_SCALE] != LIS_SCALE_NONE) return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-p bjacobi together with -scale is not served (A is untouched)\n");
	if (solver->options[LIS_OPTIONS_ADDS]) return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-p bjacobi with -adds true is not served (A is untouched)\n");
	if (result == LIS_MATRIX_VBR) return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-p bjacobi on VBR storage is not served (A is untouched)\n");
	if (lisi_format_one_rank(result)) return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-p bjacobi on %s storage is not served: such a matrix is never split (A is untouched)\n", lisi_format_name(result));
	if (result == LIS_MATRIX_BSR && bnr != bnc)
		return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-p bjacobi on %D x %D blocks is not served: a BSR matrix is split for square blocks only (A is untouched)\n", bnr, bnc);
	if (result == LIS_MATRIX_BSR && MDEV(A)->device_only)
		return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-p bjacobi on a matrix that lives in HBM only is not served: its split needs the host arrays (A is untouched)\n");
	if (solver->options[LIS_OPTIONS_SOLVER] == LIS_SOLVER_JACOBI)
		return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "the Jacobi solver with -p bjacobi (system rescaling) is not served (A is untouched)\n");
	LISCHK(lisi_convert_self(A, result, block));
	if (A->matrix_type != LIS_MATRIX_BSR) {      /* no block matrix: -p jacobi from here on (ref :233-239), lis_precon_create builds D */
		solver->options[LIS_OPTIONS_PRECON] = LIS_PRECON_TYPE_JACOBI;
		precon->precon_type = LIS_PRECON_TYPE_JACOBI;
		return LIS_SUCCESS;
	}
	LISCHK(lis_matrix_split(A));
	lisd_bjacobi *bj;
	LISCHK(get_inverse(A, &bj));
	/* precon->WD: what the reference holds there (lis_matrix_diag_duplicate + copy + inverse), its values copied home */
	const size_t count = (size_t)bj->nr * bj->bn * bj->bn;
	LIS_MATRIX_DIAG WD = (LIS_MATRIX_DIAG)calloc(1, sizeof(struct LIS_MATRIX_DIAG_STRUCT));
	if (WD) WD->value = (LIS_SCALAR *)calloc(count ? count : 1, sizeof(LIS_SCALAR));
	if (!WD || !WD->value) { wd_free(WD); return LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "malloc size = %D\n", (LIS_INT)count); }
	WD->status = LIS_MATRIX_NULL; WD->is_destroy = LIS_TRUE; WD->bn = bj->bn; WD->nr = bj->nr;
	WD->n = A->n; WD->gn = A->gn; WD->np = A->np;
	WD->comm = A->comm; WD->my_rank = A->my_rank; WD->nprocs = A->nprocs; WD->is = A->is; WD->ie = A->ie; WD->origin = A->origin;
	precon->WD = WD;                             /* (lis_precon_destroy frees it, also after the error below) */
	if (count) LISCHK(lisd_staged_d2h(WD->value, bj->inv, sizeof(double) * count));
	precon->A = A;
	return LIS_SUCCESS;
}

/* ------------------------------------------------------------------ the solve's side (the block Jacobi row of lisi_precon_kinds) */
LIS_INT lisd_bjacobi_begin(LIS_MATRIX A, LIS_SOLVER solver, lisi_precon_state *st)
{	/* checked and resolved once per solve */
	lisd_bjacobi *bj;
	(void)solver;
	st->A = A; st->n = A->n;
	LISCHK(get_inverse(A, &bj));                 /* (made now if the HBM copy was rebuilt since lis_precon_create) */
	lisg.last_bjacobi = 1; lisg.last_bjacobi_bn = bj->bn; lisg.last_bjacobi_nr = bj->nr;
	return LIS_SUCCESS;
}

LIS_INT lisd_bjacobi_apply(const lisi_precon_state *st, int transposed, const double *b, double *x)
{	/* x = M^-1 b, or M^-H b (b must NOT be x).  Per iteration: what begin resolved, read off the HBM copy with no checks between the loop's launches;
	 * only a copy that a product rebuilt in mid-solve (a host write seen by the page watch) has lost it, and then it is made again instead of applied stale */
	lisd_bjacobi *bj = (lisd_bjacobi *)MDEV(st->A)->bjacobi;
	if (!bj) LISCHK(get_inverse(st->A, &bj));
	return apply(bj, transposed, b, x);
}

/* ------------------------------------------------------------------ introspection and tools (include/lis_amd.h) */
LIS_INT lis_amd_last_solve_bjacobi(LIS_INT *bn, LIS_INT *nr, LIS_INT *fell_back)
{
	if (bn) *bn = lisg.last_bjacobi ? lisg.last_bjacobi_bn : 0;
	if (nr) *nr = lisg.last_bjacobi ? lisg.last_bjacobi_nr : 0;
	if (fell_back) *fell_back = lisg.last_bjacobi_fallback;
	return lisg.last_bjacobi;
}

static LIS_INT tool_inverse(LIS_MATRIX A, lisd_bjacobi **bj)
{
	LISCHK(lisi_matrix_check(A, LISI_CHECK_ASSEMBLED));
	LISCHK(lisd_init());
	return get_inverse(A, bj);
}

LIS_INT lis_amd_bjacobi_copy(LIS_MATRIX A, LIS_SCALAR *out)
{
	lisd_bjacobi *bj;
	LISCHK(tool_inverse(A, &bj));
	const size_t count = (size_t)bj->nr * bj->bn * bj->bn;
	if (out && count) LISCHK(lisd_staged_d2h(out, bj->inv, sizeof(double) * count));
	return LIS_SUCCESS;
}

LIS_INT lis_amd_bjacobi_psolve(LIS_MATRIX A, LIS_INT transposed, LIS_VECTOR B, LIS_VECTOR X)
{
	lisd_bjacobi *bj;
	LISCHK(tool_inverse(A, &bj));
	if (B->n != A->n || X->n != A->n || X == B) return LISI_ERR(LIS_ERR_ILL_ARG, "sizes of A, B and X do not match, or X is B\n");
	double *db, *dx;
	LISCHK(lisd_vec_in(B, &db));
	LISCHK(lisd_vec_out(X, &dx));
	const LIS_INT err = apply(bj, transposed != 0, db, dx);
	const LIS_INT done = lisd_vec_done(X);
	return err ? err : done;
}

typedef struct { LIS_MATRIX A; lisd_bjacobi *bj; const double *b; double *x; } timed_args;
static LIS_INT inverse_once(void *ctx)
{	/* in place on a scratch copy of D's blocks: the inverse of the inverse is D again to rounding, so every repetition finds blocks like A's */
	const timed_args *t = (const timed_args *)ctx;
	const lisd_bjacobi *bj = t->bj;
	HIPCHK(liship_bdiag_inverse_f64(bj->n, bj->nr, bj->bn, bj->inv, bj->inv + (size_t)bj->nr * bj->bn * bj->bn, lisg.stream));
	return LIS_SUCCESS;
}
static LIS_INT psolve_once(void *ctx) { const timed_args *t = (const timed_args *)ctx; return apply(t->bj, 0, t->b, t->x); }
static LIS_INT pmul_once(void *ctx)
{
	const timed_args *t = (const timed_args *)ctx;
	HIPCHK(liship_pmul_f64(t->bj->n, t->b, t->bj->inv, t->x, lisg.stream));       /* the Jacobi psolve: z = r .* dinv (any n doubles serve as dinv) */
	return LIS_SUCCESS;
}

LIS_INT lis_amd_bjacobi_times(LIS_MATRIX A, LIS_VECTOR B, LIS_VECTOR X, LIS_INT reps, double *inverse_ms, double *psolve_ms, double *jacobi_ms)
{	/* reps inversions of a copy of D's blocks (the kernel alone), reps psolves X = M^-1 B and reps Jacobi psolves X = B .* d of the same
	 * length, each timed by device events on the library's stream */
	lisd_bjacobi *bj;
	LISCHK(tool_inverse(A, &bj));
	if (B->n != A->n || X->n != A->n || X == B) return LISI_ERR(LIS_ERR_ILL_ARG, "sizes of A, B and X do not match, or X is B\n");
	const size_t count = (size_t)bj->nr * bj->bn * bj->bn;
	if (count < (size_t)bj->n) return LISI_ERR(LIS_ERR_ILL_ARG, "no blocks\n");
	lisd_bjacobi t = *bj;                          /* a scratch of its own: [the copy | the generic kernel's work] */
	t.inv = NULL;
	HIPCHK(lisd_malloc((void **)&t.inv, 2 * count * sizeof(double)));
	LIS_INT err = LIS_SUCCESS;
	int rc = liship_memcpy_h2d(t.inv, A->D->value, count * sizeof(double), lisg.stream);
	if (!rc) rc = liship_stream_synchronize(lisg.stream);
	if (rc) err = lisi_hip_error(__FILE__, __func__, __LINE__, rc);
	double *db = NULL, *dx = NULL;
	if (!err) err = lisd_vec_in(B, &db);
	const int x_out = !err && !(err = lisd_vec_out(X, &dx));
	if (!err) {
		timed_args scratch = {A, &t, db, dx}, live = {A, bj, db, dx};
		err = lisi_sweep_times(reps, inverse_once, &scratch, inverse_ms);
		if (!err) err = lisi_sweep_times(reps, pmul_once, &live, jacobi_ms);
		if (!err) err = lisi_sweep_times(reps, psolve_once, &live, psolve_ms);
	}
	(void)liship_free(t.inv);
	if (x_out) { const LIS_INT done = lisd_vec_done(X); if (!err) err = done; }      /* (also after a failed launch: X was handed out for writing) */
	return err;
}
