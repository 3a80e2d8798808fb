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
 * Schedule: the four sweeps (L, U, and for psolveh U^T and L^T) keep the terms whose row and column lie in the same block, are
 * listed and laid out by level by lis_sweep.c in the reference's order of additions, built on the host (O(nnz), from the split
 * parts) on first use, cached on the HBM copy of A (lisd_mat.ssor) and dropped with it (lisd_mat_free: host edits, page-watch
 * writes, conversions).
 *
 * BSR storage with square blocks of 1 .. 8 (A is BSR, or becomes BSR by -storage bsr -storage_block k: the conversion step of
 * lis_bjacobi.c): block SSOR on kernels/bsptrsv.hip.  lis_matrix_solve_bsr / lis_matrix_solveh_bsr (ref lis_matrix_bsr.c:1397-2090) hold
 * no OpenMP pragma: the block sweeps are serial in the reference at every thread count, so the block schedule has ONE block whatever the
 * reference-order mode's T is (T changes only the reductions and products of a solve).  WD = omega D block by block (alpha * d), 1.0 on
 * the diagonal of the last block's padding, every block inverted by lis_array_ge (kernels/bdiag.hip) -- made in HBM, copied home once
 * per build into A->WD->value.  The term lists of A->L / A->U (bptr, bindex) go through the same builders, a place holding bn*bn doubles
 * filled by the block gather; the first sweep of SSOR-h keeps WD^T x per block row in a work vector beside WD.
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
	size_t wd_n;                               /* doubles of it: n, or nr * bn * bn on BSR storage */
	double *work;                              /* BSR, bn > 1: nr * bn doubles, what the first sweep of SSOR-h hands on */
	double build_s;                            /* host seconds spent building schedules */
} lisd_ssor;

void lisd_ssor_free(void *p)
{
	lisd_ssor *ss = (lisd_ssor *)p;
	if (!ss) return;
	for (int t = 0; t < 2; t++) for (int w = 0; w < SW_COUNT; w++) lisi_sweep_free(&ss->s[t].sw[w]);
	(void)liship_free(ss->wd); (void)liship_free(ss->work);
	free(ss);
}

/* one sweep under T blocks: the terms whose row and column lie in the same block (T = 1: all of them), with their values */
static LIS_INT sweep_make(LIS_MATRIX A, int which, int T, sweep_t *s)
{
	const int n = A->n;
	LIS_MATRIX_CORE P = (which == SW_L || which == SW_LT) ? A->L : A->U;
	int *blk = lisi_block_of(n, T), *tp = NULL, *tc = NULL, *tid = NULL;
	double *tv = NULL;
	LIS_INT err = LIS_SUCCESS;
	if (!blk) { err = LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "malloc size = %D\n", (LIS_INT)n); goto out; }
	if ((err = lisi_sweep_terms(n, P->ptr, P->index, blk, SW_TERMS(which), &tp, &tc, &tid))) goto out;
	tv = (double *)malloc(sizeof(double) * (size_t)(tp[n] + 1));
	if (!tv) { err = LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "malloc size = %D\n", (LIS_INT)tp[n]); goto out; }
	for (int k = 0; k < tp[n]; k++) tv[k] = P->value[tid[k]];
	if ((err = lisi_sweep_build(s, n, tp, tc, tv, SW_DESC(which), NULL, NULL))) goto out;
	s->bytes = lisi_sweep_bytes(n, s->k.nnz, 24.0);
out:
	free(blk); free(tp); free(tc); free(tid); free(tv);
	return err;
}

#define IS_BLOCK(A) ((A)->matrix_type == LIS_MATRIX_BSR)
#define BLOCK_BN(A) (IS_BLOCK(A) ? (int)(A)->bnr : 1)
#define WD_COUNT(A) (IS_BLOCK(A) ? (size_t)(A)->nr * (size_t)((A)->bnr * (A)->bnr) : (size_t)(A)->n)

/* the sweeps of a block matrix (nr block rows, places of bn*bn doubles): one sweep over the term lists (bptr, bindex) of L or U, the
 * values brought into the layout by the block gather */
static LIS_INT block_sweep_make(LIS_MATRIX A, int which, sweep_t *s)
{
	const int nr = A->nr, bn = A->bnr, bs = bn * bn;
	LIS_MATRIX_CORE P = (which == SW_L || which == SW_LT) ? A->L : A->U;
	int *blk = lisi_block_of(nr, 1), *tp = NULL, *tc = NULL, *tid = NULL, *src = NULL, *d_src = NULL;
	double *d_from = NULL;
	LIS_INT err = LIS_SUCCESS;
	if (!blk) { err = LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "malloc size = %D\n", (LIS_INT)nr); goto out; }
	if ((long long)P->bnnz * bs >= 0x7fffffffLL) { err = LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "the block sweep layout does not fit\n"); goto out; }
	if ((err = lisi_sweep_terms(nr, P->bptr, P->bindex, blk, SW_TERMS(which), &tp, &tc, &tid))) goto out;
	if ((err = lisi_sweep_build_places(s, nr, tp, tc, NULL, SW_DESC(which), NULL, &src, bs))) goto out;
	const int nnz = tp[nr];
	if (nnz > 0) {
		for (int k = 0; k < nnz; k++) src[k] = tid[src[k]];
		if ((err = lisd_upload_i(&d_src, src, (size_t)nnz)) || (err = lisd_upload_d(&d_from, P->value, (size_t)P->bnnz * (size_t)bs))) goto out;
		int rc = liship_block_gather_f64(nnz, bs, d_src, d_from, s->val, lisg.stream);
		if (!rc) rc = liship_stream_synchronize(lisg.stream);          /* (the sources go below) */
		if (rc) { err = lisi_hip_error(__FILE__, __func__, __LINE__, rc); goto out; }
	}
	/* per block row: b and x, and the block of WD */
	s->bytes = lisi_sweep_bytes_places(nr, nnz, bs, 16.0 * (double)bn + 8.0 * (double)bs);
out:
	(void)liship_free(d_src); (void)liship_free(d_from);
	free(blk); free(tp); free(tc); free(tid); free(src);
	if (err) lisi_sweep_free(s);
	return err;
}

/* A: an assembled, split CSR matrix -- or BSR matrix with square blocks of 1 .. 8 -- with WD, one rank */
static LIS_INT check_split(LIS_MATRIX A)
{
	LISCHK(lisi_matrix_check(A, LISI_CHECK_ASSEMBLED));
	if (IS_BLOCK(A)) {
		if (A->bnr != A->bnc || A->bnr < 1 || A->bnr > LISI_SSOR_MAX_BN)
			return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "triangular solves on %D x %D blocks are not served: square blocks of 1 .. %d only\n", A->bnr, A->bnc, LISI_SSOR_MAX_BN);
	} else if (A->matrix_type != LIS_MATRIX_CSR) return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "triangular solves are served for CSR and BSR storage only\n");
	if (!A->is_splited || !A->L || !A->U || !A->D || !A->WD || !A->WD->value) return LISI_ERR(LIS_ERR_ILL_ARG, "matrix A is not split or has no WD (lis_precon_create with -p ssor prepares it)\n");
	if (IS_BLOCK(A) && (A->WD->bn != A->bnr || A->WD->nr != A->nr)) return LISI_ERR(LIS_ERR_ILL_ARG, "the WD of matrix A does not hold its blocks (lis_precon_create with -p ssor prepares it)\n");
	if (lisg.nprocs > 1) return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "triangular solves are served on one rank only\n");
	return LIS_SUCCESS;
}

/* the sweep `which` of the schedule for T blocks, built on first use; the HBM copy of A must be ready (its lifetime is the cache's) */
static LIS_INT get_sweep(LIS_MATRIX A, int T, int which, const liship_sweep_t **out)
{
	lisd_mat *d = MDEV(A);
	if (IS_BLOCK(A)) T = 1;                      /* the block sweeps are serial in the reference at any thread count */
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
		LISCHK(IS_BLOCK(A) ? block_sweep_make(A, which, s) : sweep_make(A, which, T, s));
		ss->build_s += lis_wtime() - t0;
	}
	*out = &s->k;
	return LIS_SUCCESS;
}

static LIS_INT upload_wd(LIS_MATRIX A, const double **out)
{
	lisd_ssor *ss = (lisd_ssor *)MDEV(A)->ssor;
	const size_t count = WD_COUNT(A);
	if (ss->wd && ss->wd_n != count) { (void)liship_free(ss->wd); (void)liship_free(ss->work); ss->wd = NULL; ss->work = NULL; }
	if (!ss->wd) { HIPCHK(lisd_malloc((void **)&ss->wd, (count + 2) * sizeof(double))); ss->wd_n = count; }
	if (!ss->work && BLOCK_BN(A) > 1) HIPCHK(lisd_malloc((void **)&ss->work, ((size_t)A->nr * (size_t)A->bnr + 2) * sizeof(double)));
	if (count) HIPCHK(liship_memcpy_h2d(ss->wd, A->WD->value, sizeof(double) * count, lisg.stream));
	*out = ss->wd;
	return LIS_SUCCESS;
}

/* ------------------------------------------------------------------ create */
/* A->WD of a split BSR matrix: the blocks of D times omega (lis_matrix_diag_scale: alpha * d), then lis_matrix_diag_inverse -- 1.0 on the
 * diagonal of the last block's padding, lis_array_ge per block (liship_bdiag_inverse_f64) -- in HBM, the result copied home */
static LIS_INT block_wd_build(LIS_MATRIX A, double w)
{
	const int bn = A->bnr, nr = A->nr;
	const size_t count = (size_t)nr * (size_t)(bn * bn);
	if (count >= 0x7fffffffULL) return LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "the blocks of WD do not fit\n");
	if (A->WD && (A->WD->bn != bn || A->WD->nr != nr)) lisi_ssor_wd_free(A);
	if (!A->WD) {
		LIS_MATRIX_DIAG WD = (LIS_MATRIX_DIAG)calloc(1, sizeof(struct LIS_MATRIX_DIAG_STRUCT));
		if (WD) WD->value = (LIS_SCALAR *)calloc(count ? count : 1, sizeof(LIS_SCALAR));
		if (!WD || !WD->value) { if (WD) free(WD); return LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "malloc size = %D\n", (LIS_INT)count); }
		WD->status = LIS_MATRIX_NULL; WD->is_destroy = LIS_TRUE; WD->bn = bn; WD->nr = nr;
		WD->n = A->n; WD->gn = A->gn; WD->np = A->np;
		WD->comm = A->comm; WD->my_rank = A->my_rank; WD->nprocs = A->nprocs; WD->is = A->is; WD->ie = A->ie; WD->origin = A->origin;
		A->WD = WD;
	}
	if (!count) return LIS_SUCCESS;
	double *d_d = NULL, *d_wd = NULL;
	LIS_INT err = lisd_upload_d(&d_d, A->D->value, count);
	int rc = 0;
	if (!err) rc = lisd_malloc((void **)&d_wd, (count + 2) * sizeof(double));
	if (!err && !rc) rc = liship_scale_to_f64((int)count, w, d_d, d_wd, lisg.stream);
	if (!err && !rc) rc = liship_bdiag_inverse_f64(A->n, nr, bn, d_wd, NULL, lisg.stream);      /* (bn <= 8: no work array) */
	if (!err && !rc) rc = liship_stream_synchronize(lisg.stream);
	if (!err && rc) err = lisi_hip_error(__FILE__, __func__, __LINE__, rc);
	if (!err) err = lisd_staged_d2h(A->WD->value, d_wd, sizeof(double) * count);
	(void)liship_free(d_d); (void)liship_free(d_wd);
	return err;
}

LIS_INT lisi_ssor_create(LIS_SOLVER solver, LIS_PRECON precon)
{
	LIS_MATRIX A = solver->A;
	const LIS_INT storage = solver->options[LIS_OPTIONS_STORAGE];
	const double w = solver->params[LIS_PARAMS_SSOR_OMEGA - LIS_OPTIONS_LEN];
	LISCHK(lisi_matrix_check(A, LISI_CHECK_ASSEMBLED));
	LIS_INT bnr, bnc;
	const LIS_INT result = lisi_storage_result(A, storage, solver->options[LIS_OPTIONS_STORAGE_BLOCK], &bnr, &bnc);   /* what A is after lis_matrix_convert_self */
	/* refusals first: A is left as it was */
	if (result == LIS_MATRIX_COO)
		return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-p ssor is served for CSR and BSR storage only; on COO storage the reference itself fails (lis_matrix_solve: not implemented, a NaN residual) (A is untouched)\n");
	if (result != LIS_MATRIX_CSR && result != LIS_MATRIX_BSR)
		return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-p ssor is served for CSR and BSR storage only (A is untouched)\n");
	if (lisg.nprocs > 1) return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-p ssor is served on one rank only (A is untouched)\n");
	if (solver->options[LIS_OPTIONS_SCALE] != LIS_SCALE_NONE) return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-p ssor together with -scale is not served (A is untouched)\n");
	if (solver->options[LIS_OPTIONS_ADDS]) return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-p ssor with -adds true is not served (A is untouched)\n");
	if (result == LIS_MATRIX_BSR) {
		if (bnr != bnc) return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-p ssor on %D x %D blocks is not served: a BSR matrix is split for square blocks only (A is untouched)\n", bnr, bnc);
		if (bnr < 1 || bnr > LISI_SSOR_MAX_BN)
			return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-p ssor on %D x %D blocks is not served: the block sweeps hold blocks of 1 .. %d, larger blocks are a follow-up (A is untouched)\n", bnr, bnc, LISI_SSOR_MAX_BN);
		if (MDEV(A)->device_only)
			return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-p ssor on a BSR matrix that lives in HBM only is not served: its split needs the host arrays (A is untouched)\n");
		LISCHK(lisd_init());                     /* WD is made in HBM: without a device the no-device code, before A changes */
	}
	LISCHK(lisi_convert_self(A, result, solver->options[LIS_OPTIONS_STORAGE_BLOCK]));
	LISCHK(lis_matrix_split(A));
	if (IS_BLOCK(A)) {                           /* WD = omega D, the padding's 1.0, every block inverted -- built only while use_wd says no WD for SOR stands */
		if (A->use_wd != LIS_SOLVER_SOR || !A->WD || A->WD->bn != A->bnr || A->WD->nr != A->nr) {
			LISCHK(block_wd_build(A, w));
			A->use_wd = LIS_SOLVER_SOR;
		}
		precon->A = A;
		return LIS_SUCCESS;
	}
	if (A->use_wd != LIS_SOLVER_SOR || (A->WD && A->WD->bn > 1)) {           /* WD = D, scaled by omega, inverted (lis_matrix_diag_scale / _inverse) */
		if (A->WD && A->WD->bn > 1) lisi_ssor_wd_free(A);      /* (blocks of an earlier life in BSR storage) */
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

/* ------------------------------------------------------------------ the solve's side (the SSOR row of lisi_precon_kinds) */
LIS_INT lisd_ssor_begin(LIS_MATRIX A, LIS_SOLVER solver, lisi_precon_state *st)
{
	const liship_sweep_t *f, *b;
	const double *wd;
	(void)solver;
	st->A = A; st->n = A->n; st->T = IS_BLOCK(A) ? 1 : lisi_sweep_blocks();
	LISCHK(get_sweep(A, st->T, SW_L, &f));
	LISCHK(get_sweep(A, st->T, SW_U, &b));
	LISCHK(upload_wd(A, &wd));
	lisg.last_ssor = 1; lisg.last_ssor_blocks = st->T; lisg.last_ssor_bn = BLOCK_BN(A);
	lisg.last_ssor_levels_fwd = f->nlev; lisg.last_ssor_levels_bwd = b->nlev;
	lisg.last_ssor_launches = f->ngroups + b->ngroups;
	return LIS_SUCCESS;
}

/* what the sweeps of one matrix run on: its size and blocks, WD and the work vector in HBM */
typedef struct { int n, bn; const double *wd; double *work; } sweep_ctx;
static sweep_ctx sweep_ctx_of(LIS_MATRIX A)
{
	const lisd_ssor *ss = (const lisd_ssor *)MDEV(A)->ssor;
	const sweep_ctx c = {(int)A->n, BLOCK_BN(A), ss->wd, ss->work};
	return c;
}

/* one sweep: the point kernels (sptrsv.hip), or the block kernels (bsptrsv.hip) from bn = 2 on */
static int one_sweep(const sweep_ctx *c, const liship_sweep_t *s, int mode, int herm, const double *b, double *x)
{
	if (c->bn == 1) return liship_sweep_f64(s, mode, b, x, c->wd, lisg.stream);
	return liship_bsweep_f64(s, c->n, c->bn, mode, herm, b, x, c->wd, c->work, lisg.stream);
}

/* the kernels of a solve with the sweep s1, then s2 (NULL: LOWER or UPPER alone); herm: X = B first (lis_matrix_solveh_csr :1774, _bsr :1787), then the scatter sweeps in place */
static LIS_INT run_sweeps(const sweep_ctx *c, const liship_sweep_t *s1, const liship_sweep_t *s2, int herm, const double *b, double *x)
{
	if (!herm) {
		HIPCHK(one_sweep(c, s1, LISHIP_SWEEP_MUL, 0, b, x));
		if (s2) HIPCHK(one_sweep(c, s2, LISHIP_SWEEP_SUB, 0, NULL, x));
		return LIS_SUCCESS;
	}
	if (x != b) HIPCHK(liship_memcpy_d2d(x, b, sizeof(double) * (size_t)c->n, lisg.stream));
	if (s2) {
		HIPCHK(one_sweep(c, s1, LISHIP_SWEEP_SCAT, 1, x, x));
		HIPCHK(one_sweep(c, s2, LISHIP_SWEEP_MUL, 1, x, x));
	} else HIPCHK(one_sweep(c, s1, LISHIP_SWEEP_MUL, 1, x, x));
	return LIS_SUCCESS;
}

LIS_INT lisd_ssor_apply(const lisi_precon_state *st, int transposed, const double *b, double *x)
{	/* x = M^-1 b, or M^-H b (b may be x): get_sweep finds the built sweep, or builds it again on a copy that a product rebuilt in mid-solve */
	const liship_sweep_t *s1, *s2;
	LISCHK(get_sweep(st->A, st->T, transposed ? SW_UT : SW_L, &s1));
	LISCHK(get_sweep(st->A, st->T, transposed ? SW_LT : SW_U, &s2));
	const sweep_ctx c = sweep_ctx_of(st->A);
	return run_sweeps(&c, s1, s2, transposed, b, x);
}

/* ------------------------------------------------------------------ lis_matrix_solve / lis_matrix_solveh (ref lis_matrix_ops.c; CSR, and BSR with square blocks of 1 .. 8)
 * LOWER / UPPER are sequential in the reference at any thread count (T = 1 here); SSOR takes the blocks of the solves. */
static LIS_INT solve_common(LIS_MATRIX A, LIS_VECTOR B, LIS_VECTOR X, LIS_INT flag, int herm)
{
	LISCHK(check_split(A));
	if (flag != LIS_MATRIX_LOWER && flag != LIS_MATRIX_UPPER && flag != LIS_MATRIX_SSOR) return LISI_ERR(LIS_ERR_ILL_ARG, "flag %D is not LOWER, UPPER or SSOR\n", flag);
	if (B->n != A->n || X->n != A->n) return LISI_ERR(LIS_ERR_ILL_ARG, "sizes of A, B and X do not match\n");
	LISCHK(lisd_mat_ready(A));
	const int T = (flag == LIS_MATRIX_SSOR && !IS_BLOCK(A)) ? lisi_sweep_blocks() : 1;
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
	const sweep_ctx c = sweep_ctx_of(A);
	LISCHK(run_sweeps(&c, s1, s2, herm, db, dx));
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

LIS_INT lis_amd_last_solve_ssor_block(void) { return lisg.last_ssor ? lisg.last_ssor_bn : 0; }

LIS_INT lis_amd_ssor_schedule_info(LIS_MATRIX A, double info[4])
{	/* {seconds spent building schedules for A, bytes per psolve, launches per psolve, levels of the forward sweep} at the solves' T */
	LISCHK(check_split(A));
	LISCHK(lisd_mat_ready(A));
	const liship_sweep_t *f, *b;
	const int T = IS_BLOCK(A) ? 1 : lisi_sweep_blocks();
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
	LISCHK(get_sweep(A, lisi_sweep_blocks(), (int)sweep, &s));
	lisi_sweep_census(s, info);
	info[5] = s->nnz;
	return LIS_SUCCESS;
}

typedef struct { lisi_precon_state st; const double *b; double *x; } psolve_args;
static LIS_INT psolve_once(void *ctx) { const psolve_args *p = (const psolve_args *)ctx; return lisd_ssor_apply(&p->st, 0, p->b, p->x); }

LIS_INT lis_amd_ssor_psolve_times(LIS_MATRIX A, LIS_VECTOR B, LIS_VECTOR X, LIS_INT reps, double *ms)
{	/* reps psolves X = M^-1 B on the library's stream, each timed by device events (ms[k]) */
	LISCHK(check_split(A));
	LISCHK(lisd_mat_ready(A));
	const double *wd;
	psolve_args args;
	LISCHK(lisd_ssor_begin(A, NULL, &args.st));
	LISCHK(upload_wd(A, &wd));
	double *db, *dx;
	LISCHK(lisd_vec_in(B, &db));
	LISCHK(lisd_vec_out(X, &dx));
	args.b = db; args.x = dx;
	LISCHK(lisi_sweep_times(reps, psolve_once, &args, ms));
	return lisd_vec_done(X);
}
