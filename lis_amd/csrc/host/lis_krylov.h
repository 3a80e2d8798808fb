/*
 * lis_krylov.h -- what every Krylov loop of liblis_amd shares: the device-side solve context (work vectors in
 * HBM, preconditioner diagonal, tolerances), the residual bookkeeping of lis_solver.c:957-1091 / :1792-1812,
 * the error-unwinding macros and the vocabulary the loops are written in.  Included by lis_solver.c (CG, BiCG, BiCGSTAB with
 * fused passes, host-driven and device-driven, and GMRES) and lis_solver_more.c (every loop that is one kernel per reference call:
 * CG, BiCG and BiCGSTAB in that form -- what a preconditioner that is no point diagonal runs -- and the other solvers).
 */
#ifndef LIS_AMD_KRYLOV_H
#define LIS_AMD_KRYLOV_H
#include "lis_internal.h"

/* ------------------------------------------------------------------ the device-side solve context */
typedef struct {
	LIS_SOLVER s;
	LIS_MATRIX A;
	int n;
	size_t len;              /* doubles per work vector: np + pad + slack (ghost slots for the halo) */
	double *b, *x;           /* HBM */
	double *dinv;            /* Jacobi 1/diag in HBM, NULL for none */
	int duniform; double dconst;   /* every dinv[i] is the double dconst (a constant diagonal): the fused CG passes take the scalar */
	const lisi_precon_kind *pk;    /* the preconditioner's row (lis_internal.h) ... */
	lisi_precon_state ps;    /* ... and what its begin resolved for this solve (ps.dinv is dinv) */
	double **work; int nwork;
	double bnrm, tol;
	int output, maxiter;
} ctx_t;

static inline LIS_INT work_alloc(ctx_t *c, int count)
{
	c->work = (double **)calloc((size_t)count, sizeof(double *));
	c->nwork = count;
	for (int i = 0; i < count; i++) {
		LISCHK(lisd_pool_get(c->len * sizeof(double), (void **)&c->work[i]));
		HIPCHK(liship_memset(c->work[i], 0, c->len * sizeof(double), lisg.stream));
	}
	return LIS_SUCCESS;
}
static inline void work_free(ctx_t *c)
{
	for (int i = 0; i < c->nwork; i++) lisd_pool_put(c->work[i], c->len * sizeof(double));
	free(c->work); c->work = NULL; c->nwork = 0;
}

static inline LIS_INT d_copy(ctx_t *c, const double *src, double *dst) { HIPCHK(liship_memcpy_d2d(dst, src, sizeof(double) * (size_t)c->n, lisg.stream)); return LIS_SUCCESS; }
/* z = M^-1 r and z = M^-H r (lis_psolve / lis_psolveh): the row's apply; which r may alias z is on the row */
static inline LIS_INT d_psolve(ctx_t *c, const double *r, double *z) { return c->pk->apply(&c->ps, 0, r, z); }
static inline LIS_INT d_psolveh(ctx_t *c, const double *r, double *z) { return c->pk->apply(&c->ps, 1, r, z); }
static inline int precon_by_calls(const ctx_t *c) { return c->pk->by_calls; }
static inline LIS_INT d_matvec(ctx_t *c, double *x, double *y) { return lisd_spmv(c->A, x, y); }
static inline LIS_INT d_resid(ctx_t *c, const double *r, double *nrm)
{	/* lis_solver_get_residual_nrm2_r (lis_solver.c:1792) / _nrm1_b (:1804) */
	if (c->s->options[LIS_OPTIONS_CONV_COND] == LIS_CONV_COND_NRM1_B) return lisd_nrm1(c->n, r, nrm);
	LISCHK(lisd_nrm2(c->n, r, nrm));
	*nrm = *nrm * c->bnrm;
	return LIS_SUCCESS;
}
static inline void note(ctx_t *c, LIS_INT iter, double nrm)
{
	if (!c->output) return;
	if ((c->output & LIS_PRINT_MEM) && iter <= c->maxiter + 1) c->s->rhistory[iter] = nrm;   /* maxiter + 2 slots (IDR(1) can step past) */
	if (c->output & LIS_PRINT_OUT) lis_printf(LIS_COMM_WORLD, "iteration: %5d  relative residual = %e\n", (int)iter, nrm);
}

/* the norms of the initial residual r (its high part in a quad solve), the scaling 1/||.||, the tolerance, the early exit: lis_solver.c:1037-1081.
 * quad: the iteration-0 entry of the history and of the printed log, which the reference writes for a quad r only (:1069-1073).
 * returns 1 when the caller must stop (converged), 0 to iterate, <0 on error (-err) */
static inline int initial_norms(ctx_t *c, const double *r, int quad)
{
	LIS_SOLVER s = c->s;
	const int conv = s->options[LIS_OPTIONS_CONV_COND];
	const double tol = s->params[LIS_PARAMS_RESID - LIS_OPTIONS_LEN], tol_w = s->params[LIS_PARAMS_RESID_WEIGHT - LIS_OPTIONS_LEN];
	LIS_INT err = 0;
	double nrm = 0.0, bn = 0.0;
	switch (conv) {
	case LIS_CONV_COND_NRM2_R: err = lisd_nrm2(c->n, r, &nrm); bn = nrm; s->tol = tol; break;
	case LIS_CONV_COND_NRM2_B: err = lisd_nrm2(c->n, r, &nrm); if (!err) err = lisd_nrm2(c->n, c->b, &bn); s->tol = tol; break;
	default:                   err = lisd_nrm1(c->n, r, &nrm); if (!err) err = lisd_nrm1(c->n, c->b, &bn); s->tol = bn * tol_w + tol; break;
	}
	if (err) return -(int)err;
	s->tol_switch = s->params[LIS_PARAMS_SWITCH_RESID - LIS_OPTIONS_LEN];
	bn = (bn == 0.0) ? 1.0 : 1.0 / bn;
	s->bnrm = bn; c->bnrm = bn; c->tol = s->tol;
	nrm = nrm * bn;
	if (quad && c->output) {
		if (c->output & LIS_PRINT_MEM) s->rhistory[0] = nrm;
		if (c->output & LIS_PRINT_OUT) lis_printf(LIS_COMM_WORLD, "iteration: %5d  relative residual = %e\n", 0, nrm);
	}
	if (nrm <= fabs(tol)) { s->retcode = LIS_SUCCESS; s->iter = 1; s->resid = nrm; return 1; }
	return 0;
}

/* r = b - A x (or b when x0 = 0), then the norms above: lis_solver.c:957-1091 */
static inline int initial_residual(ctx_t *c, double *r)
{
	LIS_INT err = 0;
	if (!c->s->options[LIS_OPTIONS_INITGUESS_ZEROS]) {
		err = d_matvec(c, c->x, r);
		if (!err && liship_xpay_f64(c->n, c->b, -1.0, r, lisg.stream)) err = LIS_ERR_NOT_IMPLEMENTED;
	} else err = d_copy(c, c->b, r);
	if (err) return -(int)err;
	return initial_norms(c, r, 0);
}

/* GMRES and FGMRES, host scalars (lis_solver_gmres.c:254-290).  The new Hessenberg column hc (entries 0 .. ii + 1) takes the earlier rotations, which lie
 * behind h at CS (cosines) and SN (sines), then its own is made, kept and applied to hc and to g; returns |g[ii + 1]| */
static inline double givens_column(double *h, double *hc, double *g, int ii, int CS, int SN)
{
	const int i1 = ii + 1;
	for (int k = 1; k <= ii; k++) {
		const int jj = k - 1;
		const double tt = hc[jj];
		double aa = h[jj + CS] * tt;  aa += h[jj + SN] * hc[k];
		double bb = -h[jj + SN] * tt; bb += h[jj + CS] * hc[k];
		hc[jj] = aa; hc[k] = bb;
	}
	double aa = hc[ii], bb = hc[i1];
	double rr = sqrt(aa * aa + bb * bb);
	if (rr == 0.0) rr = 1.0e-17;
	h[ii + CS] = aa / rr;
	h[ii + SN] = bb / rr;
	g[i1] = -h[ii + SN] * g[ii];
	g[ii] =  h[ii + CS] * g[ii];
	aa  = h[ii + CS] * hc[ii];
	aa += h[ii + SN] * hc[i1];
	hc[ii] = aa;
	return fabs(g[i1]);
}
/* ... and the back substitution: g[0 .. ii] becomes the coefficients of the update */
static inline void hessenberg_solve(const double *h, double *g, int ii, int ld)
{
	g[ii] = g[ii] / h[ii + (size_t)ii * ld];
	for (int k = 1; k <= ii; k++) {
		const int jj = ii - k;
		double tt = g[jj];
		for (int j = jj + 1; j <= ii; j++) tt -= h[jj + (size_t)j * ld] * g[j];
		g[jj] = tt / h[jj + (size_t)jj * ld];
	}
}

#define TRY(expr) do { LIS_INT e__ = (expr); if (e__) { err = e__; goto done; } } while (0)
#define KTRY(call) do { int rc__ = (call); if (rc__) { err = lisi_hip_error(__FILE__, __func__, __LINE__, rc__); goto done; } } while (0)

/* the loops' vocabulary; each names c, n, s, iter, nrm2, err and the label done of the loop it stands in */
#define AXPY(a, x, y)      KTRY(liship_axpy_f64(n, (a), (x), (y), lisg.stream))          /* y += a x     */
#define XPAY(x, a, y)      KTRY(liship_xpay_f64(n, (x), (a), (y), lisg.stream))          /* y = x + a y  */
#define AXPYZ(a, x, y, z)  KTRY(liship_axpyz_f64(n, (a), (x), (y), (z), lisg.stream))    /* z = a x + y  */
#define SCALE(a, x)        KTRY(liship_scale_f64(n, (a), (x), lisg.stream))
#define COPY(src, dst)     TRY(d_copy(c, (src), (dst)))
#define DOT(x, y, out)     TRY(lisd_dot(n, (x), (y), (out)))
#define MATVEC(x, y)       TRY(d_matvec(c, (x), (y)))
#define PSOLVE(r, z)       TRY(d_psolve(c, (r), (z)))
#define PSOLVEH(r, z)      TRY(d_psolveh(c, (r), (z)))
#define RESID(r, out)      TRY(d_resid(c, (r), (out)))
#define START(r) do { int st__ = initial_residual(c, (r)); if (st__) { err = st__ < 0 ? -st__ : 0; goto done; } } while (0)
#define FINISH(code) do { s->retcode = (code); s->iter = iter; s->resid = nrm2; err = ((code) == LIS_SUCCESS) ? 0 : (code); goto done; } while (0)

/* lis_solver_more.c */
LIS_INT lisk_cg(ctx_t *c);
LIS_INT lisk_bicg(ctx_t *c);
LIS_INT lisk_bicgstab(ctx_t *c);
LIS_INT lisk_cgs(ctx_t *c);
LIS_INT lisk_cr(ctx_t *c);
LIS_INT lisk_gpbicg(ctx_t *c);
LIS_INT lisk_tfqmr(ctx_t *c);
LIS_INT lisk_bicgsafe(ctx_t *c);
LIS_INT lisk_orthomin(ctx_t *c);
LIS_INT lisk_gpbicr(ctx_t *c);
LIS_INT lisk_bicr(ctx_t *c);
LIS_INT lisk_crs(ctx_t *c);
LIS_INT lisk_bicrstab(ctx_t *c);
LIS_INT lisk_bicrsafe(ctx_t *c);
LIS_INT lisk_fgmres(ctx_t *c);
LIS_INT lisk_minres(ctx_t *c);
LIS_INT lisk_idrs(ctx_t *c);
LIS_INT lisk_bicgstabl(ctx_t *c);
LIS_INT lisk_jacobi(ctx_t *c);
/* lis_solver_quad.c: the double-double loops of -f quad */
LIS_INT lisq_dispatch(ctx_t *c);

#endif
