/*
 * lis_solver_quad.c -- -f quad: CG, BiCG, CGS and BiCGSTAB in double-double arithmetic, iterating in HBM.
 *
 * The loops restate the reference's, statement for statement:
 *   lis_cg_quad        src/solver/lis_solver_cg.c:240-355
 *   lis_bicg_quad      src/solver/lis_solver_bicg.c:282-429
 *   lis_cgs_quad       src/solver/lis_solver_cgs.c:281-438
 *   lis_bicgstab_quad  src/solver/lis_solver_bicgstab.c:320-513
 * and the quad branch of lis_solver_get_initial_residual (src/solver/lis_solver.c:994-1035).  A vector is a pair of HBM buffers (hi, lo) from
 * the pool; one launch per reference call (kernels/quad.hip), nothing fused, nothing device-driven, never in a renumbered plan's numbering.
 * The scalars come home after each dot and the steps between the dots (lis_quad_div, _mul, _minus) run here, on kernels/dd.hpp -- the one source
 * of the arithmetic, compiled as C.  The residual norm is the plain nrm2 / nrm1 of the high parts (lis_solver_get_residual_*), i.e. the
 * double path's reduction; breakdown tests look at both parts; convergence is `tol > nrm2` as in the reference's quad loops.
 * x leaves as its high part (lis_vector_copyex_mn): the iterate's hi array is the solve context's x.
 */
#include <stdio.h>
#include "lis_krylov.h"
#include "../kernels/dd.hpp"

LIS_INT lis_amd_set_quad_precision(LIS_INT on) { lisg.quad_precision = (on != 0); return LIS_SUCCESS; }
LIS_INT lis_amd_get_quad_precision(void) { return lisg.quad_precision; }
LIS_INT lis_amd_last_solve_quad(void) { return lisg.last_quad; }

LIS_INT lis_amd_quad_scalar(LIS_INT op, const double *a, const double *b, double *out)
{
	if (!a || !out || (op != 3 && !b)) return LISI_ERR(LIS_ERR_ILL_ARG, "lis_amd_quad_scalar: NULL argument\n");
	dd_t r;
	switch (op) {
	case 0: r = dd_add(dd_make(a[0], a[1]), dd_make(b[0], b[1])); break;
	case 1: r = dd_mul(dd_make(a[0], a[1]), dd_make(b[0], b[1])); break;
	case 2: r = dd_div(dd_make(a[0], a[1]), dd_make(b[0], b[1])); break;
	case 3: r = dd_minus(dd_make(a[0], a[1])); break;
	default: return LISI_ERR(LIS_ERR_ILL_ARG, "lis_amd_quad_scalar: op %D is none of 0 .. 3\n", op);
	}
	out[0] = r.hi; out[1] = r.lo;
	return LIS_SUCCESS;
}

/* what -f quad | switch serves, decided from the options and A's state alone: nothing is touched.  Called with the switch on */
LIS_INT lisq_gate(LIS_MATRIX A, LIS_SOLVER solver)
{
	const LIS_INT *o = solver->options;
	const LIS_INT nsolver = o[LIS_OPTIONS_SOLVER], precon = o[LIS_OPTIONS_PRECON], storage = o[LIS_OPTIONS_STORAGE];
	if (o[LIS_OPTIONS_PRECISION] == LIS_PRECISION_DOUBLE) return LIS_SUCCESS;
	if (o[LIS_OPTIONS_PRECISION] != LIS_PRECISION_QUAD)
		return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-f switch (double iterations, then quad) is not served by liblis_amd: -f double and -f quad are\n");
	if (nsolver < 1 || nsolver > LIS_SOLVER_LEN) return LIS_SUCCESS;          /* check_options answers */
	if (nsolver != LIS_SOLVER_CG && nsolver != LIS_SOLVER_BICG && nsolver != LIS_SOLVER_CGS && nsolver != LIS_SOLVER_BICGSTAB) {
		char name[64] = "";
		(void)lis_solver_get_solvername(nsolver, name);
		return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-f quad: solver %s is not served in quad precision by liblis_amd (cg, bicg, cgs, bicgstab are)\n", name);
	}
	if (precon != LIS_PRECON_TYPE_NONE && precon != LIS_PRECON_TYPE_JACOBI) {
		char name[64] = "";
		if (lis_solver_get_preconname(precon, name) != LIS_SUCCESS) snprintf(name, sizeof(name), "%d", (int)precon);
		return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-f quad: preconditioner %s is not served in quad precision by liblis_amd (none and jacobi are)\n", name);
	}
	if (storage && storage != A->matrix_type)
		return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-f quad: -storage %D would convert A; a quad solve runs on the CSR matrix it is given\n", storage);
	if (A->matrix_type != LIS_MATRIX_CSR)
		return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-f quad: matrix storage type %D is not served in quad precision by liblis_amd (CSR is)\n", A->matrix_type);
	if (A->is_splited)
		return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-f quad: a split (D/L/U) matrix A is not served in quad precision by liblis_amd\n");
	if (o[LIS_OPTIONS_SCALE] != LIS_SCALE_NONE)
		return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-f quad: -scale is not served in quad precision by liblis_amd\n");
	if (lisg.nprocs > 1 || A->nprocs > 1)
		return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-f quad is served on one rank (this job has %D ranks)\n", (LIS_INT)lisg.nprocs);
	return LIS_SUCCESS;
}

/* ------------------------------------------------------------------ the loops' vocabulary */
typedef struct { double *hi, *lo; } qvec;

typedef struct {
	ctx_t *c;
	int n;
	const int *ptr, *index, *tptr, *tindex;
	const double *value, *tvalue;
	int trows;
	qvec x;
	size_t xlo_bytes;
} qctx;

static inline qvec qwork(ctx_t *c, int k) { qvec v = { c->work[2 * k], c->work[2 * k + 1] }; return v; }

#define QAXPY(a, x, y)      KTRY(liship_axpy_dd_f64(n, (a).hi, (a).lo, (x).hi, (x).lo, (y).hi, (y).lo, lisg.stream))                       /* y += a x    */
#define QXPAY(x, a, y)      KTRY(liship_xpay_dd_f64(n, (x).hi, (x).lo, (a).hi, (a).lo, (y).hi, (y).lo, lisg.stream))                       /* y = x + a y */
#define QAXPYZ(a, x, y, z)  KTRY(liship_axpyz_dd_f64(n, (a).hi, (a).lo, (x).hi, (x).lo, (y).hi, (y).lo, (z).hi, (z).lo, lisg.stream))     /* z = a x + y */
#define QCOPY(src, dst)     do { TRY(d_copy(c, (src).hi, (dst).hi)); TRY(d_copy(c, (src).lo, (dst).lo)); } while (0)
#define QDOT(x, y, out)     TRY(q_dot(q, (x), (y), &(out)))
#define QMATVEC(x, y)       KTRY(liship_spmv_csr_dd_f64(n, q->ptr, q->index, q->value, (x).hi, (x).lo, (y).hi, (y).lo, lisg.stream))
#define QMATVECH(x, y)      KTRY(liship_spmv_csr_t_dd_f64(q->trows, q->tptr, q->tindex, q->tvalue, (x).hi, (x).lo, (y).hi, (y).lo, lisg.stream))
#define QPSOLVE(r, z)       TRY(q_psolve(q, (r), (z)))
#define QZERO(a)            ((a).hi == 0.0 && (a).lo == 0.0)

/* <x, y> as lis_vector_dotex_mmm(x, y): the pair comes home */
static LIS_INT q_dot(qctx *q, qvec x, qvec y, dd_t *out)
{
	double v[2];
	HIPCHK(liship_dot_dd_f64(q->n, x.hi, x.lo, y.hi, y.lo, lisg.reduce_out, lisg.reduce_work, lisg.stream));
	LISCHK(lisd_fetch_from(lisg.reduce_out, 2, v));
	out->hi = v[0]; out->lo = v[1];
	return LIS_SUCCESS;
}

/* z = M^-1 r and M^-H r: a copy of both parts (lis_psolve_none), or r * d with d = 1 / diag in double (lis_psolve_jacobi, lis_psolveh_jacobi) */
static LIS_INT q_psolve(qctx *q, qvec r, qvec z)
{
	ctx_t *c = q->c;
	if (c->dinv) { HIPCHK(liship_muld_dd_f64(q->n, r.hi, r.lo, c->dinv, z.hi, z.lo, lisg.stream)); return LIS_SUCCESS; }
	LISCHK(d_copy(c, r.hi, z.hi));
	return d_copy(c, r.lo, z.lo);
}

/* r = b widened, or for a given x0: the quad product on (x0, 0), the DOUBLE xpay on the high part, the low part zeroed (lis_solver.c:994-1035); then the norms */
static int q_initial_residual(qctx *q, qvec r)
{
	ctx_t *c = q->c;
	const int n = q->n;
	int rc;
	if (!c->s->options[LIS_OPTIONS_INITGUESS_ZEROS]) {
		rc = liship_spmv_csr_dd_f64(n, q->ptr, q->index, q->value, q->x.hi, q->x.lo, r.hi, r.lo, lisg.stream);
		if (!rc) rc = liship_xpay_f64(n, c->b, -1.0, r.hi, lisg.stream);
		if (!rc) rc = liship_memset(r.lo, 0, sizeof(double) * (size_t)n, lisg.stream);
	} else rc = liship_widen_dd_f64(n, c->b, r.hi, r.lo, lisg.stream);
	if (rc) return -(int)lisi_hip_error(__FILE__, __func__, __LINE__, rc);
	return initial_norms(c, r.hi, 1);
}
#define QSTART(r) do { int st__ = q_initial_residual(q, (r)); if (st__) { err = st__ < 0 ? -st__ : 0; goto done; } } while (0)

static LIS_INT q_cg(qctx *q)
{
	ctx_t *c = q->c; LIS_SOLVER s = c->s;
	LIS_INT err = 0, iter;
	const int n = q->n;
	TRY(work_alloc(c, 2 * 4));
	qvec z = qwork(c, 0), qq = qwork(c, 1), r = qwork(c, 2), p = qwork(c, 3), x = q->x;
	dd_t alpha, beta, rho, rho_old = dd_make(1.0, 0.0), dot_pq;
	double nrm2 = 0.0;
	QSTART(r);
	for (iter = 1; iter <= c->maxiter; iter++) {
		QPSOLVE(r, z);
		QDOT(r, z, rho);
		beta = dd_div(rho, rho_old);
		QXPAY(z, beta, p);
		QMATVEC(p, qq);
		QDOT(p, qq, dot_pq);
		if (QZERO(dot_pq)) FINISH(LIS_BREAKDOWN);
		alpha = dd_div(rho, dot_pq);
		QAXPY(alpha, p, x);
		alpha = dd_minus(alpha);
		QAXPY(alpha, qq, r);
		RESID(r.hi, &nrm2);
		note(c, iter, nrm2);
		if (c->tol > nrm2) FINISH(LIS_SUCCESS);
		rho_old = rho;
	}
	FINISH(LIS_MAXITER);
done:
	work_free(c);
	return err;
}

static LIS_INT q_bicg(qctx *q)
{
	ctx_t *c = q->c; LIS_SOLVER s = c->s;
	LIS_INT err = 0, iter;
	const int n = q->n;
	TRY(work_alloc(c, 2 * 6));
	qvec r = qwork(c, 0), rtld = qwork(c, 1), z = qwork(c, 2), ztld = qwork(c, 3), p = qwork(c, 4), ptld = qwork(c, 5), x = q->x;
	qvec qq = z, qtld = ztld;                          /* q, qtld share z's and ztld's storage (:311-312) */
	dd_t alpha, beta, rho, rho_old = dd_make(1.0, 0.0), tmpdot1;
	double nrm2 = 0.0;
	QSTART(r);
	QCOPY(r, rtld);                                    /* lis_solver_set_shadowresidual: rtld = r0 */
	for (iter = 1; iter <= c->maxiter; iter++) {
		QPSOLVE(r, z);
		QPSOLVE(rtld, ztld);
		QDOT(z, rtld, rho);
		if (QZERO(rho)) FINISH(LIS_BREAKDOWN);
		beta = dd_div(rho, rho_old);
		QXPAY(z, beta, p);
		QMATVEC(p, qq);
		QXPAY(ztld, beta, ptld);
		QMATVECH(ptld, qtld);
		QDOT(ptld, qq, tmpdot1);
		if (QZERO(tmpdot1)) FINISH(LIS_BREAKDOWN);
		alpha = dd_div(rho, tmpdot1);
		QAXPY(alpha, p, x);
		alpha = dd_minus(alpha);
		QAXPY(alpha, qq, r);
		RESID(r.hi, &nrm2);
		note(c, iter, nrm2);
		if (c->tol > nrm2) FINISH(LIS_SUCCESS);
		QAXPY(alpha, qtld, rtld);
		rho_old = rho;
	}
	FINISH(LIS_MAXITER);
done:
	work_free(c);
	return err;
}

static LIS_INT q_cgs(qctx *q)
{
	ctx_t *c = q->c; LIS_SOLVER s = c->s;
	LIS_INT err = 0, iter;
	const int n = q->n;
	TRY(work_alloc(c, 2 * 7));
	qvec r = qwork(c, 0), rtld = qwork(c, 1), p = qwork(c, 2), phat = qwork(c, 3), qq = qwork(c, 4), qhat = qwork(c, 5), x = q->x;
	qvec u = qwork(c, 5), uhat = qwork(c, 6), vhat = qwork(c, 6);     /* u shares qhat's storage, uhat vhat's (:308-311) */
	dd_t alpha, beta, rho, rho_old = dd_make(1.0, 0.0), tmpdot1;
	const dd_t one = dd_make(1.0, 0.0);
	double nrm2 = 0.0;
	QSTART(r);
	QCOPY(r, rtld);
	for (iter = 1; iter <= c->maxiter; iter++) {
		QDOT(rtld, r, rho);
		if (QZERO(rho)) FINISH(LIS_BREAKDOWN);
		beta = dd_div(rho, rho_old);
		QAXPYZ(beta, qq, r, u);                        /* u = r + beta q */
		QXPAY(qq, beta, p);                            /* p = u + beta (q + beta p) */
		QXPAY(u, beta, p);
		QPSOLVE(p, phat);
		QMATVEC(phat, vhat);
		QDOT(rtld, vhat, tmpdot1);
		if (QZERO(tmpdot1)) FINISH(LIS_BREAKDOWN);
		alpha = dd_div(rho, tmpdot1);
		alpha = dd_minus(alpha);
		QAXPYZ(alpha, vhat, u, qq);                    /* q = u - alpha vhat */
		QAXPYZ(one, u, qq, phat);                      /* phat = u + q */
		QPSOLVE(phat, uhat);
		alpha = dd_minus(alpha);
		QAXPY(alpha, uhat, x);
		QMATVEC(uhat, qhat);
		alpha = dd_minus(alpha);
		QAXPY(alpha, qhat, r);
		RESID(r.hi, &nrm2);
		note(c, iter, nrm2);
		if (c->tol > nrm2) FINISH(LIS_SUCCESS);
		rho_old = rho;
	}
	FINISH(LIS_MAXITER);
done:
	work_free(c);
	return err;
}

static LIS_INT q_bicgstab(qctx *q)
{
	ctx_t *c = q->c; LIS_SOLVER s = c->s;
	LIS_INT err = 0, iter;
	const int n = q->n;
	TRY(work_alloc(c, 2 * 7));
	qvec rtld = qwork(c, 0), r = qwork(c, 1), t = qwork(c, 2), p = qwork(c, 3), v = qwork(c, 4), phat = qwork(c, 5), shat = qwork(c, 6), x = q->x;
	qvec sv = r;                                       /* s shares r's storage (:343-344) */
	dd_t alpha = dd_make(1.0, 0.0), omega = dd_make(1.0, 0.0), beta, rho, rho_old = dd_make(1.0, 0.0), tmpdot1, tmpdot2;
	double nrm2 = 0.0;
	QSTART(r);
	QCOPY(r, rtld);
	for (iter = 1; iter <= c->maxiter; iter++) {
		QDOT(rtld, r, rho);
		if (QZERO(rho)) FINISH(LIS_BREAKDOWN);
		if (iter == 1) QCOPY(r, p);
		else {
			beta = dd_div(rho, rho_old);
			tmpdot1 = dd_div(alpha, omega);
			beta = dd_mul(beta, tmpdot1);
			omega = dd_minus(omega);                   /* p = r + beta (p - omega v) */
			QAXPY(omega, v, p);
			QXPAY(r, beta, p);
		}
		QPSOLVE(p, phat);
		QMATVEC(phat, v);
		QDOT(rtld, v, tmpdot1);
		alpha = dd_div(rho, tmpdot1);
		alpha = dd_minus(alpha);
		QAXPY(alpha, v, r);                            /* s = r - alpha v */
		RESID(sv.hi, &nrm2);
		if (c->tol > nrm2) {
			note(c, iter, nrm2);
			alpha = dd_minus(alpha);
			QAXPY(alpha, phat, x);
			FINISH(LIS_SUCCESS);
		}
		QPSOLVE(sv, shat);
		QMATVEC(shat, t);
		QDOT(t, sv, tmpdot1);
		QDOT(t, t, tmpdot2);
		omega = dd_div(tmpdot1, tmpdot2);
		alpha = dd_minus(alpha);
		QAXPY(alpha, phat, x);
		QAXPY(omega, shat, x);
		omega = dd_minus(omega);
		QAXPY(omega, t, r);                            /* r = s - omega t */
		omega = dd_minus(omega);
		RESID(r.hi, &nrm2);
		note(c, iter, nrm2);
		if (c->tol > nrm2) FINISH(LIS_SUCCESS);
		if (QZERO(omega)) FINISH(LIS_BREAKDOWN);
		rho_old = rho;
	}
	FINISH(LIS_MAXITER);
done:
	work_free(c);
	return err;
}

/* the quad solve behind lis_solve_kernel's dispatch: the context holds b, the iterate's high part c->x (0 or x0) and the Jacobi diagonal */
LIS_INT lisq_dispatch(ctx_t *c)
{
	const LIS_INT nsolver = c->s->options[LIS_OPTIONS_SOLVER];
	lisd_mat *d = MDEV(c->A);
	qctx q;
	LIS_INT err;
	memset(&q, 0, sizeof(q));
	if (d->type != LIS_MATRIX_CSR || !d->ptr || !d->index || !d->value || d->solve_holds)
		return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-f quad: the HBM copy of A does not hold plain CSR arrays\n");
	q.c = c; q.n = c->n;
	q.ptr = d->ptr; q.index = d->index; q.value = d->value;
	if (nsolver == LIS_SOLVER_BICG) {
		LISCHK(lisd_mat_ready_t(c->A));
		q.tptr = d->t_ptr; q.tindex = d->t_index; q.tvalue = d->t_value; q.trows = d->t_rows;
	}
	q.xlo_bytes = c->len * sizeof(double);
	q.x.hi = c->x;
	LISCHK(lisd_pool_get(q.xlo_bytes, (void **)&q.x.lo));
	const int rc = liship_memset(q.x.lo, 0, q.xlo_bytes, lisg.stream);                                        /* lis_vector_copyex_nm(x, xx): lo = 0 */
	err = rc ? lisi_hip_error(__FILE__, __func__, __LINE__, rc) : LIS_SUCCESS;
	if (!err) switch (nsolver) {
	case LIS_SOLVER_CG:       err = q_cg(&q); break;
	case LIS_SOLVER_BICG:     err = q_bicg(&q); break;
	case LIS_SOLVER_CGS:      err = q_cgs(&q); break;
	default:                  err = q_bicgstab(&q); break;
	}
	(void)liship_stream_synchronize(lisg.stream);
	lisd_pool_put(q.x.lo, q.xlo_bytes);
	return err;
}
