/*
 * lis_esolver_single.c -- the eigensolvers of one pair (reference src/esolver/lis_esolver_pi.c, _ii.c, _rqi.c, _cg.c), on the frame of lis_eloop.h.
 *
 * The standard problem: power (-e pi), inverse (-e ii), Rayleigh quotient (-e rqi), CG (-e cg) and CR (-e cr, the default) iteration.  The Gram blocks of CG
 * (12 inner products over 6 vectors) and CR (5 over 3, 4 over 4) are taken in one pass each by lisd_multidot (gram, lis_eloop.h).
 *
 * The generalized problem A x = lambda B x: -e gpi | gii | grqi | gcr (lis_esolver_pi.c:305-464, _ii.c:357-520, _rqi.c:350-501, _cg.c:1063-1265) -- the
 * reference's four loops that work (lis_egcg never updates x or p from its Ritz vector and ends in NaN: refused in lis_gesolve), statement for statement.
 * Sums that share a vector go through one lisd_multidot pass -- rho and <B v, B v> of -e grqi, the three dot groups of -e gcr --, the bits of the separate dots.
 */
#include "lis_eloop.h"

/* ------------------------------------------------------------------ power and inverse iteration, standard and generalized: lis_esolver_pi.c:127-226 (pi),
 * lis_esolver_ii.c:127-277 (ii), lis_esolver_pi.c:305-464 (gpi: the preconditioner is B's, the solves are with B), lis_esolver_ii.c:357-520 (gii).  One frame:
 * the generalized forms put w = M v, scaled with v by <v,w>^1/2, in front (M = A for gpi, B for gii) and iterate on w where the standard forms iterate on v;
 * the inverse forms and gpi solve with the other matrix of the pencil where pi multiplies by A.  pi creates no inner solver at all */
LIS_INT lisi_epi_ii(LIS_ESOLVER esolver)
{
	ectx_t cx, *c = &cx;
	ectx_begin(c, esolver, 1);
	const LIS_INT nesolver = esolver->options[LIS_EOPTIONS_ESOLVER];
	const int power = nesolver == LIS_ESOLVER_PI || nesolver == LIS_ESOLVER_GPI;
	LIS_MATRIX A = c->A, B = c->B, S = power ? B : A;        /* S: the matrix of the inner solves (none for pi) */
	LIS_VECTOR v = esolver->x, *wk = esolver->work, w = B ? wk[0] : v, y = B ? wk[1] : wk[0], q = B ? wk[2] : wk[1];
	LIS_SCALAR eta, theta = 0.0;
	LIS_REAL nrm2, resid = 0.0;
	LIS_INT err = 0, iter = 0, iter2, code = LIS_MAXITER;
	ETRY(ebegin(c, v));
	if (S) {
		ETRY(inner_solver(c, "-i bicg -p none"));
		c->solver->A = S;
		ETRY(lis_precon_create(c->solver, &c->precon));
	}
	while (iter < c->emaxiter) {
		iter = iter + 1;
		ETRY(lis_vector_nrm2(v, &nrm2));                     /* v = v / ||v||_2 */
		ETRY(lis_vector_scale(1.0 / nrm2, v));
		if (B) {
			ETRY(lis_matvec(power ? A : B, v, w));           /* w = A * v (gpi), w = B * v (gii) */
			ETRY(power ? lis_vector_dot(v, w, &eta) : lis_vector_dot(w, v, &eta));   /* v = v / <v,w>^1/2, w = w / <v,w>^1/2 (gpi); <w,v> (gii) */
			eta = sqrt(eta);
			ETRY(lis_vector_scale(1.0 / eta, v));
			ETRY(lis_vector_scale(1.0 / eta, w));
		}
		if (S) {
			ETRY(inner_solve_on(c, S, w, y, 0));             /* y = A^-1 * v (ii), y = B^-1 * w (gpi), y = A^-1 * w (gii) */
			lis_solver_get_iter(c->solver, &iter2);
		} else ETRY(lis_matvec(A, v, y));                    /* y = A * v (pi) */
		ETRY(lis_vector_dot(w, y, &theta));                  /* theta = <v,y>; <w,y> in the generalized forms */
		ETRY(lis_vector_axpyz(-theta, v, y, q));             /* resid = ||y - theta * v||_2 / |theta| */
		ETRY(lis_vector_nrm2(q, &resid));
		resid = resid / fabs(theta);
		ETRY(lis_vector_copy(y, v));                         /* v = y */
		if (S) inner_times(c);
		enote(c, iter, resid);
		if (c->tol >= resid) { code = LIS_SUCCESS; break; }
	}
	esolver->retcode = code;
	esolver->iter[0] = iter;
	esolver->resid[0] = resid;
	esolver->evalue[0] = (power ? theta : 1.0 / theta) + c->oshift;
	ETRY(normalize(v));
	err = code;
done:
	err = eend(c, err);
	inner_destroy(c);
	return err;
}

/* ------------------------------------------------------------------ Rayleigh quotient iteration, lis_esolver_rqi.c:129-268 (no -shift: rho is the shift) */
LIS_INT lisi_erqi(LIS_ESOLVER esolver)
{
	ectx_t cx, *c = &cx;
	ectx_begin(c, esolver, 0);
	LIS_MATRIX A = c->A;
	LIS_VECTOR v = esolver->x, y = esolver->work[0], q = esolver->work[1];
	LIS_SCALAR theta, dotvy, rho = 0.0;
	LIS_REAL nrm2, resid = 0.0;
	LIS_INT err = 0, iter = 0, iter2, code = LIS_MAXITER;
	int shifted = 0;
	if (esolver->options[LIS_EOPTIONS_INITGUESS_ONES]) ETRY(lis_vector_set_all(1.0, v));
	ETRY(inner_solver(c, "-i bicg -p none"));
	c->solver->A = A;
	ETRY(lis_precon_create(c->solver, &c->precon));
	ETRY(lis_vector_nrm2(v, &nrm2));                         /* v = v / ||v||_2 */
	ETRY(lis_vector_scale(1.0 / nrm2, v));
	ETRY(lis_matvec(A, v, y));                               /* rho = <v,A*v> / <v,v> */
	ETRY(lis_vector_dot(v, y, &rho));
	while (iter < c->emaxiter) {
		iter = iter + 1;
		ETRY(eshift(c, rho));                                /* y = (A - rho * I)^-1 * v */
		shifted = 1;
		ETRY(inner_solve_on(c, A, v, y, 0));
		ETRY(eshift(c, -rho));
		shifted = 0;
		lis_solver_get_iter(c->solver, &iter2);
		ETRY(lis_vector_nrm2(y, &theta));                    /* theta = ||y||_2 */
		ETRY(lis_vector_dot(v, y, &dotvy));                  /* <v,y> */
		rho = rho + dotvy / (theta * theta);                 /* rho = rho + <v,y> / theta^2 */
		ETRY(lis_vector_axpyz(-dotvy, v, y, q));             /* resid = ||y - <v,y> * v||_2 / <v,y> */
		ETRY(lis_vector_nrm2(q, &resid));
		resid = resid / fabs(dotvy);
		ETRY(lis_vector_scale(1.0 / theta, y));              /* v = y / theta */
		ETRY(lis_vector_copy(y, v));
		enote(c, iter, resid);
		inner_times(c);
		if (c->tol >= resid) { code = LIS_SUCCESS; break; }
	}
	esolver->retcode = code;
	esolver->iter[0] = iter;
	esolver->resid[0] = resid;
	esolver->evalue[0] = rho;
	ETRY(normalize(v));
	err = code;
done:
	if (shifted) (void)eshift(c, -rho);                      /* an inner solve failed between the two shifts: A goes back */
	inner_destroy(c);
	return err;
}

/* ------------------------------------------------------------------ generalized Rayleigh quotient iteration, lis_esolver_rqi.c:350-501 (no -shift: rho is the shift;
 * the preconditioner is made once, of the unshifted A) */
LIS_INT lisi_egrqi(LIS_ESOLVER esolver)
{
	ectx_t cx, *c = &cx;
	ectx_begin(c, esolver, 0);
	LIS_MATRIX A = c->A, B = c->B;
	LIS_VECTOR v = esolver->x, w = esolver->work[0], y = esolver->work[1];
	LIS_SCALAR theta, eta, dotww, rho = 0.0;
	LIS_REAL nrm2, resid = 0.0;
	LIS_INT err = 0, iter = 0, iter2, code = LIS_MAXITER;
	int shifted = 0;
	if (esolver->options[LIS_EOPTIONS_INITGUESS_ONES]) ETRY(lis_vector_set_all(1.0, v));
	ETRY(inner_solver(c, "-i bicg -p none"));
	c->solver->A = A;
	ETRY(lis_precon_create(c->solver, &c->precon));
	ETRY(lis_vector_nrm2(v, &nrm2));                         /* v = v / ||v||_2 */
	ETRY(lis_vector_scale(1.0 / nrm2, v));
	ETRY(lis_matvec(B, v, w));                               /* w = B * v */
	ETRY(lis_matvec(A, v, y));                               /* rho = <B*v,A*v> / <B*v,B*v>: two sums over {w, y}, one pass */
	{
		LIS_VECTOR vs[2] = {w, y};
		static const int pairs[2][2] = {{0, 1}, {0, 0}};
		double g[2];
		ETRY(gram(v->n, 2, vs, 2, pairs, g));
		rho = g[0]; dotww = g[1];
	}
	rho = rho / dotww;
	while (iter < c->emaxiter) {
		iter = iter + 1;
		ETRY(eshift(c, rho));                                /* y = (A - rho * B)^-1 * w */
		shifted = 1;
		ETRY(inner_solve_on(c, A, w, y, 0));
		ETRY(eshift(c, -rho));
		shifted = 0;
		lis_solver_get_iter(c->solver, &iter2);
		ETRY(lis_vector_dot(w, y, &theta));                  /* theta = <w,y> */
		ETRY(lis_matvec(B, y, w));                           /* w = B * y */
		ETRY(lis_vector_dot(w, y, &eta));                    /* eta = <w,y>^1/2 */
		eta = sqrt(eta);
		ETRY(lis_vector_scale(1.0 / eta, y));                /* v = y / eta */
		ETRY(lis_vector_copy(y, v));
		ETRY(lis_vector_scale(1.0 / eta, w));                /* w = w / eta */
		rho = rho + theta / (eta * eta);                     /* rho = rho + theta / eta^2 */
		resid = 1.0 / fabs(theta);                           /* resid = 1 / |theta| */
		enote(c, iter, resid);
		inner_times(c);
		if (c->tol >= resid) { code = LIS_SUCCESS; break; }
	}
	esolver->retcode = code;
	esolver->iter[0] = iter;
	esolver->resid[0] = resid;
	esolver->evalue[0] = rho;
	ETRY(normalize(v));
	err = code;
done:
	if (shifted) (void)eshift(c, -rho);                      /* an inner solve failed between the two shifts: A goes back */
	inner_destroy(c);
	return err;
}

/* ------------------------------------------------------------------ the 3 x 3 Rayleigh-Ritz step of CG, lis_esolver_cg.c:290-305: inverse iteration on
 * A3 z = B3 v with the lis_array_* routines of src/array/lis_array.c restated operation for operation (column-major 3 x 3, n = 3 branches):
 * nrm2 :366, scale :172, matvec :449-453, solve :987-1019 (LU without pivoting into W3, the reciprocal pivots on its diagonal), dot :310, axpyz :155 */
static void ritz3(const LIS_SCALAR *A3, const LIS_SCALAR *B3, LIS_SCALAR *v3, LIS_INT emaxiter, LIS_REAL tol)
{
	LIS_SCALAR W3[9], B3v3[3], z3[3], q3[3], mu3, t;
	LIS_REAL nrm2, resid3;
	LIS_INT iter3 = 0;
	v3[0] = 1.0; v3[1] = 1.0; v3[2] = 1.0;
	while (iter3 < emaxiter) {
		iter3 = iter3 + 1;
		t = 0.0;
		for (int i = 0; i < 3; i++) t += v3[i] * v3[i];
		nrm2 = sqrt(t);
		for (int i = 0; i < 3; i++) v3[i] = (1.0 / nrm2) * v3[i];
		B3v3[0] = B3[0] * v3[0] + B3[3] * v3[1] + B3[6] * v3[2];
		B3v3[1] = B3[1] * v3[0] + B3[4] * v3[1] + B3[7] * v3[2];
		B3v3[2] = B3[2] * v3[0] + B3[5] * v3[1] + B3[8] * v3[2];
		for (int i = 0; i < 9; i++) W3[i] = A3[i];
		for (int k = 0; k < 3; k++) {
			W3[k + k * 3] = 1.0 / W3[k + k * 3];
			for (int i = k + 1; i < 3; i++) {
				t = W3[i + k * 3] * W3[k + k * 3];
				for (int j = k + 1; j < 3; j++) W3[i + j * 3] -= t * W3[k + j * 3];
				W3[i + k * 3] = t;
			}
		}
		for (int i = 0; i < 3; i++) {
			z3[i] = B3v3[i];
			for (int j = 0; j < i; j++) z3[i] -= W3[i + j * 3] * z3[j];
		}
		for (int i = 2; i >= 0; i--) {
			for (int j = i + 1; j < 3; j++) z3[i] -= W3[i + j * 3] * z3[j];
			z3[i] *= W3[i + i * 3];
		}
		mu3 = 0;
		for (int i = 0; i < 3; i++) mu3 = mu3 + B3v3[i] * z3[i];
		for (int i = 0; i < 3; i++) q3[i] = -mu3 * B3v3[i] + z3[i];
		t = 0.0;
		for (int i = 0; i < 3; i++) t += q3[i] * q3[i];
		resid3 = sqrt(t);
		if (resid3 < tol) break;
		for (int i = 0; i < 3; i++) v3[i] = z3[i];
	}
}

/* how cg, cr and gcr end.  err: what cut the loop short, 0 after a loop that ran to its end -- whose count, residual and eigenvalue are then stored, x
 * normalised (cr, gcr; cg hands NULL: its x is normalised inside the loop) and the times taken over.  Then, always: the preconditioner leaves the solver, both
 * are destroyed, the pencil is shifted back; the answer is LIS_SUCCESS or LIS_MAXITER from resid < tol */
static LIS_INT cg_family_end(ectx_t *c, LIS_INT err, LIS_INT iter, LIS_REAL resid, LIS_SCALAR lambda, double ptime, LIS_VECTOR x)
{
	LIS_ESOLVER esolver = c->e;
	if (!err) {
		esolver->iter[0] = iter;
		esolver->resid[0] = resid;
		esolver->evalue[0] = lambda + c->oshift;
		if (x) err = normalize(x);
	}
	if (!err) {
		esolver->ptime = ptime;
		esolver->itime = c->solver->itime; esolver->p_c_time = c->solver->p_c_time; esolver->p_i_time = c->solver->p_i_time;
	}
	if (c->solver) c->solver->precon = NULL;
	inner_destroy(c);
	err = eend(c, err);
	if (err) return err;
	esolver->retcode = (resid < c->tol) ? LIS_SUCCESS : LIS_MAXITER;
	return esolver->retcode;
}

/* ------------------------------------------------------------------ CG, lis_esolver_cg.c:126-367 */
LIS_INT lisi_ecg(LIS_ESOLVER esolver)
{
	ectx_t cx, *c = &cx;
	ectx_begin(c, esolver, 1);
	LIS_MATRIX A = c->A;
	LIS_VECTOR x = esolver->x;
	LIS_VECTOR r = esolver->work[0], w = esolver->work[1], p = esolver->work[2], Ax = esolver->work[3], Aw = esolver->work[4], Ap = esolver->work[5];
	LIS_SCALAR lambda = 0.0, A3[9], B3[9], v3[3];
	LIS_REAL nrm2, resid = 0.0;
	LIS_INT err = 0, iter = 0;
	double ptime = 0.0, time;
	ETRY(ebegin(c, x));
	ETRY(lis_vector_nrm2(x, &nrm2));
	ETRY(lis_vector_scale(1.0 / nrm2, x));
	ETRY(lis_matvec(A, x, Ax));
	ETRY(inner_solver(c, "-i cg -p none"));
	ETRY(inner_solve_on(c, A, x, p, 1));                     /* p = A^-1 * x */
	ETRY(lis_vector_copy(x, Ap));
	ETRY(lis_precon_create(c->solver, &c->precon));
	ETRY(psolve_begin(c));
	while (iter < c->emaxiter) {
		iter = iter + 1;
		ETRY(lis_vector_dot(x, Ax, &lambda));                /* mu = <x,x> / <x,A*x>, where mu = 1 / lambda */
		ETRY(lis_vector_axpyz(-1.0 / lambda, Ax, x, r));     /* r = x - mu * A * x */
		ETRY(lis_vector_nrm2(r, &nrm2));
		resid = nrm2;
		enote(c, iter, resid);
		if (resid < c->tol) break;
		time = lis_wtime();
		ETRY(psolve(c, r, w));                               /* w = M^-1 * r */
		ptime += lis_wtime() - time;
		ETRY(lis_vector_nrm2(w, &nrm2));
		ETRY(lis_vector_scale(1.0 / nrm2, w));
		ETRY(lis_matvec(A, w, Aw));
		{	/* Rayleigh-Ritz on span {w, x, p}: A3 = (w x p)^T A (w x p), B3 = (w x p)^T (w x p), symmetric halves copied (:269-288).  One pass */
			LIS_VECTOR vs[6] = {w, x, p, Aw, Ax, Ap};
			static const int pairs[12][2] = {{0, 3}, {1, 3}, {2, 3}, {1, 4}, {2, 4}, {2, 5}, {0, 0}, {1, 0}, {2, 0}, {1, 1}, {2, 1}, {2, 2}};
			double g[12];
			ETRY(gram(x->n, 6, vs, 12, pairs, g));
			A3[0] = g[0]; A3[3] = g[1]; A3[6] = g[2]; A3[1] = A3[3]; A3[4] = g[3]; A3[7] = g[4]; A3[2] = A3[6]; A3[5] = A3[7]; A3[8] = g[5];
			B3[0] = g[6]; B3[3] = g[7]; B3[6] = g[8]; B3[1] = B3[3]; B3[4] = g[9]; B3[7] = g[10]; B3[2] = B3[6]; B3[5] = B3[7]; B3[8] = g[11];
		}
		ritz3(A3, B3, v3, c->emaxiter, c->tol);
		ETRY(lis_vector_scale(v3[0], w));                    /* update x and p */
		ETRY(lis_vector_axpy(v3[2], p, w));
		ETRY(lis_vector_xpay(w, v3[1], x));
		ETRY(lis_vector_copy(w, p));
		ETRY(lis_vector_scale(v3[0], Aw));                   /* update A*x and A*p */
		ETRY(lis_vector_axpy(v3[2], Ap, Aw));
		ETRY(lis_vector_xpay(Aw, v3[1], Ax));
		ETRY(lis_vector_copy(Aw, Ap));
		ETRY(lis_vector_nrm2(x, &nrm2));                     /* the Ritz vector of the smallest Ritz value, normalised */
		ETRY(lis_vector_scale(1.0 / nrm2, x));
		ETRY(lis_vector_scale(1.0 / nrm2, Ax));
		ETRY(lis_vector_nrm2(p, &nrm2));
		ETRY(lis_vector_scale(1.0 / nrm2, p));
		ETRY(lis_vector_scale(1.0 / nrm2, Ap));
	}
done:
	return cg_family_end(c, err, iter, resid, lambda, ptime, NULL);
}

/* ------------------------------------------------------------------ CR, lis_esolver_cg.c:780-979 */
LIS_INT lisi_ecr(LIS_ESOLVER esolver)
{
	ectx_t cx, *c = &cx;
	ectx_begin(c, esolver, 1);
	LIS_MATRIX A = c->A;
	LIS_VECTOR x = esolver->x;
	LIS_VECTOR r = esolver->work[0], p = esolver->work[1], w = esolver->work[2], Ax = esolver->work[3], Ap = esolver->work[4], Aw = esolver->work[5];
	LIS_SCALAR lambda = 0.0, alpha, beta;
	LIS_SCALAR rAp, rp, ApAp, pAp, pp, AwAp, pAw, wAp, wp;
	LIS_REAL nrm2, resid = 0.0;
	LIS_INT err = 0, iter = 0;
	double ptime = 0.0, time;
	ETRY(ebegin(c, x));
	ETRY(lis_vector_nrm2(x, &nrm2));
	ETRY(lis_vector_scale(1.0 / nrm2, x));
	ETRY(lis_matvec(A, x, Ax));
	ETRY(lis_vector_set_all(0.0, p));
	ETRY(lis_vector_set_all(0.0, Ap));
	ETRY(inner_solver(c, "-i bicg -p none"));
	c->solver->A = A;                                        /* lis_solve_setup(A, solver): the solver made ready for preconditioning */
	ETRY(lis_precon_create(c->solver, &c->precon));
	ETRY(psolve_begin(c));
	ETRY(lis_vector_dot(x, Ax, &lambda));                    /* lambda = <A*x,x> / <x,x> */
	ETRY(lis_vector_axpyz(-lambda, x, Ax, r));               /* r = lambda * x - A * x */
	ETRY(lis_vector_scale(-1.0, r));
	ETRY(lis_vector_copy(r, p));
	ETRY(lis_matvec(A, p, Ap));
	while (iter < c->emaxiter) {
		iter = iter + 1;
		{	/* alpha = (<r,A*p> - lambda * <r,p>) / (<A*p,A*p> - 2 * lambda * <A*p,p> + lambda^2 * <p,p>): five sums, one pass */
			LIS_VECTOR vs[3] = {r, p, Ap};
			static const int pairs[5][2] = {{0, 2}, {0, 1}, {2, 2}, {1, 2}, {1, 1}};
			double g[5];
			ETRY(gram(x->n, 3, vs, 5, pairs, g));
			rAp = g[0]; rp = g[1]; ApAp = g[2]; pAp = g[3]; pp = g[4];
		}
		alpha = (rAp - lambda * rp) / (ApAp - 2.0 * lambda * pAp + lambda * lambda * pp);
		ETRY(lis_vector_axpy(alpha, p, x));                  /* x = x + alpha * p */
		ETRY(lis_matvec(A, x, Ax));                          /* lambda = <A*x,x> / <x,x> */
		ETRY(lis_vector_dot(x, Ax, &lambda));
		ETRY(lis_vector_nrm2(x, &nrm2));
		lambda = lambda / (nrm2 * nrm2);
		ETRY(lis_vector_axpyz(-lambda, x, Ax, r));           /* r = lambda * x - A * x */
		ETRY(lis_vector_scale(-1.0, r));
		time = lis_wtime();
		ETRY(psolve(c, r, w));                               /* w = M^-1 * r */
		ptime += lis_wtime() - time;
		ETRY(lis_matvec(A, w, Aw));
		{	/* beta = -[<A*w,A*p> - lambda * (<A*w,p> + <A*p,w>) + lambda^2 * <w,p>] / [the denominator of alpha]: four sums, one pass */
			LIS_VECTOR vs[4] = {Aw, Ap, p, w};
			static const int pairs[4][2] = {{0, 1}, {2, 0}, {3, 1}, {3, 2}};
			double g[4];
			ETRY(gram(x->n, 4, vs, 4, pairs, g));
			AwAp = g[0]; pAw = g[1]; wAp = g[2]; wp = g[3];
		}
		beta = -(AwAp - lambda * (pAw + wAp) + lambda * lambda * wp) / (ApAp - 2.0 * lambda * pAp + lambda * lambda * pp);
		ETRY(lis_vector_xpay(w, beta, p));                   /* p = w + beta * p */
		ETRY(lis_vector_xpay(Aw, beta, Ap));                 /* A*p = A*w + beta * A*p */
		ETRY(lis_vector_nrm2(r, &nrm2));                     /* convergence check */
		resid = nrm2 / fabs(lambda);
		enote(c, iter, resid);
		if (resid < c->tol) break;
	}
done:
	return cg_family_end(c, err, iter, resid, lambda, ptime, x);
}

/* ------------------------------------------------------------------ generalized CR, lis_esolver_cg.c:1063-1265 */
LIS_INT lisi_egcr(LIS_ESOLVER esolver)
{
	ectx_t cx, *c = &cx;
	ectx_begin(c, esolver, 1);
	LIS_MATRIX A = c->A, B = c->B;
	LIS_VECTOR x = esolver->x;
	LIS_VECTOR r = esolver->work[0], p = esolver->work[1], w = esolver->work[2], Ax = esolver->work[3], Ap = esolver->work[4], Aw = esolver->work[5];
	LIS_VECTOR Bx = esolver->work[6], Bp = esolver->work[7], Bw = esolver->work[8];
	LIS_SCALAR lambda = 0.0, alpha, beta;
	LIS_SCALAR rAp, rBp, BxBx, ApAp, ApBp, BpBp, AwAp, AwBp, ApBw, BwBp;
	LIS_REAL nrm2, resid = 0.0;
	LIS_INT err = 0, iter = 0;
	double ptime = 0.0, time;
	static const int xpairs[2][2] = {{0, 1}, {1, 1}};        /* <A*x,B*x>, <B*x,B*x> over {Ax, Bx} */
	ETRY(ebegin(c, x));
	ETRY(lis_vector_nrm2(x, &nrm2));
	ETRY(lis_vector_scale(1.0 / nrm2, x));
	ETRY(lis_matvec(A, x, Ax));
	ETRY(lis_matvec(B, x, Bx));
	ETRY(inner_solver(c, "-i bicg -p none"));
	c->solver->A = A;                                        /* lis_solve_setup(A, solver): the solver made ready for preconditioning */
	ETRY(lis_precon_create(c->solver, &c->precon));
	ETRY(psolve_begin(c));
	{	/* lambda = <A*x,B*x> / <B*x,B*x> */
		LIS_VECTOR vs[2] = {Ax, Bx};
		double g[2];
		ETRY(gram(x->n, 2, vs, 2, xpairs, g));
		lambda = g[0]; BxBx = g[1];
	}
	lambda = lambda / BxBx;
	ETRY(lis_vector_axpyz(-lambda, Bx, Ax, r));              /* r = lambda * B * x - A * x */
	ETRY(lis_vector_scale(-1.0, r));
	ETRY(lis_vector_copy(r, p));
	ETRY(lis_matvec(A, p, Ap));
	ETRY(lis_matvec(B, p, Bp));
	while (iter < c->emaxiter) {
		iter = iter + 1;
		{	/* alpha = (<r,A*p> - lambda * <r,B*p>) / (<A*p,A*p> - 2 * lambda * <A*p,B*p> + lambda^2 * <B*p,B*p>): five sums, one pass */
			LIS_VECTOR vs[3] = {r, Ap, Bp};
			static const int pairs[5][2] = {{0, 1}, {0, 2}, {1, 1}, {1, 2}, {2, 2}};
			double g[5];
			ETRY(gram(x->n, 3, vs, 5, pairs, g));
			rAp = g[0]; rBp = g[1]; ApAp = g[2]; ApBp = g[3]; BpBp = g[4];
		}
		alpha = (rAp - lambda * rBp) / (ApAp - 2.0 * lambda * ApBp + lambda * lambda * BpBp);
		ETRY(lis_vector_axpy(alpha, p, x));                  /* x = x + alpha * p */
		ETRY(lis_matvec(A, x, Ax));                          /* lambda = <A*x,B*x> / <B*x,B*x> */
		ETRY(lis_matvec(B, x, Bx));
		{
			LIS_VECTOR vs[2] = {Ax, Bx};
			double g[2];
			ETRY(gram(x->n, 2, vs, 2, xpairs, g));
			lambda = g[0]; BxBx = g[1];
		}
		lambda = lambda / BxBx;
		ETRY(lis_vector_axpyz(-lambda, Bx, Ax, r));          /* r = lambda * B * x - A * x */
		ETRY(lis_vector_scale(-1.0, r));
		time = lis_wtime();
		ETRY(psolve(c, r, w));                               /* w = M^-1 * r */
		ptime += lis_wtime() - time;
		ETRY(lis_matvec(A, w, Aw));
		ETRY(lis_matvec(B, w, Bw));
		{	/* beta = -[<A*w,A*p> - lambda * (<A*w,B*p> + <A*p,B*w>) + lambda^2 * <B*w,B*p>] / [the denominator of alpha]: four sums, one pass */
			LIS_VECTOR vs[4] = {Aw, Ap, Bp, Bw};
			static const int pairs[4][2] = {{0, 1}, {0, 2}, {1, 3}, {3, 2}};
			double g[4];
			ETRY(gram(x->n, 4, vs, 4, pairs, g));
			AwAp = g[0]; AwBp = g[1]; ApBw = g[2]; BwBp = g[3];
		}
		beta = -(AwAp - lambda * (AwBp + ApBw) + lambda * lambda * BwBp) / (ApAp - 2.0 * lambda * ApBp + lambda * lambda * BpBp);
		ETRY(lis_vector_xpay(w, beta, p));                   /* p = w + beta * p */
		ETRY(lis_vector_xpay(Aw, beta, Ap));                 /* A*p = A*w + beta * A*p */
		ETRY(lis_vector_xpay(Bw, beta, Bp));                 /* B*p = B*w + beta * B*p */
		ETRY(lis_vector_nrm2(r, &nrm2));                     /* convergence check */
		resid = nrm2 / fabs(lambda);
		enote(c, iter, resid);
		if (resid < c->tol) break;
	}
done:
	return cg_family_end(c, err, iter, resid, lambda, ptime, x);
}
