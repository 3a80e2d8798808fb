/*
 * lis_esolver_multi.c -- several eigenpairs per solve, on the frame of lis_eloop.h: subspace (-e si, -ie pi | ii), Lanczos (-e li) and Arnoldi (-e ai) iteration
 * with -ss >= 2 (reference src/esolver/lis_esolver_si.c, _li.c, _ai.c), and their generalized forms -e gsi (-ige gpi | gii), -e gli and -e gai (-ige gpi | gii |
 * grqi | gcr) (lis_esolver_si.c:456-719, _li.c:456-694, _ai.c:491-750), statement for statement, with the small dense QR they call (lis_array.c).
 *
 * The orthogonalisation pairs of -e si | gsi and the Hessenberg columns of -e ai | gai are taken as a chain whose coefficients stay in HBM (hdev): liship_dot_f64
 * forms the first, liship_mgs_step_f64 applies one and forms the next, and nothing waits for the host in between.  The tail of a subspace iteration is two passes
 * (liship_multidot_f64, liship_ritz_tail_f64) and one read-back.  The generalized forms add the two pair passes liship_scale2_inv_sqrt_f64 and
 * liship_scale2_to_f64 (kernels/vector_ops.hip); no sum is taken from a product's fused-dot epilogue, whose tree is not liship_dot_f64's.  LIS_AMD_NO_FUSION=1 /
 * LIS_AMD_LOOP_UNFUSED brings the lis_vector_* calls of the reference's text back: the same bits, in the tree mode and in the reference-order mode
 * (tests/test_esolve_multi_gpu.py, tests/test_gesolve_multi_gpu.py).  Lanczos and Arnoldi refine each mode through lis_gesolve with -ie's / -ige's solver.
 */
#include "lis_eloop.h"

/* the "inner eigensolver" line, then the linear solver "-i bicg -p none" with the command line's options and its two banner lines: kept by the generalized loops,
 * which solve with it; -e li | ai create it for these lines only (lis_esolver_li.c:192-206) */
static void inner_name(ectx_t *c, LIS_INT ninner)
{
	char esolvername[128];
	lis_esolver_get_esolvername(ninner, esolvername);
	if (c->output) lis_printf(LIS_COMM_WORLD, "inner eigensolver     : %s\n", esolvername);
}
static LIS_INT inner_banner(ectx_t *c, LIS_INT ninner, int keep)
{
	inner_name(c, ninner);
	const LIS_INT err = inner_solver(c, "-i bicg -p none");
	if (!keep) inner_destroy(c);
	return err;
}

/* the five lines that report a mode: of a subspace iteration, of a refinement */
static void mode_report(const char *label, LIS_INT mode, LIS_SCALAR evalue, double time, LIS_INT iter, LIS_REAL resid)
{
	lis_printf(LIS_COMM_WORLD, "%s: mode number          = %D\n", label, mode);
	lis_printf(LIS_COMM_WORLD, "%s: eigenvalue           = %e\n", label, (double)evalue);
	lis_printf(LIS_COMM_WORLD, "%s: elapsed time         = %e sec.\n", label, time);
	lis_printf(LIS_COMM_WORLD, "%s: number of iterations = %D\n", label, iter);
	lis_printf(LIS_COMM_WORLD, "%s: relative residual    = %e\n\n", label, (double)resid);
}

/* the coefficients of a chain (HBM, where the loop runs fused) and its basis as device pointers */
static LIS_INT chain_alloc(LIS_INT ss, int fused, double **hdev, double ***dv)
{
	if (fused) { const int rc = lisd_malloc((void **)hdev, sizeof(double) * (size_t)(ss + 2)); if (rc) return lisi_hip_error(__FILE__, __func__, __LINE__, rc); }
	if (!(*dv = (double **)malloc(sizeof(double *) * (size_t)(ss + 1)))) return LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "malloc size = %D\n", ss + 1);
	return LIS_SUCCESS;
}

/* ================================================================== subspace iteration, standard and generalized: the frame the two loops share */
/* QR factorization V*R = Z for starting vector Z of the two subspace iterations: v(j) against v(1) .. v(j-1), dot then axpy, pair by pair (lis_esolver_si.c:248-252,
 * :589-593) -- as one chain in HBM, or the lis_vector_* calls */
static LIS_INT orthogonalise(LIS_INT n, LIS_INT j, LIS_VECTOR *v, int fused, double *hdev, double **dv)
{
	LIS_INT err = 0, k;
	LIS_SCALAR dot;
	if (fused && j > 1) {
		double *vj;
		ETRY(lisd_vec_in(v[j], &vj));
		for (k = 1; k < j; k++) ETRY(lisd_vec_in(v[k], &dv[k - 1]));
		EHIP(liship_dot_f64(n, vj, dv[0], hdev, lisg.reduce_work, lisg.stream));
		ETRY(lisd_mgs_chain(n, j - 1, dv, vj, hdev));
		EHIP(liship_scale_to_f64(1, -1.0, hdev + j - 2, hdev + j - 1, lisg.stream));      /* the last coefficient negated in HBM: the axpy below adds */
		EHIP(liship_axpy_dev_f64(n, hdev + j - 1, dv[j - 2], vj, lisg.stream));
		ETRY(lisd_vec_done(v[j]));
	} else {
		for (k = 1; k < j; k++) {
			ETRY(lis_vector_dot(v[j], v[k], &dot));
			ETRY(lis_vector_axpy(-dot, v[k], v[j]));
		}
	}
done:
	return err;
}

/* how both begin: the start vector of ones, normalised; the shift and its banner; after the inner solver's lines (the caller's) the two lines and the chain */
static LIS_INT subspace_begin(ectx_t *c, LIS_VECTOR y)
{
	LIS_REAL nrm2;
	LISCHK(lis_vector_set_all(1.0, y));
	LISCHK(lis_vector_nrm2(y, &nrm2));
	LISCHK(lis_vector_scale(1.0 / nrm2, y));
	return ebegin(c, NULL);
}
static LIS_INT subspace_chain(ectx_t *c, LIS_INT ss, double **hdev, double ***dv)
{
	if (c->output) {
		lis_printf(LIS_COMM_WORLD, "size of subspace      : %D\n\n", ss);
		lis_printf(LIS_COMM_WORLD, "compute eigenpairs in subspace:\n\n");
	}
	return chain_alloc(ss, !lisg.no_fusion, hdev, dv);
}

/* the fused tail of an iteration: nrm2 = ||y||_2 and theta = <partner, y> in one pass, then resid = ||y - theta * v(j)||_2 / |theta|, y = y / ||y||_2 and
 * v(j) = y in the other, and the one read-back of the iteration.  partner is v(j) itself in the standard loop, w in the generalized one */
static LIS_INT subspace_tail(LIS_INT n, LIS_VECTOR y, LIS_VECTOR partner, LIS_VECTOR vj, LIS_REAL *nrm2, LIS_SCALAR *theta, LIS_REAL *resid)
{
	static const int pairs[2][2] = {{0, 0}, {1, 0}};
	double *dy, *dp, *dvj, sums[3];
	LIS_INT err = 0;
	ETRY(lisd_vec_in(y, &dy)); ETRY(lisd_vec_in(partner, &dp));
	if (partner == vj) dvj = dp;
	else ETRY(lisd_vec_in(vj, &dvj));
	const double *dyp[2] = {dy, dp};
	EHIP(liship_multidot_f64(n, 2, dyp, 2, pairs, lisg.reduce_out, lisg.reduce_work, lisg.stream));
	EHIP(liship_ritz_tail_f64(n, lisg.reduce_out, dy, dvj, lisg.reduce_out + 2, lisg.reduce_work, lisg.stream));
	ETRY(lisd_vec_done(y)); ETRY(lisd_vec_done(vj));
	ETRY(lisd_fetch(3, sums));
	*nrm2 = sqrt(sums[0]); *theta = sums[1]; *resid = sqrt(sums[2]);
	*resid = *resid / fabs(*theta);
done:
	return err;
}

static void subspace_note(ectx_t *c, LIS_INT j, LIS_INT iter, LIS_REAL resid)
{	/* convergence check: the history and iter[0] are mode 0's */
	if (j == 1) {
		if (c->output & LIS_EPRINT_MEM) c->e->rhistory[iter] = resid;
		c->e->iter[j - 1] = iter;
	}
	if (c->output & LIS_EPRINT_OUT) lis_printf(LIS_COMM_WORLD, "iteration: %5d  relative residual = %E\n", (int)iter, (double)resid);
}

/* what a mode leaves: its eigenvalue (theta of the power forms, 1 / theta of the inverse forms, shifted back), residual, count and vector, and its report */
static LIS_INT subspace_mode_end(ectx_t *c, const char *label, LIS_INT j, int power, LIS_SCALAR theta, LIS_REAL resid, LIS_INT iter, LIS_VECTOR vj, double etime0)
{
	LIS_ESOLVER esolver = c->e;
	const LIS_INT ss = esolver->options[LIS_EOPTIONS_SUBSPACE];
	esolver->evalue[j - 1] = power ? theta + c->oshift : 1.0 / theta + c->oshift;
	esolver->resid[j - 1] = resid;
	esolver->iter[j - 1] = iter;
	LISCHK(lis_vector_copy(vj, esolver->evector[j - 1]));
	const double etime = lis_wtime() - etime0;
	if (c->output & (ss > 1)) mode_report(label, j - 1, esolver->evalue[j - 1], etime, iter, resid);      /* (as written there: the MEM bit of -eprint) */
	return LIS_SUCCESS;
}

static LIS_INT subspace_end(ectx_t *c, LIS_INT err, double *hdev, double **dv)
{
	if (hdev) (void)liship_free(hdev);
	free(dv);
	err = eend(c, err);
	inner_destroy(c);
	if (!err) err = lis_vector_copy(c->e->evector[0], c->e->x);
	return err;                                              /* LIS_SUCCESS also when a mode stopped at -emaxiter, as there */
}

/* ------------------------------------------------------------------ subspace iteration, lis_esolver_si.c:137-370 (-e si), and generalized subspace iteration,
 * lis_esolver_si.c:456-719 (-e gsi), on one frame: under a B, w = M v(j) scaled with v(j) by <v,w>^1/2 comes in front (M = A for -ige gpi, B for gii) and the
 * iteration runs on w.  As written there for -e gsi: v(j) is orthogonalised against the earlier v(k) with the plain dot, not the B-inner product;
 * eta = <v,w>^1/2 without fabs, so a negative sum gives NaN from there on; work[4] (Ax there) is v(1) and has no use of its own.  With -ige gii the reference
 * creates a preconditioner on A and then, falling through, on B, and leaks both per mode: each is created once per mode here and freed, B's being the one the
 * solves run with.  -e si creates one per mode too (the earlier one is freed, the reference leaks it); -ie pi needs no linear solver at all */
LIS_INT lisi_esi(LIS_ESOLVER esolver)
{
	ectx_t cx, *c = &cx;
	ectx_begin(c, esolver, 1);
	LIS_MATRIX A = c->A, B = c->B;
	const LIS_INT ss = esolver->options[LIS_EOPTIONS_SUBSPACE], n = A->n;
	const LIS_INT ninner = esolver->options[B ? LIS_EOPTIONS_INNER_GENERALIZED_ESOLVER : LIS_EOPTIONS_INNER_ESOLVER];
	const int power = ninner == (B ? LIS_ESOLVER_GPI : LIS_ESOLVER_PI);
	LIS_MATRIX S = power ? B : A;                            /* the matrix of the inner solves: none for -e si -ie pi */
	LIS_VECTOR *wk = esolver->work, y = wk[0], w = B ? wk[1] : NULL, q = B ? wk[2] : wk[1], *v = B ? &wk[3] : &wk[2];      /* (y is r there in -e si) */
	LIS_SCALAR theta = 0.0, eta;
	LIS_REAL nrm2, resid = 0.0;
	LIS_INT err = 0, iter, j;
	double etime0, *hdev = NULL, **dv = NULL;
	ETRY(subspace_begin(c, y));
	if (B) ETRY(inner_banner(c, ninner, 1));
	else {
		inner_name(c, ninner);
		if (S) ETRY(inner_solver(c, "-i bicg -p none"));
	}
	ETRY(subspace_chain(c, ss, &hdev, &dv));
	j = 0;
	while (j < ss) {
		etime0 = lis_wtime();
		ETRY(lis_vector_duplicate(A, &esolver->evector[j]));
		j = j + 1;
		ETRY(lis_vector_copy(y, v[j]));
		if (S) {                                             /* a preconditioner per mode, as there: A's in -e si, B's in -e gsi */
			if (c->precon) { lis_precon_destroy(c->precon); c->precon = NULL; }
			if (B && !power) {
				c->solver->A = A;
				ETRY(lis_precon_create(c->solver, &c->precon));
				lis_precon_destroy(c->precon); c->precon = NULL;
			}
			c->solver->A = B ? B : A;
			ETRY(lis_precon_create(c->solver, &c->precon));
		}
		const int fused = chain_ready(n, y, v[j]) && (!B || chain_ready(n, w, w));
		iter = 0;
		while (iter < c->emaxiter) {
			iter = iter + 1;
			/* QR factorization V*R = Z for starting vector Z */
			ETRY(orthogonalise(n, j, v, fused, hdev, dv));
			/* kernel: y = A * v or y = A^-1 * v; under a B: w = A * v (gpi) or w = B * v (gii); v = v / <v,w>^1/2, w = w / <v,w>^1/2; y = B^-1 * w or y = A^-1 * w */
			if (B) {
				ETRY(lis_matvec(power ? A : B, v[j], w));
				if (fused) {
					double *dvj, *dw;
					ETRY(lisd_vec_in(v[j], &dvj)); ETRY(lisd_vec_in(w, &dw));
					EHIP(liship_dot_f64(n, dvj, dw, lisg.reduce_out, lisg.reduce_work, lisg.stream));
					EHIP(liship_scale2_inv_sqrt_f64(n, lisg.reduce_out, dvj, dw, lisg.stream));
					ETRY(lisd_vec_done(v[j])); ETRY(lisd_vec_done(w));
				} else {
					ETRY(lis_vector_dot(v[j], w, &eta));
					eta = sqrt(eta);
					ETRY(lis_vector_scale(1.0 / eta, v[j]));
					ETRY(lis_vector_scale(1.0 / eta, w));
				}
			}
			if (S) ETRY(inner_solve_on(c, S, B ? w : v[j], y, 0));
			else ETRY(lis_matvec(A, v[j], y));
			if (j == 1 && S) inner_times(c);
			/* theta = <v,y>, <w,y> under a B; resid = ||y - theta * v||_2 / |theta|; y = y / ||y||_2; v = y.  Unfused, each loop takes ||y||_2 where it does there */
			if (fused) ETRY(subspace_tail(n, y, B ? w : v[j], v[j], &nrm2, &theta, &resid));
			else {
				if (!B) ETRY(lis_vector_nrm2(y, &nrm2));
				ETRY(lis_vector_dot(B ? w : v[j], y, &theta));
				ETRY(lis_vector_axpyz(-theta, v[j], y, q));
				ETRY(lis_vector_nrm2(q, &resid));
				resid = resid / fabs(theta);
				if (B) ETRY(lis_vector_nrm2(y, &nrm2));
				ETRY(lis_vector_scale(1.0 / nrm2, y));
				ETRY(lis_vector_copy(y, v[j]));
			}
			subspace_note(c, j, iter, resid);
			if (c->tol > resid) break;
		}
		ETRY(subspace_mode_end(c, B ? "Generalized Subspace" : "Subspace", j, power, theta, resid, iter, v[j], etime0));
	}
done:
	return subspace_end(c, err, hdev, dv);
}

/* ================================================================== what Lanczos and Arnoldi share */
/* the refinements after the Ritz values (lis_esolver_li.c:285-346, :627-683, lis_esolver_ai.c:322-381, :684-739): per mode a fresh eigensolver of one pair --
 * -ie's solver, or -ige's under a B, with the outer -emaxiter, -etol and -eprint, shifted by the Ritz value -- run by lis_gesolve on evector[i]; mode 0's
 * history, times, count and residual go into the outer object.  Whatever the inner eigensolver returned, the answer is LIS_SUCCESS, as there.  Under a B each
 * refinement shifts A by its Ritz value and back (lis_matrix_shift_matrix), so A's arrays carry that drift afterwards, as the reference's do. */
static LIS_INT refine_modes(ectx_t *c, const char *name)
{
	LIS_ESOLVER esolver = c->e, esolver2;
	LIS_MATRIX B = c->B;                                     /* the generalized forms refine through lis_gesolve(A, B, ...) with -ige's solver */
	const LIS_INT ss = esolver->options[LIS_EOPTIONS_SUBSPACE];
	if (c->output) lis_printf(LIS_COMM_WORLD, "computing refined eigenpairs using inner eigensolver:\n\n");
	for (LIS_INT i = 0; i < ss; i++) {
		LIS_SCALAR evalue = 0.0;
		LISCHK(lis_esolver_create(&esolver2));
		esolver2->options[LIS_EOPTIONS_ESOLVER] = esolver->options[B ? LIS_EOPTIONS_INNER_GENERALIZED_ESOLVER : LIS_EOPTIONS_INNER_ESOLVER];
		esolver2->options[LIS_EOPTIONS_SUBSPACE] = 1;
		esolver2->options[LIS_EOPTIONS_MAXITER] = c->emaxiter;
		esolver2->options[LIS_EOPTIONS_OUTPUT] = esolver->options[LIS_EOPTIONS_OUTPUT];
		esolver2->params[LIS_EPARAMS_RESID - LIS_EOPTIONS_LEN] = c->tol;
		LIS_INT err = lis_vector_duplicate(c->A, &esolver->evector[i]);
		if (err) { lis_esolver_destroy(esolver2); return err; }
		esolver2->ishift = esolver->evalue[i];
		(void)lis_gesolve(c->A, B, esolver->evector[i], &evalue, esolver2);
		if (esolver2->evalue) {
			esolver->evalue[i] = esolver2->evalue[0];
			esolver->iter[i] = esolver2->iter[0];
			esolver->resid[i] = esolver2->resid[0];
			if (i == 0) {
				if (c->output & LIS_EPRINT_MEM) for (LIS_INT ic = 0; ic < esolver2->iter[0] + 1; ic++) esolver->rhistory[ic] = esolver2->rhistory[ic];
				esolver->time = esolver2->time;
				esolver->ptime += esolver2->ptime; esolver->itime += esolver2->itime;
				esolver->p_c_time += esolver2->p_c_time; esolver->p_i_time += esolver2->p_i_time;
			}
			if (c->output) mode_report(name, i, esolver->evalue[i], esolver2->time, esolver2->iter[0], esolver2->resid[0]);
		}
		lis_esolver_destroy(esolver2);
	}
	return lis_vector_copy(esolver->evector[0], esolver->x);
}

/* the ss x ss matrix of Lanczos (tridiagonal) and of Arnoldi (Hessenberg, with `more` = 1: one entry more than there, h(ss, ss-1), which the last column's norm
 * is written to), zeroed, and the two arrays lis_array_qr works in */
static LIS_INT qr_arrays(LIS_INT ss, size_t more, LIS_SCALAR **t, LIS_SCALAR **tq, LIS_SCALAR **tr)
{
	*t = (LIS_SCALAR *)calloc((size_t)ss * ss + more, sizeof(LIS_SCALAR));
	*tq = (LIS_SCALAR *)malloc((size_t)ss * ss * sizeof(LIS_SCALAR));
	*tr = (LIS_SCALAR *)malloc((size_t)ss * ss * sizeof(LIS_SCALAR));
	if (!*t || !*tq || !*tr) return LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "malloc size = %D\n", (LIS_INT)(ss * ss * sizeof(LIS_SCALAR)));
	return LIS_SUCCESS;
}

/* how both Lanczos loops end: the eigenvalues of the symmetric tridiagonal matrix, their lines, the refinements unless -rval true (iter[] and resid[] stay 0
 * then: heap contents there).  As written there: the heading of -e gli has a space before its colon, and its elapsed-time line says Lanczos alone */
static LIS_INT lanczos_end(ectx_t *c, LIS_INT ss, LIS_SCALAR *t, LIS_SCALAR *tq, LIS_SCALAR *tr, const char *label, const char *heading)
{
	LIS_ESOLVER esolver = c->e;
	LIS_REAL qrerr;
	LIS_INT i, qriter;
	const double time0 = lis_wtime();
	LISCHK(lis_array_qr(ss, t, tq, tr, &qriter, &qrerr));
	const double time = lis_wtime() - time0;
	for (i = 0; i < ss; i++) esolver->evalue[i] = t[i * ss + i];
	if (c->output) {
		lis_printf(LIS_COMM_WORLD, "size of subspace      : %D\n\n", ss);
		lis_printf(LIS_COMM_WORLD, "%s\n\n", heading);
		for (i = 0; i < ss; i++) {
			lis_printf(LIS_COMM_WORLD, "%s: mode number          = %D\n", label, i);
			lis_printf(LIS_COMM_WORLD, "%s: Ritz value           = %e\n", label, (double)esolver->evalue[i]);
		}
		lis_printf(LIS_COMM_WORLD, "Lanczos: elapsed time         = %e sec.\n\n", time);
	}
	return esolver->options[LIS_EOPTIONS_RVAL] ? LIS_SUCCESS : refine_modes(c, label);
}

/* ------------------------------------------------------------------ Lanczos, lis_esolver_li.c:149-356 */
LIS_INT lisi_eli(LIS_ESOLVER esolver)
{
	ectx_t cx, *c = &cx;
	ectx_begin(c, esolver, 0);
	LIS_MATRIX A = c->A;
	const LIS_INT ss = esolver->options[LIS_EOPTIONS_SUBSPACE], niesolver = esolver->options[LIS_EOPTIONS_INNER_ESOLVER];
	LIS_VECTOR r = esolver->work[0], *v = &esolver->work[1];
	LIS_SCALAR dot, *t = NULL, *tq = NULL, *tr = NULL;
	LIS_REAL nrm2;
	LIS_INT err = 0, j, k;
	ETRY(qr_arrays(ss, 0, &t, &tq, &tr));
	ETRY(lis_vector_set_all(0.0, v[0]));
	ETRY(lis_vector_set_all(1.0, r));
	ETRY(lis_vector_nrm2(r, &nrm2));
	ETRY(inner_banner(c, niesolver, 0));
	j = 0;
	while (j < ss - 1) {
		j = j + 1;
		ETRY(lis_vector_copy(r, v[j]));
		/* v(j) = r / beta(j-1); r = A * v(j); r = r - beta(j-1) * v(j-1) */
		if (j == 1) {
			ETRY(lis_vector_scale(1.0 / nrm2, v[j]));
			ETRY(lis_matvec(A, v[j], r));
		} else {
			ETRY(lis_vector_scale(1.0 / t[(j - 2) * ss + j - 1], v[j]));
			ETRY(lis_matvec(A, v[j], r));
			ETRY(lis_vector_axpy(-t[(j - 2) * ss + j - 1], v[j - 1], r));
		}
		ETRY(lis_vector_dot(v[j], r, &t[(j - 1) * ss + j - 1]));             /* alpha(j) = <v(j), r> */
		ETRY(lis_vector_axpy(-t[(j - 1) * ss + j - 1], v[j], r));            /* r = r - alpha(j) * v(j) */
		for (k = 1; k < j; k++) {                                            /* reorthogonalization: of v(j), after r was formed from it, as written there */
			ETRY(lis_vector_dot(v[j], v[k], &dot));
			ETRY(lis_vector_axpy(-dot, v[k], v[j]));
		}
		ETRY(lis_vector_nrm2(r, &t[(j - 1) * ss + j]));                      /* beta(j) = ||r||_2 */
		if (fabs(t[(j - 1) * ss + j]) < c->tol) break;                       /* convergence check */
		t[j * ss + j - 1] = t[(j - 1) * ss + j];
	}
	err = lanczos_end(c, ss, t, tq, tr, "Lanczos", "Ritz values:");
done:
	free(t); free(tq); free(tr);
	return err;
}

/* ------------------------------------------------------------------ generalized Lanczos, lis_esolver_li.c:456-694.  As written there: w = &work[2] and
 * v = &work[3], so w(j+1) and v(j) are one vector -- the copy r -> w(j) overwrites v(j-1), and the reorthogonalisation of v(j) runs against overwritten vectors
 * (it does not feed t[]); the start is r = B * q with beta = |<q,r>|^1/2, B q = r is solved every step, and t(j, j-1) is |<q,r>|^1/2, not a 2-norm. */
LIS_INT lisi_egli(LIS_ESOLVER esolver)
{
	ectx_t cx, *c = &cx;
	ectx_begin(c, esolver, 0);
	LIS_MATRIX A = c->A, B = c->B;
	const LIS_INT ss = esolver->options[LIS_EOPTIONS_SUBSPACE], nigesolver = esolver->options[LIS_EOPTIONS_INNER_GENERALIZED_ESOLVER], n = A->n;
	LIS_VECTOR q = esolver->work[0], r = esolver->work[1], *w = &esolver->work[2], *v = &esolver->work[3];
	LIS_SCALAR beta, dot, div, *t = NULL, *tq = NULL, *tr = NULL;
	LIS_INT err = 0, j, k;
	ETRY(qr_arrays(ss, 0, &t, &tq, &tr));
	ETRY(lis_vector_set_all(0.0, w[0]));
	ETRY(lis_vector_set_all(0.0, v[0]));
	ETRY(lis_vector_set_all(1.0, q));
	ETRY(inner_banner(c, nigesolver, 1));
	c->solver->A = B;
	ETRY(lis_precon_create(c->solver, &c->precon));
	j = 0;
	while (j < ss - 1) {
		j = j + 1;
		/* w(j) = r / beta(j-1); v(j) = q / beta(j-1); r = A * v(j); r = r - beta(j-1) * w(j-1) */
		if (j == 1) {
			ETRY(lis_matvec(B, q, r));
			ETRY(lis_vector_dot(q, r, &beta));
			beta = sqrt(fabs(beta));
			div = beta;
		} else div = t[(j - 2) * ss + j - 1];
		if (chain_ready(n, r, q) && chain_ready(n, w[j], v[j])) {            /* copy, copy, scale, scale: one pass */
			double *dr, *dq, *dwj, *dvj;
			ETRY(lisd_vec_in(r, &dr)); ETRY(lisd_vec_in(q, &dq));
			ETRY(lisd_vec_out(w[j], &dwj)); ETRY(lisd_vec_out(v[j], &dvj));
			EHIP(liship_scale2_to_f64(n, 1.0 / div, dr, dq, dwj, dvj, lisg.stream));
			ETRY(lisd_vec_done(w[j])); ETRY(lisd_vec_done(v[j]));
		} else {
			ETRY(lis_vector_copy(r, w[j]));
			ETRY(lis_vector_copy(q, v[j]));
			ETRY(lis_vector_scale(1.0 / div, w[j]));
			ETRY(lis_vector_scale(1.0 / div, v[j]));
		}
		ETRY(lis_matvec(A, v[j], r));
		ETRY(lis_vector_axpy(-div, w[j - 1], r));
		ETRY(lis_vector_dot(v[j], r, &t[(j - 1) * ss + j - 1]));             /* alpha(j) = <v(j), r> */
		ETRY(lis_vector_axpy(-t[(j - 1) * ss + j - 1], w[j], r));            /* r = r - alpha(j) * w(j) */
		for (k = 1; k < j; k++) {                                            /* reorthogonalization, as written there */
			ETRY(lis_vector_dot(v[j], v[k], &dot));
			ETRY(lis_vector_axpy(-dot, v[k], v[j]));
		}
		ETRY(inner_solve_on(c, B, r, q, 0));                                 /* solve B * q = r */
		ETRY(lis_vector_dot(q, r, &beta));                                   /* beta(j) = |<q,r>|^1/2 */
		beta = sqrt(fabs(beta));
		t[(j - 1) * ss + j] = beta;
		if (fabs(t[(j - 1) * ss + j]) < c->tol) break;                       /* convergence check */
		t[j * ss + j - 1] = t[(j - 1) * ss + j];
	}
	err = lanczos_end(c, ss, t, tq, tr, "Generalized Lanczos", "Ritz values :");
done:
	inner_destroy(c);
	free(t); free(tq); free(tr);
	return err;
}

/* ================================================================== Arnoldi, standard and generalized */
/* column j of the Hessenberg matrix: h(i,j) = <v(i), w>; w = w - h(i,j) * v(i), i = 0 .. j; h(j+1,j) = ||w||_2 -- with hdev as one chain and one read-back per
 * column (it comes home through the page-locked landing zone), or the lis_vector_* calls */
static LIS_INT hessenberg_column(LIS_INT n, LIS_INT ss, LIS_INT j, LIS_VECTOR *v, LIS_VECTOR w, LIS_SCALAR *h, double *hdev, double **dv)
{
	LIS_INT err = 0, i;
	if (hdev) {
		double *dw;
		ETRY(lisd_vec_in(w, &dw));
		for (i = 0; i <= j; i++) ETRY(lisd_vec_in(v[i], &dv[i]));
		EHIP(liship_dot_f64(n, dv[0], dw, hdev, lisg.reduce_work, lisg.stream));
		ETRY(lisd_mgs_chain(n, j + 1, dv, dw, hdev));
		EHIP(liship_mgs_step_f64(n, hdev + j, dv[j], dw, NULL, hdev + j + 1, lisg.reduce_work, lisg.stream));
		ETRY(lisd_vec_done(w));
		ETRY(lisd_fetch_from(hdev, j + 2, h + j * ss));                     /* the column h(0..j, j) and, in h(j+1, j), the sum of squares */
		h[j + 1 + j * ss] = sqrt(h[j + 1 + j * ss]);
	} else {
		for (i = 0; i <= j; i++) {
			ETRY(lis_vector_dot(v[i], w, &h[i + j * ss]));
			ETRY(lis_vector_axpy(-h[i + j * ss], v[i], w));
		}
		ETRY(lis_vector_nrm2(w, &h[j + 1 + j * ss]));                        /* h(j+1,j) = ||w||_2 */
	}
done:
	return err;
}

/* the Ritz values from the upper Hessenberg matrix QR left: the diagonal and the 2 x 2 blocks (a complex pair gives its real part twice), with their lines.
 * pad: the blanks between `mode number` and `=`, which differ between -e ai (10) and -e gai (14) there */
static void ritz_values(ectx_t *c, LIS_INT ss, const LIS_SCALAR *h, const char *label, int pad)
{
	LIS_ESOLVER esolver = c->e;
	LIS_REAL D;
	LIS_INT i = 0;
	while (i < ss) {
		i = i + 1;
		if (c->output) lis_printf(LIS_COMM_WORLD, "%s: mode number%*s= %D\n", label, pad, "", i - 1);
		if (!(ss == i || fabs(h[i + (i - 1) * ss]) < c->tol)) {
			D = (h[i - 1 + (i - 1) * ss] + h[i + i * ss]) * (h[i - 1 + (i - 1) * ss] + h[i + i * ss])
			    - 4 * (h[i - 1 + (i - 1) * ss] * h[i + i * ss] - h[i - 1 + i * ss] * h[i + (i - 1) * ss]);
			if (D < 0) {
				if (c->output) {
					lis_printf(LIS_COMM_WORLD, "%s: Ritz value%*s= (%e, %e)\n", label, pad + 1, "", (double)((h[i - 1 + (i - 1) * ss] + h[i + i * ss]) / 2), (double)sqrt(-D) / 2);
					lis_printf(LIS_COMM_WORLD, "%s: mode number%*s= %D\n", label, pad, "", i);
					lis_printf(LIS_COMM_WORLD, "%s: Ritz value%*s= (%e, %e)\n", label, pad + 1, "", (double)((h[i - 1 + (i - 1) * ss] + h[i + i * ss]) / 2), (double)-sqrt(-D) / 2);
				}
				esolver->evalue[i - 1] = (h[i - 1 + (i - 1) * ss] + h[i + i * ss]) / 2;
				esolver->evalue[i] = (h[i - 1 + (i - 1) * ss] + h[i + i * ss]) / 2;
				i = i + 1;
				continue;
			}
		}
		if (c->output) lis_printf(LIS_COMM_WORLD, "%s: Ritz value%*s= %e\n", label, pad + 1, "", (double)(h[i - 1 + (i - 1) * ss]));
		esolver->evalue[i - 1] = h[i - 1 + (i - 1) * ss];
	}
}

/* ------------------------------------------------------------------ Arnoldi, lis_esolver_ai.c:151-391, and generalized Arnoldi, lis_esolver_ai.c:491-750: the
 * same loop with w = B^-1 * (A * v(j)) -- solve, then copy y -> w -- in front of the Hessenberg column, a linear solver that is kept and a preconditioner on B.
 * (At i = ss the reference's generalized read-out reads h(ss, ss-1) and h(ss, ss), past its array; the last mode's Ritz value is the diagonal entry here.) */
LIS_INT lisi_eai(LIS_ESOLVER esolver)
{
	ectx_t cx, *c = &cx;
	ectx_begin(c, esolver, 0);
	LIS_MATRIX A = c->A, B = c->B;
	const LIS_INT ss = esolver->options[LIS_EOPTIONS_SUBSPACE], n = A->n;
	const LIS_INT ninner = esolver->options[B ? LIS_EOPTIONS_INNER_GENERALIZED_ESOLVER : LIS_EOPTIONS_INNER_ESOLVER];
	const char *label = B ? "Generalized Arnoldi" : "Arnoldi";
	LIS_VECTOR w = esolver->work[0], y = esolver->work[1], *v = &esolver->work[B ? 2 : 1];      /* y: of the generalized loop only */
	LIS_SCALAR *h = NULL, *hq = NULL, *hr = NULL;
	LIS_REAL nrm2, hqrerr;
	LIS_INT err = 0, j, hqriter;
	double time, time0, *hdev = NULL, **dv = NULL;
	ETRY(qr_arrays(ss, 1, &h, &hq, &hr));
	ETRY(lis_vector_set_all(1.0, v[0]));
	ETRY(lis_vector_nrm2(v[0], &nrm2));
	ETRY(lis_vector_scale(1.0 / nrm2, v[0]));
	ETRY(inner_banner(c, ninner, B != NULL));
	if (B) {
		c->solver->A = B;
		ETRY(lis_precon_create(c->solver, &c->precon));
	}
	ETRY(chain_alloc(ss, !lisg.no_fusion && ss + 1 <= 256, &hdev, &dv));     /* (a column comes home through the page-locked landing zone) */
	j = -1;
	while (j < ss - 1) {
		j = j + 1;
		ETRY(lis_matvec(A, v[j], w));                                        /* w = A * v(j) */
		if (B) {
			ETRY(inner_solve_on(c, B, w, y, 0));                             /* w = B^-1 * w */
			ETRY(lis_vector_copy(y, w));
		}
		ETRY(hessenberg_column(n, ss, j, v, w, h, hdev, dv));
		if (fabs(h[j + 1 + j * ss]) < c->tol) break;                         /* convergence check */
		ETRY(lis_vector_scale(1 / h[j + 1 + j * ss], w));                    /* v(j+1) = w / h(j+1,j) */
		ETRY(lis_vector_copy(w, v[j + 1]));
	}
	/* eigenvalues of the upper Hessenberg matrix */
	time0 = lis_wtime();
	ETRY(lis_array_qr(ss, h, hq, hr, &hqriter, &hqrerr));
	time = lis_wtime() - time0;
	if (c->output) {
		lis_printf(LIS_COMM_WORLD, "size of subspace      : %D\n\n", ss);
		lis_printf(LIS_COMM_WORLD, "Ritz values:\n\n");
	}
	ritz_values(c, ss, h, label, B ? 14 : 10);
	lis_printf(LIS_COMM_WORLD, "%s: elapsed time         = %e sec.\n\n", label, time);      /* (printed at -eprint none too, as there) */
	if (!esolver->options[LIS_EOPTIONS_RVAL]) err = refine_modes(c, label);
done:
	inner_destroy(c);
	if (hdev) (void)liship_free(hdev);
	free(dv);
	free(h); free(hq); free(hr);
	return err;
}
