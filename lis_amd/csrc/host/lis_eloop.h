/*
 * lis_eloop.h -- what the eigensolver loops of liblis_amd share: the loop context, the error-unwinding macros, the inner linear solver and its
 * preconditioner, the pencil shift, the loop prologue and the Gram block.  Included by lis_esolver.c (the object, the descriptor table, lis_gesolve),
 * lis_esolver_single.c (the loops of one pair) and lis_esolver_multi.c (the loops of several pairs).
 *
 * Each loop is the reference's recurrence statement for statement; its vectors stay in HBM (the lis_vector_* calls are the library's device passes), its
 * scalars go through the host, its inner linear solves are this library's own lis_solve / lis_solve_kernel with the option string the reference gives them
 * ("-i bicg -p none", "-i cg -p none" for -e cg, then lis_solver_set_optionC), its shifts are lis_matrix_shift_diagonal and, under a B,
 * lis_matrix_shift_matrix (lis_shift.c, kernels/spgeam.hip: A - sigma B merged row by row in HBM where the reference goes through two dense n x n copies).
 * With lis_amd_set_reference_reductions(T) a whole esolve carries the bits of the reference at T threads (tests/test_esolve_gpu.py).
 */
#ifndef LIS_AMD_ELOOP_H
#define LIS_AMD_ELOOP_H
#include <stdio.h>
#include <stdint.h>
#include "lis_internal.h"

/* the run functions of the descriptor table (lis_esolver.c): one pair (lis_esolver_single.c), several pairs (lis_esolver_multi.c) */
LIS_INT lisi_epi_ii(LIS_ESOLVER esolver);      /* -e pi | ii | gpi | gii */
LIS_INT lisi_erqi(LIS_ESOLVER esolver);
LIS_INT lisi_egrqi(LIS_ESOLVER esolver);
LIS_INT lisi_ecg(LIS_ESOLVER esolver);
LIS_INT lisi_ecr(LIS_ESOLVER esolver);
LIS_INT lisi_egcr(LIS_ESOLVER esolver);
LIS_INT lisi_esi(LIS_ESOLVER esolver);         /* -e si | gsi */
LIS_INT lisi_eli(LIS_ESOLVER esolver);
LIS_INT lisi_egli(LIS_ESOLVER esolver);
LIS_INT lisi_eai(LIS_ESOLVER esolver);         /* -e ai | gai */

#define ETRY(expr) do { LIS_INT e__ = (expr); if (e__) { err = e__; goto done; } } while (0)
#define EHIP(call) do { int rc__ = (call); if (rc__) { err = lisi_hip_error(__FILE__, __func__, __LINE__, rc__); goto done; } } while (0)

typedef struct {
	LIS_ESOLVER e;
	LIS_MATRIX A, B;          /* B: NULL in the standard problem */
	LIS_INT emaxiter, output;
	LIS_REAL tol;
	LIS_SCALAR oshift;
	int shifted;              /* ebegin shifted the pencil by oshift: eend shifts it back */
	LIS_SOLVER solver;        /* the inner linear solver and its preconditioner (all but pi) */
	LIS_PRECON precon;
	const lisi_precon_kind *pk;   /* cg, cr, gcr: lis_psolve(solver, r, w) through the preconditioner's row ... */
	lisi_precon_state ps;         /* ... resolved once, after the precon was created (no shift happens inside those loops) */
} ectx_t;

static inline void ectx_begin(ectx_t *c, LIS_ESOLVER e, int shifts)
{
	memset(c, 0, sizeof(*c));
	c->e = e; c->A = e->A; c->B = e->B;
	c->emaxiter = e->options[LIS_EOPTIONS_MAXITER];
	c->tol = e->params[LIS_EPARAMS_RESID - LIS_EOPTIONS_LEN];
	c->output = e->options[LIS_EOPTIONS_OUTPUT];
	c->oshift = e->params[LIS_EPARAMS_SHIFT - LIS_EOPTIONS_LEN];
	if (shifts && e->ishift != 0.0) c->oshift = e->ishift;
}

static inline void enote(ectx_t *c, LIS_INT iter, LIS_REAL resid)
{	/* the convergence-check block of every loop (lis_esolver_pi.c:197-201); lis_print_rhistory: src/system/lis_error.c:193-203 */
	if (!c->output) return;
	if (c->output & LIS_EPRINT_MEM) c->e->rhistory[iter] = resid;
	if (c->output & LIS_EPRINT_OUT) lis_printf(LIS_COMM_WORLD, "iteration: %5d  relative residual = %E\n", (int)iter, (double)resid);
}

/* lis_solver_create, the reference's option string, the command line's options, the two banner lines (lis_esolver_ii.c:182-194) */
static inline LIS_INT inner_solver(ectx_t *c, char *options)
{
	char solvername[128], preconname[128];
	LIS_INT nsol, precon_type;
	LISCHK(lis_solver_create(&c->solver));
	LISCHK(lis_solver_set_option(options, c->solver));
	LISCHK(lis_solver_set_optionC(c->solver));
	lis_solver_get_solver(c->solver, &nsol);
	lis_solver_get_precon(c->solver, &precon_type);
	if (c->output) {
		if (lis_solver_get_solvername(nsol, solvername) == LIS_SUCCESS) lis_printf(LIS_COMM_WORLD, "linear solver         : %s\n", solvername);
		if (lis_solver_get_preconname(precon_type, preconname) == LIS_SUCCESS) lis_printf(LIS_COMM_WORLD, "preconditioner        : %s\n", preconname);
	}
	return LIS_SUCCESS;
}

static inline void inner_times(ectx_t *c)
{	/* lis_esolver_ii.c:237-241 */
	c->e->ptime += c->solver->ptime; c->e->itime += c->solver->itime;
	c->e->p_c_time += c->solver->p_c_time; c->e->p_i_time += c->solver->p_i_time;
}

static inline void inner_destroy(ectx_t *c)
{
	if (c->precon) lis_precon_destroy(c->precon);
	if (c->solver) lis_solver_destroy(c->solver);
	c->precon = NULL; c->solver = NULL;
}

/* An inner solve: y = M^-1 b by lis_solve_kernel with the loop's preconditioner, or (whole) by lis_solve.  It always runs in the library's default loop form:
 * lis_solve's own passes do NOT give the same bits fused and unfused in the tree mode (the product's fused dot epilogue sums in another order than
 * liship_dot_f64: `lis_solve -i cg` on the 10 x 10 Laplacian ends with another x under LIS_AMD_NO_FUSION=1), so inside an esolve that switch selects the
 * esolver's own passes only -- the Gram blocks, the chains, the pair passes -- and a fused and an unfused esolve agree in every bit (tests/test_esolve_gpu.py) */
static inline LIS_INT inner_solve_on(ectx_t *c, LIS_MATRIX M, LIS_VECTOR b, LIS_VECTOR y, int whole)
{
	const int held = lisg.no_fusion;
	lisg.no_fusion = 0;
	const LIS_INT err = whole ? lis_solve(M, b, y, c->solver) : lis_solve_kernel(M, b, y, c->solver, c->precon);
	lisg.no_fusion = held;
	return err;
}

/* the preconditioner of cg / cr / gcr made ready for lis_psolve calls outside a solve: the row's begin, as lis_solve_kernel runs it */
static inline LIS_INT psolve_begin(ectx_t *c)
{
	c->pk = lisi_precon_kind_of(c->precon->precon_type);
	if (!c->pk) return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "preconditioner %D is not served by liblis_amd\n", c->precon->precon_type);
	LISCHK(lisd_mat_ready(c->A));
	c->solver->precon = c->precon;
	return c->pk->begin(c->A, c->solver, &c->ps);
}
static inline LIS_INT psolve(ectx_t *c, LIS_VECTOR r, LIS_VECTOR w)
{	/* w = M^-1 r (lis_psolve) */
	double *dr, *dw;
	LISCHK(lisd_vec_in(r, &dr)); LISCHK(lisd_vec_out(w, &dw));
	LISCHK(c->pk->apply(&c->ps, 0, dr, dw));
	return lisd_vec_done(w);
}

/* a Gram block: out[k] = <v[pairs[k][0]], v[pairs[k][1]]>, one pass (lisd_multidot) -- the bits of the separate dots, which LIS_AMD_NO_FUSION=1 /
 * lis_amd_set_loop_mode(LIS_AMD_LOOP_UNFUSED) brings back */
static inline LIS_INT gram(LIS_INT n, int nvec, LIS_VECTOR *v, int K, const int (*pairs)[2], double *out)
{
	const double *dv[LISHIP_MULTIDOT_MAX_VECS];
	for (int i = 0; i < nvec; i++) { double *p; LISCHK(lisd_vec_in(v[i], &p)); dv[i] = p; }
	return lisd_multidot(n, nvec, dv, K, pairs, out);
}

static inline LIS_INT normalize(LIS_VECTOR v)
{	/* v = v / ||v||_2 */
	LIS_REAL nrm2;
	LISCHK(lis_vector_nrm2(v, &nrm2));
	return lis_vector_scale(1.0 / nrm2, v);
}

static inline int chain_ready(LIS_INT n, LIS_VECTOR a, LIS_VECTOR b)
{	/* liship_ritz_tail_f64 takes 16 B aligned arrays (every vector the library allocates is) */
	double *pa, *pb;
	if (lisg.no_fusion || n <= 0) return 0;
	if (lisd_vec_in(a, &pa) || lisd_vec_in(b, &pb)) return 0;
	return (((uintptr_t)pa | (uintptr_t)pb) & 15u) == 0;
}

/* ------------------------------------------------------------------ the pencil shift: A - sigma B under a B, A - sigma I otherwise */
static inline LIS_INT eshift(ectx_t *c, LIS_SCALAR sigma)
{
	return c->B ? lis_matrix_shift_matrix(c->A, c->B, sigma) : lis_matrix_shift_diagonal(c->A, sigma);
}
static inline LIS_INT eunshift(ectx_t *c, LIS_SCALAR sigma, LIS_INT err)
{	/* the shift taken back; its own failure is the answer only where the loop had none (LIS_MAXITER is none) */
	const LIS_INT e2 = eshift(c, -sigma);
	return e2 && (!err || err == LIS_MAXITER) ? e2 : err;
}

/* how pi, ii, cg, cr, gpi, gii and gcr begin: -initx_ones, the shift where there is one, its banner line.  si and gsi begin with the last two (x = NULL) */
static inline LIS_INT ebegin(ectx_t *c, LIS_VECTOR x)
{
	if (x && c->e->options[LIS_EOPTIONS_INITGUESS_ONES]) LISCHK(lis_vector_set_all(1.0, x));
	if (c->oshift != 0.0) { LISCHK(eshift(c, c->oshift)); c->shifted = 1; }
	if (c->output) lis_printf(LIS_COMM_WORLD, "shift                 : %e\n", (double)c->oshift);
	return LIS_SUCCESS;
}
static inline LIS_INT eend(ectx_t *c, LIS_INT err) { return c->shifted ? eunshift(c, c->oshift, err) : err; }
#endif
