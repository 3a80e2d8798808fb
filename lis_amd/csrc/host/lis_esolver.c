/*
 * lis_esolver.c -- lis_esolve: the eigen half of the Lis C API (reference src/esolver/lis_esolver.c and lis_esolver_pi.c, _ii.c, _rqi.c, _cg.c).
 *
 * Served: the five standard eigensolvers of one eigenpair -- power (-e pi), inverse (-e ii), Rayleigh quotient (-e rqi), CG (-e cg) and CR (-e cr, the
 * default) iteration.  Each loop below is the reference's recurrence statement for statement; its vectors stay in HBM (the lis_vector_* calls are the
 * library's device passes), its scalars go through the host, its inner linear solves are this library's own lis_solve / lis_solve_kernel with the option
 * string the reference gives them ("-i bicg -p none", "-i cg -p none" for -e cg, then lis_solver_set_optionC), its shifts are lis_matrix_shift_diagonal
 * (lis_shift.c).  With lis_amd_set_reference_reductions(T) a whole esolve carries the bits of the reference at T threads (tests/test_esolve_gpu.py).
 * The Gram blocks of CG (12 inner products over 6 vectors) and CR (5 over 3, 4 over 4) are taken in one pass each by lisd_multidot -- the bits of the
 * separate dots, which LIS_AMD_NO_FUSION=1 / lis_amd_set_loop_mode(LIS_AMD_LOOP_UNFUSED) brings back (the inner solves keep the default loop form: inner_solve).
 *
 * Refused, with LIS_ERR_NOT_IMPLEMENTED and before A or x is touched: the subspace, Lanczos and Arnoldi solvers (-e si | li | ai), every generalized solver
 * (-e gpi .. gai, lis_gesolve with a B), a job of several ranks, and the getters only those solvers fill (lis_esolver_get_evectors, lis_esolver_get_specific_*).
 * -ef quad | switch answers as lis_solve does for -f quad.
 *
 * Deliberate differences from the reference, all outside a converging solve: the arrays of the object start zeroed instead of holding heap contents; a
 * negative -emaxiter is refused; an inner solve that fails hands its code back as the return value (the reference returns LIS_SUCCESS and leaves A shifted
 * in -e rqi); work vectors of an earlier solve are released instead of leaked.
 */
#include <stdio.h>
#include <ctype.h>
#include "lis_internal.h"

static const char *esolver_keys[] = {"pi", "ii", "rqi", "cg", "cr", "si", "li", "ai", "gpi", "gii", "grqi", "gcg", "gcr", "gsi", "gli", "gai"};   /* ref lis_esolver.c:118 */
static const char *eprint_keys[] = {"none", "mem", "out", "all"};
static const char *etruefalse_keys[] = {"false", "true"};
static const char *estorage_keys[] = {"csr", "csc", "msr", "dia", "ell", "jad", "bsr", "bsc", "vbr", "coo", "dns"};
static const char *eprecision_keys[] = {"double", "quad", "switch"};
static const char *esolver_names[] = {"", "Power", "Inverse", "Rayleigh Quotient", "CG", "CR", "Subspace", "Lanczos", "Arnoldi", "Generalized Power", "Generalized Inverse",
	"Generalized Rayleigh Quotient", "Generalized CG", "Generalized CR", "Generalized Subspace", "Generalized Lanczos", "Generalized Arnoldi"};       /* ref :124 */
static const char *estorage_names[] = {"CSR", "CSC", "MSR", "DIA", "ELL", "JAD", "BSR", "BSC", "VBR", "COO", "DNS"};
static const char *ereturncode_names[] = {"LIS_SUCCESS", "LIS_ILL_OPTION", "LIS_BREAKDOWN", "LIS_OUT_OF_MEMORY", "LIS_MAXITER", "LIS_NOT_IMPLEMENTED", "LIS_ERR_FILE_IO"};
#define COUNT(a) ((int)(sizeof(a) / sizeof((a)[0])))

/* ------------------------------------------------------------------ the object */
static void esolver_init(LIS_ESOLVER e)
{	/* ref lis_esolver_init, :143-187 */
	memset(e, 0, sizeof(*e));
	e->eprecision = LIS_PRECISION_DOUBLE;
	e->options[LIS_EOPTIONS_ESOLVER] = LIS_ESOLVER_CR;
	e->options[LIS_EOPTIONS_MAXITER] = 1000;
	e->options[LIS_EOPTIONS_SUBSPACE] = 1;
	e->options[LIS_EOPTIONS_MODE] = 0;
	e->options[LIS_EOPTIONS_OUTPUT] = LIS_FALSE;
	e->options[LIS_EOPTIONS_INITGUESS_ONES] = LIS_TRUE;
	e->options[LIS_EOPTIONS_INNER_ESOLVER] = LIS_ESOLVER_II;
	e->options[LIS_EOPTIONS_INNER_GENERALIZED_ESOLVER] = LIS_ESOLVER_GII;
	e->options[LIS_EOPTIONS_STORAGE] = 0;
	e->options[LIS_EOPTIONS_STORAGE_BLOCK] = 2;
	e->options[LIS_EOPTIONS_PRECISION] = LIS_PRECISION_DOUBLE;
	e->options[LIS_EOPTIONS_RVAL] = LIS_FALSE;
	e->params[LIS_EPARAMS_RESID - LIS_EOPTIONS_LEN] = 1.0e-12;
	e->params[LIS_EPARAMS_SHIFT - LIS_EOPTIONS_LEN] = 0.0;
	e->params[LIS_EPARAMS_SHIFT_IM - LIS_EOPTIONS_LEN] = 0.0;
}

LIS_INT lis_esolver_create(LIS_ESOLVER *esolver)
{
	*esolver = (LIS_ESOLVER)malloc(sizeof(struct LIS_ESOLVER_STRUCT));
	if (!*esolver) return LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "malloc size = %D\n", (LIS_INT)sizeof(struct LIS_ESOLVER_STRUCT));
	esolver_init(*esolver);
	return LIS_SUCCESS;
}

static void work_destroy(LIS_ESOLVER e)
{	/* ref lis_esolver_work_destroy, :211-227 */
	if (e && e->work) {
		for (LIS_INT i = 0; i < e->worklen; i++) lis_vector_destroy(e->work[i]);
		free(e->work);
		e->work = NULL; e->worklen = 0;
	}
}

LIS_INT lis_esolver_destroy(LIS_ESOLVER e)
{	/* ref :231-259 (evector holds vectors for the subspace solvers only: not served) */
	if (e) {
		work_destroy(e);
		free(e->rhistory); free(e->evalue); free(e->resid); free(e->iter); free(e->iter2); free(e->evector);
		free(e);
	}
	return LIS_SUCCESS;
}

/* ------------------------------------------------------------------ options, ref :103-122 (tables), :726-1052 (lis_esolver_set_option2 and its helpers) */
static LIS_INT epick(const char *val, char lo, char hi, const char **keys, int nkeys, int base, LIS_INT *slot, const char *what)
{	/* a leading digit in [lo, hi]: the number (no range check here, as there); else the name; else ILL_ARG */
	if (val[0] >= lo && val[0] <= hi) { sscanf(val, "%d", slot); return LIS_SUCCESS; }
	for (int i = 0; i < nkeys; i++) if (strcmp(val, keys[i]) == 0) { *slot = i + base; return LIS_SUCCESS; }
	return LISI_ERR(LIS_ERR_ILL_ARG, "Parameter %s is not correct\n", what);
}

static LIS_INT eset_one(const char *name, const char *val, LIS_ESOLVER e)
{
	static const struct { const char *name; int slot; } table[] = {
		{"-emaxiter", LIS_EOPTIONS_MAXITER}, {"-etol", LIS_EPARAMS_RESID}, {"-e", LIS_EOPTIONS_ESOLVER}, {"-ss", LIS_EOPTIONS_SUBSPACE}, {"-m", LIS_EOPTIONS_MODE},
		{"-shift", LIS_EPARAMS_SHIFT}, {"-shift_im", LIS_EPARAMS_SHIFT_IM}, {"-eprint", LIS_EOPTIONS_OUTPUT}, {"-initx_ones", LIS_EOPTIONS_INITGUESS_ONES},
		{"-ie", LIS_EOPTIONS_INNER_ESOLVER}, {"-ige", LIS_EOPTIONS_INNER_GENERALIZED_ESOLVER}, {"-estorage", LIS_EOPTIONS_STORAGE},
		{"-estorage_block", LIS_EOPTIONS_STORAGE_BLOCK}, {"-ef", LIS_EOPTIONS_PRECISION}, {"-rval", LIS_EOPTIONS_RVAL},
	};
	LIS_INT *o = e->options;
	for (int i = 0; i < COUNT(table); i++) {
		if (strcmp(name, table[i].name) != 0) continue;
		const int slot = table[i].slot;
		switch (slot) {
		case LIS_EOPTIONS_ESOLVER:        return epick(val, '0', '9', esolver_keys, COUNT(esolver_keys), 1, &o[slot], "LIS_EOPTIONS_ESOLVER");
		case LIS_EOPTIONS_INNER_ESOLVER:  return epick(val, '0', '9', esolver_keys, COUNT(esolver_keys), 1, &o[slot], "LIS_EOPTIONS_INNER_ESOLVER");
		case LIS_EOPTIONS_INNER_GENERALIZED_ESOLVER: return epick(val, '0', '9', esolver_keys, COUNT(esolver_keys), 1, &o[slot], "LIS_EOPTIONS_INNER_GENERALIZED_ESOLVER");
		case LIS_EOPTIONS_OUTPUT:         return epick(val, '0', '3', eprint_keys, COUNT(eprint_keys), 0, &o[slot], "LIS_EOPTIONS_OUTPUT");
		case LIS_EOPTIONS_INITGUESS_ONES: case LIS_EOPTIONS_RVAL:
		                                  return epick(val, '0', '1', etruefalse_keys, COUNT(etruefalse_keys), 0, &o[slot], "LIS_EOPTIONS_TRUEFALSE");
		case LIS_EOPTIONS_STORAGE:        return epick(val, '0', '9', estorage_keys, COUNT(estorage_keys), 1, &o[slot], "LIS_EOPTIONS_STORAGE");
		case LIS_EOPTIONS_PRECISION:      return epick(val, '0', '1', eprecision_keys, COUNT(eprecision_keys), 0, &o[slot], "LIS_EOPTIONS_PRECISION");
		default:
			if (slot < LIS_EOPTIONS_LEN) sscanf(val, "%d", &o[slot]);
			else { double v; if (sscanf(val, "%lg", &v) == 1) e->params[slot - LIS_EOPTIONS_LEN] = v; }
			return LIS_SUCCESS;
		}
	}
	return LIS_SUCCESS;      /* unknown options are ignored, as in the reference */
}

static LIS_INT eset_from_tokens(char **tok, int n, LIS_ESOLVER e)
{	/* the pairs lis_text2args / lis_initialize keep (src/system/lis_args.c): "-name value", both lower-cased */
	for (int i = 0; i + 1 < n; i++) {
		if (tok[i][0] != '-' || (tok[i][1] >= '0' && tok[i][1] <= '9')) continue;
		char name[64], val[256];
		size_t k;
		for (k = 0; tok[i][k] && k + 1 < sizeof(name); k++) name[k] = (char)tolower((unsigned char)tok[i][k]);
		name[k] = 0;
		for (k = 0; tok[i + 1][k] && k + 1 < sizeof(val); k++) val[k] = (char)tolower((unsigned char)tok[i + 1][k]);
		val[k] = 0;
		const LIS_INT err = eset_one(name, val, e);
		if (err) { work_destroy(e); e->retcode = err; return err; }
	}
	return LIS_SUCCESS;
}

LIS_INT lis_esolver_set_option(char *text, LIS_ESOLVER esolver)
{
	char **tok;
	const int n = lisi_tokenize(text, &tok);
	const LIS_INT err = eset_from_tokens(tok, n, esolver);
	lisi_tokens_free(tok, n);
	return err;
}

LIS_INT lis_esolver_set_optionC(LIS_ESOLVER esolver) { return eset_from_tokens(lisi_cmd_argv, lisi_cmd_argc, esolver); }

/* ------------------------------------------------------------------ getters, ref :1056-1384 */
LIS_INT lis_esolver_get_iter(LIS_ESOLVER e, LIS_INT *iter) { *iter = e->iter[0]; return LIS_SUCCESS; }
LIS_INT lis_esolver_get_iterex(LIS_ESOLVER e, LIS_INT *iter, LIS_INT *iter_double, LIS_INT *iter_quad)
{ *iter = e->iter[0]; *iter_double = e->iter2[0]; *iter_quad = e->iter[0] - e->iter2[0]; return LIS_SUCCESS; }
LIS_INT lis_esolver_get_time(LIS_ESOLVER e, double *time) { *time = e->time; return LIS_SUCCESS; }
LIS_INT lis_esolver_get_timeex(LIS_ESOLVER e, double *time, double *itime, double *ptime, double *p_c_time, double *p_i_time)
{
	*time = e->time;
	if (itime) *itime = e->itime;
	if (ptime) *ptime = e->ptime;
	if (p_c_time) *p_c_time = e->p_c_time;
	if (p_i_time) *p_i_time = e->p_i_time;
	return LIS_SUCCESS;
}
LIS_INT lis_esolver_get_residualnorm(LIS_ESOLVER e, LIS_REAL *residual) { *residual = e->resid[0]; return LIS_SUCCESS; }
LIS_INT lis_esolver_get_status(LIS_ESOLVER e, LIS_INT *status) { *status = e->retcode; return LIS_SUCCESS; }
LIS_INT lis_esolver_get_esolver(LIS_ESOLVER e, LIS_INT *nesol) { *nesol = e->options[LIS_EOPTIONS_ESOLVER]; return LIS_SUCCESS; }
LIS_INT lis_esolver_get_esolvername(LIS_INT esolver, char *esolvername)
{
	if (esolver < 1 || esolver > LIS_ESOLVER_LEN) return LIS_FAILS;
	strcpy(esolvername, esolver_names[esolver]);
	return LIS_SUCCESS;
}

static LIS_INT history_len(LIS_ESOLVER e)
{	/* ref :1138-1142: the entries 0 .. iter of a solve that converged, 0 .. iter - 1 otherwise */
	LIS_INT len = e->iter[0] + 1;
	if (e->retcode != LIS_SUCCESS) len--;
	return len;
}

LIS_INT lis_esolver_get_rhistory(LIS_ESOLVER e, LIS_VECTOR v)
{
	const LIS_INT n = _min(v->n, history_len(e));
	LISCHK(lisd_vec_host_write(v, 1));
	for (LIS_INT i = 0; i < n; i++) v->value[i] = e->rhistory[i];
	lis_amd_vector_host_modified(v);
	return LIS_SUCCESS;
}

LIS_INT lis_esolver_output_rhistory(LIS_ESOLVER e, char *filename)
{	/* ref src/system/lis_output.c:659-728 */
	if (e->rhistory == NULL) return LISI_ERR(LIS_ERR_ILL_ARG, "eigensolver's residual history is empty\n");
	FILE *file = fopen(filename, "w");
	if (file == NULL) return LISI_ERR(LIS_ERR_FILE_IO, "cannot open file %s\n", filename);
	const LIS_INT len = history_len(e);
	for (LIS_INT i = 0; i < len; i++) fprintf(file, "%e\n", (double)e->rhistory[i]);
	fclose(file);
	return LIS_SUCCESS;
}

/* what the subspace, Lanczos and Arnoldi solvers fill.  The reference answers LIS_ERR_ILL_ARG for any other solver (:1159-1163 and alike); none of
 * those that could ask is served, and the answer says so */
static LIS_INT subspace_only(const char *what)
{
	return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "%s is filled by the subspace, Lanczos and Arnoldi eigensolvers only, which liblis_amd does not serve\n", what);
}
/* the three that copy the object's arrays of ss entries into a vector (ref :1153-1179, :1261-1287, :1309-1337): as there, LIS_ERR_ILL_ARG unless
 * -e names a subspace, Lanczos or Arnoldi solver -- and those never ran here, so there is nothing to copy for them either */
static LIS_INT per_mode(LIS_ESOLVER e, LIS_VECTOR v, int what)
{
	const LIS_INT nesolver = e->options[LIS_EOPTIONS_ESOLVER];
	if (nesolver != LIS_ESOLVER_SI && nesolver != LIS_ESOLVER_LI && nesolver != LIS_ESOLVER_AI && nesolver != LIS_ESOLVER_GSI && nesolver != LIS_ESOLVER_GLI && nesolver != LIS_ESOLVER_GAI)
		return LISI_ERR(LIS_ERR_ILL_ARG, "Parameter LIS_EOPTIONS_ESOLVER is %D (Set Subspace, Lanczos, Arnoldi, Generalized Subspace, Generalized Lanczos, or Generalized Arnoldi)\n", nesolver);
	if (!e->evalue || !e->resid || !e->iter) return LISI_ERR(LIS_ERR_ILL_ARG, "no eigensolve has filled the esolver\n");
	const LIS_INT ss = e->options[LIS_EOPTIONS_SUBSPACE];
	LIS_INT n, gn, is, ie;
	LISCHK(lis_vector_set_size(v, 0, ss));
	LISCHK(lis_vector_get_size(v, &n, &gn));
	LISCHK(lis_vector_get_range(v, &is, &ie));
	for (LIS_INT i = 0; i < n; i++) {
		const LIS_INT ii = i + (v->origin ? 1 : 0);
		LISCHK(lis_vector_set_value(LIS_INS_VALUE, ii + is, what == 0 ? e->evalue[i + is] : what == 1 ? e->resid[i + is] : (LIS_SCALAR)e->iter[i + is], v));
	}
	if (what == 2) v->intvalue = 1;
	return LIS_SUCCESS;
}
LIS_INT lis_esolver_get_evalues(LIS_ESOLVER e, LIS_VECTOR v) { return per_mode(e, v, 0); }
LIS_INT lis_esolver_get_residualnorms(LIS_ESOLVER e, LIS_VECTOR v) { return per_mode(e, v, 1); }
LIS_INT lis_esolver_get_iters(LIS_ESOLVER e, LIS_VECTOR v) { return per_mode(e, v, 2); }
LIS_INT lis_esolver_get_evectors(LIS_ESOLVER e, LIS_MATRIX M) { (void)e; (void)M; return subspace_only("lis_esolver_get_evectors"); }
LIS_INT lis_esolver_get_specific_evalue(LIS_ESOLVER e, LIS_INT mode, LIS_SCALAR *evalue) { (void)e; (void)mode; (void)evalue; return subspace_only("lis_esolver_get_specific_evalue"); }
LIS_INT lis_esolver_get_specific_evector(LIS_ESOLVER e, LIS_INT mode, LIS_VECTOR x) { (void)e; (void)mode; (void)x; return subspace_only("lis_esolver_get_specific_evector"); }
LIS_INT lis_esolver_get_specific_residualnorm(LIS_ESOLVER e, LIS_INT mode, LIS_REAL *residual) { (void)e; (void)mode; (void)residual; return subspace_only("lis_esolver_get_specific_residualnorm"); }
LIS_INT lis_esolver_get_specific_iter(LIS_ESOLVER e, LIS_INT mode, LIS_INT *iter) { (void)e; (void)mode; (void)iter; return subspace_only("lis_esolver_get_specific_iter"); }

/* ------------------------------------------------------------------ what the five loops share */
#define ETRY(expr) do { LIS_INT e__ = (expr); if (e__) { err = e__; goto done; } } while (0)

typedef struct {
	LIS_ESOLVER e;
	LIS_MATRIX A;
	LIS_INT emaxiter, output;
	LIS_REAL tol;
	LIS_SCALAR oshift;
	LIS_SOLVER solver;        /* the inner linear solver and its preconditioner (ii, rqi, cg, cr) */
	LIS_PRECON precon;
	const lisi_precon_kind *pk;   /* cg, cr: lis_psolve(solver, r, w) through the preconditioner's row ... */
	lisi_precon_state ps;         /* ... resolved once, after the precon was created (no shift happens inside those loops) */
} ectx_t;

static void ectx_begin(ectx_t *c, LIS_ESOLVER e, int shifts)
{
	memset(c, 0, sizeof(*c));
	c->e = e; c->A = e->A;
	c->emaxiter = e->options[LIS_EOPTIONS_MAXITER];
	c->tol = e->params[LIS_EPARAMS_RESID - LIS_EOPTIONS_LEN];
	c->output = e->options[LIS_EOPTIONS_OUTPUT];
	c->oshift = e->params[LIS_EPARAMS_SHIFT - LIS_EOPTIONS_LEN];
	if (shifts && e->ishift != 0.0) c->oshift = e->ishift;
}

static void enote(ectx_t *c, LIS_INT iter, LIS_REAL resid)
{	/* the convergence-check block of every loop (lis_esolver_pi.c:197-201); lis_print_rhistory: src/system/lis_error.c:193-203 */
	if (!c->output) return;
	if (c->output & LIS_EPRINT_MEM) c->e->rhistory[iter] = resid;
	if (c->output & LIS_EPRINT_OUT) lis_printf(LIS_COMM_WORLD, "iteration: %5d  relative residual = %E\n", (int)iter, (double)resid);
}

/* lis_solver_create, the reference's option string, the command line's options, the two banner lines (lis_esolver_ii.c:182-194) */
static LIS_INT inner_solver(ectx_t *c, char *options)
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

static void inner_times(ectx_t *c)
{	/* lis_esolver_ii.c:237-241 */
	c->e->ptime += c->solver->ptime; c->e->itime += c->solver->itime;
	c->e->p_c_time += c->solver->p_c_time; c->e->p_i_time += c->solver->p_i_time;
}

static void inner_destroy(ectx_t *c)
{
	if (c->precon) lis_precon_destroy(c->precon);
	if (c->solver) lis_solver_destroy(c->solver);
	c->precon = NULL; c->solver = NULL;
}

/* An inner solve: y = A^-1 b by lis_solve_kernel with the loop's preconditioner, or (whole) by lis_solve.  It always runs in the library's default loop form:
 * lis_solve's own passes do NOT give the same bits fused and unfused in the tree mode (the product's fused dot epilogue sums in another order than
 * liship_dot_f64: `lis_solve -i cg` on the 10 x 10 Laplacian ends with another x under LIS_AMD_NO_FUSION=1), so inside an esolve that switch selects the
 * esolver's own passes only -- the Gram blocks -- and a fused and an unfused esolve agree in every bit (tests/test_esolve_gpu.py) */
static LIS_INT inner_solve(ectx_t *c, LIS_VECTOR b, LIS_VECTOR y, int whole)
{
	const int held = lisg.no_fusion;
	lisg.no_fusion = 0;
	const LIS_INT err = whole ? lis_solve(c->A, b, y, c->solver) : lis_solve_kernel(c->A, b, y, c->solver, c->precon);
	lisg.no_fusion = held;
	return err;
}

/* the preconditioner of cg / cr made ready for lis_psolve calls outside a solve: the row's begin, as lis_solve_kernel runs it */
static LIS_INT psolve_begin(ectx_t *c)
{
	c->pk = lisi_precon_kind_of(c->precon->precon_type);
	if (!c->pk) return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "preconditioner %D is not served by liblis_amd\n", c->precon->precon_type);
	LISCHK(lisd_mat_ready(c->A));
	c->solver->precon = c->precon;
	return c->pk->begin(c->A, c->solver, &c->ps);
}
static LIS_INT psolve(ectx_t *c, LIS_VECTOR r, LIS_VECTOR w)
{	/* w = M^-1 r (lis_psolve) */
	double *dr, *dw;
	LISCHK(lisd_vec_in(r, &dr)); LISCHK(lisd_vec_out(w, &dw));
	LISCHK(c->pk->apply(&c->ps, 0, dr, dw));
	return lisd_vec_done(w);
}

/* a Gram block: out[k] = <v[pairs[k][0]], v[pairs[k][1]]> */
static LIS_INT gram(LIS_INT n, int nvec, LIS_VECTOR *v, int K, const int (*pairs)[2], double *out)
{
	const double *dv[LISHIP_MULTIDOT_MAX_VECS];
	for (int i = 0; i < nvec; i++) { double *p; LISCHK(lisd_vec_in(v[i], &p)); dv[i] = p; }
	return lisd_multidot(n, nvec, dv, K, pairs, out);
}

static LIS_INT normalize(LIS_VECTOR v)
{	/* v = v / ||v||_2 */
	LIS_REAL nrm2;
	LISCHK(lis_vector_nrm2(v, &nrm2));
	return lis_vector_scale(1.0 / nrm2, v);
}

static void eshift_banner(ectx_t *c) { if (c->output) lis_printf(LIS_COMM_WORLD, "shift                 : %e\n", (double)c->oshift); }

/* ------------------------------------------------------------------ power iteration, lis_esolver_pi.c:127-226 */
static LIS_INT lis_epi(LIS_ESOLVER esolver)
{
	ectx_t cx, *c = &cx;
	ectx_begin(c, esolver, 1);
	LIS_MATRIX A = c->A;
	LIS_VECTOR v = esolver->x, y = esolver->work[0], q = esolver->work[1];
	LIS_SCALAR theta = 0.0;
	LIS_REAL nrm2, resid = 0.0;
	LIS_INT err = 0, iter = 0, code = LIS_MAXITER;
	int shifted = 0;
	if (esolver->options[LIS_EOPTIONS_INITGUESS_ONES]) ETRY(lis_vector_set_all(1.0, v));
	if (c->oshift != 0.0) { ETRY(lis_matrix_shift_diagonal(A, c->oshift)); shifted = 1; }
	eshift_banner(c);
	while (iter < c->emaxiter) {
		iter = iter + 1;
		ETRY(lis_vector_nrm2(v, &nrm2));                     /* v = v / ||v||_2 */
		ETRY(lis_vector_scale(1.0 / nrm2, v));
		ETRY(lis_matvec(A, v, y));                           /* y = A * v */
		ETRY(lis_vector_dot(v, y, &theta));                  /* theta = <v,y> */
		ETRY(lis_vector_axpyz(-theta, v, y, q));             /* resid = ||y - theta * v||_2 / |theta| */
		ETRY(lis_vector_nrm2(q, &resid));
		resid = resid / fabs(theta);
		ETRY(lis_vector_copy(y, v));                         /* v = y */
		enote(c, iter, resid);
		if (c->tol >= resid) { code = LIS_SUCCESS; break; }
	}
	esolver->retcode = code;
	esolver->iter[0] = iter;
	esolver->resid[0] = resid;
	esolver->evalue[0] = theta + c->oshift;
	ETRY(normalize(v));
	err = code;
done:
	if (shifted) { const LIS_INT e2 = lis_matrix_shift_diagonal(A, -c->oshift); if (e2 && (!err || err == LIS_MAXITER)) err = e2; }
	return err;
}

/* ------------------------------------------------------------------ inverse iteration, lis_esolver_ii.c:127-277 */
static LIS_INT lis_eii(LIS_ESOLVER esolver)
{
	ectx_t cx, *c = &cx;
	ectx_begin(c, esolver, 1);
	LIS_MATRIX A = c->A;
	LIS_VECTOR v = esolver->x, y = esolver->work[0], q = esolver->work[1];
	LIS_SCALAR theta = 0.0;
	LIS_REAL nrm2, resid = 0.0;
	LIS_INT err = 0, iter = 0, iter2, code = LIS_MAXITER;
	int shifted = 0;
	if (esolver->options[LIS_EOPTIONS_INITGUESS_ONES]) ETRY(lis_vector_set_all(1.0, v));
	if (c->oshift != 0.0) { ETRY(lis_matrix_shift_diagonal(A, c->oshift)); shifted = 1; }
	eshift_banner(c);
	ETRY(inner_solver(c, "-i bicg -p none"));
	c->solver->A = A;
	ETRY(lis_precon_create(c->solver, &c->precon));
	while (iter < c->emaxiter) {
		iter = iter + 1;
		ETRY(lis_vector_nrm2(v, &nrm2));                     /* v = v / ||v||_2 */
		ETRY(lis_vector_scale(1.0 / nrm2, v));
		ETRY(inner_solve(c, v, y, 0));                        /* y = A^-1 * v */
		lis_solver_get_iter(c->solver, &iter2);
		ETRY(lis_vector_dot(v, y, &theta));                  /* theta = <v,y> */
		ETRY(lis_vector_axpyz(-theta, v, y, q));             /* resid = ||y - theta * v||_2 / |theta| */
		ETRY(lis_vector_nrm2(q, &resid));
		resid = resid / fabs(theta);
		ETRY(lis_vector_copy(y, v));                         /* v = y */
		inner_times(c);
		enote(c, iter, resid);
		if (c->tol >= resid) { code = LIS_SUCCESS; break; }
	}
	esolver->retcode = code;
	esolver->iter[0] = iter;
	esolver->resid[0] = resid;
	esolver->evalue[0] = 1.0 / theta + c->oshift;
	ETRY(normalize(v));
	err = code;
done:
	if (shifted) { const LIS_INT e2 = lis_matrix_shift_diagonal(A, -c->oshift); if (e2 && (!err || err == LIS_MAXITER)) err = e2; }
	inner_destroy(c);
	return err;
}

/* ------------------------------------------------------------------ Rayleigh quotient iteration, lis_esolver_rqi.c:129-268 (no -shift: rho is the shift) */
static LIS_INT lis_erqi(LIS_ESOLVER esolver)
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
		ETRY(lis_matrix_shift_diagonal(A, rho));             /* y = (A - rho * I)^-1 * v */
		shifted = 1;
		ETRY(inner_solve(c, v, y, 0));
		ETRY(lis_matrix_shift_diagonal(A, -rho));
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
	if (shifted) (void)lis_matrix_shift_diagonal(A, -rho);  /* an inner solve failed between the two shifts: A goes back */
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

/* ------------------------------------------------------------------ CG, lis_esolver_cg.c:126-367 */
static LIS_INT lis_ecg(LIS_ESOLVER esolver)
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
	int shifted = 0;
	if (esolver->options[LIS_EOPTIONS_INITGUESS_ONES]) ETRY(lis_vector_set_all(1.0, x));
	if (c->oshift != 0.0) { ETRY(lis_matrix_shift_diagonal(A, c->oshift)); shifted = 1; }
	eshift_banner(c);
	ETRY(lis_vector_nrm2(x, &nrm2));
	ETRY(lis_vector_scale(1.0 / nrm2, x));
	ETRY(lis_matvec(A, x, Ax));
	ETRY(inner_solver(c, "-i cg -p none"));
	ETRY(inner_solve(c, x, p, 1));                           /* p = A^-1 * x */
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
	esolver->iter[0] = iter;
	esolver->resid[0] = resid;
	esolver->evalue[0] = lambda + c->oshift;
	esolver->ptime = ptime;
	esolver->itime = c->solver->itime; esolver->p_c_time = c->solver->p_c_time; esolver->p_i_time = c->solver->p_i_time;
done:
	if (c->solver) c->solver->precon = NULL;
	inner_destroy(c);
	if (shifted) { const LIS_INT e2 = lis_matrix_shift_diagonal(A, -c->oshift); if (e2 && !err) err = e2; }
	if (err) return err;
	esolver->retcode = (resid < c->tol) ? LIS_SUCCESS : LIS_MAXITER;
	return esolver->retcode;
}

/* ------------------------------------------------------------------ CR, lis_esolver_cg.c:780-979 */
static LIS_INT lis_ecr(LIS_ESOLVER esolver)
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
	int shifted = 0;
	if (esolver->options[LIS_EOPTIONS_INITGUESS_ONES]) ETRY(lis_vector_set_all(1.0, x));
	if (c->oshift != 0.0) { ETRY(lis_matrix_shift_diagonal(A, c->oshift)); shifted = 1; }
	eshift_banner(c);
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
	esolver->iter[0] = iter;
	esolver->resid[0] = resid;
	esolver->evalue[0] = lambda + c->oshift;
	ETRY(normalize(x));
	esolver->ptime = ptime;
	esolver->itime = c->solver->itime; esolver->p_c_time = c->solver->p_c_time; esolver->p_i_time = c->solver->p_i_time;
done:
	if (c->solver) c->solver->precon = NULL;
	inner_destroy(c);
	if (shifted) { const LIS_INT e2 = lis_matrix_shift_diagonal(A, -c->oshift); if (e2 && !err) err = e2; }
	if (err) return err;
	esolver->retcode = (resid < c->tol) ? LIS_SUCCESS : LIS_MAXITER;
	return esolver->retcode;
}

/* ------------------------------------------------------------------ lis_esolve / lis_gesolve, ref :263-666 */
static LIS_INT work_alloc(LIS_ESOLVER e, LIS_INT count)
{	/* lis_e<xx>_malloc_work: NWORK duplicates of A's row layout */
	work_destroy(e);
	e->work = (LIS_VECTOR *)calloc((size_t)count, sizeof(LIS_VECTOR));
	if (!e->work) return LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "malloc size = %D\n", (LIS_INT)(count * sizeof(LIS_VECTOR)));
	for (LIS_INT i = 0; i < count; i++) {
		const LIS_INT err = lis_vector_duplicate(e->A, &e->work[i]);
		if (err) { for (LIS_INT j = 0; j < i; j++) lis_vector_destroy(e->work[j]); free(e->work); e->work = NULL; return err; }
	}
	e->worklen = count;
	return LIS_SUCCESS;
}

LIS_INT lis_gesolve(LIS_MATRIX A, LIS_MATRIX B, LIS_VECTOR x, LIS_SCALAR *evalue0, LIS_ESOLVER esolver)
{
	LIS_VECTOR xx = NULL;
	LIS_INT err;
	/* parameter check, ref :310-435 */
	LISCHK(lisi_matrix_check(A, LISI_CHECK_ASSEMBLED));
	if (x == NULL) return LISI_ERR(LIS_ERR_ILL_ARG, "vector x is undefined\n");
	if (A->n != x->n) return LIS_ERR_ILL_ARG;
	if (A->gn <= 0) return LISI_ERR(LIS_ERR_ILL_ARG, "Size n(=%D) of matrix A is less than 0\n", A->gn);
	const LIS_INT nesolver = esolver->options[LIS_EOPTIONS_ESOLVER], ss = esolver->options[LIS_EOPTIONS_SUBSPACE], mode = esolver->options[LIS_EOPTIONS_MODE];
	const LIS_INT emaxiter = esolver->options[LIS_EOPTIONS_MAXITER], output = esolver->options[LIS_EOPTIONS_OUTPUT];
	const LIS_INT estorage = esolver->options[LIS_EOPTIONS_STORAGE], eblock = esolver->options[LIS_EOPTIONS_STORAGE_BLOCK];
	const LIS_INT eprecision = esolver->options[LIS_EOPTIONS_PRECISION];
	if (nesolver < 1 || nesolver > LIS_ESOLVER_LEN) return LISI_ERR(LIS_ERR_ILL_ARG, "Parameter LIS_EOPTIONS_ESOLVER is %D (Set between 1 to %D)\n", nesolver, LIS_ESOLVER_LEN);
	/* what is not served, said before A or x is touched */
	if (B != NULL) { esolver->retcode = LIS_ERR_NOT_IMPLEMENTED; return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "generalized eigenproblems (lis_gesolve with a matrix B) are not served by liblis_amd\n"); }
	if (nesolver > LIS_ESOLVER_CR) {
		esolver->retcode = LIS_ERR_NOT_IMPLEMENTED;
		return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "eigensolver %s (-e %s) is not served by liblis_amd (pi, ii, rqi, cg, cr)\n", esolver_names[nesolver], esolver_keys[nesolver - 1]);
	}
	if (lisg.nprocs > 1 || A->nprocs > 1) { esolver->retcode = LIS_ERR_NOT_IMPLEMENTED; return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "lis_esolve is served on one rank (this job has %D)\n", (LIS_INT)lisg.nprocs); }
	if (eprecision != LIS_PRECISION_DOUBLE) { esolver->retcode = LIS_ERR_ILL_ARG; return LISI_ERR(LIS_ERR_ILL_ARG, "Quad precision is not enabled\n"); }
	if (estorage > 0 && estorage != A->matrix_type && !lisi_format_served(estorage)) {
		esolver->retcode = LIS_ERR_NOT_IMPLEMENTED;
		return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-estorage %D: storage format is not served by liblis_amd\n", estorage);
	}
	if (emaxiter < 0) { esolver->retcode = LIS_ERR_ILL_ARG; return LISI_ERR(LIS_ERR_ILL_ARG, "Parameter LIS_EOPTIONS_MAXITER(=%D) is less than 0\n", emaxiter); }
	if (ss < 1 || mode < 0 || mode > ss + 1) { esolver->retcode = LIS_ERR_ILL_ARG; return LISI_ERR(LIS_ERR_ILL_ARG, "Parameters LIS_EOPTIONS_SUBSPACE(=%D), LIS_EOPTIONS_MODE(=%D) are out of range\n", ss, mode); }
	if (MDEV(A)->device_only && A->matrix_type != LIS_MATRIX_CSR) { esolver->retcode = LIS_ERR_NOT_IMPLEMENTED; return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "a matrix that lives in HBM only is shifted in CSR storage\n"); }
	esolver->eprecision = eprecision;

	/* the arrays of the object (ss + 2 entries each, ref :438-550), zeroed */
	free(esolver->evalue); free(esolver->resid); free(esolver->iter); free(esolver->iter2); free(esolver->evector); free(esolver->rhistory);
	esolver->evalue = (LIS_SCALAR *)calloc((size_t)ss + 2, sizeof(LIS_SCALAR));
	esolver->resid = (LIS_REAL *)calloc((size_t)ss + 2, sizeof(LIS_REAL));
	esolver->iter = (LIS_INT *)calloc((size_t)ss + 2, sizeof(LIS_SCALAR));
	esolver->iter2 = (LIS_INT *)calloc((size_t)ss + 2, sizeof(LIS_SCALAR));
	esolver->evector = (LIS_VECTOR *)calloc((size_t)ss + 2, sizeof(LIS_VECTOR));
	esolver->rhistory = (LIS_REAL *)calloc((size_t)emaxiter + 2, sizeof(LIS_REAL));
	if (!esolver->evalue || !esolver->resid || !esolver->iter || !esolver->iter2 || !esolver->evector || !esolver->rhistory) {
		esolver->retcode = LIS_ERR_OUT_OF_MEMORY;
		return LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "malloc size = %D\n", (LIS_INT)((emaxiter + 2) * sizeof(LIS_REAL)));
	}
	esolver->evalue[0] = 1.0;
	esolver->evalue[ss - 1] = 1.0;
	esolver->rhistory[0] = 1.0;

	/* the initial vector, ref :481-529 */
	if ((err = lis_vector_duplicate(A, &xx))) { esolver->retcode = err; return err; }
	if (esolver->options[LIS_EOPTIONS_INITGUESS_ONES]) {
		if (output) lis_printf(LIS_COMM_WORLD, "initial vector x      : all components set to 1\n");
		err = lis_vector_set_all(1.0, xx);
	} else {
		if (output) lis_printf(LIS_COMM_WORLD, "initial vector x      : user defined\n");
		err = lis_vector_copy(x, xx);
	}
	if (err) goto fail;
	/* -estorage: the caller's matrix itself is converted and stays converted, ref :553-570 (as -storage in lis_solve) */
	if (estorage > 0 && A->matrix_type != estorage && (err = lisi_matrix_retype(A, estorage, estorage == LIS_MATRIX_BSR ? eblock : 0))) goto fail;

	esolver->A = A; esolver->B = NULL;
	if (output) {
		lis_printf(LIS_COMM_WORLD, "precision             : %s\n", eprecision_keys[eprecision]);
		lis_printf(LIS_COMM_WORLD, "eigensolver           : %s\n", esolver_names[nesolver]);
		lis_printf(LIS_COMM_WORLD, "convergence condition : ||lx-(B^-1)Ax||_2 <= %6.1e * ||lx||_2\n", (double)esolver->params[LIS_EPARAMS_RESID - LIS_EOPTIONS_LEN]);
		if (A->matrix_type == LIS_MATRIX_BSR) lis_printf(LIS_COMM_WORLD, "matrix storage format : %s(%D x %D)\n", estorage_names[A->matrix_type - 1], eblock, eblock);
		else lis_printf(LIS_COMM_WORLD, "matrix storage format : %s\n", estorage_names[A->matrix_type - 1]);
	}
	double time = lis_wtime();
	esolver->ptime = 0; esolver->itime = 0; esolver->p_c_time = 0; esolver->p_i_time = 0;
	if ((err = work_alloc(esolver, nesolver == LIS_ESOLVER_CG || nesolver == LIS_ESOLVER_CR ? 6 : 2))) goto fail;
	esolver->x = xx; esolver->xx = x;

	switch (nesolver) {
	case LIS_ESOLVER_PI:  err = lis_epi(esolver); break;
	case LIS_ESOLVER_II:  err = lis_eii(esolver); break;
	case LIS_ESOLVER_RQI: err = lis_erqi(esolver); break;
	case LIS_ESOLVER_CG:  err = lis_ecg(esolver); break;
	default:              err = lis_ecr(esolver); break;
	}
	esolver->retcode = err;
	esolver->x = x;
	if (err && err != LIS_MAXITER) goto fail;                /* an inner solve or a device call failed: nothing to hand back */
	*evalue0 = esolver->evalue[0];
	if ((err = lis_vector_copy(xx, x))) goto fail;
	{
		const int rc = liship_stream_synchronize(lisg.stream);
		if (rc != 0) { err = lisi_hip_error(__FILE__, __func__, __LINE__, rc); goto fail; }
	}
	esolver->time = lis_wtime() - time;
	if (output) {
		if (esolver->retcode) lis_printf(LIS_COMM_WORLD, "eigensolver status    : %s(code=%D)\n\n", ereturncode_names[esolver->retcode], esolver->retcode);
		else lis_printf(LIS_COMM_WORLD, "eigensolver status    : normal end\n\n");
	}
	esolver->iter2[mode] = esolver->iter[mode];
	lis_vector_destroy(xx);
	return LIS_SUCCESS;
fail:
	esolver->retcode = err;
	esolver->x = x;
	lis_vector_destroy(xx);
	return err;
}

LIS_INT lis_esolve(LIS_MATRIX A, LIS_VECTOR x, LIS_SCALAR *evalue0, LIS_ESOLVER esolver)
{
	const LIS_INT err = lis_gesolve(A, NULL, x, evalue0, esolver);
	if (err) { esolver->retcode = err; return err; }
	return LIS_SUCCESS;
}
