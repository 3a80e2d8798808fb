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
 * Served as well: several eigenpairs per solve -- subspace (-e si, -ie pi | ii), Lanczos (-e li) and Arnoldi (-e ai) iteration with -ss >= 2 (lis_esolver_si.c,
 * _li.c, _ai.c), the getters only they fill, and the small dense QR they call (lis_array.c).  Their device chains and the fused tail of a subspace iteration
 * (liship_ritz_tail_f64) stand in the section "several eigenpairs per solve" below.
 *
 * Served as well: the generalized problem A x = lambda B x through lis_gesolve with a matrix B and -e gpi | gii | grqi | gcr (lis_esolver_pi.c:305-464,
 * _ii.c:357-520, _rqi.c:350-501, _cg.c:1063-1265), in the section "the generalized problem" below.  Their shift is lis_matrix_shift_matrix (lis_shift.c,
 * kernels/spgeam.hip): A - sigma B merged row by row in HBM where the reference goes through two dense n x n copies.
 *
 * Served as well: several pairs of the generalized problem -- -e gsi (-ige gpi | gii), -e gli and -e gai (-ige gpi | gii | grqi | gcr) with -ss >= 2
 * (lis_esolver_si.c:456-719, _li.c:456-694, _ai.c:491-750), in the section "several pairs of the generalized problem" below, with the two pair passes
 * liship_scale2_inv_sqrt_f64 and liship_scale2_to_f64 (kernels/vector_ops.hip).  Lanczos and Arnoldi refine each mode through lis_gesolve with -ige's solver.
 *
 * Refused, with LIS_ERR_NOT_IMPLEMENTED and before A, B or x is touched: -e si | li | ai | gsi | gli | gai with -ss 1 (the default: one pair is what -e pi / -e ii
 * and -e gpi / -e gii serve), -e si with an -ie other than pi or ii, -e gsi with an -ige other than gpi or gii (the reference's loop then applies neither matrix),
 * -e gli | gai with -ige gcg or a standard solver, a B together with a standard -e (the reference silently ignores B there), a generalized -e through lis_esolve
 * or with B = NULL (the reference's loops multiply by that NULL), -e gcg (the reference's loop never updates x and ends in NaN: -e gcr is the one that works), a
 * job of several ranks.
 * -ef quad | switch answers as lis_solve does for -f quad.
 *
 * Deliberate differences from the reference, all outside a converging solve: the arrays of the object start zeroed instead of holding heap contents; a
 * negative -emaxiter is refused; an inner solve that fails hands its code back as the return value (the reference returns LIS_SUCCESS and leaves A shifted
 * in -e rqi); work vectors of an earlier solve are released instead of leaked.
 */
#include <stdio.h>
#include <ctype.h>
#include <stdint.h>
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

static int is_multi(LIS_INT nesolver) { return nesolver == LIS_ESOLVER_SI || nesolver == LIS_ESOLVER_LI || nesolver == LIS_ESOLVER_AI; }
static int is_generalized(LIS_INT nesolver) { return nesolver >= LIS_ESOLVER_GPI && nesolver <= LIS_ESOLVER_GAI; }
static int is_gmulti(LIS_INT nesolver) { return nesolver == LIS_ESOLVER_GSI || nesolver == LIS_ESOLVER_GLI || nesolver == LIS_ESOLVER_GAI; }
static int is_multi_or_generalized(LIS_INT nesolver) { return is_multi(nesolver) || is_gmulti(nesolver); }

/* the arrays of the object and the eigenvectors an earlier solve left: evector has two slots more than vectors and is filled from slot 0, so the first NULL ends them */
static void arrays_free(LIS_ESOLVER e)
{
	if (e->evector) for (LIS_INT i = 0; e->evector[i]; i++) lis_vector_destroy(e->evector[i]);
	free(e->rhistory); free(e->evalue); free(e->resid); free(e->iter); free(e->iter2); free(e->evector);
	e->rhistory = NULL; e->evalue = NULL; e->resid = NULL; e->iter = NULL; e->iter2 = NULL; e->evector = NULL;
}

LIS_INT lis_esolver_destroy(LIS_ESOLVER e)
{	/* ref :231-259 */
	if (e) {
		work_destroy(e);
		arrays_free(e);
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

/* what the subspace, Lanczos and Arnoldi solvers fill (ref :1153-1355).  On an esolver whose -e names none of them (nor a generalized form) the three that fill
 * a vector answer LIS_ERR_ILL_ARG as the reference does (:1159-1163) and the others say that they belong to those solvers; on one that names such a solver but
 * holds no ended solve -- never run, refused, failed -- every getter answers LIS_ERR_ILL_ARG */
static LIS_INT subspace_only(const char *what)
{
	return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "%s is filled by the subspace, Lanczos and Arnoldi eigensolvers only (-e si | li | ai | gsi | gli | gai)\n", what);
}
static LIS_INT multi_filled(LIS_ESOLVER e, const char *what, LIS_INT mode, int vectors)
{
	const LIS_INT nesolver = e->options[LIS_EOPTIONS_ESOLVER], ss = e->options[LIS_EOPTIONS_SUBSPACE];
	if (!is_multi_or_generalized(nesolver)) return subspace_only(what);
	if (!e->evalue || !e->resid || !e->iter || !e->evector) return LISI_ERR(LIS_ERR_ILL_ARG, "%s: no eigensolve has filled the esolver\n", what);
	if (mode < 0 || mode >= ss) return LISI_ERR(LIS_ERR_ILL_ARG, "%s: mode %D is outside the subspace of %D\n", what, mode, ss);
	if (vectors) for (LIS_INT i = 0; i <= mode; i++) if (!e->evector[i]) return LISI_ERR(LIS_ERR_ILL_ARG, "%s: the solve left no eigenvector %D (-rval true computes Ritz values only)\n", what, i);
	return LIS_SUCCESS;
}
/* the three that copy the object's arrays of ss entries into a vector (ref :1153-1179, :1261-1287, :1309-1337) */
static LIS_INT per_mode(LIS_ESOLVER e, LIS_VECTOR v, int what)
{
	const LIS_INT nesolver = e->options[LIS_EOPTIONS_ESOLVER];
	if (!is_multi_or_generalized(nesolver))
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
LIS_INT lis_esolver_get_specific_evalue(LIS_ESOLVER e, LIS_INT mode, LIS_SCALAR *evalue)
{ LISCHK(multi_filled(e, "lis_esolver_get_specific_evalue", mode, 0)); *evalue = e->evalue[mode]; return LIS_SUCCESS; }
LIS_INT lis_esolver_get_specific_residualnorm(LIS_ESOLVER e, LIS_INT mode, LIS_REAL *residual)
{ LISCHK(multi_filled(e, "lis_esolver_get_specific_residualnorm", mode, 0)); *residual = e->resid[mode]; return LIS_SUCCESS; }
LIS_INT lis_esolver_get_specific_iter(LIS_ESOLVER e, LIS_INT mode, LIS_INT *iter)
{ LISCHK(multi_filled(e, "lis_esolver_get_specific_iter", mode, 0)); *iter = e->iter[mode]; return LIS_SUCCESS; }
LIS_INT lis_esolver_get_specific_evector(LIS_ESOLVER e, LIS_INT mode, LIS_VECTOR x)
{ LISCHK(multi_filled(e, "lis_esolver_get_specific_evector", mode, 1)); return lis_vector_copy(e->evector[mode], x); }

/* ref :1201-1239: M sized gn x gn, column j = eigenvector j, every entry set (zeros included), then type and assemble.  The reference makes M a COO matrix;
 * COO is not a storage liblis_amd serves, so M is assembled as CSR -- the same entries in the same order, row by row.  Each vector comes home from HBM once */
LIS_INT lis_esolver_get_evectors(LIS_ESOLVER e, LIS_MATRIX M)
{
	const LIS_INT ss = e->options[LIS_EOPTIONS_SUBSPACE];
	LISCHK(multi_filled(e, "lis_esolver_get_evectors", ss - 1, 1));
	LIS_INT n, gn, is, ie, js = 0, err = LIS_SUCCESS;
	LISCHK(lis_matrix_set_size(M, 0, e->evector[0]->gn));
	LISCHK(lis_matrix_get_size(M, &n, &gn));
	LISCHK(lis_matrix_get_range(M, &is, &ie));
	if (e->evector[0]->origin) { is++; js++; }
	LIS_SCALAR *col = (LIS_SCALAR *)malloc((size_t)(n > 0 ? n : 1) * sizeof(LIS_SCALAR));
	if (!col) return LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "malloc size = %D\n", (LIS_INT)(n * sizeof(LIS_SCALAR)));
	for (LIS_INT j = 0; j < ss && !err; j++) {
		err = lis_vector_gather(e->evector[j], col);
		for (LIS_INT i = 0; i < n && !err; i++) err = lis_matrix_set_value(LIS_INS_VALUE, i + is, j + js, col[i], M);
	}
	free(col);
	if (err) return err;
	LISCHK(lis_matrix_set_type(M, LIS_MATRIX_CSR));
	return lis_matrix_assemble(M);
}

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
static LIS_INT inner_solve_on(ectx_t *c, LIS_MATRIX M, LIS_VECTOR b, LIS_VECTOR y, int whole)
{
	const int held = lisg.no_fusion;
	lisg.no_fusion = 0;
	const LIS_INT err = whole ? lis_solve(M, b, y, c->solver) : lis_solve_kernel(M, b, y, c->solver, c->precon);
	lisg.no_fusion = held;
	return err;
}
static LIS_INT inner_solve(ectx_t *c, LIS_VECTOR b, LIS_VECTOR y, int whole) { return inner_solve_on(c, c->A, b, y, whole); }

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

/* ================================================================== several eigenpairs per solve: subspace, Lanczos, Arnoldi
 * The orthogonalisation pairs of -e si and the Hessenberg columns of -e ai are taken as a chain whose coefficients stay in HBM (hdev): liship_dot_f64 forms
 * the first, liship_mgs_step_f64 applies one and forms the next, and nothing waits for the host in between.  The tail of a subspace iteration is two passes
 * (liship_multidot_f64, liship_ritz_tail_f64) and one read-back.  LIS_AMD_NO_FUSION=1 / LIS_AMD_LOOP_UNFUSED brings the lis_vector_* calls of the reference's
 * text back: the same bits, in the tree mode and in the reference-order mode (tests/test_esolve_multi_gpu.py). */
#define EHIP(call) do { int rc__ = (call); if (rc__) { err = lisi_hip_error(__FILE__, __func__, __LINE__, rc__); goto done; } } while (0)

static int chain_ready(LIS_INT n, LIS_VECTOR a, LIS_VECTOR b)
{	/* liship_ritz_tail_f64 takes 16 B aligned arrays (every vector the library allocates is) */
	double *pa, *pb;
	if (lisg.no_fusion || n <= 0) return 0;
	if (lisd_vec_in(a, &pa) || lisd_vec_in(b, &pb)) return 0;
	return (((uintptr_t)pa | (uintptr_t)pb) & 15u) == 0;
}

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

/* ------------------------------------------------------------------ subspace iteration, lis_esolver_si.c:137-370 */
static LIS_INT lis_esi(LIS_ESOLVER esolver)
{
	ectx_t cx, *c = &cx;
	ectx_begin(c, esolver, 1);
	LIS_MATRIX A = c->A;
	const LIS_INT ss = esolver->options[LIS_EOPTIONS_SUBSPACE], niesolver = esolver->options[LIS_EOPTIONS_INNER_ESOLVER], n = A->n;
	LIS_VECTOR r = esolver->work[0], q = esolver->work[1], *v = &esolver->work[2];
	LIS_SCALAR theta = 0.0;
	LIS_REAL nrm2, resid = 0.0;
	LIS_INT err = 0, iter, j;
	double etime0, etime, *hdev = NULL, **dv = NULL;         /* the chain's coefficients (HBM) and its basis as device pointers */
	char esolvername[128];
	int shifted = 0;
	ETRY(lis_vector_set_all(1.0, r));
	ETRY(lis_vector_nrm2(r, &nrm2));
	ETRY(lis_vector_scale(1.0 / nrm2, r));
	if (c->oshift != 0.0) { ETRY(lis_matrix_shift_diagonal(A, c->oshift)); shifted = 1; }
	eshift_banner(c);
	lis_esolver_get_esolvername(niesolver, esolvername);
	if (c->output) lis_printf(LIS_COMM_WORLD, "inner eigensolver     : %s\n", esolvername);
	if (niesolver == LIS_ESOLVER_II) ETRY(inner_solver(c, "-i bicg -p none"));
	if (c->output) {
		lis_printf(LIS_COMM_WORLD, "size of subspace      : %D\n\n", ss);
		lis_printf(LIS_COMM_WORLD, "compute eigenpairs in subspace:\n\n");
	}
	if (!lisg.no_fusion) EHIP(lisd_malloc((void **)&hdev, sizeof(double) * (size_t)(ss + 2)));
	if (!(dv = (double **)malloc(sizeof(double *) * (size_t)(ss + 1)))) { err = LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "malloc size = %D\n", ss + 1); goto done; }
	j = 0;
	while (j < ss) {
		etime0 = lis_wtime();
		ETRY(lis_vector_duplicate(A, &esolver->evector[j]));
		j = j + 1;
		ETRY(lis_vector_copy(r, v[j]));
		if (niesolver == LIS_ESOLVER_II) {                   /* a preconditioner per mode, as there; the earlier one is freed (the reference leaks it) */
			if (c->precon) { lis_precon_destroy(c->precon); c->precon = NULL; }
			c->solver->A = A;
			ETRY(lis_precon_create(c->solver, &c->precon));
		}
		const int fused = chain_ready(n, r, v[j]);
		iter = 0;
		while (iter < c->emaxiter) {
			iter = iter + 1;
			/* QR factorization V*R = Z for starting vector Z */
			ETRY(orthogonalise(n, j, v, fused, hdev, dv));
			/* kernel: R = A * V or R = A^-1 * V */
			if (niesolver == LIS_ESOLVER_PI) ETRY(lis_matvec(A, v[j], r));
			else ETRY(inner_solve(c, v[j], r, 0));
			if (j == 1 && niesolver == LIS_ESOLVER_II) inner_times(c);
			/* Z = V*R; resid = ||Z - V*R||_2 / |theta|; r = r / ||r||_2; v(j) = r */
			if (fused) {
				static const int pairs[2][2] = {{0, 0}, {1, 0}};
				double *dr, *dvj, sums[3];
				ETRY(lisd_vec_in(r, &dr)); ETRY(lisd_vec_in(v[j], &dvj));
				const double *dv[2] = {dr, dvj};
				EHIP(liship_multidot_f64(n, 2, dv, 2, pairs, lisg.reduce_out, lisg.reduce_work, lisg.stream));
				EHIP(liship_ritz_tail_f64(n, lisg.reduce_out, dr, dvj, lisg.reduce_out + 2, lisg.reduce_work, lisg.stream));
				ETRY(lisd_vec_done(r)); ETRY(lisd_vec_done(v[j]));
				ETRY(lisd_fetch(3, sums));                       /* the one read-back of the iteration */
				nrm2 = sqrt(sums[0]); theta = sums[1]; resid = sqrt(sums[2]);
				resid = resid / fabs(theta);
			} else {
				ETRY(lis_vector_nrm2(r, &nrm2));
				ETRY(lis_vector_dot(v[j], r, &theta));
				ETRY(lis_vector_axpyz(-theta, v[j], r, q));
				ETRY(lis_vector_nrm2(q, &resid));
				resid = resid / fabs(theta);
				ETRY(lis_vector_scale(1.0 / nrm2, r));
				ETRY(lis_vector_copy(r, v[j]));
			}
			/* convergence check: the history and iter[0] are mode 0's */
			if (j == 1) {
				if (c->output & LIS_EPRINT_MEM) esolver->rhistory[iter] = resid;
				esolver->iter[j - 1] = iter;
			}
			if (c->output & LIS_EPRINT_OUT) lis_printf(LIS_COMM_WORLD, "iteration: %5d  relative residual = %E\n", (int)iter, (double)resid);
			if (c->tol > resid) break;
		}
		esolver->evalue[j - 1] = (niesolver == LIS_ESOLVER_PI) ? theta + c->oshift : 1 / theta + c->oshift;
		esolver->resid[j - 1] = resid;
		esolver->iter[j - 1] = iter;
		ETRY(lis_vector_copy(v[j], esolver->evector[j - 1]));
		etime = lis_wtime() - etime0;
		if (c->output & (ss > 1)) {                           /* (as written there: the MEM bit of -eprint) */
			lis_printf(LIS_COMM_WORLD, "Subspace: mode number          = %D\n", j - 1);
			lis_printf(LIS_COMM_WORLD, "Subspace: eigenvalue           = %e\n", (double)esolver->evalue[j - 1]);
			lis_printf(LIS_COMM_WORLD, "Subspace: elapsed time         = %e sec.\n", etime);
			lis_printf(LIS_COMM_WORLD, "Subspace: number of iterations = %D\n", iter);
			lis_printf(LIS_COMM_WORLD, "Subspace: relative residual    = %e\n\n", (double)resid);
		}
	}
done:
	if (hdev) (void)liship_free(hdev);
	free(dv);
	if (shifted) { const LIS_INT e2 = lis_matrix_shift_diagonal(A, -c->oshift); if (e2 && !err) err = e2; }
	inner_destroy(c);
	if (!err) err = lis_vector_copy(esolver->evector[0], esolver->x);
	return err;                                              /* LIS_SUCCESS also when a mode stopped at -emaxiter, as there */
}

/* ------------------------------------------------------------------ what Lanczos and Arnoldi share */
static LIS_INT multi_banner(ectx_t *c, LIS_INT niesolver)
{	/* lis_esolver_li.c:192-206: the reference creates a linear solver for these three lines only */
	char esolvername[128];
	lis_esolver_get_esolvername(niesolver, esolvername);
	if (c->output) lis_printf(LIS_COMM_WORLD, "inner eigensolver     : %s\n", esolvername);
	const LIS_INT err = inner_solver(c, "-i bicg -p none");
	inner_destroy(c);
	return err;
}

/* the refinements after the Ritz values (lis_esolver_li.c:285-346, :627-683, lis_esolver_ai.c:322-381, :684-739): per mode a fresh eigensolver of one pair --
 * -ie's solver, or -ige's under a B, with the outer -emaxiter, -etol and -eprint, shifted by the Ritz value -- run by lis_gesolve on evector[i]; mode 0's
 * history, times, count and residual go into the outer object.  Whatever the inner eigensolver returned, the answer is LIS_SUCCESS, as there.  Under a B each
 * refinement shifts A by its Ritz value and back (lis_matrix_shift_matrix), so A's arrays carry that drift afterwards, as the reference's do. */
static LIS_INT refine_modes(ectx_t *c, const char *name)
{
	LIS_ESOLVER esolver = c->e, esolver2;
	LIS_MATRIX B = esolver->B;                               /* the generalized forms refine through lis_gesolve(A, B, ...) with -ige's solver */
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
			if (c->output) {
				lis_printf(LIS_COMM_WORLD, "%s: mode number          = %D\n", name, i);
				lis_printf(LIS_COMM_WORLD, "%s: eigenvalue           = %e\n", name, (double)esolver->evalue[i]);
				lis_printf(LIS_COMM_WORLD, "%s: elapsed time         = %e sec.\n", name, esolver2->time);
				lis_printf(LIS_COMM_WORLD, "%s: number of iterations = %D\n", name, esolver2->iter[0]);
				lis_printf(LIS_COMM_WORLD, "%s: relative residual    = %e\n\n", name, (double)esolver2->resid[0]);
			}
		}
		lis_esolver_destroy(esolver2);
	}
	return lis_vector_copy(esolver->evector[0], esolver->x);
}

/* ------------------------------------------------------------------ Lanczos, lis_esolver_li.c:149-356 */
static LIS_INT lis_eli(LIS_ESOLVER esolver)
{
	ectx_t cx, *c = &cx;
	ectx_begin(c, esolver, 0);
	LIS_MATRIX A = c->A;
	const LIS_INT ss = esolver->options[LIS_EOPTIONS_SUBSPACE], niesolver = esolver->options[LIS_EOPTIONS_INNER_ESOLVER];
	LIS_VECTOR r = esolver->work[0], *v = &esolver->work[1];
	LIS_SCALAR dot, *t = NULL, *tq = NULL, *tr = NULL;
	LIS_REAL nrm2, qrerr;
	LIS_INT err = 0, i, j, k, qriter;
	double time, time0;
	t = (LIS_SCALAR *)calloc((size_t)ss * ss, sizeof(LIS_SCALAR));
	tq = (LIS_SCALAR *)malloc((size_t)ss * ss * sizeof(LIS_SCALAR));
	tr = (LIS_SCALAR *)malloc((size_t)ss * ss * sizeof(LIS_SCALAR));
	if (!t || !tq || !tr) { err = LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "malloc size = %D\n", (LIS_INT)(ss * ss * sizeof(LIS_SCALAR))); goto done; }
	ETRY(lis_vector_set_all(0.0, v[0]));
	ETRY(lis_vector_set_all(1.0, r));
	ETRY(lis_vector_nrm2(r, &nrm2));
	ETRY(multi_banner(c, niesolver));
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
	/* eigenvalues of the symmetric tridiagonal matrix */
	time0 = lis_wtime();
	ETRY(lis_array_qr(ss, t, tq, tr, &qriter, &qrerr));
	time = lis_wtime() - time0;
	for (i = 0; i < ss; i++) esolver->evalue[i] = t[i * ss + i];
	if (c->output) {
		lis_printf(LIS_COMM_WORLD, "size of subspace      : %D\n\n", ss);
		lis_printf(LIS_COMM_WORLD, "Ritz values:\n\n");
		for (i = 0; i < ss; i++) {
			lis_printf(LIS_COMM_WORLD, "Lanczos: mode number          = %D\n", i);
			lis_printf(LIS_COMM_WORLD, "Lanczos: Ritz value           = %e\n", (double)esolver->evalue[i]);
		}
		lis_printf(LIS_COMM_WORLD, "Lanczos: elapsed time         = %e sec.\n\n", time);
	}
	if (!esolver->options[LIS_EOPTIONS_RVAL]) err = refine_modes(c, "Lanczos");     /* -rval true: iter[] and resid[] stay 0 (heap contents there) */
done:
	free(t); free(tq); free(tr);
	return err;
}

/* ------------------------------------------------------------------ Arnoldi, lis_esolver_ai.c:151-391 */
static LIS_INT lis_eai(LIS_ESOLVER esolver)
{
	ectx_t cx, *c = &cx;
	ectx_begin(c, esolver, 0);
	LIS_MATRIX A = c->A;
	const LIS_INT ss = esolver->options[LIS_EOPTIONS_SUBSPACE], niesolver = esolver->options[LIS_EOPTIONS_INNER_ESOLVER], n = A->n;
	LIS_VECTOR w = esolver->work[0], *v = &esolver->work[1];
	LIS_SCALAR *h = NULL, *hq = NULL, *hr = NULL;
	LIS_REAL nrm2, hqrerr, D;
	LIS_INT err = 0, i, j, hqriter;
	double time, time0, *hdev = NULL, **dv = NULL;
	const int fused = !lisg.no_fusion && ss + 1 <= 256;                     /* (a column comes home through the page-locked landing zone) */
	h = (LIS_SCALAR *)calloc((size_t)ss * ss + 1, sizeof(LIS_SCALAR));      /* (one more than there: h(ss, ss-1), which the last column's norm is written to) */
	hq = (LIS_SCALAR *)malloc((size_t)ss * ss * sizeof(LIS_SCALAR));
	hr = (LIS_SCALAR *)malloc((size_t)ss * ss * sizeof(LIS_SCALAR));
	if (!h || !hq || !hr) { err = LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "malloc size = %D\n", (LIS_INT)(ss * ss * sizeof(LIS_SCALAR))); goto done; }
	ETRY(lis_vector_set_all(1.0, v[0]));
	ETRY(lis_vector_nrm2(v[0], &nrm2));
	ETRY(lis_vector_scale(1.0 / nrm2, v[0]));
	ETRY(multi_banner(c, niesolver));
	if (fused) EHIP(lisd_malloc((void **)&hdev, sizeof(double) * (size_t)(ss + 2)));
	if (!(dv = (double **)malloc(sizeof(double *) * (size_t)(ss + 1)))) { err = LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "malloc size = %D\n", ss + 1); goto done; }
	j = -1;
	while (j < ss - 1) {
		j = j + 1;
		ETRY(lis_matvec(A, v[j], w));                                        /* w = A * v(j) */
		if (fused) {
			/* h(i,j) = <v(i), w>; w = w - h(i,j) * v(i), i = 0 .. j, then ||w||^2: one chain, one read-back per column */
			double *dw;
			ETRY(lisd_vec_in(w, &dw));
			for (i = 0; i <= j; i++) ETRY(lisd_vec_in(v[i], &dv[i]));
			EHIP(liship_dot_f64(n, dv[0], dw, hdev, lisg.reduce_work, lisg.stream));
			ETRY(lisd_mgs_chain(n, j + 1, dv, dw, hdev));
			EHIP(liship_mgs_step_f64(n, hdev + j, dv[j], dw, NULL, hdev + j + 1, lisg.reduce_work, lisg.stream));
			ETRY(lisd_vec_done(w));
			ETRY(lisd_fetch_from(hdev, j + 2, h + j * ss));                 /* the column h(0..j, j) and, in h(j+1, j), the sum of squares */
			h[j + 1 + j * ss] = sqrt(h[j + 1 + j * ss]);
		} else {
			for (i = 0; i <= j; i++) {
				ETRY(lis_vector_dot(v[i], w, &h[i + j * ss]));
				ETRY(lis_vector_axpy(-h[i + j * ss], v[i], w));
			}
			ETRY(lis_vector_nrm2(w, &h[j + 1 + j * ss]));                    /* h(j+1,j) = ||w||_2 */
		}
		if (fabs(h[j + 1 + j * ss]) < c->tol) break;                         /* convergence check */
		ETRY(lis_vector_scale(1 / h[j + 1 + j * ss], w));                    /* v(j+1) = w / h(j+1,j) */
		ETRY(lis_vector_copy(w, v[j + 1]));
	}
	/* eigenvalues of the upper Hessenberg matrix: the diagonal and the 2 x 2 blocks QR leaves (a complex pair gives its real part twice) */
	time0 = lis_wtime();
	ETRY(lis_array_qr(ss, h, hq, hr, &hqriter, &hqrerr));
	time = lis_wtime() - time0;
	if (c->output) {
		lis_printf(LIS_COMM_WORLD, "size of subspace      : %D\n\n", ss);
		lis_printf(LIS_COMM_WORLD, "Ritz values:\n\n");
	}
	i = 0;
	while (i < ss) {
		i = i + 1;
		if (ss == i || fabs(h[i + (i - 1) * ss]) < c->tol) {
			if (c->output) {
				lis_printf(LIS_COMM_WORLD, "Arnoldi: mode number          = %D\n", i - 1);
				lis_printf(LIS_COMM_WORLD, "Arnoldi: Ritz value           = %e\n", (double)(h[i - 1 + (i - 1) * ss]));
			}
			esolver->evalue[i - 1] = h[i - 1 + (i - 1) * ss];
		} else {
			D = (h[i - 1 + (i - 1) * ss] + h[i + i * ss]) * (h[i - 1 + (i - 1) * ss] + h[i + i * ss])
			    - 4 * (h[i - 1 + (i - 1) * ss] * h[i + i * ss] - h[i - 1 + i * ss] * h[i + (i - 1) * ss]);
			if (D < 0) {
				if (c->output) {
					lis_printf(LIS_COMM_WORLD, "Arnoldi: mode number          = %D\n", i - 1);
					lis_printf(LIS_COMM_WORLD, "Arnoldi: Ritz value           = (%e, %e)\n", (double)((h[i - 1 + (i - 1) * ss] + h[i + i * ss]) / 2), (double)sqrt(-D) / 2);
					lis_printf(LIS_COMM_WORLD, "Arnoldi: mode number          = %D\n", i);
					lis_printf(LIS_COMM_WORLD, "Arnoldi: Ritz value           = (%e, %e)\n", (double)((h[i - 1 + (i - 1) * ss] + h[i + i * ss]) / 2), (double)-sqrt(-D) / 2);
				}
				esolver->evalue[i - 1] = (h[i - 1 + (i - 1) * ss] + h[i + i * ss]) / 2;
				esolver->evalue[i] = (h[i - 1 + (i - 1) * ss] + h[i + i * ss]) / 2;
				i = i + 1;
			} else {
				if (c->output) {
					lis_printf(LIS_COMM_WORLD, "Arnoldi: mode number          = %D\n", i - 1);
					lis_printf(LIS_COMM_WORLD, "Arnoldi: Ritz value           = %e\n", (double)(h[i - 1 + (i - 1) * ss]));
				}
				esolver->evalue[i - 1] = h[i - 1 + (i - 1) * ss];
			}
		}
	}
	lis_printf(LIS_COMM_WORLD, "Arnoldi: elapsed time         = %e sec.\n\n", time);      /* (printed at -eprint none too, as there) */
	if (!esolver->options[LIS_EOPTIONS_RVAL]) err = refine_modes(c, "Arnoldi");
done:
	if (hdev) (void)liship_free(hdev);
	free(dv);
	free(h); free(hq); free(hr);
	return err;
}

/* ================================================================== the generalized problem A x = lambda B x: power, inverse, Rayleigh quotient, CR
 * The reference's four loops that work (lis_egcg never updates x or p from its Ritz vector and ends in NaN: refused in lis_gesolve), statement for statement
 * in the helpers above.  A - sigma B is lis_matrix_shift_matrix (lis_shift.c): kernels on the HBM copies.  Sums that share a vector go through one
 * lisd_multidot pass -- rho and <B v, B v> of -e grqi, the three dot groups of -e gcr --, the bits of the separate dots (LIS_AMD_NO_FUSION=1 runs those). */
static LIS_INT gshift_back(LIS_MATRIX A, LIS_MATRIX B, LIS_SCALAR sigma, LIS_INT err)
{
	const LIS_INT e2 = lis_matrix_shift_matrix(A, B, -sigma);
	return (e2 && (!err || err == LIS_MAXITER)) ? e2 : err;
}

/* ------------------------------------------------------------------ generalized power iteration, lis_esolver_pi.c:305-464 (the preconditioner is B's, the solves are with B) */
static LIS_INT lis_egpi(LIS_ESOLVER esolver)
{
	ectx_t cx, *c = &cx;
	ectx_begin(c, esolver, 1);
	LIS_MATRIX A = c->A, B = esolver->B;
	LIS_VECTOR v = esolver->x, w = esolver->work[0], y = esolver->work[1], q = esolver->work[2];
	LIS_SCALAR eta, theta = 0.0;
	LIS_REAL nrm2, resid = 0.0;
	LIS_INT err = 0, iter = 0, iter2, code = LIS_MAXITER;
	int shifted = 0;
	if (esolver->options[LIS_EOPTIONS_INITGUESS_ONES]) ETRY(lis_vector_set_all(1.0, v));
	if (c->oshift != 0.0) { ETRY(lis_matrix_shift_matrix(A, B, c->oshift)); shifted = 1; }
	eshift_banner(c);
	ETRY(inner_solver(c, "-i bicg -p none"));
	c->solver->A = B;
	ETRY(lis_precon_create(c->solver, &c->precon));
	while (iter < c->emaxiter) {
		iter = iter + 1;
		ETRY(lis_vector_nrm2(v, &nrm2));                     /* v = v / ||v||_2 */
		ETRY(lis_vector_scale(1.0 / nrm2, v));
		ETRY(lis_matvec(A, v, w));                           /* w = A * v */
		ETRY(lis_vector_dot(v, w, &eta));                    /* v = v / <v,w>^1/2, w = w / <v,w>^1/2 */
		eta = sqrt(eta);
		ETRY(lis_vector_scale(1.0 / eta, v));
		ETRY(lis_vector_scale(1.0 / eta, w));
		ETRY(inner_solve_on(c, B, w, y, 0));                 /* y = B^-1 * w */
		lis_solver_get_iter(c->solver, &iter2);
		ETRY(lis_vector_dot(w, y, &theta));                  /* theta = <w,y> */
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
	esolver->evalue[0] = theta + c->oshift;
	ETRY(normalize(v));
	err = code;
done:
	if (shifted) err = gshift_back(A, B, c->oshift, err);
	inner_destroy(c);
	return err;
}

/* ------------------------------------------------------------------ generalized inverse iteration, lis_esolver_ii.c:357-520 */
static LIS_INT lis_egii(LIS_ESOLVER esolver)
{
	ectx_t cx, *c = &cx;
	ectx_begin(c, esolver, 1);
	LIS_MATRIX A = c->A, B = esolver->B;
	LIS_VECTOR v = esolver->x, w = esolver->work[0], y = esolver->work[1], q = esolver->work[2];
	LIS_SCALAR eta, theta = 0.0;
	LIS_REAL nrm2, resid = 0.0;
	LIS_INT err = 0, iter = 0, iter2, code = LIS_MAXITER;
	int shifted = 0;
	if (esolver->options[LIS_EOPTIONS_INITGUESS_ONES]) ETRY(lis_vector_set_all(1.0, v));
	if (c->oshift != 0.0) { ETRY(lis_matrix_shift_matrix(A, B, c->oshift)); shifted = 1; }
	eshift_banner(c);
	ETRY(inner_solver(c, "-i bicg -p none"));
	c->solver->A = A;
	ETRY(lis_precon_create(c->solver, &c->precon));
	while (iter < c->emaxiter) {
		iter = iter + 1;
		ETRY(lis_vector_nrm2(v, &nrm2));                     /* v = v / ||v||_2 */
		ETRY(lis_vector_scale(1.0 / nrm2, v));
		ETRY(lis_matvec(B, v, w));                           /* w = B * v */
		ETRY(lis_vector_dot(w, v, &eta));                    /* v = v / <w,v>^1/2, w = w / <w,v>^1/2 */
		eta = sqrt(eta);
		ETRY(lis_vector_scale(1.0 / eta, v));
		ETRY(lis_vector_scale(1.0 / eta, w));
		ETRY(inner_solve(c, w, y, 0));                       /* y = A^-1 * w */
		lis_solver_get_iter(c->solver, &iter2);
		ETRY(lis_vector_dot(w, y, &theta));                  /* theta = <w,y> */
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
	if (shifted) err = gshift_back(A, B, c->oshift, err);
	inner_destroy(c);
	return err;
}

/* ------------------------------------------------------------------ generalized Rayleigh quotient iteration, lis_esolver_rqi.c:350-501 (no -shift: rho is the shift;
 * the preconditioner is made once, of the unshifted A) */
static LIS_INT lis_egrqi(LIS_ESOLVER esolver)
{
	ectx_t cx, *c = &cx;
	ectx_begin(c, esolver, 0);
	LIS_MATRIX A = c->A, B = esolver->B;
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
		ETRY(lis_matrix_shift_matrix(A, B, rho));            /* y = (A - rho * B)^-1 * w */
		shifted = 1;
		ETRY(inner_solve(c, w, y, 0));
		ETRY(lis_matrix_shift_matrix(A, B, -rho));
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
	if (shifted) (void)lis_matrix_shift_matrix(A, B, -rho);  /* an inner solve failed between the two shifts: A goes back */
	inner_destroy(c);
	return err;
}

/* ------------------------------------------------------------------ generalized CR, lis_esolver_cg.c:1063-1265 */
static LIS_INT lis_egcr(LIS_ESOLVER esolver)
{
	ectx_t cx, *c = &cx;
	ectx_begin(c, esolver, 1);
	LIS_MATRIX A = c->A, B = esolver->B;
	LIS_VECTOR x = esolver->x;
	LIS_VECTOR r = esolver->work[0], p = esolver->work[1], w = esolver->work[2], Ax = esolver->work[3], Ap = esolver->work[4], Aw = esolver->work[5];
	LIS_VECTOR Bx = esolver->work[6], Bp = esolver->work[7], Bw = esolver->work[8];
	LIS_SCALAR lambda = 0.0, alpha, beta;
	LIS_SCALAR rAp, rBp, BxBx, ApAp, ApBp, BpBp, AwAp, AwBp, ApBw, BwBp;
	LIS_REAL nrm2, resid = 0.0;
	LIS_INT err = 0, iter = 0;
	double ptime = 0.0, time;
	int shifted = 0;
	static const int xpairs[2][2] = {{0, 1}, {1, 1}};        /* <A*x,B*x>, <B*x,B*x> over {Ax, Bx} */
	if (esolver->options[LIS_EOPTIONS_INITGUESS_ONES]) ETRY(lis_vector_set_all(1.0, x));
	if (c->oshift != 0.0) { ETRY(lis_matrix_shift_matrix(A, B, c->oshift)); shifted = 1; }
	eshift_banner(c);
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
	esolver->iter[0] = iter;
	esolver->resid[0] = resid;
	esolver->evalue[0] = lambda + c->oshift;
	ETRY(normalize(x));
	esolver->ptime = ptime;
	esolver->itime = c->solver->itime; esolver->p_c_time = c->solver->p_c_time; esolver->p_i_time = c->solver->p_i_time;
done:
	if (c->solver) c->solver->precon = NULL;
	inner_destroy(c);
	if (shifted) { const LIS_INT e2 = lis_matrix_shift_matrix(A, B, -c->oshift); if (e2 && !err) err = e2; }
	if (err) return err;
	esolver->retcode = (resid < c->tol) ? LIS_SUCCESS : LIS_MAXITER;
	return esolver->retcode;
}

/* ================================================================== several pairs of the generalized problem: subspace, Lanczos, Arnoldi
 * lis_egsi, lis_egli and lis_egai of the reference statement for statement, with the helpers of the two sections above.  The fused forms keep what those of
 * -e si / -e ai keep in HBM and add the two pair passes (liship_scale2_inv_sqrt_f64, liship_scale2_to_f64); no sum is taken from a product's fused-dot epilogue,
 * whose tree is not liship_dot_f64's, so fused and unfused agree in every bit (tests/test_gesolve_multi_gpu.py).  LIS_AMD_NO_FUSION=1 runs the lis_vector_* calls. */

/* the banner of the three and the linear solver they keep: "-i bicg -p none", then the command line's options */
static LIS_INT gmulti_solver(ectx_t *c, LIS_INT nigesolver)
{
	char esolvername[128];
	lis_esolver_get_esolvername(nigesolver, esolvername);
	if (c->output) lis_printf(LIS_COMM_WORLD, "inner eigensolver     : %s\n", esolvername);
	return inner_solver(c, "-i bicg -p none");
}

/* ------------------------------------------------------------------ generalized subspace iteration, lis_esolver_si.c:456-719.  As written there: v(j) is
 * orthogonalised against the earlier v(k) with the plain dot, not the B-inner product; eta = <v,w>^1/2 without fabs, so a negative sum gives NaN from there on;
 * work[4] (Ax there) is v(1) and has no use of its own.  With -ige gii the reference creates a preconditioner on A and then, falling through, on B, and leaks
 * both per mode: each is created once per mode here and freed, B's being the one the solves run with. */
static LIS_INT lis_egsi(LIS_ESOLVER esolver)
{
	ectx_t cx, *c = &cx;
	ectx_begin(c, esolver, 1);
	LIS_MATRIX A = c->A, B = esolver->B;
	const LIS_INT ss = esolver->options[LIS_EOPTIONS_SUBSPACE], nigesolver = esolver->options[LIS_EOPTIONS_INNER_GENERALIZED_ESOLVER], n = A->n;
	const int power = nigesolver == LIS_ESOLVER_GPI;
	LIS_VECTOR y = esolver->work[0], w = esolver->work[1], q = esolver->work[2], *v = &esolver->work[3];
	LIS_SCALAR theta = 0.0, eta;
	LIS_REAL nrm2, resid = 0.0;
	LIS_INT err = 0, iter, j;
	double etime0, etime, *hdev = NULL, **dv = NULL;         /* the chain's coefficients (HBM) and its basis as device pointers */
	int shifted = 0;
	ETRY(lis_vector_set_all(1.0, y));
	ETRY(lis_vector_nrm2(y, &nrm2));
	ETRY(lis_vector_scale(1.0 / nrm2, y));
	if (c->oshift != 0.0) { ETRY(lis_matrix_shift_matrix(A, B, c->oshift)); shifted = 1; }
	eshift_banner(c);
	ETRY(gmulti_solver(c, nigesolver));
	if (c->output) {
		lis_printf(LIS_COMM_WORLD, "size of subspace      : %D\n\n", ss);
		lis_printf(LIS_COMM_WORLD, "compute eigenpairs in subspace:\n\n");
	}
	if (!lisg.no_fusion) EHIP(lisd_malloc((void **)&hdev, sizeof(double) * (size_t)(ss + 2)));
	if (!(dv = (double **)malloc(sizeof(double *) * (size_t)(ss + 1)))) { err = LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "malloc size = %D\n", ss + 1); goto done; }
	j = 0;
	while (j < ss) {
		etime0 = lis_wtime();
		ETRY(lis_vector_duplicate(A, &esolver->evector[j]));
		j = j + 1;
		ETRY(lis_vector_copy(y, v[j]));
		if (c->precon) { lis_precon_destroy(c->precon); c->precon = NULL; }
		if (!power) {
			c->solver->A = A;
			ETRY(lis_precon_create(c->solver, &c->precon));
			lis_precon_destroy(c->precon); c->precon = NULL;
		}
		c->solver->A = B;
		ETRY(lis_precon_create(c->solver, &c->precon));
		const int fused = chain_ready(n, y, v[j]) && chain_ready(n, w, w);
		iter = 0;
		while (iter < c->emaxiter) {
			iter = iter + 1;
			/* QR factorization V*R = Z for starting vector Z */
			ETRY(orthogonalise(n, j, v, fused, hdev, dv));
			/* kernel: w = A * v (gpi) or w = B * v (gii); v = v / <v,w>^1/2, w = w / <v,w>^1/2; y = B^-1 * w or y = A^-1 * w */
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
			ETRY(inner_solve_on(c, power ? B : A, w, y, 0));
			if (j == 1) inner_times(c);
			/* theta = <w,y>; resid = ||y - theta * v||_2 / |theta|; y = y / ||y||_2; v = y */
			if (fused) {
				static const int pairs[2][2] = {{0, 0}, {1, 0}};
				double *dy, *dw, *dvj, sums[3];
				ETRY(lisd_vec_in(y, &dy)); ETRY(lisd_vec_in(w, &dw)); ETRY(lisd_vec_in(v[j], &dvj));
				const double *dyw[2] = {dy, dw};
				EHIP(liship_multidot_f64(n, 2, dyw, 2, pairs, lisg.reduce_out, lisg.reduce_work, lisg.stream));
				EHIP(liship_ritz_tail_f64(n, lisg.reduce_out, dy, dvj, lisg.reduce_out + 2, lisg.reduce_work, lisg.stream));
				ETRY(lisd_vec_done(y)); ETRY(lisd_vec_done(v[j]));
				ETRY(lisd_fetch(3, sums));                       /* the one read-back of the iteration */
				nrm2 = sqrt(sums[0]); theta = sums[1]; resid = sqrt(sums[2]);
				resid = resid / fabs(theta);
			} else {
				ETRY(lis_vector_dot(w, y, &theta));
				ETRY(lis_vector_axpyz(-theta, v[j], y, q));
				ETRY(lis_vector_nrm2(q, &resid));
				resid = resid / fabs(theta);
				ETRY(lis_vector_nrm2(y, &nrm2));
				ETRY(lis_vector_scale(1.0 / nrm2, y));
				ETRY(lis_vector_copy(y, v[j]));
			}
			/* convergence check: the history and iter[0] are mode 0's */
			if (j == 1) {
				if (c->output & LIS_EPRINT_MEM) esolver->rhistory[iter] = resid;
				esolver->iter[j - 1] = iter;
			}
			if (c->output & LIS_EPRINT_OUT) lis_printf(LIS_COMM_WORLD, "iteration: %5d  relative residual = %E\n", (int)iter, (double)resid);
			if (c->tol > resid) break;
		}
		esolver->evalue[j - 1] = power ? theta + c->oshift : 1.0 / theta + c->oshift;
		esolver->resid[j - 1] = resid;
		esolver->iter[j - 1] = iter;
		ETRY(lis_vector_copy(v[j], esolver->evector[j - 1]));
		etime = lis_wtime() - etime0;
		if (c->output & (ss > 1)) {                           /* (as written there: the MEM bit of -eprint) */
			lis_printf(LIS_COMM_WORLD, "Generalized Subspace: mode number          = %D\n", j - 1);
			lis_printf(LIS_COMM_WORLD, "Generalized Subspace: eigenvalue           = %e\n", (double)esolver->evalue[j - 1]);
			lis_printf(LIS_COMM_WORLD, "Generalized Subspace: elapsed time         = %e sec.\n", etime);
			lis_printf(LIS_COMM_WORLD, "Generalized Subspace: number of iterations = %D\n", iter);
			lis_printf(LIS_COMM_WORLD, "Generalized Subspace: relative residual    = %e\n\n", (double)resid);
		}
	}
done:
	if (hdev) (void)liship_free(hdev);
	free(dv);
	if (shifted) { const LIS_INT e2 = lis_matrix_shift_matrix(A, B, -c->oshift); if (e2 && !err) err = e2; }
	inner_destroy(c);
	if (!err) err = lis_vector_copy(esolver->evector[0], esolver->x);
	return err;                                              /* LIS_SUCCESS also when a mode stopped at -emaxiter, as there */
}

/* ------------------------------------------------------------------ generalized Lanczos, lis_esolver_li.c:456-694.  As written there: w = &work[2] and
 * v = &work[3], so w(j+1) and v(j) are one vector -- the copy r -> w(j) overwrites v(j-1), and the reorthogonalisation of v(j) runs against overwritten vectors
 * (it does not feed t[]); the start is r = B * q with beta = |<q,r>|^1/2, B q = r is solved every step, and t(j, j-1) is |<q,r>|^1/2, not a 2-norm. */
static LIS_INT lis_egli(LIS_ESOLVER esolver)
{
	ectx_t cx, *c = &cx;
	ectx_begin(c, esolver, 0);
	LIS_MATRIX A = c->A, B = esolver->B;
	const LIS_INT ss = esolver->options[LIS_EOPTIONS_SUBSPACE], nigesolver = esolver->options[LIS_EOPTIONS_INNER_GENERALIZED_ESOLVER], n = A->n;
	LIS_VECTOR q = esolver->work[0], r = esolver->work[1], *w = &esolver->work[2], *v = &esolver->work[3];
	LIS_SCALAR beta, dot, div, *t = NULL, *tq = NULL, *tr = NULL;
	LIS_REAL qrerr;
	LIS_INT err = 0, i, j, k, qriter;
	double time, time0;
	t = (LIS_SCALAR *)calloc((size_t)ss * ss, sizeof(LIS_SCALAR));
	tq = (LIS_SCALAR *)malloc((size_t)ss * ss * sizeof(LIS_SCALAR));
	tr = (LIS_SCALAR *)malloc((size_t)ss * ss * sizeof(LIS_SCALAR));
	if (!t || !tq || !tr) { err = LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "malloc size = %D\n", (LIS_INT)(ss * ss * sizeof(LIS_SCALAR))); goto done; }
	ETRY(lis_vector_set_all(0.0, w[0]));
	ETRY(lis_vector_set_all(0.0, v[0]));
	ETRY(lis_vector_set_all(1.0, q));
	ETRY(gmulti_solver(c, nigesolver));
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
	/* eigenvalues of the symmetric tridiagonal matrix */
	time0 = lis_wtime();
	ETRY(lis_array_qr(ss, t, tq, tr, &qriter, &qrerr));
	time = lis_wtime() - time0;
	for (i = 0; i < ss; i++) esolver->evalue[i] = t[i * ss + i];
	if (c->output) {
		lis_printf(LIS_COMM_WORLD, "size of subspace      : %D\n\n", ss);
		lis_printf(LIS_COMM_WORLD, "Ritz values :\n\n");
		for (i = 0; i < ss; i++) {
			lis_printf(LIS_COMM_WORLD, "Generalized Lanczos: mode number          = %D\n", i);
			lis_printf(LIS_COMM_WORLD, "Generalized Lanczos: Ritz value           = %e\n", (double)esolver->evalue[i]);
		}
		lis_printf(LIS_COMM_WORLD, "Lanczos: elapsed time         = %e sec.\n\n", time);
	}
	if (!esolver->options[LIS_EOPTIONS_RVAL]) err = refine_modes(c, "Generalized Lanczos");     /* -rval true: iter[] and resid[] stay 0 (heap contents there) */
done:
	inner_destroy(c);
	free(t); free(tq); free(tr);
	return err;
}

/* ------------------------------------------------------------------ generalized Arnoldi, lis_esolver_ai.c:491-750: lis_eai with w = B^-1 * (A * v(j)) -- solve,
 * then copy y -> w -- in front of the Hessenberg column, which is taken as lis_eai takes it.  (At i = ss the reference reads h(ss, ss-1) and h(ss, ss), past
 * its array; the last mode's Ritz value is the diagonal entry here, as in lis_eai.) */
static LIS_INT lis_egai(LIS_ESOLVER esolver)
{
	ectx_t cx, *c = &cx;
	ectx_begin(c, esolver, 0);
	LIS_MATRIX A = c->A, B = esolver->B;
	const LIS_INT ss = esolver->options[LIS_EOPTIONS_SUBSPACE], nigesolver = esolver->options[LIS_EOPTIONS_INNER_GENERALIZED_ESOLVER], n = A->n;
	LIS_VECTOR w = esolver->work[0], y = esolver->work[1], *v = &esolver->work[2];
	LIS_SCALAR *h = NULL, *hq = NULL, *hr = NULL;
	LIS_REAL nrm2, hqrerr, D;
	LIS_INT err = 0, i, j, hqriter;
	double time, time0, *hdev = NULL, **dv = NULL;
	const int fused = !lisg.no_fusion && ss + 1 <= 256;                     /* (a column comes home through the page-locked landing zone) */
	h = (LIS_SCALAR *)calloc((size_t)ss * ss + 1, sizeof(LIS_SCALAR));      /* (one more than there: h(ss, ss-1), which the last column's norm is written to) */
	hq = (LIS_SCALAR *)malloc((size_t)ss * ss * sizeof(LIS_SCALAR));
	hr = (LIS_SCALAR *)malloc((size_t)ss * ss * sizeof(LIS_SCALAR));
	if (!h || !hq || !hr) { err = LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "malloc size = %D\n", (LIS_INT)(ss * ss * sizeof(LIS_SCALAR))); goto done; }
	ETRY(lis_vector_set_all(1.0, v[0]));
	ETRY(lis_vector_nrm2(v[0], &nrm2));
	ETRY(lis_vector_scale(1.0 / nrm2, v[0]));
	ETRY(gmulti_solver(c, nigesolver));
	c->solver->A = B;
	ETRY(lis_precon_create(c->solver, &c->precon));
	if (fused) EHIP(lisd_malloc((void **)&hdev, sizeof(double) * (size_t)(ss + 2)));
	if (!(dv = (double **)malloc(sizeof(double *) * (size_t)(ss + 1)))) { err = LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "malloc size = %D\n", ss + 1); goto done; }
	j = -1;
	while (j < ss - 1) {
		j = j + 1;
		ETRY(lis_matvec(A, v[j], w));                                        /* w = A * v(j) */
		ETRY(inner_solve_on(c, B, w, y, 0));                                 /* w = B^-1 * w */
		ETRY(lis_vector_copy(y, w));
		if (fused) {
			/* h(i,j) = <v(i), w>; w = w - h(i,j) * v(i), i = 0 .. j, then ||w||^2: one chain, one read-back per column */
			double *dw;
			ETRY(lisd_vec_in(w, &dw));
			for (i = 0; i <= j; i++) ETRY(lisd_vec_in(v[i], &dv[i]));
			EHIP(liship_dot_f64(n, dv[0], dw, hdev, lisg.reduce_work, lisg.stream));
			ETRY(lisd_mgs_chain(n, j + 1, dv, dw, hdev));
			EHIP(liship_mgs_step_f64(n, hdev + j, dv[j], dw, NULL, hdev + j + 1, lisg.reduce_work, lisg.stream));
			ETRY(lisd_vec_done(w));
			ETRY(lisd_fetch_from(hdev, j + 2, h + j * ss));                 /* the column h(0..j, j) and, in h(j+1, j), the sum of squares */
			h[j + 1 + j * ss] = sqrt(h[j + 1 + j * ss]);
		} else {
			for (i = 0; i <= j; i++) {
				ETRY(lis_vector_dot(v[i], w, &h[i + j * ss]));
				ETRY(lis_vector_axpy(-h[i + j * ss], v[i], w));
			}
			ETRY(lis_vector_nrm2(w, &h[j + 1 + j * ss]));                    /* h(j+1,j) = ||w||_2 */
		}
		if (fabs(h[j + 1 + j * ss]) < c->tol) break;                         /* convergence check */
		ETRY(lis_vector_scale(1 / h[j + 1 + j * ss], w));                    /* v(j+1) = w / h(j+1,j) */
		ETRY(lis_vector_copy(w, v[j + 1]));
	}
	/* eigenvalues of the upper Hessenberg matrix: the diagonal and the 2 x 2 blocks QR leaves (a complex pair gives its real part twice) */
	time0 = lis_wtime();
	ETRY(lis_array_qr(ss, h, hq, hr, &hqriter, &hqrerr));
	time = lis_wtime() - time0;
	if (c->output) {
		lis_printf(LIS_COMM_WORLD, "size of subspace      : %D\n\n", ss);
		lis_printf(LIS_COMM_WORLD, "Ritz values:\n\n");
	}
	i = 0;
	while (i < ss) {
		i = i + 1;
		if (ss == i || fabs(h[i + (i - 1) * ss]) < c->tol) {
			if (c->output) {
				lis_printf(LIS_COMM_WORLD, "Generalized Arnoldi: mode number              = %D\n", i - 1);
				lis_printf(LIS_COMM_WORLD, "Generalized Arnoldi: Ritz value               = %e\n", (double)(h[i - 1 + (i - 1) * ss]));
			}
			esolver->evalue[i - 1] = h[i - 1 + (i - 1) * ss];
		} else {
			D = (h[i - 1 + (i - 1) * ss] + h[i + i * ss]) * (h[i - 1 + (i - 1) * ss] + h[i + i * ss])
			    - 4 * (h[i - 1 + (i - 1) * ss] * h[i + i * ss] - h[i - 1 + i * ss] * h[i + (i - 1) * ss]);
			if (D < 0) {
				if (c->output) {
					lis_printf(LIS_COMM_WORLD, "Generalized Arnoldi: mode number              = %D\n", i - 1);
					lis_printf(LIS_COMM_WORLD, "Generalized Arnoldi: Ritz value               = (%e, %e)\n", (double)((h[i - 1 + (i - 1) * ss] + h[i + i * ss]) / 2), (double)sqrt(-D) / 2);
					lis_printf(LIS_COMM_WORLD, "Generalized Arnoldi: mode number              = %D\n", i);
					lis_printf(LIS_COMM_WORLD, "Generalized Arnoldi: Ritz value               = (%e, %e)\n", (double)((h[i - 1 + (i - 1) * ss] + h[i + i * ss]) / 2), (double)-sqrt(-D) / 2);
				}
				esolver->evalue[i - 1] = (h[i - 1 + (i - 1) * ss] + h[i + i * ss]) / 2;
				esolver->evalue[i] = (h[i - 1 + (i - 1) * ss] + h[i + i * ss]) / 2;
				i = i + 1;
			} else {
				if (c->output) {
					lis_printf(LIS_COMM_WORLD, "Generalized Arnoldi: mode number              = %D\n", i - 1);
					lis_printf(LIS_COMM_WORLD, "Generalized Arnoldi: Ritz value               = %e\n", (double)(h[i - 1 + (i - 1) * ss]));
				}
				esolver->evalue[i - 1] = h[i - 1 + (i - 1) * ss];
			}
		}
	}
	lis_printf(LIS_COMM_WORLD, "Generalized Arnoldi: elapsed time         = %e sec.\n\n", time);      /* (printed at -eprint none too, as there) */
	if (!esolver->options[LIS_EOPTIONS_RVAL]) err = refine_modes(c, "Generalized Arnoldi");
done:
	inner_destroy(c);
	if (hdev) (void)liship_free(hdev);
	free(dv);
	free(h); free(hq); free(hr);
	return err;
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
	if (B != NULL) {                                         /* ref :323-336 */
		LISCHK(lisi_matrix_check(B, LISI_CHECK_ASSEMBLED));
		if (B->n != x->n) return LISI_ERR(LIS_ERR_ILL_ARG, "matrix B (n = %D) and vector x (n = %D) differ in size\n", B->n, x->n);
		if (B->gn <= 0) return LISI_ERR(LIS_ERR_ILL_ARG, "Size n(=%D) of matrix B is less than 0\n", B->gn);
	}
	const LIS_INT nesolver = esolver->options[LIS_EOPTIONS_ESOLVER], ss = esolver->options[LIS_EOPTIONS_SUBSPACE], mode = esolver->options[LIS_EOPTIONS_MODE];
	const LIS_INT emaxiter = esolver->options[LIS_EOPTIONS_MAXITER], output = esolver->options[LIS_EOPTIONS_OUTPUT];
	const LIS_INT estorage = esolver->options[LIS_EOPTIONS_STORAGE], eblock = esolver->options[LIS_EOPTIONS_STORAGE_BLOCK];
	const LIS_INT eprecision = esolver->options[LIS_EOPTIONS_PRECISION];
	if (nesolver < 1 || nesolver > LIS_ESOLVER_LEN) return LISI_ERR(LIS_ERR_ILL_ARG, "Parameter LIS_EOPTIONS_ESOLVER is %D (Set between 1 to %D)\n", nesolver, LIS_ESOLVER_LEN);
	/* what is not served, said before A or x is touched */
	if (B != NULL && !is_generalized(nesolver)) {             /* (the reference runs the standard loop and never reads B) */
		esolver->retcode = LIS_ERR_NOT_IMPLEMENTED;
		return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "generalized eigenproblems (lis_gesolve with a matrix B) are served by -e gpi | gii | grqi | gcr | gsi | gli | gai: %s (-e %s) is a standard eigensolver, which would ignore B\n",
		                esolver_names[nesolver], esolver_keys[nesolver - 1]);
	}
	if (is_generalized(nesolver) && B == NULL) {              /* (the reference's loops multiply by that NULL) */
		esolver->retcode = LIS_ERR_NOT_IMPLEMENTED;
		return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "eigensolver %s (-e %s) is not served by liblis_amd without a matrix B: lis_esolve serves pi, ii, rqi, cg, cr, si, li, ai, lis_gesolve with a B gpi, gii, grqi, gcr, gsi, gli, gai\n",
		                esolver_names[nesolver], esolver_keys[nesolver - 1]);
	}
	if (nesolver == LIS_ESOLVER_GCG) {
		esolver->retcode = LIS_ERR_NOT_IMPLEMENTED;
		return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "eigensolver Generalized CG (-e gcg) is not served by liblis_amd: the reference's loop never updates x from its Ritz vector and ends in NaN at every thread count; -e gcr is the generalized solver of that family that works\n");
	}
	if (is_gmulti(nesolver) && ss == 1) {
		esolver->retcode = LIS_ERR_NOT_IMPLEMENTED;
		return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "eigensolver %s (-e %s) serves several pairs; a subspace of one vector (-ss 1, the default) is not served by liblis_amd: one pair is what -e gpi / -e gii serve\n",
		                esolver_names[nesolver], esolver_keys[nesolver - 1]);
	}
	if (is_multi(nesolver) && ss == 1) {
		esolver->retcode = LIS_ERR_NOT_IMPLEMENTED;
		return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "eigensolver %s (-e %s) with a subspace of one vector (-ss 1, the default) is not served by liblis_amd: one eigenpair is what -e pi / -e ii serve\n",
		                esolver_names[nesolver], esolver_keys[nesolver - 1]);
	}
	if (lisg.nprocs > 1 || A->nprocs > 1) { esolver->retcode = LIS_ERR_NOT_IMPLEMENTED; return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "lis_esolve is served on one rank (this job has %D)\n", (LIS_INT)lisg.nprocs); }
	if (eprecision != LIS_PRECISION_DOUBLE) { esolver->retcode = LIS_ERR_ILL_ARG; return LISI_ERR(LIS_ERR_ILL_ARG, "Quad precision is not enabled\n"); }
	if (estorage > 0 && estorage != A->matrix_type && !lisi_format_served(estorage)) {
		esolver->retcode = LIS_ERR_NOT_IMPLEMENTED;
		return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-estorage %D: storage format is not served by liblis_amd\n", estorage);
	}
	if (emaxiter < 0) { esolver->retcode = LIS_ERR_ILL_ARG; return LISI_ERR(LIS_ERR_ILL_ARG, "Parameter LIS_EOPTIONS_MAXITER(=%D) is less than 0\n", emaxiter); }
	if (ss < 1 || mode < 0 || mode > ss + 1) { esolver->retcode = LIS_ERR_ILL_ARG; return LISI_ERR(LIS_ERR_ILL_ARG, "Parameters LIS_EOPTIONS_SUBSPACE(=%D), LIS_EOPTIONS_MODE(=%D) are out of range\n", ss, mode); }
	if (is_multi(nesolver) || is_gmulti(nesolver)) {         /* ref :389-411, and the inner eigensolvers the loops can run */
		const LIS_INT niesolver = esolver->options[LIS_EOPTIONS_INNER_ESOLVER], nigesolver = esolver->options[LIS_EOPTIONS_INNER_GENERALIZED_ESOLVER];
		if (ss > A->gn) { esolver->retcode = LIS_ERR_ILL_ARG; return LISI_ERR(LIS_ERR_ILL_ARG, "Parameter LIS_EOPTIONS_SUBSPACE is %D (Set less than or equal to matrix size %D)\n", ss, A->gn); }
		if (mode >= ss) { esolver->retcode = LIS_ERR_ILL_ARG; return LISI_ERR(LIS_ERR_ILL_ARG, "Parameter LIS_EOPTIONS_MODE is %D (Set less than subspace size %D)\n", mode, ss); }
		if (is_multi(nesolver) && (nesolver == LIS_ESOLVER_SI ? (niesolver != LIS_ESOLVER_PI && niesolver != LIS_ESOLVER_II) : (niesolver < LIS_ESOLVER_PI || niesolver > LIS_ESOLVER_CR))) {
			esolver->retcode = LIS_ERR_NOT_IMPLEMENTED;       /* (the reference's subspace loop applies A for -ie pi and -ie ii only) */
			return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "inner eigensolver %D (-ie) is not served by liblis_amd for -e %s (%s)\n", niesolver, esolver_keys[nesolver - 1],
			                nesolver == LIS_ESOLVER_SI ? "pi, ii" : "pi, ii, rqi, cg, cr");
		}
		if (nesolver == LIS_ESOLVER_GSI ? (nigesolver != LIS_ESOLVER_GPI && nigesolver != LIS_ESOLVER_GII)
		                                : is_gmulti(nesolver) && nigesolver != LIS_ESOLVER_GPI && nigesolver != LIS_ESOLVER_GII && nigesolver != LIS_ESOLVER_GRQI && nigesolver != LIS_ESOLVER_GCR) {
			esolver->retcode = LIS_ERR_NOT_IMPLEMENTED;       /* (the reference's generalized subspace loop applies neither matrix for another -ige; its gcg ends in NaN) */
			return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "inner generalized eigensolver %D (-ige) is not served by liblis_amd for -e %s (%s)\n", nigesolver, esolver_keys[nesolver - 1],
			                nesolver == LIS_ESOLVER_GSI ? "gpi, gii" : "gpi, gii, grqi, gcr");
		}
	}
	if (B != NULL && (lisi_format_coo_dns(A->matrix_type) || lisi_format_coo_dns(B->matrix_type) || lisi_format_coo_dns(estorage))) {
		esolver->retcode = LIS_ERR_NOT_IMPLEMENTED;              /* (explicit: a COO copy looks like CSR in HBM, and lis_matrix_shift_matrix refuses both) */
		return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "lis_gesolve: A and B in COO or DNS storage (or -estorage coo | dns) are not served: lis_matrix_shift_matrix does not take them (A, B and x are untouched)\n");
	}
	if (B != NULL && (A->is_splited || B->is_splited || !lisi_format_swept(B->matrix_type) || B->np != B->n || A->np != A->n)) {
		esolver->retcode = LIS_ERR_NOT_IMPLEMENTED;
		return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "lis_gesolve: A and B must be unsplit matrices in a served storage format without ghost columns (lis_matrix_shift_matrix)\n");
	}
	if (MDEV(A)->device_only && A->matrix_type != LIS_MATRIX_CSR) { esolver->retcode = LIS_ERR_NOT_IMPLEMENTED; return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "a matrix that lives in HBM only is shifted in CSR storage\n"); }
	esolver->eprecision = eprecision;

	/* the arrays of the object (ss + 2 entries each, ref :438-550), zeroed */
	arrays_free(esolver);                                    /* (with the eigenvectors an earlier solve left) */
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

	esolver->A = A; esolver->B = B;
	if (output) {
		lis_printf(LIS_COMM_WORLD, "precision             : %s\n", eprecision_keys[eprecision]);
		lis_printf(LIS_COMM_WORLD, "eigensolver           : %s\n", esolver_names[nesolver]);
		lis_printf(LIS_COMM_WORLD, "convergence condition : ||lx-(B^-1)Ax||_2 <= %6.1e * ||lx||_2\n", (double)esolver->params[LIS_EPARAMS_RESID - LIS_EOPTIONS_LEN]);
		if (A->matrix_type == LIS_MATRIX_BSR) lis_printf(LIS_COMM_WORLD, "matrix storage format : %s(%D x %D)\n", estorage_names[A->matrix_type - 1], eblock, eblock);
		else lis_printf(LIS_COMM_WORLD, "matrix storage format : %s\n", estorage_names[A->matrix_type - 1]);
	}
	double time = lis_wtime();
	esolver->ptime = 0; esolver->itime = 0; esolver->p_c_time = 0; esolver->p_i_time = 0;
	if ((err = work_alloc(esolver, nesolver == LIS_ESOLVER_CG || nesolver == LIS_ESOLVER_CR ? 6 : nesolver == LIS_ESOLVER_SI ? 4 + ss : is_multi(nesolver) ? 2 + ss :
	                               nesolver == LIS_ESOLVER_GSI ? 5 + ss : nesolver == LIS_ESOLVER_GLI ? 4 + ss : nesolver == LIS_ESOLVER_GAI ? 3 + ss :
	                               nesolver == LIS_ESOLVER_GCR ? 9 : is_generalized(nesolver) ? 3 : 2))) goto fail;
	esolver->x = xx; esolver->xx = x;

	switch (nesolver) {
	case LIS_ESOLVER_PI:  err = lis_epi(esolver); break;
	case LIS_ESOLVER_II:  err = lis_eii(esolver); break;
	case LIS_ESOLVER_RQI: err = lis_erqi(esolver); break;
	case LIS_ESOLVER_CG:  err = lis_ecg(esolver); break;
	case LIS_ESOLVER_SI:  err = lis_esi(esolver); break;
	case LIS_ESOLVER_LI:  err = lis_eli(esolver); break;
	case LIS_ESOLVER_AI:  err = lis_eai(esolver); break;
	case LIS_ESOLVER_GPI: err = lis_egpi(esolver); break;
	case LIS_ESOLVER_GII: err = lis_egii(esolver); break;
	case LIS_ESOLVER_GRQI: err = lis_egrqi(esolver); break;
	case LIS_ESOLVER_GCR: err = lis_egcr(esolver); break;
	case LIS_ESOLVER_GSI: err = lis_egsi(esolver); break;
	case LIS_ESOLVER_GLI: err = lis_egli(esolver); break;
	case LIS_ESOLVER_GAI: err = lis_egai(esolver); break;
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
	if (is_multi(nesolver) || is_gmulti(nesolver)) arrays_free(esolver);            /* the getters of several pairs answer for a solve that ended */
	return err;
}

LIS_INT lis_esolve(LIS_MATRIX A, LIS_VECTOR x, LIS_SCALAR *evalue0, LIS_ESOLVER esolver)
{
	const LIS_INT err = lis_gesolve(A, NULL, x, evalue0, esolver);
	if (err) { esolver->retcode = err; return err; }
	return LIS_SUCCESS;
}
